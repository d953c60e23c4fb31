"""The cross entropy options on HIP (csrc/loss.hip: lg_cross_entropy_opt_fwd / _bwd; models/loss.py:
leakgnn::cross_entropy_opt, CrossEntropyLoss, distance_smoothing, loss_from_args): class weights w,
label smoothing eps over a (C, C) table U (absent: torch's uniform 1 / C) and the mean / sum / none
reductions, through the C ABI of include/leakgnn.h and through the module.

Truth: -sum_c a[c] * log_softmax(x)[c] with a[c] = w[c] * ((1 - eps) * [c == y] + eps * U[y, c]),
composed in torch on the CPU in float64 (and, where torch has the configuration, checked there
against F.cross_entropy in float64); the float32 CPU run of the same expression is the yardstick.
The bar is that of tests/test_gpu_step_tail.py::_bar,
    max|got - ref64| <= max(4 * max|ref32 - ref64|, rt * max|ref64|),
rt = 1e-6 for loss, lse and row losses, 1e-5 for dlogits.  eps enters the reference as the fp32
value the ABI receives.  Every case prints its RATIO lines (error / limit; 1.0 would be the bar).
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import LTA_INP, lta_ids

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LG_OK = 0
NAN, INF = float("nan"), float("inf")
RED = {"mean": 0, "sum": 1, "none": 2}
EPS = torch.tensor(0.15, dtype=torch.float32).item()  # the fp32 value the ABI receives


def _lib():
    from models import _native as nat
    return nat, nat.load_library()


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _bar(name: str, got, ref32, ref64, rt: float, what: str = "") -> None:
    """max|got - ref64| <= max(4 * max|ref32 - ref64|, rt * max|ref64|) (+1e-12, as helpers)."""
    t = ref64.detach().double().cpu()
    eg = (got.detach().double().cpu() - t).abs().max().item() if t.numel() else 0.0
    ec = (ref32.detach().double().cpu() - t).abs().max().item() if t.numel() else 0.0
    lim = max(4.0 * ec, rt * (t.abs().max().item() if t.numel() else 0.0)) + 1e-12
    print(f"RATIO {name} {eg / lim:.3f} err {eg:.3e} fp32-ref err {ec:.3e} lim {lim:.3e} [{what}]")
    assert eg <= lim, f"{what} {name}: err {eg:.3e} > {lim:.3e} (fp32 reference err {ec:.3e})"


# ------------------------------------------------------------------ the reference

def _ref(x, t, w, eps, U, red, ignore, g, dtype):
    """The formula of include/leakgnn.h on the CPU in `dtype`.  x (B, C), t (B,), w (C,) or None, U
    (C, C) or None, g a float (mean, sum) or a (B,) tensor (none).  Rows that are not counted
    (ignored, or a target outside [0, C)) have a = 0.  Returns loss (or the rows), lse, S, dlogits."""
    B, C = x.shape
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    counted = (t != ignore) & (t >= 0) & (t < C)
    tt = t.clamp(0, C - 1)
    base = U.to(dtype)[tt] if U is not None else torch.full((B, C), 1.0 / C, dtype=dtype)
    a = (1.0 - eps) * F.one_hot(tt, C).to(dtype) + eps * base
    if w is not None:
        a = a * w.to(dtype)[None, :]
    a = a * counted[:, None].to(dtype)
    lp = torch.log_softmax(xx, dim=1)
    rows = -torch.where(a != 0, a * lp, torch.zeros((), dtype=dtype)).sum(dim=1)
    den = ((w.to(dtype)[tt] if w is not None else torch.ones(B, dtype=dtype)) * counted.to(dtype)).sum()
    out = {"mean": rows.sum() / den, "sum": rows.sum(), "none": rows}[red]
    if B:
        ((out * g).sum()).backward()
    grad = xx.grad if xx.grad is not None else torch.zeros_like(xx)
    return out.detach(), torch.logsumexp(xx.detach(), dim=1), a.sum(dim=1), grad


def _torch_ce64(x, t, w, eps, red, ignore):
    return F.cross_entropy(x.double(), t, weight=None if w is None else w.double(), ignore_index=ignore,
                           reduction=red, label_smoothing=eps)


# ------------------------------------------------------------------ the ABI

def _abi(x, t, w=None, eps=0.0, U=None, red="mean", ignore=-100, g=1.0, strided=False, U_dev=None):
    """lg_cross_entropy_opt_fwd then _bwd on CPU tensors.  strided: the logits are columns 3 .. 3 + C
    of a NaN-filled (B, C + 7) buffer, dlogits columns 1 .. 1 + C of a NaN-filled (B, C + 3) one
    and the table columns 0 .. C of a NaN-filled (C, C + 5) one.  U_dev: (device tensor, ldu) to
    pass as the table instead of U.  Returns loss (a scalar, or the (B,) rows), lse, S, dlogits
    (CPU) and the dlogits buffer."""
    nat, lib = _lib()
    B, C = x.shape
    ldx, ox, ldd, od = (C + 7, 3, C + 3, 1) if strided else (C, 0, C, 0)
    xb = torch.full((B, ldx), NAN, device=DEV)
    xb[:, ox:ox + C] = x.to(DEV)
    db = torch.full((B, ldd), NAN, device=DEV)
    td = t.to(DEV)
    wd = None if w is None else w.to(DEV)
    ud, ldu = None, 0
    if U_dev is not None:
        ud, ldu = U_dev
    elif U is not None:
        ldu = C + 5 if strided else C
        ud = torch.full((C, ldu), NAN, device=DEV)
        ud[:, :C] = U.to(DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    denom = torch.full((1,), 7.0, device=DEV)
    lse, rowloss, rowsum = (torch.full((B,), NAN, device=DEV) for _ in range(3))
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    gd = (g.to(DEV).float() if torch.is_tensor(g) else torch.tensor([g], dtype=torch.float32, device=DEV))
    st = nat.stream_of(xb)
    p = nat.ptr
    assert lib.lg_cross_entropy_opt_fwd(xb.data_ptr() + 4 * ox, p(td), B, C, ldx, ignore, p(wd), p(ud), ldu, eps,
                                        RED[red], p(loss), p(lse), p(rowloss), p(rowsum), p(denom), p(counter),
                                        st) == LG_OK
    assert lib.lg_cross_entropy_opt_bwd(xb.data_ptr() + 4 * ox, p(td), p(lse), p(rowsum), p(denom), p(gd), B, C, ldx,
                                        ignore, p(wd), p(ud), ldu, eps, RED[red], db.data_ptr() + 4 * od, ldd,
                                        st) == LG_OK
    torch.cuda.synchronize()
    assert int(counter.item()) == 0, "completion counter not back at 0"
    out = rowloss.cpu() if red == "none" else loss[0].cpu()
    return out, lse.cpu(), rowsum.cpu(), db[:, od:od + C].cpu().contiguous(), db.cpu()


def _check(x, t, w=None, eps=0.0, U=None, red="mean", ignore=-100, g=1.0, what=""):
    """Contiguous and strided ABI calls: bit-equal to each other, the dlogits padding untouched,
    ignored rows exactly 0, and loss / lse / S / dlogits within the bar of the fp64 reference."""
    B, C = x.shape
    if red == "none" and not torch.is_tensor(g):
        g = torch.randn(B, generator=torch.Generator().manual_seed(B + C))
    out, lse, S, dl, _ = _abi(x, t, w, eps, U, red, ignore, g)
    out_s, lse_s, S_s, dl_s, buf = _abi(x, t, w, eps, U, red, ignore, g, strided=True)
    assert torch.equal(out_s, out) and torch.equal(lse_s, lse) and torch.equal(S_s, S) and torch.equal(dl_s, dl), \
        f"{what}: strided != contiguous"
    assert torch.isnan(buf[:, :1]).all() and torch.isnan(buf[:, 1 + C:]).all(), f"{what}: dlogits padding written"
    assert not (dl[t == ignore] != 0).any(), f"{what}: ignored rows' dlogits not exactly 0"
    if red == "none":
        assert not (out[t == ignore] != 0).any(), f"{what}: ignored rows' losses not exactly 0"
    r32, r64 = (_ref(x, t, w, eps, U, red, ignore, g, dt) for dt in (torch.float32, torch.float64))
    if U is None and bool(((t == ignore) | ((t >= 0) & (t < C))).all()):  # torch has this configuration
        tc = _torch_ce64(x, t, w, eps, red, ignore)
        assert torch.allclose(tc, r64[0], rtol=1e-12, atol=1e-12, equal_nan=True), f"{what}: reference != torch fp64"
    _bar("loss", out, r32[0], r64[0], 1e-6, what)
    _bar("lse", lse, r32[1], r64[1], 1e-6, what)
    _bar("rowsum", S, r32[2], r64[2], 1e-6, what)
    _bar("dlogits", dl, r32[3], r64[3], 1e-5, what)
    return out, lse, dl


def _inputs(B, C, vals, seed):
    scale, shift = {"x1": (1.0, 0.0), "x30": (30.0, 0.0), "+1e4": (1.0, 1e4), "+25": (1.0, 25.0)}[vals]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * scale + shift
    t = torch.randint(0, C, (B,), generator=g)
    if B >= 5:  # ignored rows at the front, scattered, and as the last row
        t[0] = -100
        t[3::7] = -100
        t[B - 1] = -100
    return x, t


@functools.lru_cache(maxsize=None)
def _weight(C):
    return torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5


@functools.lru_cache(maxsize=None)
def _tbl(C):
    """A random (C, C) table: rows sum to 1 (fp32), about a third of the entries exactly 0."""
    g = torch.Generator().manual_seed(7 * C + 1)
    u = torch.rand(C, C, generator=g, dtype=torch.float64)
    u = u * (torch.rand(C, C, generator=g) > 0.33)
    u[:, 0] += 1e-3  # no empty row
    return (u / u.sum(dim=1, keepdim=True)).float()


OPTS = {"w": (True, 0.0, False), "eps": (False, EPS, False), "w+eps": (True, EPS, False),
        "eps+U": (False, EPS, True), "w+eps+U": (True, EPS, True)}


def _opt(name, C):
    hw, eps, hu = OPTS[name]
    return (_weight(C) if hw else None), eps, (_tbl(C) if hu else None)


WIDTHS = (1, 63, 64, 65, 1024, 1025, 2500)
VALS = ("x1", "x30", "+1e4", "+25")
REDS = ("mean", "sum", "none")
# every option meets every width (B = 5), the reduction and the logit distribution rotating so
# that every option also meets every reduction and every distribution
CASES = [(C, 5, VALS[(wi + 2 * oi) % 4], o, REDS[(wi + oi) % 3])
         for wi, C in enumerate(WIDTHS) for oi, o in enumerate(OPTS)]
# everything on at once: every distribution with every reduction, either side of the register-resident width
CASES += [(C, 5, v, "w+eps+U", r) for C in (65, 1025) for v in VALS for r in REDS
          if (C, 5, v, "w+eps+U", r) not in CASES]
# one row, and a batch at which the capped forward grid loops
CASES += [(C, B, v, o, r) for C, B, v, o, r in (
    (1, 1, "x1", "w+eps", "mean"), (65, 1, "x30", "eps+U", "sum"), (2500, 1, "+1e4", "w+eps+U", "none"),
    (64, "4cu+3", "x1", "w", "sum"), (65, "4cu+3", "+25", "w+eps+U", "mean"), (1024, "4cu+3", "x30", "eps", "none"),
    (1025, "4cu+3", "+1e4", "eps+U", "mean"), (1025, "4cu+3", "x1", "w+eps", "sum"),
    (2500, "4cu+3", "x30", "w+eps+U", "mean"))]


@pytest.mark.parametrize("C,B,vals,opt,red", CASES)
def test_ce_options_abi_matches_fp64(C, B, vals, opt, red):
    """Widths at the lane-count edges (63, 64, 65), the last register-resident width and the
    streaming branch (1024, 1025), a ragged last streaming pass (2500) and C = 1; batches of 1, 5
    (not a multiple of the 4 waves per workgroup) and 4 x CU count + 3 (the capped forward grid
    loops); logits of scale 1, 30, shifted by 1e4 and by 25 (either side of the |lse| < 32 switch
    of forms).  Strided logits, dlogits and table == the contiguous call, bit for bit."""
    B = 4 * _cus() + 3 if B == "4cu+3" else B
    x, t = _inputs(B, C, vals, seed=1000 * C + B)
    w, eps, U = _opt(opt, C)
    _check(x, t, w, eps, U, red, g=-0.75, what=f"C={C} B={B} {vals} {opt} {red}")


def test_ce_options_reduce_to_known_cases():
    """w = 1, eps = 0, mean against the existing op (within the bar of the fp64 reference, both);
    U = identity with any eps against eps = 0 (a[c] is the same up to the rounding of (1 - eps) +
    eps); U = 1 / C as a table against U absent.  Each side within the bar of the fp64 reference."""
    from models import loss  # noqa: F401  (registers leakgnn::cross_entropy)
    for C in (65, 1025):
        x, t = _inputs(9, C, "x1", seed=C)
        what = f"C={C} known cases"
        ones = torch.ones(C)
        out, lse, _, dl, _ = _abi(x, t, ones, 0.0, None, "mean", g=1.0)
        xd = x.to(DEV).requires_grad_(True)
        l0, lse0 = torch.ops.leakgnn.cross_entropy(xd, t.to(DEV), -100)
        l0.backward()
        r32, r64 = (_ref(x, t, None, 0.0, None, "mean", -100, 1.0, dt) for dt in (torch.float32, torch.float64))
        for name, got, k, rt in (("loss", out, 0, 1e-6), ("loss (existing op)", l0, 0, 1e-6), ("lse", lse, 1, 1e-6),
                                 ("dlogits", dl, 3, 1e-5), ("dlogits (existing op)", xd.grad, 3, 1e-5)):
            _bar(name, got, r32[k], r64[k], rt, what)
        _bar("lse (existing op)", lse0, r32[1], r64[1], 1e-6, what)
        # U = identity
        w = _weight(C)
        a = _abi(x, t, w, 0.0, None, "sum", g=2.0)
        b = _abi(x, t, w, 0.37, torch.eye(C), "sum", g=2.0)
        r32, r64 = (_ref(x, t, w, 0.0, None, "sum", -100, 2.0, dt) for dt in (torch.float32, torch.float64))
        _bar("loss, U = identity", b[0], r32[0], r64[0], 1e-6, what)
        _bar("dlogits, U = identity", b[3], r32[3], r64[3], 1e-5, what)
        _bar("loss, eps = 0", a[0], r32[0], r64[0], 1e-6, what)
        # U = 1 / C as a table
        a = _abi(x, t, w, EPS, None, "mean", g=1.0)
        b = _abi(x, t, w, EPS, torch.full((C, C), 1.0 / C), "mean", g=1.0)
        r32, r64 = (_ref(x, t, w, EPS, None, "mean", -100, 1.0, dt) for dt in (torch.float32, torch.float64))
        for k, name, rt in ((0, "loss", 1e-6), (3, "dlogits", 1e-5)):
            _bar(name + ", U absent", a[k], r32[k], r64[k], rt, what)
            _bar(name + ", U = 1/C table", b[k], r32[k], r64[k], rt, what)


@pytest.mark.parametrize("C", [65, 1025])
def test_ce_options_special_rows_and_targets(C):
    """-inf in non-target columns with eps = 0, and with a table whose row is 0 there (finite
    results, gradient exactly 0 there); uniform smoothing over a -inf logit: +inf, as torch; a custom
    ignore_index; every row ignored (mean NaN as torch, sum 0, dlogits exactly 0); targets C and -1
    with a table that ends its buffer (NaN before it): NaN loss, finite dlogits, the in-range rows as
    the formula."""
    g = torch.Generator().manual_seed(C)
    B = 6
    x = torch.randn(B, C, generator=g) * 3
    t = torch.randint(0, C, (B,), generator=g)
    t[1], t[2] = 5, 7
    x[1, 10:40] = -INF
    x[1, C - 1] = -INF
    x[2, 7] = x[2].max() - 60.0
    t[4] = -100
    w = _weight(C)
    U = _tbl(C).clone()
    U[5, 10:40] = 0.0
    U[5, C - 1] = 0.0
    U[5] /= U[5].double().sum().float()
    for eps, tab, red in ((0.0, None, "mean"), (EPS, U, "mean"), (EPS, U, "none"), (EPS, U, "sum")):
        out, lse, dl = _check(x, t, w, eps, tab, red, g=-0.25, what=f"C={C} -inf columns eps={eps:.2f} {red}")
        assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dl).all()
        assert not (dl[1, 10:40] != 0).any() and dl[1, C - 1] == 0, "-inf columns: gradient not exactly 0"
    out = _abi(x, t, w, EPS, None, "mean")[0]
    assert out == INF and _torch_ce64(x, t, w, EPS, "mean", -100) == INF
    # a custom ignore_index: rows whose target is 2 do not count
    t2 = torch.randint(0, C, (B,), generator=g)
    t2[0], t2[1], t2[3] = 2, 5, 2
    for red in REDS:
        _check(x, t2, w, EPS, U, red, ignore=2, g=1.5, what=f"C={C} ignore_index=2 {red}")
    # every row ignored
    ta = torch.full((B,), -100, dtype=torch.int64)
    for red, want in (("mean", NAN), ("sum", 0.0)):
        out, _, _, dl, _ = _abi(x, ta, w, EPS, U, red)
        assert torch.isnan(out) if want != want else out == 0.0, red
        assert not (dl != 0).any()
    assert torch.isnan(F.cross_entropy(x, ta, weight=w, label_smoothing=EPS))
    out, _, _, dl, _ = _abi(x, ta, w, EPS, U, "none")
    assert not (out != 0).any() and not (dl != 0).any()
    # targets C and -1 (ignore_index stays -100); the table is the END of its allocation and NaN
    # stands before it, so a read at row -1 would show and a read at row C would leave the buffer
    tb = t.clone()
    tb[0], tb[3] = C, -1
    buf = torch.full(((C + 2) * C,), NAN, device=DEV)
    buf[2 * C:] = U.to(DEV).reshape(-1)
    tab = (buf[2 * C:], C)
    ok = (tb >= 0) & (tb < C)
    for red in REDS:
        gg = torch.randn(B, generator=g) if red == "none" else 0.5
        out, lse, S, dl, _ = _abi(x, tb, w, EPS, None, red, g=gg, U_dev=tab)
        r32, r64 = (_ref(x, tb, w, EPS, U, red, -100, gg, dt) for dt in (torch.float32, torch.float64))
        what = f"C={C} out-of-range targets {red}"
        assert torch.isfinite(dl).all() and torch.isfinite(lse).all(), what
        _bar("lse", lse, r32[1], r64[1], 1e-6, what)
        _bar("dlogits", dl, r32[3], r64[3], 1e-5, what)
        if red == "none":
            assert torch.isnan(out[~ok & (tb != -100)]).all(), what
            keep = ok | (tb == -100)
            _bar("rows in range", out[keep], r32[0][keep], r64[0][keep], 1e-6, what)
        else:
            assert torch.isnan(out), what


def test_ce_options_empty_batch():
    """B == 0: mean NaN, sum 0, none an empty tensor; through the ABI (null row pointers) and the module."""
    from models.loss import CrossEntropyLoss
    nat, lib = _lib()
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    gl = torch.ones(1, device=DEV)
    st = nat.stream_of(gl)
    for red, want in (("mean", NAN), ("sum", 0.0), ("none", 7.0)):
        loss, denom = torch.full((1,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
        assert lib.lg_cross_entropy_opt_fwd(None, None, 0, 5, 5, -100, None, None, 0, 0.1, RED[red], loss.data_ptr(),
                                            None, None, None, denom.data_ptr(), counter.data_ptr(), st) == LG_OK
        assert lib.lg_cross_entropy_opt_bwd(None, None, None, None, denom.data_ptr(), gl.data_ptr(), 0, 5, 5, -100,
                                            None, None, 0, 0.1, RED[red], None, 5, st) == LG_OK
        torch.cuda.synchronize()
        assert torch.isnan(loss).all() if want != want else float(loss) == want, red
        assert int(counter.item()) == 0
        x = torch.zeros(0, 5, device=DEV, requires_grad=True)
        out = CrossEntropyLoss(reduction=red, label_smoothing=0.1)(x, torch.zeros(0, dtype=torch.int64, device=DEV))
        assert out.shape == ((0,) if red == "none" else ())
        if red != "none":
            assert torch.isnan(out) if want != want else float(out.detach()) == 0.0
        out.sum().backward()
        assert x.grad.shape == (0, 5)


# ------------------------------------------------------------------ module, autograd, dispatch

def test_ce_options_module_and_autograd():
    """(loss * 3.5).backward() for mean and sum and a random (B,) upstream gradient for none,
    against fp64; non-contiguous logits give the contiguous call's bits; two runs are
    bit-identical; .to(device) moves the table (a non-persistent buffer)."""
    from models.loss import CrossEntropyLoss
    B, C = 37, 1025
    x, t = _inputs(B, C, "x1", seed=11)
    x = x * 3
    w, U = _weight(C), _tbl(C)
    gv = torch.randn(B, generator=torch.Generator().manual_seed(5))
    for red in REDS:
        mod = CrossEntropyLoss(weight=w, reduction=red, label_smoothing=EPS, smoothing=U)
        assert mod.smoothing.device.type == "cpu" and "smoothing" not in mod.state_dict()
        mod = mod.to(DEV)
        assert mod.smoothing.is_cuda and mod.weight.is_cuda
        up = gv if red == "none" else 3.5
        runs = []
        for xin in (x.to(DEV), x.to(DEV), x.t().contiguous().to(DEV).t()):  # the last: a (B, C) view of (C, B)
            xin = xin.requires_grad_(True)
            out = mod(xin, t.to(DEV))
            (out * (up.to(DEV) if torch.is_tensor(up) else up)).sum().backward()
            runs.append((out.detach(), xin.grad))
        for o, d in runs[1:]:
            assert torch.equal(o, runs[0][0]) and torch.equal(d, runs[0][1]), f"{red}: runs differ"
        r32, r64 = (_ref(x, t, w, EPS, U, red, -100, up, dt) for dt in (torch.float32, torch.float64))
        _bar("loss", runs[0][0], r32[0], r64[0], 1e-6, f"module {red}")
        _bar("dlogits", runs[0][1], r32[3], r64[3], 1e-5, f"module {red}")
        assert not (runs[0][1][t.to(DEV) == -100] != 0).any()


def test_ce_options_dispatch(monkeypatch):
    """With torch's own forward out of the way, the weighted, smoothed and sum / none modules
    still return on fp32 GPU input (they run the HIP op), the bf16 one raises (it still falls
    through).  Fails before leakgnn::cross_entropy_opt existed."""
    from models import loss as L
    assert hasattr(torch.ops.leakgnn, "cross_entropy_opt") and hasattr(torch.ops.leakgnn, "cross_entropy_opt_backward")

    def boom(self, input, target):
        raise AssertionError("torch's route taken")

    monkeypatch.setattr(torch.nn.CrossEntropyLoss, "forward", boom)
    C = 65
    x, t = _inputs(5, C, "x1", seed=3)
    xd, td = x.to(DEV), t.to(DEV)
    for kw in ({"weight": _weight(C)}, {"label_smoothing": 0.1}, {"reduction": "sum"}, {"reduction": "none"},
               {"label_smoothing": 0.1, "smoothing": _tbl(C)}, {}):
        out = L.CrossEntropyLoss(**kw).to(DEV)(xd, td)
        assert torch.isfinite(out).all(), kw
    with pytest.raises(AssertionError, match="torch's route taken"):
        L.CrossEntropyLoss(weight=_weight(C)).to(DEV)(xd.bfloat16(), td)
    with pytest.raises(NotImplementedError):
        L.CrossEntropyLoss(label_smoothing=0.1, smoothing=_tbl(C)).to(DEV)(xd.bfloat16(), td)


def test_ce_options_capture():
    """After one eager call, the loss forward and backward alone in torch.cuda.graph at (5, 65) with
    weights, eps and a table, mean reduction; two replays on new logits and labels copied into the
    static tensors give the eager call's bits."""
    from models.loss import CrossEntropyLoss
    B, C = 5, 65
    mod = CrossEntropyLoss(weight=_weight(C), label_smoothing=EPS, smoothing=_tbl(C)).to(DEV)

    def eager(x, t):
        xin = x.to(DEV).requires_grad_(True)
        out = mod(xin, t.to(DEV))
        out.backward()
        return out.detach().clone(), xin.grad.clone()

    x0, t0 = _inputs(B, C, "x1", seed=1)
    eager(x0, t0)
    sx = x0.to(DEV).requires_grad_(True)
    st_ = t0.to(DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one warm-up on the capture stream: its counter slot is taken eagerly
        (gx,) = torch.autograd.grad(mod(sx, st_), sx)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph, stream=side):
        sl = mod(sx, st_)
        (gx,) = torch.autograd.grad(sl, sx)
    for seed, vals in ((2, "x30"), (3, "+25")):
        x, t = _inputs(B, C, vals, seed=seed)
        want = eager(x, t)
        with torch.no_grad():
            sx.copy_(x.to(DEV))
        st_.copy_(t.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sl.detach(), want[0]) and torch.equal(gx, want[1]), f"replay {seed} != eager"


# ------------------------------------------------------------------ end to end

def test_ce_options_detector_step_end_to_end():
    """A LeakDetector on L-TOWN-A at B = 4 with the loss of --label_smoothing 0.1 --smooth_sigma_m 200
    --noleak_weight 0.5 (loss_from_args: the table from the real pipe distances): one eager ClipAdamW
    step; the loss is finite, every gradient is finite, and the loss is the fp64 expression on the
    detector's own logits within the bar."""
    from models.detector import LeakDetector
    from models.loss import loss_from_args
    from models.optim import ClipAdamW
    sensors, pipes = lta_ids()
    C = len(pipes) + 1
    loss_fn = loss_from_args({"label_smoothing": 0.1, "smooth_sigma_m": 200.0, "noleak_weight": 0.5}, LTA_INP, pipes)
    U, w = loss_fn.smoothing.clone(), loss_fn.weight.clone()
    assert tuple(U.shape) == (C, C) and float(w[C - 1]) == 0.5 and float(w[:C - 1].min()) == 1.0
    loss_fn = loss_fn.to(DEV)
    torch.manual_seed(0)
    m = LeakDetector(LTA_INP, sensors, pipes, dropout=0.1).to(DEV).train()
    opt = ClipAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, max_norm=1.0)
    gen = torch.Generator().manual_seed(4)
    r, tf = torch.randn(4, 36, 29, generator=gen).to(DEV), torch.randn(4, 36, 9, generator=gen).to(DEV)
    lab = torch.tensor([3, C - 1, 700, C - 1])
    logits = m(r, tf)
    loss = loss_fn(logits, lab.to(DEV))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    opt.step()
    eps = torch.tensor(0.1, dtype=torch.float32).item()
    lg = logits.detach().cpu()
    r32, r64 = (_ref(lg, lab, w, eps, U, "mean", -100, 1.0, dt) for dt in (torch.float32, torch.float64))
    _bar("loss", loss, r32[0], r64[0], 1e-6, "detector step")
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
