"""The three launches that end every training step, each against a plain high-precision
reference and through the C ABI of include/leakgnn.h as well as the Python wrappers:

  A. lg_cross_entropy_fwd / _bwd (csrc/loss.hip, models/loss.py) against torch's CPU
     cross_entropy in float64, with the CPU float32 run as the fp32 yardstick;
  B. lg_clip_adamw / lg_clip_adamw_seeds (csrc/optim.hip, models/optim.py) in every mode
     against an fp64 clip + AdamW written here, with torch's clip_grad_norm_ + fused AdamW on
     the GPU as the fp32 yardstick;
  C. the dropout seed draws of lg_seed_slots_advance (csrc/reduce.hip) and
     lg_clip_adamw_seeds against a Python-int splitmix64, bit for bit.

Tolerances.  Besides bit equality and the project's bars (1e-5 / 1e-6 of the tensor's scale,
helpers.assert_close), one rule is used, that of helpers.assert_grads_match_truth: the
kernel's max-abs error against the fp64 reference is at most the larger of 4 x the fp32
yardstick's own error against fp64 and RT x the reference's max (RT = 1e-5 for dlogits, 1e-6
for loss, lse and every AdamW output).
Worst observed error / limit per output on an MI355X (1.0 would be the bar):
  cross entropy   loss 0.12   lse 0.12   dlogits 0.03
  AdamW           update 0.32   clipped grad 0.07   exp_avg 0.08   exp_avg_sq 0.15   norm 0.06
Before rows with a large logsumexp took the row loss as (max - x[target]) + log(sum), the loss
of the logits shifted by 1e4 stood at 50.6 (C = 63, B = 5: error 2.4e-4, limit 4.7e-6) and
their dlogits at 3.3 (error 1.6e-5, limit 5.0e-6).
"""
from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LG_OK, LG_EINVAL, LG_EUNSUPPORTED = 0, -1, -2
NAN, INF = float("nan"), float("inf")


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


# ------------------------------------------------------------------ A. cross entropy

def _ce_abi(x, t, ignore=-100, grad_loss=1.0, strided=False):
    """lg_cross_entropy_fwd then _bwd on CPU tensors x (B, C) fp32, t (B,) int64.  strided: the
    logits are columns 3 .. 3 + C of a NaN-filled (B, C + 7) buffer and dlogits columns 1 .. 1 + C
    of a NaN-filled (B, C + 3) one.  Returns loss, lse, dlogits (CPU), the dlogits buffer."""
    nat, lib = _lib()
    B, C = x.shape
    ldx, ox, ldd, od = (C + 7, 3, C + 3, 1) if strided else (C, 0, C, 0)
    xb = torch.full((B, ldx), NAN, device=DEV)
    xb[:, ox:ox + C] = x.to(DEV)
    db = torch.full((B, ldd), NAN, device=DEV)
    td = t.to(DEV)
    loss = torch.full((1,), 7.0, device=DEV)
    lse = torch.full((B,), NAN, device=DEV)
    rowloss = torch.full((B,), NAN, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    gl = torch.tensor([grad_loss], dtype=torch.float32, device=DEV)
    st = nat.stream_of(xb)
    assert lib.lg_cross_entropy_fwd(xb.data_ptr() + 4 * ox, td.data_ptr(), B, C, ldx, ignore, loss.data_ptr(),
                                    lse.data_ptr(), rowloss.data_ptr(), counter.data_ptr(), st) == LG_OK
    assert lib.lg_cross_entropy_bwd(xb.data_ptr() + 4 * ox, td.data_ptr(), lse.data_ptr(), gl.data_ptr(), B, C, ldx,
                                    ignore, db.data_ptr() + 4 * od, ldd, st) == LG_OK
    torch.cuda.synchronize()
    assert int(counter.item()) == 0, "completion counter not back at 0"
    return loss[0].cpu(), lse.cpu(), db[:, od:od + C].cpu().contiguous(), db.cpu()


def _ce_ref(x, t, ignore, grad_loss, dtype):
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(xx, t, ignore_index=ignore)
    (loss * grad_loss).backward()
    return loss.detach(), torch.logsumexp(xx.detach(), dim=1), xx.grad


def _ce_check(x, t, ignore=-100, grad_loss=1.0, what=""):
    """Contiguous and strided ABI calls: bit-equal to each other, the dlogits padding untouched,
    ignored rows exactly 0, and loss / lse / dlogits within the bar of the fp64 reference."""
    B, C = x.shape
    loss, lse, dl, _ = _ce_abi(x, t, ignore, grad_loss)
    loss_s, lse_s, dl_s, buf = _ce_abi(x, t, ignore, grad_loss, strided=True)
    assert torch.equal(loss_s, loss) and torch.equal(lse_s, lse) and torch.equal(dl_s, dl), f"{what}: strided != contiguous"
    assert torch.isnan(buf[:, :1]).all() and torch.isnan(buf[:, 1 + C:]).all(), f"{what}: dlogits padding written"
    assert not (dl[t == ignore] != 0).any(), f"{what}: ignored rows' dlogits not exactly 0"
    r32, r64 = _ce_ref(x, t, ignore, grad_loss, torch.float32), _ce_ref(x, t, ignore, grad_loss, torch.float64)
    _bar("loss", loss, r32[0], r64[0], 1e-6, what)
    _bar("lse", lse, r32[1], r64[1], 1e-6, what)
    _bar("dlogits", dl, r32[2], r64[2], 1e-5, what)
    return loss, lse, dl


def _ce_inputs(B, C, scale, shift, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * scale + shift
    t = torch.randint(0, C, (B,), generator=g)
    if B >= 5:  # ignored rows at the front, scattered, and as the last row
        t[0] = -100
        t[3::7] = -100
        t[B - 1] = -100
    return x, t


CE_WIDTHS = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
CE_CASES = ([(C, 5, v) for C in CE_WIDTHS for v in ("x1", "x30", "+1e4")]
            + [(C, 5, "+25") for C in (65, 1025)]  # lse just under / over 32, where loss.hip changes forms
            + [(1025, B, v) for B in (1, "4cu+3") for v in ("x1", "x30", "+1e4")]
            + [(1, 1, "x1"), (64, "4cu+3", "x1"), (1024, "4cu+3", "x30"), (2500, 1, "+1e4")])


@pytest.mark.parametrize("C,B,vals", CE_CASES)
def test_cross_entropy_abi_matches_fp64(C, B, vals):
    """Widths at the lane-count edges (63, 64, 65), around the last register-resident width
    (1023, 1024, 1025: the streaming branch) and 2500 (a ragged last streaming pass); batches
    of 1, 5 (not a multiple of the 4 waves per workgroup) and 4 x CU count + 3 (the capped
    forward grid loops); logits of scale 1, 30 and shifted by 1e4 (the row maximum has to come
    off before exp, and neither the row loss nor the softmax may inherit the rounding of a
    logsumexp near 1e4: rows with |lse| >= 32 take the max-based forms, + 25 puts lse on
    either side of that).  Strided call == contiguous call, bit for bit."""
    B = 4 * _cus() + 3 if B == "4cu+3" else B
    scale, shift = {"x1": (1.0, 0.0), "x30": (30.0, 0.0), "+1e4": (1.0, 1e4), "+25": (1.0, 25.0)}[vals]
    x, t = _ce_inputs(B, C, scale, shift, seed=1000 * C + B)
    _ce_check(x, t, what=f"C={C} B={B} {vals}")


@pytest.mark.parametrize("C", [65, 1025])
def test_cross_entropy_special_rows_and_targets(C):
    """-inf in non-target columns (finite results, gradient exactly 0 there), a target logit
    far below the row maximum, a custom ignore_index, grad_loss = -0.25 through the ABI, every
    row ignored (NaN loss as torch, dlogits exactly 0), and targets outside [0, C): NaN loss, no
    out-of-range read, finite backward rows, the in-range rows as the formula of the header."""
    g = torch.Generator().manual_seed(C)
    B = 6
    x = torch.randn(B, C, generator=g) * 3
    t = torch.randint(0, C, (B,), generator=g)
    t[1], t[2] = 5, 7
    x[1, 10:40] = -INF
    x[1, C - 1] = -INF
    x[2, 7] = x[2].max() - 60.0
    t[4] = -100
    loss, lse, dl = _ce_check(x, t, grad_loss=-0.25, what=f"C={C} special rows")
    assert torch.isfinite(loss) and torch.isfinite(lse).all() and torch.isfinite(dl).all()
    assert not (dl[1, 10:40] != 0).any() and dl[1, C - 1] == 0, "-inf columns: gradient not exactly 0"
    # a custom ignore_index: rows whose target is 2 do not count
    t2 = torch.randint(0, C, (B,), generator=g)
    t2[0], t2[1], t2[3] = 2, 5, 2  # row 1: a target outside its -inf columns
    _ce_check(x, t2, ignore=2, what=f"C={C} ignore_index=2")
    # every row ignored
    ta = torch.full((B,), -100, dtype=torch.int64)
    loss, _, dl, _ = _ce_abi(x, ta)
    assert torch.isnan(torch.nn.functional.cross_entropy(x, ta)) and torch.isnan(loss)
    assert not (dl != 0).any()
    # targets C and -1 (ignore_index stays -100)
    tb = t.clone()
    tb[0], tb[3] = C, -1
    for strided in (False, True):
        loss, lse, dl, _ = _ce_abi(x, tb, strided=strided)
        assert torch.isnan(loss)
        assert torch.isfinite(dl).all()
        assert_close(lse, torch.logsumexp(x.double(), 1), rtol=1e-6, what="lse with out-of-range targets")
        ok = (tb >= 0) & (tb < C)
        n = int((tb != -100).sum())
        want = torch.softmax(x.double(), 1)
        want[ok, tb[ok]] -= 1.0
        want[tb == -100] = 0.0
        assert_close(dl[ok | (tb == -100)], (want / n)[ok | (tb == -100)], rtol=1e-5, what="dlogits of the in-range rows")


def test_cross_entropy_abi_empty_batch():
    """B == 0: the forward returns LG_OK and writes NaN to loss, the backward returns LG_OK."""
    nat, lib = _lib()
    loss = torch.full((1,), 7.0, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    gl = torch.ones(1, device=DEV)
    st = nat.stream_of(loss)
    assert lib.lg_cross_entropy_fwd(None, None, 0, 5, 5, -100, loss.data_ptr(), None, None, counter.data_ptr(), st) == LG_OK
    assert lib.lg_cross_entropy_bwd(None, None, None, gl.data_ptr(), 0, 5, 5, -100, None, 5, st) == LG_OK
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and int(counter.item()) == 0


def test_cross_entropy_wrapper_upstream_gradient_and_fall_through():
    """models/loss.py: (loss * 3.5).backward() through the op against fp64; non-contiguous
    (B, C) logits (a transposed view) give the contiguous call's bits; bf16 logits, weight=
    and reduction="sum" equal torch's own module."""
    from models.loss import CrossEntropyLoss
    B, C = 37, 1025
    x, t = _ce_inputs(B, C, 3.0, 0.0, seed=9)
    xa = x.to(DEV).requires_grad_(True)
    la = CrossEntropyLoss()(xa, t.to(DEV))
    (la * 3.5).backward()
    r32, r64 = _ce_ref(x, t, -100, 3.5, torch.float32), _ce_ref(x, t, -100, 3.5, torch.float64)
    _bar("loss", la, r32[0], r64[0], 1e-6, "wrapper")
    _bar("dlogits", xa.grad, r32[2], r64[2], 1e-5, "wrapper, upstream 3.5")
    assert not (xa.grad[t.to(DEV) == -100] != 0).any()
    xt = x.t().contiguous().to(DEV).t().requires_grad_(True)  # (B, C) view of a (C, B) buffer
    assert not xt.is_contiguous()
    lt = CrossEntropyLoss()(xt, t.to(DEV))
    (lt * 3.5).backward()
    assert torch.equal(lt, la) and torch.equal(xt.grad, xa.grad)
    w = torch.rand(C, device=DEV) + 0.5
    xd, td = x.to(DEV), t.to(DEV)
    for kw, inp in (({}, xd.bfloat16()), ({"weight": w}, xd), ({"reduction": "sum"}, xd)):
        assert_close(CrossEntropyLoss(**kw)(inp, td).float(), torch.nn.CrossEntropyLoss(**kw)(inp, td).float(),
                     rtol=1e-6, what=f"fall-through {kw or 'bf16'}")


# ------------------------------------------------------------------ B. clip + AdamW

HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
KEYS = ("update", "g", "m", "v")
NAMES = {"update": "update", "g": "clipped grad", "m": "exp_avg", "v": "exp_avg_sq"}


def _f32(x: float) -> float:
    return torch.tensor(x, dtype=torch.float32).item()


def _cat(L):
    return torch.cat([x.detach().reshape(-1).double().cpu() for x in L]) if L else torch.zeros(0, dtype=torch.float64)


def _adam_state(sizes, seed, gscale=1.0, moments=False):
    """Flat fp32 CPU tensors: parameters ~0.1 (so one update, ~lr, is well above a parameter's
    rounding), gradients, and the moments (zeros, or random m and random v >= 0)."""
    g = torch.Generator().manual_seed(seed)
    P = [torch.randn(n, generator=g) * 0.1 for n in sizes]
    G = [torch.randn(n, generator=g) * gscale for n in sizes]
    M = [torch.randn(n, generator=g) * 0.1 * gscale if moments else torch.zeros(n) for n in sizes]
    V = [torch.rand(n, generator=g) * 0.01 * gscale ** 2 if moments else torch.zeros(n) for n in sizes]
    return P, G, M, V


def _ref_adamw(P, G, M, V, t0, hp, max_norm):
    """fp64 clip + AdamW, the formulas of csrc/optim.hip's header; the hyper-parameters as the
    fp32 values the ABI receives.  Returns update, clipped g, m, v (flat fp64) and the norm."""
    lr, b1, b2, eps, wd, mx = [_f32(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd")] + [_f32(max_norm)]
    p, g, m, v = _cat(P), _cat(G), _cat(M), _cat(V)
    norm = math.sqrt(float((g * g).sum()))
    if mx > 0:
        g = g * min(1.0, mx / (norm + 1e-6))
    t = t0 + 1
    p1 = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p1 = p1 - lr / (1.0 - b1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return {"update": p1 - p, "g": g, "m": m, "v": v, "p": p1, "norm": torch.tensor(norm, dtype=torch.float64)}


class _Abi:
    """One lg_clip_adamw table over device copies of P, G, M, V (a zero-length tensor gets a
    valid dummy pointer), its step words and workspace."""

    def __init__(self, P, G, M, V, t0=0):
        self.nat, self.lib = _lib()
        self.P0 = [x.clone() for x in P]
        self.p, self.g, self.m, self.v = ([x.clone().to(DEV) for x in L] for L in (P, G, M, V))
        self.dummy = torch.zeros(4, device=DEV)
        T = self.T = len(P)
        ptr = lambda x: x.data_ptr() if x.numel() else self.dummy.data_ptr()  # noqa: E731
        self.table = (ctypes.c_int64 * (4 * T))(*[ptr(x) for q in zip(self.p, self.g, self.m, self.v) for x in q])
        self.sizes = (ctypes.c_int64 * T)(*[x.numel() for x in P])
        self.step_t = torch.zeros(4, device=DEV)
        self.step_t[0] = float(t0)
        nws = int(self.lib.lg_clip_adamw_workspace_bytes(ctypes.addressof(self.sizes) if T else None, T))
        self.nws = nws if nws > 0 else 8  # an error code (T > 48): the call under test rejects T itself
        self.ws = torch.zeros(self.nws, dtype=torch.uint8, device=DEV)
        self.norm = torch.full((1,), -7.0, device=DEV)

    def set_grads(self, G):
        for d, s in zip(self.g, G):
            d.copy_(s)

    def step(self, hp, max_norm, norm=True, seeds=None):
        T = self.T
        args = (ctypes.addressof(self.table) if T else None, ctypes.addressof(self.sizes) if T else None, T,
                self.step_t.data_ptr(), hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], max_norm,
                self.norm.data_ptr() if norm else None, self.ws.data_ptr(), self.nws)
        st = self.nat.stream_of(self.step_t)
        if seeds is None:
            rc = self.lib.lg_clip_adamw(*args, st)
        else:
            rc = self.lib.lg_clip_adamw_seeds(*args, seeds[0].data_ptr(), seeds[0].numel(), seeds[1].data_ptr(), st)
        torch.cuda.synchronize()
        return rc

    def words(self):
        """(step count, ticket word, error word)"""
        return (self.step_t[0].item(), *self.step_t[1:3].view(torch.int32).tolist())

    def out(self, P_before=None):
        P_before = self.P0 if P_before is None else P_before
        return {"update": _cat(self.p) - _cat(P_before), "g": _cat(self.g), "m": _cat(self.m), "v": _cat(self.v),
                "p": _cat(self.p), "norm": self.norm[0].double().cpu()}


def _torch_step(P, G, M, V, t0, hp, max_norm):
    """The fp32 yardstick: clip_grad_norm_ + torch.optim.AdamW(fused=True) on the GPU from the
    same state (zero-length tensors left out: they have no elements to compare)."""
    keep = [k for k, x in enumerate(P) if x.numel()]
    P, G, M, V = ([L[k] for k in keep] for L in (P, G, M, V))
    ps = [torch.nn.Parameter(x.clone().to(DEV)) for x in P]
    for p, g in zip(ps, G):
        p.grad = g.clone().to(DEV)
    opt = torch.optim.AdamW(ps, lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"], fused=True)
    for p, m, v in zip(ps, M, V):
        opt.state[p] = {"step": torch.tensor(float(t0), device=DEV), "exp_avg": m.clone().to(DEV),
                        "exp_avg_sq": v.clone().to(DEV)}
    if max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    else:
        norm = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in ps]))
    opt.step()
    torch.cuda.synchronize()
    return {"update": _cat(ps) - _cat(P), "g": _cat([p.grad for p in ps]), "p": _cat(ps),
            "m": _cat([opt.state[p]["exp_avg"] for p in ps]), "v": _cat([opt.state[p]["exp_avg_sq"] for p in ps]),
            "norm": norm.double().cpu()}


def _adam_bars(got, yard, ref, what, norm=True):
    for k in KEYS:
        _bar(NAMES[k], got[k], yard[k], ref[k], 1e-6, what)
    if norm:
        _bar("norm", got["norm"], yard["norm"], ref["norm"], 1e-6, what)


def _one_step(P, G, M, V, t0, hp, max_norm, what):
    """One lg_clip_adamw step from the given state against fp64 and the yardstick."""
    a = _Abi(P, G, M, V, t0)
    assert a.step(hp, max_norm) == LG_OK
    assert a.words() == (t0 + 1, 0, 0), f"{what}: step / ticket / error words {a.words()}"
    got, ref = a.out(), _ref_adamw(P, G, M, V, t0, hp, max_norm)
    _adam_bars(got, _torch_step(P, G, M, V, t0, hp, max_norm), ref, what)
    return a, got, ref


def _one_step_vs_fp64(sizes, t0, hp, max_norm, seed, what, moments=False):
    P, G, M, V = _adam_state(sizes, seed, moments=moments)
    return _one_step(P, G, M, V, t0, hp, max_norm, what) + (P,)


LAYOUT = [1, 1023, 0, 1025, 2048, 7]  # tensor boundaries before, on and after the 1024-element slice boundaries


@pytest.mark.parametrize("sizes", [LAYOUT, [(1, 3, 1024, 17)[k % 4] for k in range(48)]], ids=["mixed6", "T48"])
def test_clip_adamw_abi_layout_against_fp64(sizes):
    """Two steps (bias corrections at t = 1 and t = 2) with the clip active, over a table with a
    zero-length tensor and boundaries on both sides of the slice boundaries, and over the
    maximum of 48 tensors: update, clipped gradients, moments and norm against fp64."""
    P, G, M, V = _adam_state(sizes, seed=len(sizes))
    a = _Abi(P, G, M, V)
    for t0, Gt in enumerate((G, _adam_state(sizes, seed=77)[1])):
        before = [x.cpu() for x in a.p]
        a.set_grads(Gt)
        Mt, Vt = [x.cpu() for x in a.m], [x.cpu() for x in a.v]
        assert a.step(HP, 1.0) == LG_OK
        assert a.words() == (t0 + 1, 0, 0)
        ref = _ref_adamw(before, Gt, Mt, Vt, t0, HP, 1.0)
        assert ref["norm"] > 10.0  # the clip is active
        _adam_bars(a.out(before), _torch_step(before, Gt, Mt, Vt, t0, HP, 1.0), ref, f"T={len(sizes)} step {t0 + 1}")


def test_clip_adamw_abi_tensor_count_limits():
    """T == 0 is legal: LG_OK, the step word advances by 1, the ticket and error words stay 0.
    T == 49 is LG_EUNSUPPORTED."""
    a = _Abi([], [], [], [], t0=3)
    for norm in (True, False):
        t = a.words()[0]
        assert a.step(HP, 1.0 if norm else 0.0, norm=norm) == LG_OK
        assert a.words() == (t + 1, 0, 0)
    P, G, M, V = _adam_state([2] * 49, seed=1)
    b = _Abi(P, G, M, V)
    assert b.lib.lg_clip_adamw_workspace_bytes(ctypes.addressof(b.sizes), 49) == LG_EUNSUPPORTED
    b.nws, b.ws = 8, torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert b.step(HP, 1.0) == LG_EUNSUPPORTED
    assert torch.equal(_cat(b.p), _cat(P)) and b.words() == (0, 0, 0)


def test_clip_adamw_three_modes_against_fp64():
    """max_norm > 0 with norm_out, max_norm = 0 with norm_out (gradients bit-identical, the norm
    still written) and max_norm = 0 with norm_out NULL (k_adam<kAdamNoNorm>) from the same
    state, starting at step 5 over 4 full slices, each against fp64."""
    P, G, M, V = _adam_state(LAYOUT, seed=21, moments=True)
    for max_norm, norm in ((1.0, True), (0.0, True), (0.0, False)):
        a = _Abi(P, G, M, V, t0=5)
        assert a.step(HP, max_norm, norm=norm) == LG_OK
        assert a.words() == (6, 0, 0)
        got, ref = a.out(), _ref_adamw(P, G, M, V, 5, HP, max_norm)
        _adam_bars(got, _torch_step(P, G, M, V, 5, HP, max_norm), ref, f"max_norm={max_norm} norm_out={norm}", norm)
        if max_norm == 0.0:
            assert torch.equal(_cat(a.g), _cat(G)), "max_norm = 0 changed the gradients"
        if norm:
            assert_close(got["norm"], ref["norm"], rtol=1e-6, what="norm_out")
        else:
            assert a.norm.item() == -7.0


def test_clip_adamw_modes_bit_identical_below_threshold():
    """Gradients below the clip threshold (coefficient exactly 1): the three modes give
    bit-identical p, exp_avg and exp_avg_sq after 3 steps from step 5, as does
    lg_clip_adamw_seeds in the no-norm mode.  The no-norm launch has 4 full 1024-thread
    workgroups, every wave of which needs the step count thread 0 leaves in LDS; this mode had
    no barrier between that store and the other waves' read.  On the code the compiler emits
    today the race did not show on an MI355X even without the barrier (every wave reaches its
    LDS read behind a dependent load of its tensor's pointers, thread 0 behind one load), so
    this test pins the mode's results; the barrier itself rests on reading the kernel."""
    P, G, M, V = _adam_state(LAYOUT, seed=22, gscale=1e-3, moments=True)
    grads = [G] + [_adam_state(LAYOUT, seed=30 + k, gscale=1e-3)[1] for k in range(2)]
    slots, state = torch.zeros(16, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    runs = {}
    for name, max_norm, norm, seeds in (("clip", 1.0, True, None), ("norm only", 0.0, True, None),
                                        ("no norm", 0.0, False, None), ("no norm + seeds", 0.0, False, (slots, state))):
        a = _Abi(P, G, M, V, t0=5)
        for Gk in grads:
            a.set_grads(Gk)
            assert a.step(HP, max_norm, norm=norm, seeds=seeds) == LG_OK
        assert a.words() == (8, 0, 0), f"{name}: {a.words()}"
        runs[name] = a.out()
    ref, Pk, Mk, Vk = None, P, M, V
    for k, Gk in enumerate(grads):  # the fp64 trajectory, re-seeded from fp32 state each step as the kernel's is
        ref = _ref_adamw(Pk, Gk, Mk, Vk, 5 + k, HP, 0.0)
        if k < 2:
            Pk, Mk, Vk = [ref["p"].float()], [ref["m"].float()], [ref["v"].float()]
    for name, got in runs.items():
        for k in ("p", "m", "v"):
            bad = (got[k] != runs["clip"][k]).nonzero().reshape(-1)
            assert bad.numel() == 0, (f"{name}: {k} differs from the clip mode at {bad.numel()} of {got[k].numel()} "
                                      f"elements, first at flat index {bad[0].item()} (thread {bad[0].item() % 1024})")
        assert_close(got["m"], ref["m"], rtol=1e-6, what=f"{name}: exp_avg after 3 steps")
        assert_close(got["v"], ref["v"], rtol=1e-6, what=f"{name}: exp_avg_sq after 3 steps")
    assert state.item() == 3 and slots.tolist() == [_slot(3, 16, i) for i in range(16)]


def test_clip_adamw_residency_boundary():
    """1024 x CU count elements: one launch, every CU holding one workgroup of the grid barrier;
    one element more: the two-launch form.  Both against fp64; the slices' fp64 partial sums of
    the shared elements agree bit for bit; ticket and error words 0 after each."""
    N = 1024 * _cus()
    P, G, M, V = _adam_state([N - 5, 6], seed=23)
    ws = []
    for extra in (0, 1):
        Pc, Gc, Mc, Vc = ([L[0], L[1][:5 + extra]] for L in (P, G, M, V))
        a, got, ref = _one_step(Pc, Gc, Mc, Vc, 0, HP, 1.0, f"N = 1024 * CUs + {extra}")
        assert_close(got["norm"], ref["norm"], rtol=1e-6, what="norm")
        ws.append(a.ws.view(torch.float64).cpu())
    assert ws[0].numel() == _cus() and ws[1].numel() == _cus() + 1
    assert torch.equal(ws[0], ws[1][:_cus()])
    assert ws[1][_cus()].item() == float(G[1][5].double() ** 2)


@pytest.mark.parametrize("t0", [999, 99999])
def test_clip_adamw_step_counter_far_from_one(t0):
    """One step from step 999 and 99999 with seeded moments: beta1^t underflows to a bias
    correction of exactly 1, and the step word afterwards is t + 1 exactly."""
    _one_step_vs_fp64(LAYOUT, t0, HP, 1.0, seed=t0, what=f"t0={t0}", moments=True)


def test_clip_adamw_hyper_parameters():
    """lr = 0 (only the moments and clipped gradients change), weight_decay = 0, betas = (0, 0),
    eps = 0 with gradient entries of exactly 0 in a fresh state (0 / 0: NaN there, as torch's
    fused AdamW gives, documented in include/leakgnn.h), and the LG_EINVAL hyper-parameters."""
    _, got, _, P = _one_step_vs_fp64(LAYOUT, 2, dict(HP, lr=0.0), 1.0, seed=41, what="lr=0", moments=True)
    assert torch.equal(got["p"], _cat(P)), "lr = 0 moved the parameters"
    _one_step_vs_fp64(LAYOUT, 2, dict(HP, wd=0.0), 1.0, seed=42, what="wd=0", moments=True)
    _one_step_vs_fp64(LAYOUT, 0, dict(HP, b1=0.0, b2=0.0), 1.0, seed=43, what="betas=0")
    _one_step_vs_fp64(LAYOUT, 4, dict(HP, b1=0.0, b2=0.0), 0.0, seed=44, what="betas=0, t0=4", moments=True)
    hp = dict(HP, eps=0.0)
    P, G, M, V = _adam_state(LAYOUT, seed=45)
    zero = [G[1][::5], G[4][1000:1100]]
    for z in zero:
        z.zero_()
    a = _Abi(P, G, M, V)
    assert a.step(hp, 1.0) == LG_OK
    got, yard, ref = a.out(), _torch_step(P, G, M, V, 0, hp, 1.0), _ref_adamw(P, G, M, V, 0, hp, 1.0)
    is0 = _cat(G) == 0
    assert is0.sum() == 305
    assert torch.equal(torch.isnan(yard["p"]), is0), "torch's fused AdamW: eps = 0, zero gradient"
    assert torch.equal(torch.isnan(got["p"]), is0)
    _bar("update", got["update"][~is0], yard["update"][~is0], ref["update"][~is0], 1e-6, "eps=0")
    for k in ("g", "m", "v"):
        _bar(NAMES[k], got[k], yard[k], ref[k], 1e-6, "eps=0")
    P, G, M, V = _adam_state([8], seed=46)
    for bad in (dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(b1=NAN), dict(b2=NAN)):
        b = _Abi(P, G, M, V)
        assert b.step(dict(HP, **bad), 1.0) == LG_EINVAL, bad
        assert b.words() == (0, 0, 0) and torch.equal(_cat(b.p), _cat(P))


def _wrapper_params(sizes, seed):
    P = _adam_state(sizes, seed)[0]
    return P, [torch.nn.Parameter(x.clone().to(DEV)) for x in P]


def test_clip_adamw_wrapper_without_clipping():
    """ClipAdamW(max_norm=None) over 3 steps against plain torch.optim.AdamW and the fp64
    reference: .grad bit-unchanged, last_grad_norm the fp64 norm to 1e-6."""
    from models.optim import ClipAdamW
    sizes = [1023, 1025, 2048, 7]
    P, ps = _wrapper_params(sizes, seed=51)
    opt = ClipAdamW(ps, lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"], max_norm=None)
    for it in range(3):
        G = _adam_state(sizes, seed=60 + it)[1]
        before = [p.detach().cpu() for p in ps]
        M = [opt.state[p]["exp_avg"].cpu() if opt.state[p] else torch.zeros_like(b) for p, b in zip(ps, before)]
        V = [opt.state[p]["exp_avg_sq"].cpu() if opt.state[p] else torch.zeros_like(b) for p, b in zip(ps, before)]
        for p, g in zip(ps, G):
            p.grad = g.clone().to(DEV)
        opt.step()
        torch.cuda.synchronize()
        ref = _ref_adamw(before, G, M, V, it, HP, 0.0)
        got = {"update": _cat(ps) - _cat(before), "g": _cat([p.grad for p in ps]),
               "m": _cat([opt.state[p]["exp_avg"] for p in ps]), "v": _cat([opt.state[p]["exp_avg_sq"] for p in ps]),
               "norm": opt.last_grad_norm[0].double().cpu()}
        assert torch.equal(got["g"], _cat(G)), ".grad changed without clipping"
        _adam_bars(got, _torch_step(before, G, M, V, it, HP, 0.0), ref, f"ClipAdamW(max_norm=None) step {it + 1}")
        assert_close(got["norm"], ref["norm"], rtol=1e-6, what="last_grad_norm")
    assert opt.param_groups[0]["step_t"][0].item() == 3


def test_clip_adamw_wrapper_groups_and_schedules():
    """A parameter without .grad is skipped and keeps an empty state; a changed group["lr"]
    (a scheduler) takes effect on the next step; max_norm with two live groups raises; 49
    parameters in a group raise."""
    from models.optim import ClipAdamW
    sizes = [100, 1024, 5]
    P, ps = _wrapper_params(sizes, seed=52)
    G = _adam_state(sizes, seed=53)[1]
    opt = ClipAdamW(ps, lr=1e-2, weight_decay=1e-2, max_norm=1.0)
    ps[0].grad, ps[2].grad = G[0].clone().to(DEV), G[2].clone().to(DEV)
    opt.step()
    assert torch.equal(ps[1].detach().cpu(), P[1]) and len(opt.state[ps[1]]) == 0
    ref = _ref_adamw([P[0], P[2]], [G[0], G[2]], [torch.zeros(100), torch.zeros(5)], [torch.zeros(100), torch.zeros(5)],
                     0, HP, 1.0)
    assert_close(_cat([ps[0], ps[2]]) - _cat([P[0], P[2]]), ref["update"], rtol=1e-5, what="update without ps[1]")
    # lr change: the second step moves by the new lr
    before = [ps[0].detach().cpu(), ps[2].detach().cpu()]
    M = [opt.state[p]["exp_avg"].cpu() for p in (ps[0], ps[2])]
    V = [opt.state[p]["exp_avg_sq"].cpu() for p in (ps[0], ps[2])]
    opt.param_groups[0]["lr"] = 1e-4
    ps[0].grad, ps[2].grad = G[0].clone().to(DEV), G[2].clone().to(DEV)
    opt.step()
    ref = _ref_adamw(before, [G[0], G[2]], M, V, 1, dict(HP, lr=1e-4), 1.0)
    assert_close(_cat([ps[0], ps[2]]) - _cat(before), ref["update"], rtol=1e-5, what="update after group['lr'] = 1e-4")
    two = ClipAdamW([{"params": [ps[0]]}, {"params": [ps[2]]}], max_norm=1.0)
    with pytest.raises(RuntimeError, match="more than one param group"):
        two.step()
    many = [torch.nn.Parameter(torch.zeros(2, device=DEV)) for _ in range(49)]
    for p in many:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="at most 48"):
        ClipAdamW(many, max_norm=1.0).step()


@pytest.mark.parametrize("bad", [INF, NAN], ids=["inf", "nan"])
def test_clip_adamw_non_finite_gradient_as_torch(bad):
    """One inf, then one NaN, gradient entry in a 3-slice parameter set with max_norm = 1:
    clipped gradients, parameters and last_grad_norm as clip_grad_norm_ + AdamW give them from
    the same input (torch's clamp propagates a NaN coefficient: every gradient and parameter
    becomes NaN): the same NaN / inf pattern, and the finite values equal."""
    from models.optim import ClipAdamW
    sizes = [1000, 1024, 900]
    P, ps = _wrapper_params(sizes, seed=54)
    G = _adam_state(sizes, seed=55)[1]
    G[1][1000] = bad
    for p, g in zip(ps, G):
        p.grad = g.clone().to(DEV)
    opt = ClipAdamW(ps, lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"], max_norm=1.0)
    opt.step()
    Z = [torch.zeros(n) for n in sizes]
    yard = _torch_step(P, G, Z, Z, 0, HP, 1.0)
    got = {"g": _cat([p.grad for p in ps]), "p": _cat(ps), "norm": opt.last_grad_norm[0].double().cpu().reshape(1)}
    for k, want in (("g", yard["g"]), ("p", yard["p"]), ("norm", yard["norm"].reshape(1))):
        assert torch.equal(torch.isnan(got[k]), torch.isnan(want)), \
            f"{k}: {int(torch.isnan(got[k]).sum())} NaN entries, torch has {int(torch.isnan(want).sum())} of {want.numel()}"
        assert torch.equal(torch.isinf(got[k]), torch.isinf(want)), f"{k}: inf pattern"
        fin = torch.isfinite(want)
        assert_close(got[k][fin], want[fin], rtol=1e-6, what=f"finite {k}")
    assert opt.param_groups[0]["step_t"][1:3].view(torch.int32).tolist() == [0, 0]


# ------------------------------------------------------------------ C. seed draws

M64 = (1 << 64) - 1


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _slot(state: int, n: int, i: int) -> int:
    """slot i of n right after the state word became `state`"""
    return _splitmix64((state * n + i + 1) & M64) & ((1 << 62) - 1)


@pytest.mark.parametrize("s0", [0, (1 << 62) - 1])
@pytest.mark.parametrize("n", [1, 16, 64, 65, 4096])
def test_seed_slots_advance_matches_specification(n, s0):
    """Slot i after the k-th advance from state s0 is splitmix64((s0 + k) * n + i + 1) & (2^62 - 1)
    and the state becomes s0 + k; from s0 = 2^62 - 1 the product wraps mod 2^64."""
    nat, lib = _lib()
    slots = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    state = torch.tensor([s0], dtype=torch.int64, device=DEV)
    for k in (1, 2, 3):
        assert lib.lg_seed_slots_advance(slots.data_ptr(), n, state.data_ptr(), nat.stream_of(slots)) == LG_OK
        torch.cuda.synchronize()
        assert state.item() == s0 + k
        assert slots[:n].tolist() == [_slot(s0 + k, n, i) for i in range(n)]
        assert slots[n].item() == -1
    if s0:
        assert (s0 + 1) * n + 1 > M64 or n == 1  # the wrap is exercised


@pytest.mark.parametrize("n", [16, 65])
def test_clip_adamw_seeds_draws_as_seed_slots_advance(n):
    """lg_clip_adamw_seeds (one tiny tensor) leaves the slots and state lg_seed_slots_advance
    leaves from the same state (the splitmix64 arithmetic exists twice)."""
    nat, lib = _lib()
    s0 = (1 << 40) + 12345
    P, G, M, V = _adam_state([3], seed=n)
    a = _Abi(P, G, M, V)
    sa, sb = (torch.full((n + 1,), -1, dtype=torch.int64, device=DEV) for _ in range(2))
    ta, tb = (torch.tensor([s0], dtype=torch.int64, device=DEV) for _ in range(2))
    for k in (1, 2):
        assert a.step(HP, 1.0, seeds=(sa[:n], ta)) == LG_OK
        assert lib.lg_seed_slots_advance(sb.data_ptr(), n, tb.data_ptr(), nat.stream_of(sb)) == LG_OK
        torch.cuda.synchronize()
        assert torch.equal(sa, sb) and torch.equal(ta, tb)
        assert ta.item() == s0 + k and sa[:n].tolist() == [_slot(s0 + k, n, i) for i in range(n)]
    assert a.words() == (2, 0, 0)


def test_seed_slots_advance_argument_edges():
    """n == 0 is a no-op returning LG_OK; n == 4097 is LG_EINVAL."""
    nat, lib = _lib()
    slots = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    state = torch.tensor([9], dtype=torch.int64, device=DEV)
    st = nat.stream_of(slots)
    assert lib.lg_seed_slots_advance(slots.data_ptr(), 0, state.data_ptr(), st) == LG_OK
    assert lib.lg_seed_slots_advance(slots.data_ptr(), 4097, state.data_ptr(), st) == LG_EINVAL
    torch.cuda.synchronize()
    assert state.item() == 9 and slots.tolist() == [-1] * 4
