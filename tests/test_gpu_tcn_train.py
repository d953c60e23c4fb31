"""NormalPredictorTCN training on the library (lg_tcn_conv_train_fwd / lg_tcn_conv_bwd,
leakgnn::tcn_predictor) against a plain-torch restatement run on the CPU in fp64 (truth) and fp32
(yardstick).  Forwards: helpers.assert_close (1e-5 of the tensor's scale); gradients:
helpers.assert_grads_match_truth.  ReLU / dropout kinks: the references take every stage's combined
active-and-kept mask from the op's saved s > 0, and every place where that mask disagrees with
fp64's own ReLU sign among kept elements must pass helpers.check_relu_ties.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, assert_grads_match_truth, check_relu_ties
from oracle import dropout_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 128
EPS = 1e-5
NAN = float("nan")


def _nat():
    from models import _native as nat
    return nat, nat.load_library()


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _keep(seed, salt, rows, p):
    """The library's keep mask of `rows` global rows x 128 channels (oracle/dropout_ref.py)."""
    if p == 0.0:
        return torch.ones(rows, C, dtype=torch.bool)
    idx = np.arange(rows * C, dtype=np.uint64)
    return torch.from_numpy(dropout_ref.keep_mask(seed, salt, idx, p).reshape(rows, C))


# ------------------------------------------------------------------ one stage: reference
def _gather(x, idx, nseg, rows):
    """x (nseg * rows, C) gathered by segment-local rows idx (-1 = zero row) -> (nseg, len(idx), C)."""
    xz = torch.cat([x.view(nseg, rows, C), torch.zeros(nseg, 1, C, dtype=x.dtype)], 1)
    idx = idx.long()
    return xz[:, torch.where(idx < 0, torch.full_like(idx, rows), idx)]


def _stage_ref(t, dt, mask, scale, nseg, rows_in, rows_blk, dy, dres, table_t, rows_res):
    """One stage and its gradients in dtype dt on the CPU.  t: dict of fp32 CPU tensors (x, blk or None,
    table, w, b, lw, lb); mask: the (rows, C) active-and-kept decisions; dy: upstream gradient of out.
    dx also takes dres gathered by table_t's 4th column, as lg_tcn_conv_bwd's does."""
    x, w, b, lw, lb = (t[k].to(dt).clone().requires_grad_(True) for k in ("x", "w", "b", "lw", "lb"))
    table = t["table"]
    g = torch.cat([_gather(x, table[:, j], nseg, rows_in) for j in range(3)], -1)      # taps t, t-d, t-2d
    wt = w.flip(-1).permute(0, 2, 1).reshape(C, 3 * C)                                  # tap j <-> kernel index 2 - j
    z = (g @ wt.t() + b).reshape(-1, C)
    z.retain_grad()
    mu, var = z.mean(-1, keepdim=True), z.var(-1, unbiased=False, keepdim=True)
    rstd = (var + EPS).rsqrt()
    xhat = (z - mu) * rstd
    ln = xhat * lw + lb
    s = ln * mask.to(dt) * scale
    out = s
    if t["blk"] is not None:
        out = s + _gather(t["blk"].to(dt), table[:, 3], nseg, rows_blk).reshape(-1, C)
    (out * dy.to(dt)).sum().backward()
    dx = x.grad
    if dres is not None:
        dx = dx + _gather(dres.to(dt), table_t[:, 3], nseg, rows_res).reshape(-1, C)
    fwd = {"s": s.detach(), "out": out.detach(), "xhat": xhat.detach(), "rstd": rstd.detach().reshape(-1), "ln": ln.detach()}
    return fwd, {"dz": z.grad, "dx": dx, "dw": w.grad, "db": b.grad, "dgamma": lw.grad, "dbeta": lb.grad}


def _stage_gpu(t, p, seed, salt, nseg, rows_in, rows_blk, rows_out, dy=None, dres=None, table_t=None, rows_res=0,
               want_dx=True, save=True):
    """lg_tcn_conv_train_fwd (and, with dy, lg_tcn_conv_bwd) on NaN-filled outputs."""
    nat, lib = _nat()
    d = {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}
    st = nat.stream_of(d["x"])
    n = lib.lg_tcn_packed_weight_floats(C)
    pk, pkt = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    nat.check(lib.lg_tcn_pack_weight(nat.ptr(d["w"]), nat.ptr(pk), C, st), "pack")
    nat.check(lib.lg_tcn_pack_weight_t(nat.ptr(d["w"]), nat.ptr(pkt), C, st), "pack_t")
    R = nseg * rows_out
    f = {"s": _nan(R, C), "out": _nan(R, C) if d["blk"] is not None else None, "xhat": _nan(R, C) if save else None,
         "rstd": _nan(R) if save else None}
    seed_arg = seed.data_ptr() if torch.is_tensor(seed) else seed
    nat.check(lib.lg_tcn_conv_train_fwd(nat.ptr(d["x"]), nat.ptr(d["blk"]), nat.ptr(d["table"]), nat.ptr(pk),
                                        nat.ptr(d["b"]), nat.ptr(d["lw"]), nat.ptr(d["lb"]), EPS, p, seed_arg, salt,
                                        nat.ptr(f["s"]), nat.ptr(f["out"]), nat.ptr(f["xhat"]), nat.ptr(f["rstd"]),
                                        nseg, rows_in, rows_blk, rows_out, C, st), "lg_tcn_conv_train_fwd")
    if f["out"] is None:
        f["out"] = f["s"]
    if dy is None:
        torch.cuda.synchronize()
        return f, None
    g = {"dz": _nan(R, C), "dx": _nan(nseg * rows_in, C) if want_dx else None, "dw": _nan(C, C, 3), "db": _nan(C),
         "dgamma": _nan(C), "dbeta": _nan(C)}
    need = lib.lg_tcn_conv_bwd_workspace_bytes(nseg, rows_out, C)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dres_d = dres.to(DEV) if (dres is not None and want_dx) else None
    tt = table_t.to(DEV) if table_t is not None else None
    nat.check(lib.lg_tcn_conv_bwd(nat.ptr(dy.to(DEV)), nat.ptr(f["s"]), nat.ptr(f["xhat"]), nat.ptr(f["rstd"]),
                                  nat.ptr(d["x"]), nat.ptr(dres_d), nat.ptr(d["table"]), nat.ptr(tt) if want_dx else None,
                                  nat.ptr(pkt) if want_dx else None, nat.ptr(d["lw"]), p, nat.ptr(g["dz"]),
                                  nat.ptr(g["dx"]), nat.ptr(g["dw"]), nat.ptr(g["db"]), nat.ptr(g["dgamma"]),
                                  nat.ptr(g["dbeta"]), nseg, rows_in, rows_res if dres_d is not None else 0, rows_out, C,
                                  nat.ptr(ws), need, st), "lg_tcn_conv_bwd")
    torch.cuda.synchronize()
    return f, g


def _rand_stage(g, nseg, rows_in, rows_blk, table):
    return {"x": torch.randn(nseg * rows_in, C, generator=g),
            "blk": torch.randn(nseg * rows_blk, C, generator=g) if rows_blk else None,
            "table": table, "w": torch.randn(C, C, 3, generator=g) * 0.05, "b": torch.randn(C, generator=g) * 0.3,
            "lw": 1.0 + 0.3 * torch.randn(C, generator=g), "lb": 0.3 * torch.randn(C, generator=g)}


def _check_stage(t, p, seed, salt, nseg, rows_in, rows_blk, rows_out, dy, dres, table_t, rows_res, what,
                 names=("dz", "dx", "dw", "db", "dgamma", "dbeta"), want_dx=True):
    """Forward and backward of one stage against the references; returns the GPU results."""
    f, g = _stage_gpu(t, p, seed, salt, nseg, rows_in, rows_blk, rows_out, dy, dres, table_t, rows_res, want_dx)
    for k, v in {**f, **g}.items():
        assert v is None or not torch.isnan(v).any(), f"{what}: {k} has rows that were never written"
    mask = (f["s"] > 0).cpu()
    scale = 1.0 / (1.0 - p)
    f64, g64 = _stage_ref(t, torch.float64, mask, scale, nseg, rows_in, rows_blk, dy, dres, table_t, rows_res)
    _, g32 = _stage_ref(t, torch.float32, mask, scale, nseg, rows_in, rows_blk, dy, dres, table_t, rows_res)
    check_relu_ties({"stage": f64["ln"]}, {"stage": mask}, keep={"stage": _keep(seed, salt & 0x7FFFFFFF, nseg * rows_out, p)})
    for k in ("s", "out", "xhat", "rstd"):
        assert_close(f[k], f64[k], what=f"{what}: {k}")
    assert_grads_match_truth({k: g[k] for k in names}, {k: g32[k] for k in names}, {k: g64[k] for k in names})
    return f, g


# ------------------------------------------------------------------ 1. single stage, causal tables
@pytest.mark.parametrize("nseg,rows", [(1, 1), (1, 3), (7, 5), (1, 17), (3, 36), (40, 36)])
def test_stage_train_fwd_bwd(nseg, rows):
    from models.ops import TCN_SALT
    from models.tcn_plan import train_tables
    gen = torch.Generator().manual_seed(100 * nseg + rows)
    for d in (1, 8):
        fwd, tr = train_tables(rows, (d,))
        for residual in (False, True):
            # conv1 form: no forward residual, dx takes the bypass gradient dres; conv2 form: the reverse
            table, table_t = torch.from_numpy(fwd[int(residual)]), torch.from_numpy(tr[int(residual)])
            for p in (0.0, 0.25):
                t = _rand_stage(gen, nseg, rows, rows if residual else 0, table)
                dy = torch.randn(nseg * rows, C, generator=gen)
                dres = None if residual else torch.randn(nseg * rows, C, generator=gen)
                what = f"stage nseg={nseg} rows={rows} d={d} residual={residual} p={p}"
                args = (t, p, 1234 + d, TCN_SALT + 5, nseg, rows, rows if residual else 0, rows, dy, dres, table_t, rows)
                f, g = _check_stage(*args, what)
                f2, g2 = _stage_gpu(*args)                                  # two runs: bit-identical
                for k in f:
                    assert torch.equal(f[k], f2[k]), f"{what}: {k} differs between two runs"
                for k in g:
                    assert torch.equal(g[k], g2[k]), f"{what}: {k} differs between two runs"
                _, g3 = _stage_gpu(*args, want_dx=False)                    # dx = NULL: the rest unchanged
                for k in ("dz", "dw", "db", "dgamma", "dbeta"):
                    assert torch.equal(g[k], g3[k]), f"{what}: {k} changes when dx is NULL"


def test_stage_p0_without_saves_is_the_inference_launch():
    """p = 0 with no save buffers: lg_tcn_conv_fwd's result, bit for bit, in s (conv1) or out (conv2)."""
    from models.tcn_plan import train_tables
    nat, lib = _nat()
    gen = torch.Generator().manual_seed(5)
    nseg, rows = 3, 21
    fwd, _ = train_tables(rows, (2,))
    for residual in (False, True):
        t = _rand_stage(gen, nseg, rows, rows if residual else 0, torch.from_numpy(fwd[int(residual)]))
        f, _ = _stage_gpu(t, 0.0, 0, 0, nseg, rows, rows if residual else 0, rows, save=False)
        d = {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}
        pk = torch.empty(lib.lg_tcn_packed_weight_floats(C), device=DEV)
        st = nat.stream_of(pk)
        nat.check(lib.lg_tcn_pack_weight(nat.ptr(d["w"]), nat.ptr(pk), C, st), "pack")
        want = _nan(nseg * rows, C)
        nat.check(lib.lg_tcn_conv_fwd(nat.ptr(d["x"]), nat.ptr(d["blk"]), nat.ptr(d["table"]), nat.ptr(pk), nat.ptr(d["b"]),
                                      nat.ptr(d["lw"]), nat.ptr(d["lb"]), EPS, nat.ptr(want), nseg, rows,
                                      rows if residual else 0, rows, C, st), "lg_tcn_conv_fwd")
        torch.cuda.synchronize()
        assert torch.equal(f["out"], want)


# ------------------------------------------------------------------ 2. dropout mask
def test_stage_dropout_mask_and_scale():
    from models.ops import TCN_SALT
    from models.tcn_plan import train_tables
    nat, _ = _nat()
    gen = torch.Generator().manual_seed(11)
    nseg, rows, p, seed = 9, 36, 0.25, (5 << 32) + 77
    fwd, _ = train_tables(rows, (4,))
    t = _rand_stage(gen, nseg, rows, rows, torch.from_numpy(fwd[1]))
    for i in (0, 3, 7):
        f0, _ = _stage_gpu(t, 0.0, seed, TCN_SALT + i, nseg, rows, rows, rows)
        fp, _ = _stage_gpu(t, p, seed, TCN_SALT + i, nseg, rows, rows, rows)
        s0, sp = f0["s"].cpu(), fp["s"].cpu()
        active = s0 > 0
        keep = _keep(seed, TCN_SALT + i, nseg * rows, p)
        assert 0.70 < keep.float().mean().item() < 0.80
        assert torch.equal((sp != 0)[active], keep[active]), f"conv {i}: keep mask differs from the counter RNG"
        assert (sp[~active] == 0).all()
        both = active & keep
        want = s0[both] * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
        ulps = (sp[both].view(torch.int32) - want.view(torch.int32)).abs().max().item()
        assert ulps <= 1, f"conv {i}: kept values are {ulps} ulp off the p = 0 run times 1 / (1 - p)"
        assert torch.equal(fp["xhat"], f0["xhat"]) and torch.equal(fp["rstd"], f0["rstd"])
        # the same seed read from the device (salt bit 31)
        dseed = torch.tensor([seed], dtype=torch.int64, device=DEV)
        fd, _ = _stage_gpu(t, p, dseed, (TCN_SALT + i) | nat.LG_SALT_SEED_PTR, nseg, rows, rows, rows)
        assert torch.equal(fd["s"], fp["s"]) and torch.equal(fd["out"], fp["out"])
    # another salt draws another mask
    fq, _ = _stage_gpu(t, p, seed, TCN_SALT + 6, nseg, rows, rows, rows)
    assert not torch.equal(fq["s"] != 0, fp["s"] != 0)


# ------------------------------------------------------------------ 3. random tables
def test_stage_random_tables():
    from models.ops import TCN_SALT
    gen = torch.Generator().manual_seed(9)
    # (a) any table: zero taps, repeated tap rows, no residual rows for some outputs; dx not asked for
    nseg, rows_in, rows_blk, rows_out = 5, 40, 29, 37
    table = torch.randint(-1, rows_in, (rows_out, 4), generator=gen, dtype=torch.int32)
    table[:, 3] = torch.randint(-1, rows_blk, (rows_out,), generator=gen, dtype=torch.int32)
    table[3, :3] = 7                                                    # one input row through all three taps
    table[4, :3] = -1                                                   # a row that reads nothing
    t = _rand_stage(gen, nseg, rows_in, rows_blk, table)
    dy = torch.randn(nseg * rows_out, C, generator=gen)
    _check_stage(t, 0.25, 99, TCN_SALT + 1, nseg, rows_in, rows_blk, rows_out, dy, None, None, 0, "random table",
                 names=("dz", "dw", "db", "dgamma", "dbeta"), want_dx=False)
    # (b) at most one consumer per (input row, tap): the transposed table exists, so dx is checked too
    nseg, rows_in, rows_blk, rows_out, rows_res = 3, 23, 7, 19, 5
    table = torch.full((rows_out, 4), -1, dtype=torch.int32)
    for j in range(3):
        table[:, j] = torch.randperm(rows_in, generator=gen)[:rows_out].int()
    drop = torch.rand(rows_out, 3, generator=gen) < 0.2
    table[:, :3][drop] = -1
    table[:, 3] = torch.randint(-1, rows_blk, (rows_out,), generator=gen, dtype=torch.int32)
    table_t = torch.full((rows_in, 4), -1, dtype=torch.int32)
    for r in range(rows_out):
        for j in range(3):
            if table[r, j] >= 0:
                assert table_t[table[r, j], j] == -1
                table_t[table[r, j], j] = r
    table_t[:, 3] = torch.randint(-1, rows_res, (rows_in,), generator=gen, dtype=torch.int32)
    t = _rand_stage(gen, nseg, rows_in, rows_blk, table)
    dy = torch.randn(nseg * rows_out, C, generator=gen)
    dres = torch.randn(nseg * rows_res, C, generator=gen)
    _check_stage(t, 0.0, 0, 0, nseg, rows_in, rows_blk, rows_out, dy, dres, table_t, rows_res, "injective table")


# ------------------------------------------------------------------ 4. module
def _tcn_ref(sd, x, xt, nb, dt, masks, scale, up):
    """Plain-torch NormalPredictorTCN (reference models/predictor.py:17-81) in dtype dt on the CPU with the
    given active-and-kept masks; returns (output, gradients by name incl. x / x_time, LayerNorm outputs)."""
    P = {k: v.detach().cpu().to(dt).clone().requires_grad_(True) for k, v in sd.items()}
    x, xt = x.to(dt).clone().requires_grad_(True), xt.to(dt).clone().requires_grad_(True)
    h = F.conv1d(torch.cat([x, xt], -1).transpose(1, 2), P["input_proj.weight"], P["input_proj.bias"])  # (B, C, L)
    pre = {}
    for b in range(nb):
        d, r = 2 ** b, h
        for j in (1, 2):
            z = F.conv1d(F.pad(h, (2 * d, 0)), P[f"tcn.{b}.conv{j}.conv.weight"], P[f"tcn.{b}.conv{j}.conv.bias"], dilation=d)
            ln = F.layer_norm(z.transpose(1, 2), (C,), P[f"tcn.{b}.norm{j}.weight"], P[f"tcn.{b}.norm{j}.bias"], EPS)
            site = f"c{2 * b + j - 1}"
            pre[site] = ln.detach()
            h = (ln * masks[site].to(dt) * scale).transpose(1, 2)
        h = r + h
    out = h[:, :, -1] @ P["head.weight"].t() + P["head.bias"]
    (out * up.to(dt)).sum().backward()
    grads = {k: v.grad for k, v in P.items()}
    grads["x"], grads["x_time"] = x.grad, xt.grad
    return out.detach(), grads, pre


class _Spy:
    """Records the outputs of leakgnn::tcn_predictor calls made by the module."""

    def __init__(self, monkeypatch, seed=None):
        from models import library
        self.calls = []
        orig = torch.ops.leakgnn.tcn_predictor

        def spy(*a):
            out = orig(*a)
            self.calls.append((a, out))
            return out
        monkeypatch.setattr(torch.ops.leakgnn, "tcn_predictor", spy)
        if seed is not None:
            monkeypatch.setattr(library, "seed_tensor", lambda device: torch.tensor([seed], dtype=torch.int64))


def _module(nb, seed, **kw):
    from models.predictor import NormalPredictorTCN
    torch.manual_seed(seed)
    m = NormalPredictorTCN(29, 9, num_blocks=nb, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.1 * torch.randn(q.shape, generator=g))
    return m.to(DEV)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("B,L", [(2, 1), (3, 7), (5, 36)])
@pytest.mark.parametrize("nb", [1, 4])
def test_module_matches_reference(monkeypatch, nb, B, L, train):
    from models.ops import TCN_SALT
    seed, p = 4242 + L, 0.1 if train else 0.0
    spy = _Spy(monkeypatch, seed)
    m = _module(nb, 7 * nb + L).train(train)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(B + L)
    x, xt, up = torch.randn(B, L, 29, generator=g), torch.randn(B, L, 9, generator=g), torch.randn(B, 29, generator=g)
    xd, xtd = x.to(DEV).requires_grad_(True), xt.to(DEV).requires_grad_(True)
    out = m(xd, xtd)
    assert len(spy.calls) == 1, "the module did not take the HIP path"
    args, saved = spy.calls[0]
    assert args[6] == p and args[8] is True
    (out * up.to(DEV)).sum().backward(retain_graph=True)
    grads = {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters()}
    grads["x"], grads["x_time"] = xd.grad.cpu().clone(), xtd.grad.cpu().clone()
    n = 2 * nb
    masks = {f"c{i}": (saved[1 + i] > 0).cpu().view(B, L, C) for i in range(n)}
    keep = {f"c{i}": _keep(seed, TCN_SALT + i, B * L, p).view(B, L, C) for i in range(n)}
    scale = 1.0 / (1.0 - p)
    out64, g64, pre64 = _tcn_ref(sd, x, xt, nb, torch.float64, masks, scale, up)
    _, g32, _ = _tcn_ref(sd, x, xt, nb, torch.float32, masks, scale, up)
    check_relu_ties(pre64, masks, keep=keep)
    if train:  # every dropped unit is one the counter RNG drops
        for i in range(n):
            act = pre64[f"c{i}"] > 1e-4
            assert torch.equal(masks[f"c{i}"][act], keep[f"c{i}"][act]), f"conv {i}: mask differs from the counter RNG"
    assert_close(out, out64, what=f"module output nb={nb} B={B} L={L} train={train}")
    assert_grads_match_truth(grads, g32, g64)
    # a second backward over the same graph: equal gradients, nothing accumulated inside the op
    for q in list(m.parameters()) + [xd, xtd]:
        q.grad = None
    (out * up.to(DEV)).sum().backward()
    again = {k: v.grad.detach().cpu() for k, v in m.named_parameters()}
    again["x"], again["x_time"] = xd.grad.cpu(), xtd.grad.cpu()
    for k in grads:
        assert torch.equal(grads[k], again[k]), f"{k} differs on the second backward"


def test_module_routes(monkeypatch):
    """What stays on the stock module: other widths, eval-mode no_grad calls; and save=False refuses a backward."""
    spy = _Spy(monkeypatch, 1)
    g = torch.Generator().manual_seed(3)
    x, xt = torch.randn(4, 12, 29, generator=g).to(DEV), torch.randn(4, 12, 9, generator=g).to(DEV)

    def stock(m):
        return m.head(m.tcn(m.input_proj(torch.cat([x, xt], -1).transpose(1, 2)))[:, :, -1])

    m64 = _module(2, 5, hidden_channels=64).eval()
    stock(m64)                                      # MIOpen picks its solvers on the first call of a shape
    out = m64(x, xt)
    assert not spy.calls and torch.equal(out, stock(m64)) and out.requires_grad
    m = _module(4, 6).eval()
    with torch.no_grad():                           # (two stock calls at this width are not bit-equal: MIOpen)
        out = m(x, xt)
        assert not spy.calls
        assert_close(out, stock(m), what="eval-mode no_grad forward vs the stock composition")
    hip = m(x, xt)                                  # eval mode under autograd: the library, p = 0
    assert len(spy.calls) == 1 and spy.calls[0][0][6] == 0.0
    assert_close(hip, out, what="HIP eval-mode forward vs stock")
    m.train()
    with torch.no_grad():                           # train mode without grad: dropout drawn, nothing saved
        m(x, xt)
    a, saved = spy.calls[1]
    assert a[6] == pytest.approx(0.1) and a[8] is False and all(t.numel() == 0 for t in saved[1:])
    from models import library
    with pytest.raises(RuntimeError, match="save=False"):
        library.tcn_predictor_backward(torch.zeros(4, C, device=DEV), torch.zeros(4, 12, C, device=DEV),
                                       list(a[1]), list(a[3]), list(saved[1:9]), list(saved[9:17]), list(saved[17:25]),
                                       list(saved[25:]), 0.1, True)


def test_opcheck_tcn_predictor():
    m = _module(1, 9).eval()
    stages = [(c.conv, n) for blk in m.tcn for c, n in ((blk.conv1, blk.norm1), (blk.conv2, blk.norm2))]
    h = torch.randn(2, 5, C, device=DEV, requires_grad=True)
    args = (h, [c.weight for c, _ in stages], [c.bias for c, _ in stages], [n.weight for _, n in stages],
            [n.bias for _, n in stages], EPS, 0.0, torch.zeros(1, dtype=torch.int64), True)
    torch.library.opcheck(torch.ops.leakgnn.tcn_predictor, args,
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


# ------------------------------------------------------------------ 5. weight cache
def test_packed_weight_cache_follows_optimizer_steps():
    from models.predictor import NormalPredictorTCN
    m = _module(2, 31).eval()
    g = torch.Generator().manual_seed(8)
    x, xt = torch.randn(3, 9, 29, generator=g).to(DEV), torch.randn(3, 9, 9, generator=g).to(DEV)
    first = m(x, xt).detach()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    m(x, xt).square().sum().backward()
    opt.step()                                       # in place: same addresses, new versions
    with torch.no_grad():
        m.tcn[1].conv2.conv.weight.mul_(1.5)
    second = m(x, xt).detach()
    fresh = NormalPredictorTCN(29, 9, num_blocks=2).to(DEV).eval()
    fresh.load_state_dict(m.state_dict())
    want = fresh(x, xt).detach()
    assert not torch.equal(first, second)
    assert torch.equal(second, want), "the forward after an optimizer step used a stale packed weight"
    # and the backward's transposed pack
    for mod in (m, fresh):
        mod.zero_grad()
        mod(x, xt).square().sum().backward()
    for (k, a), (_, b) in zip(m.named_parameters(), fresh.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
