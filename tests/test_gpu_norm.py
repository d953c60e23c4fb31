"""Pre-norm residual trunk on the GPU: the two LayerNorm row kernels (csrc/norm.hip) against
F.layer_norm and its autograd in fp64, then LeakDetector(skip="residual", norm="layer") against a
pre-norm restatement of the oracle (eval parity at 2, 4 and 12 layers, learned edge weights, the
general-width path, train mode on the kernels' own dropout masks), the default's guard, a captured
training step and opcheck of gnn_trunk_norm.

The oracle is a test-local subclass of oracle/detector_ref.LeakDetectorRef whose layer loop is
x = x + dropout(relu(conv(LN_l(x)))) with the heads on LN_L(x); it keeps relu_masks and trace.  The
conv sites' kink decisions come from LeakDetector.capture["fmask"], the sign behind |h_u - h_v|
from capture["xns"][-1] (the tensor the heads read)."""
from __future__ import annotations

import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import LTA_INP, RTOL, assert_close, assert_grads_match_truth, check_relu_ties, hip_relu_masks, lta_ids
from test_gpu_edge_weight import conv_ref
from test_gpu_skip import _batch, _fixed_seed, _log_w

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LW = "edge_log_weight"
EPS = 1e-5
MASK_OUT = 0x10


# ----------------------------------------------------------------------------- 1. the kernels alone
def _rows(N, B, D):
    """randn rows with three planted ones: all zero, constant (zero variance), and mean 100 with
    standard deviation 1 (where a one-pass E[x^2] - mean^2 variance loses its digits)."""
    gen = torch.Generator().manual_seed(1000 * D + B)
    x = torch.randn(N * B, D, generator=gen)
    x[0] = 0.0
    x[1] = 3.7
    x[2] = 100.0 + torch.randn(D, generator=gen)
    gamma = 1.0 + 0.5 * torch.randn(D, generator=gen)
    beta = 0.3 * torch.randn(D, generator=gen)
    return gen, x, gamma, beta


def _bound(name, got, truth, ref32):
    """max(RTOL x scale, 2 x torch's own fp32 error), scale = max |truth|; prints both errors."""
    got, truth, ref32 = got.detach().double().cpu(), truth.double().cpu(), ref32.detach().double().cpu()
    scale = truth.abs().max().item()
    e, e32 = (got - truth).abs().max().item(), (ref32 - truth).abs().max().item()
    lim = max(RTOL * scale, 2 * e32)
    print(f"  {name}: err {e:.3e}, torch fp32 err {e32:.3e}, scale {scale:.3e}, bound {lim:.3e}")
    assert bool(torch.isfinite(got).all()), name
    assert e <= lim, f"{name}: err {e:.3e} > {lim:.3e} (torch fp32 {e32:.3e}, scale {scale:.3e})"


PAD = 8  # guard rows behind every output: the ragged last row group must not write past the end


def _out(rows, D):
    return torch.full((rows + PAD, D), float("nan"), device=DEV)


def _untouched(t, rows):
    return bool(torch.isnan(t[rows:]).all()) and bool(torch.isfinite(t[:rows]).all())


def _fwd(lib, x, f, gamma, beta, stats=True):
    from models._native import ptr
    rows, D = x.shape
    st = torch.cuda.current_stream(DEV).cuda_stream
    xsum = _out(rows, D) if f is not None else None
    xn = _out(rows, D)
    sts = torch.full((rows + PAD, 2), float("nan"), device=DEV) if stats else None
    rc = lib.lg_add_layernorm_fwd(ptr(x), ptr(f), ptr(gamma), ptr(beta), ptr(xsum), ptr(xn), ptr(sts), rows, D, EPS, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _untouched(xn, rows) and (xsum is None or _untouched(xsum, rows)) and (sts is None or _untouched(sts, rows))
    return (xsum[:rows] if xsum is not None else None), xn[:rows], (sts[:rows] if stats else None)


@pytest.mark.parametrize("B", [1, 20])
@pytest.mark.parametrize("D", [32, 64])
def test_add_layernorm_fwd_vs_fp64(D, B):
    """N = 41 nodes x B windows: 41 rows leave a ragged last row group at both widths (4 or 8 rows a
    wave), 820 rows take several workgroups.  Truth: F.layer_norm in fp64 on the same fp32 inputs."""
    from models import _native as nat
    lib = nat.load_library()
    gen, x, gamma, beta = _rows(41, B, D)
    f = torch.relu(torch.randn(x.shape, generator=gen))
    xd, fd, gd, bd = (t.to(DEV) for t in (x, f, gamma, beta))
    print(f"layernorm fwd D={D} rows={x.shape[0]}")
    # the entry norm (f = NULL) on the planted rows
    _, xn, st = _fwd(lib, xd, None, gd, bd)
    truth = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), EPS)
    t32, m32, r32 = torch.native_layer_norm(xd, [D], gd, bd, EPS)
    _bound("xn", xn, truth, t32)
    mean64 = x.double().mean(1)
    rstd64 = (x.double().var(1, unbiased=False) + EPS).rsqrt()
    _bound("mean", st[:, 0], mean64, m32.reshape(-1))
    _bound("rstd", st[:, 1], rstd64, r32.reshape(-1))
    assert torch.equal(xn[1], bd) and torch.equal(xn[0], bd)  # zero variance: xn is beta, exactly
    # the row with mean 100, std 1: a one-pass variance is off by ~1e-3 relative here
    assert abs(st[2, 1].item() / rstd64[2].item() - 1.0) < 1e-5
    # f = zeros is the entry norm, bit for bit; stats = NULL (inference) changes nothing
    xs0, xn0, st0 = _fwd(lib, xd, torch.zeros_like(xd), gd, bd)
    assert torch.equal(xn0, xn) and torch.equal(st0, st) and torch.equal(xs0, xd)
    assert torch.equal(_fwd(lib, xd, None, gd, bd, stats=False)[1], xn)
    # x + f: one fp32 add, then the norm of that sum
    xs, xn2, st2 = _fwd(lib, xd, fd, gd, bd)
    assert torch.equal(xs, xd + fd)
    truth2 = F.layer_norm((x + f).double(), (D,), gamma.double(), beta.double(), EPS)
    _bound("xn(x + f)", xn2, truth2, F.layer_norm(xd + fd, (D,), gd, bd, EPS))
    assert torch.equal(_fwd(lib, xd, fd, gd, bd, stats=False)[1], xn2)


def _bwd(lib, dxn, x, stats, gamma, carry, flags, scale_out):
    from models._native import ptr
    rows, D = x.shape
    st = torch.cuda.current_stream(DEV).cuda_stream
    ws = torch.empty(int(lib.lg_layernorm_bwd_workspace_bytes(D)), dtype=torch.uint8, device=DEV)
    dx = _out(rows, D)
    dg, db = torch.full((D,), float("nan"), device=DEV), torch.full((D,), float("nan"), device=DEV)
    rc = lib.lg_layernorm_bwd(ptr(dxn), ptr(x), ptr(stats), ptr(gamma), ptr(carry), ptr(dx), ptr(dg), ptr(db), rows, D,
                              flags, scale_out, ptr(ws), ws.numel(), st)
    torch.cuda.synchronize()
    assert rc == 0 and _untouched(dx, rows)
    return dx[:rows], dg, db


@pytest.mark.parametrize("B", [1, 20])
@pytest.mark.parametrize("D", [32, 64])
def test_layernorm_bwd_vs_fp64(D, B):
    """dx, dgamma, dbeta against F.layer_norm's autograd in fp64 on the same fp32 inputs; the carry
    and the node init's mask as exact statements on top of the plain call; two calls bit-equal."""
    from models import _native as nat
    lib = nat.load_library()
    gen, x, gamma, beta = _rows(41, B, D)
    dxn = torch.randn(x.shape, generator=gen)
    carry = torch.randn(x.shape, generator=gen)
    xd, gd, bd, dd, cd = (t.to(DEV) for t in (x, gamma, beta, dxn, carry))
    _, _, stats = _fwd(lib, xd, None, gd, bd)
    print(f"layernorm bwd D={D} rows={x.shape[0]}")

    def autograd(xi, gi, bi, up):
        xi, gi, bi = (t.detach().clone().requires_grad_(True) for t in (xi, gi, bi))
        F.layer_norm(xi, (D,), gi, bi, EPS).backward(up)
        return xi.grad, gi.grad, bi.grad

    t_dx, t_dg, t_db = autograd(x.double(), gamma.double(), beta.double(), dxn.double())
    r_dx, r_dg, r_db = autograd(xd, gd, bd, dd)
    dx, dg, db = _bwd(lib, dd, xd, stats, gd, None, 0, 1.0)
    _bound("dx", dx, t_dx, r_dx)
    _bound("dgamma", dg, t_dg, r_dg)
    _bound("dbeta", db, t_db, r_db)
    assert bool(torch.isfinite(dx[1]).all())  # the zero-variance row
    # the carry: one fp32 add after everything else
    dx_c, dg_c, db_c = _bwd(lib, dd, xd, stats, gd, cd, 0, 1.0)
    assert torch.equal(dx_c, dx + cd) and torch.equal(dg_c, dg) and torch.equal(db_c, db)
    # the node init's mask: the last arithmetic, on x's own sign
    s = 1.0 / 0.9
    zero = torch.zeros_like(dx)
    dx_m, dg_m, db_m = _bwd(lib, dd, xd, stats, gd, cd, MASK_OUT, s)
    assert torch.equal(dx_m, torch.where(xd > 0, (dx + cd) * s, zero))
    assert torch.equal(dg_m, dg) and torch.equal(db_m, db)
    assert torch.equal(_bwd(lib, dd, xd, stats, gd, None, MASK_OUT, s)[0], torch.where(xd > 0, dx * s, zero))
    # run to run
    again = _bwd(lib, dd, xd, stats, gd, cd, MASK_OUT, s)
    assert torch.equal(again[0], dx_m) and torch.equal(again[1], dg_m) and torch.equal(again[2], db_m)


# ----------------------------------------------------------------------------- the pre-norm oracle
@functools.lru_cache(maxsize=None)
def _norm_ref_cls():
    from oracle import gcn_ref, graph_ref
    from oracle.detector_ref import LeakDetectorRef

    class NormRef(LeakDetectorRef):
        """LeakDetectorRef with `norms` and the layer loop x = x + dropout(relu(conv(LN_l(x)))); the
        heads read LN_L(x)."""

        def __init__(self, *a, gnn_layers=2, node_hidden=64, **kw):
            super().__init__(*a, gnn_layers=gnn_layers, node_hidden=node_hidden, **kw)
            self.norms = torch.nn.ModuleList(torch.nn.LayerNorm(node_hidden) for _ in range(gnn_layers + 1))

        def forward(self, residual, tfeat=None):
            B, L, S = residual.shape
            N = len(self.node_names)
            h_s = self.sensor_encoder(residual, tfeat)
            dev = residual.device
            h0 = torch.zeros(B, N, h_s.shape[-1], dtype=residual.dtype, device=dev)
            idx = self.sensor_node_idx.to(dev)
            h0[:, idx, :] = h_s
            mask = torch.zeros(N, 1, dtype=residual.dtype, device=dev)
            mask[idx, 0] = 1.0
            h = torch.cat([h0, mask.unsqueeze(0).expand(B, -1, -1)], dim=-1)
            h = self.dropout(self._relu("init", self.sensor_to_node(h)))
            self.trace["node_init"] = h
            x = h.reshape(B * N, -1)
            ei = torch.from_numpy(graph_ref.batchify(self.edge_index_single.numpy(), N, B)).to(dev)
            for i, conv in enumerate(self.convs):
                x = x + self.dropout(self._relu(f"conv{i}", conv(self.norms[i](x), ei)))
                self.trace[f"conv{i}"] = x
            x = self.norms[len(self.convs)](x)
            h_nodes = x.view(B, N, -1)
            u, v = self.pipe_ends[:, 0].to(dev), self.pipe_ends[:, 1].to(dev)
            h_u, h_v = h_nodes[:, u, :], h_nodes[:, v, :]
            feat = torch.cat([h_u, h_v, self._abs("absdiff", h_u - h_v)], dim=-1)
            mlp = self.edge_head.mlp
            pipe_logits = mlp[3](mlp[2](self._relu("edge", mlp[0](feat)))).squeeze(-1)
            batch = torch.arange(B, device=dev).repeat_interleave(N)
            pooled = gcn_ref.global_mean_pool(x, batch, size=B)
            nmlp = self.noleak_head.mlp
            noleak = nmlp[3](nmlp[2](self._relu("noleak", nmlp[0](pooled)))).squeeze(-1).unsqueeze(-1)
            return torch.cat([pipe_logits, noleak], dim=-1)

    return NormRef


@functools.lru_cache(maxsize=None)
def _random_sd(layers: int, seed: int = 43, **kw):
    """A random state dict of the `layers`-layer pre-norm detector: conv biases off zero, the norms'
    weight and bias off 1 and 0; shared, read-only."""
    sensors, pipes = lta_ids()
    torch.manual_seed(seed)
    ref = _norm_ref_cls()(LTA_INP, sensors, pipes, gnn_layers=layers, **kw).eval()
    with torch.no_grad():
        for c in ref.convs:
            c.bias.normal_(0, 0.1)
        for n in ref.norms:
            n.weight.normal_(1.0, 0.2)
            n.bias.normal_(0, 0.1)
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _oracle(sd, r, tf, dt, dev, layers, up=None, lab=None, masks=None, log_w=None, kw=None):
    """The pre-norm oracle in eval mode: (logits, parameter grads, pre-activations, upstream gradient);
    log_w as in tests/test_gpu_skip.py."""
    sensors, pipes = lta_ids()
    mr = _norm_ref_cls()(LTA_INP, sensors, pipes, gnn_layers=layers, **(kw or {})).eval()
    mr.load_state_dict(sd)
    mr = mr.to(dt).to(dev)
    mr.sensor_encoder.gru.train()  # MIOpen's RNN backward needs training mode (1 layer: no dropout)
    mr.relu_masks = masks or {}
    lw = None
    if log_w is not None:
        lw = log_w.detach().to(dt).to(dev).requires_grad_(True)
        ew = lw.exp().repeat_interleave(2).repeat(r.shape[0])
        for c in mr.convs:
            c.forward = lambda x, ei, c=c: conv_ref(x, ei, ew, c.lin.weight, c.bias, x.shape[0])
    out = mr(r.to(dt).to(dev), tf.to(dt).to(dev))
    if up is None:
        lo = out.detach().requires_grad_(True)
        F.cross_entropy(lo, lab).backward()
        up = lo.grad.clone()
    out.backward(up.to(dt).to(dev))
    pre = {k[len("pre_"):]: v.detach() for k, v in mr.trace.items() if k.startswith("pre_")}
    grads = {n: p.grad.detach().cpu() for n, p in mr.named_parameters()}
    if lw is not None:
        grads[LW] = lw.grad.detach().cpu()
    return out.detach().cpu(), grads, pre, up


def _detector(sd, layers, skip="residual", norm="layer", **kw):
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    m = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=layers, skip=skip, norm=norm, **kw).to(DEV).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"edge_weight", LW}
    assert not unexpected or (norm == "none" and all(k.startswith("norms.") for k in unexpected))
    return m


def _norm_masks(m, B, scale=None):
    """The kink decisions of a captured pre-norm forward in the oracle's shapes.  scale (train mode):
    the masks as floats, keep x 1 / (1 - p), so the eval-mode oracle's z * mask is dropout(relu(z))
    with the kernels' own keep decisions."""
    N, P = len(m.node_names), len(m.pipe_ids)
    cap = m.capture
    assert cap["node_major"] and len(cap["fmask"]) == len(m.convs) and len(cap["xns"]) == len(m.convs) + 1
    assert len(cap["xs"]) == len(m.convs) + 1
    heads_in = dict(cap, xs=list(cap["xs"][:-1]) + [cap["xns"][-1]])  # |h_u - h_v| is taken on xn_L
    masks = hip_relu_masks(heads_in, B, N, P, m.pipe_ends)
    for l, fm in enumerate(cap["fmask"]):
        assert fm.dtype == torch.bool and tuple(fm.shape) == tuple(cap["xs"][l + 1].shape)
        masks[f"conv{l}"] = fm.permute(1, 0, 2).reshape(B, N, -1).cpu()
    if scale is not None:
        masks = {k: (v.to(torch.float64) * scale if v.dtype == torch.bool else v) for k, v in masks.items()}
    return masks


def _parity(B, layers, log_w=None, learned=False, train_p=None):
    sd = _random_sd(layers)
    r, tf, lab = _batch(B)
    _, _, pre64, up = _oracle(sd, r, tf, torch.float64, "cpu", layers, lab=lab, log_w=log_w)
    kw = dict(edge_weight=log_w.exp(), learn_edge_weight=learned) if log_w is not None else {}
    if train_p is not None:
        kw["dropout"] = train_p
    m = _detector(sd, layers, **kw)
    if train_p is not None:
        m.train()
    m.capture = {}
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.float().to(DEV))
    if train_p is None:
        masks = _norm_masks(m, B)
        ties = check_relu_ties(pre64, masks)
    else:
        masks, ties = _norm_masks(m, B, scale=1.0 / (1.0 - train_p)), -1
    o64, g64, _, _ = _oracle(sd, r, tf, torch.float64, "cpu", layers, up=up, masks=masks, log_w=log_w)
    o32, g32, _, _ = _oracle(sd, r, tf, torch.float32, "cpu", layers, up=up, masks=masks, log_w=log_w)
    _, g32d, _, _ = _oracle(sd, r, tf, torch.float32, DEV, layers, up=up, masks=masks, log_w=log_w)
    got = {n: p.grad for n, p in m.named_parameters()}
    assert {f"norms.{l}.{w}" for l in range(layers + 1) for w in ("weight", "bias")} <= set(got)
    assert all(got[f"norms.{l}.weight"] is not None and float(got[f"norms.{l}.weight"].abs().max()) > 0
               for l in range(layers + 1))
    if not learned:
        for d in (g64, g32, g32d):
            d.pop(LW, None)
    scale = o64.abs().max().item()
    e_gpu = (lg.detach().double().cpu() - o64).abs().max().item()
    e_ref = (o32.double() - o64).abs().max().item()
    print(f"norm L={layers} B={B} weighted={log_w is not None} learned={learned} train_p={train_p}: logits err vs fp64 "
          f"{e_gpu:.3e} (fp32 oracle's own {e_ref:.3e}, scale {scale:.3e}, RTOL x scale {RTOL * scale:.3e}), "
          f"vs fp32 oracle {(lg.detach().double().cpu() - o32.double()).abs().max().item():.3e}, ties {ties}")
    return m, lg, (o32, o64, e_gpu, e_ref, scale), (got, g32, g64, g32d)


# ----------------------------------------------------------------------------- 2. eval parity
@pytest.mark.parametrize("B", [4, 20])
@pytest.mark.parametrize("layers", [2, 4])
def test_norm_detector_vs_oracle(layers, B):
    """L-TOWN-A, eval, random weights (the norms' too); B = 4 (fewer windows than a tile), 20 a ragged
    tile.  Logits within RTOL of the fp32 pre-norm oracle, every parameter gradient (all norms.*
    among them) against the fp64 oracle on the HIP path's side of every kink."""
    m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(B, layers)
    assert not m._fused_encoder(torch.zeros(B, 36, 29, device=DEV), None, B, 661, 64, True)
    assert_close(lg, o32, what=f"L={layers} B={B} logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_norm_detector_12_layers_vs_oracle():
    """gnn_layers = 12, B = 20.  The logits bar: the GPU's error against the fp64 oracle within
    max(RTOL x scale, 2 x the fp32 CPU oracle's own error against fp64)."""
    m, lg, (o32, o64, e_gpu, e_ref, scale), (got, g32, g64, g32d) = _parity(20, 12)
    assert e_gpu <= max(RTOL * scale, 2 * e_ref), (e_gpu, e_ref, scale)
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_norm_with_learned_edge_weights_grad():
    """learn_edge_weight under the norm, 4 layers, B = 20: every layer's lg_sddmm_nm reads xn_l, the
    carried gradient and the layer's own bits; edge_log_weight.grad against fp64."""
    m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(20, 4, log_w=_log_w(0.1), learned=True)
    assert float(got[LW].abs().max()) > 0
    e = (got[LW].double().cpu() - g64[LW]).abs().max().item()
    e32 = max((g32[LW].double() - g64[LW]).abs().max().item(), (g32d[LW].double() - g64[LW]).abs().max().item())
    print(f"norm learned weights: edge_log_weight grad err {e:.3e}, fp32 reference err {e32:.3e}, "
          f"scale {g64[LW].abs().max().item():.3e}")
    assert_close(lg, o32, what="learned weights logits")
    assert_grads_match_truth({LW: got[LW]}, {LW: g32[LW]}, {LW: g64[LW]}, ref32={LW: g32d[LW]})
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_norm_general_widths_vs_oracle():
    """(sensor_hidden, node_hidden) = (48, 40), 3 layers, B = 4: _forward_general applies self.norms
    with stock torch; logits within RTOL of the fp32 pre-norm oracle."""
    kw = dict(sensor_hidden=48, node_hidden=40)
    sd = _random_sd(3, 11, **kw)
    r, tf, lab = _batch(4, seed=12)
    o32, *_ = _oracle(sd, r, tf, torch.float32, "cpu", 3, lab=lab, kw=kw)
    m = _detector(sd, 3, **kw)
    assert not m._widths_tiled()
    with torch.no_grad():
        lg = m(r.to(DEV), tf.to(DEV))
        plain = _detector(sd, 3, norm="none", **kw)(r.to(DEV), tf.to(DEV))
    assert_close(lg, o32, what="logits (48, 40)")
    assert (lg - plain).abs().max().item() > 100 * RTOL * o32.abs().max().item()


# ----------------------------------------------------------------------------- 3. train mode, the default
def test_norm_train_mode_on_the_kernels_masks():
    """Train mode, p = 0.1, 2 layers, B = 20, one fixed seed: two forwards are bit-identical, and the
    logits and every gradient match the oracle evaluated on the kernels' own keep decisions (node
    init, every branch's fmask, both heads), each kept unit scaled by 1 / (1 - p)."""
    from models import library
    orig = _fixed_seed(987654321)
    try:
        m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(20, 2, train_p=0.1)
        with torch.no_grad():
            r, tf, _ = (t.to(DEV) for t in _batch(20))
            m.capture = None
            again = m(r, tf)
    finally:
        library.seed_tensor = orig
    assert torch.equal(again, lg.detach())
    assert_close(lg, o32, what="train-mode logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


@pytest.mark.parametrize("B", [3, 16])
def test_norm_train_mode_with_learned_edge_weights(B):
    """Train mode, p = 0.1, 3 layers, learned edge weights, one fixed seed; B = 3 (fewer windows than
    a tile) and 16: dropout's rescale and the edge-weight gradient together (every layer's
    lg_sddmm_nm on the carried gradient, xn_l and the layer's own bits, scaled by 1 / (1 - p)).
    The bars of test_norm_train_mode_on_the_kernels_masks and test_norm_with_learned_edge_weights_grad."""
    from models import library
    orig = _fixed_seed(987654321)
    try:
        m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(B, 3, log_w=_log_w(0.1), learned=True, train_p=0.1)
    finally:
        library.seed_tensor = orig
    assert float(got[LW].abs().max()) > 0
    assert_close(lg, o32, what="train-mode logits, learned weights")
    assert_grads_match_truth({LW: got[LW]}, {LW: g32[LW]}, {LW: g64[LW]}, ref32={LW: g32d[LW]})
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_norm_none_is_the_skip_model():
    """LeakDetector(skip="residual", norm="none") gives logits torch.equal to
    LeakDetector(skip="residual"); norm="layer" with the same weights moves them by far more than RTOL."""
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    sd = _random_sd(4)
    r, tf, _ = (t.to(DEV) for t in _batch(20))
    outs = []
    for kw in ({}, {"norm": "none"}):
        m = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=4, skip="residual", **kw).to(DEV).eval()
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("norms.")})
        assert not hasattr(m, "norms")
        with torch.no_grad():
            outs.append(m(r, tf))
    assert torch.equal(outs[0], outs[1])
    with torch.no_grad():
        ln = _detector(sd, 4)(r, tf)
    assert (ln - outs[0]).abs().max().item() > 100 * RTOL * outs[0].abs().max().item()


# ----------------------------------------------------------------------------- 4. captured step
def test_captured_step_with_norm_matches_eager():
    """A 4-layer pre-norm model at B = 32, dropout 0: warm-up + replays of a CapturedTrainStep (3
    steps in all after the warm-up pair) equal the eager steps (tests/test_graph_step.py's bars)."""
    from models import library
    from models.detector import LeakDetector
    from models.graph_step import CapturedTrainStep
    sensors, pipes = lta_ids()
    torch.manual_seed(0)
    m1 = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=4, dropout=0.0, skip="residual", norm="layer").to(DEV).train()
    m2 = copy.deepcopy(m1)
    r, tf, lab = (t.to(DEV) for t in _batch(32, seed=1))
    mk = lambda m: torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, fused=True, capturable=True)  # noqa: E731
    o1, o2 = mk(m1), mk(m2)

    def eager():
        o1.zero_grad(set_to_none=True)
        loss = F.cross_entropy(m1(r, tf), lab)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m1.parameters(), 1.0)
        o1.step()
        return loss

    step = CapturedTrainStep(m2, F.cross_entropy, o2, (r, tf), lab, clip=1.0, warmup=2)
    for _ in range(2):
        eager()
    for _ in range(3):
        l1, l2 = eager(), step()
    torch.cuda.synchronize()
    assert_close(l2, l1, rtol=1e-6, what="loss")
    for (n, a), b in zip(m2.named_parameters(), m1.parameters()):
        assert bool(torch.isfinite(a).all()), n
        assert_close(a, b, rtol=1e-5, what=n)
    moved = [n for n, p in m2.named_parameters() if n.startswith("norms.") and n.endswith("weight")
             and not torch.equal(p, torch.ones_like(p))]
    assert len(moved) == 5  # every norm trains
    word = ctypes.c_uint32(0)
    assert library.load_library().lg_spin_errors(ctypes.byref(word), 0) == 0 and word.value == 0


# ----------------------------------------------------------------------------- 5. opcheck
@pytest.mark.parametrize("B", [3, 16])
def test_opcheck_gnn_trunk_norm(B):
    """gnn_trunk_norm, three layers, with dropout and with edge_w requiring grad."""
    m = _detector(_random_sd(3), 3, edge_weight=_log_w().exp(), learn_edge_weight=True)
    g, inc, slot, sidx, live, nons = m._device_state(DEV)
    seed = torch.tensor([12345], dtype=torch.long)
    h_s = torch.randn(B, 29, 64, device=DEV, requires_grad=True)
    Wn = torch.randn(64, 65, device=DEV).div_(8).requires_grad_(True)
    nb = torch.randn(64, device=DEV, requires_grad=True)
    wts = [c.lin.weight.detach().clone().requires_grad_(True) for c in m.convs]
    bs = [c.bias.detach().clone().normal_(0, 0.1).requires_grad_(True) for c in m.convs]
    gms = [n.weight.detach().clone().requires_grad_(True) for n in m.norms]
    bts = [n.bias.detach().clone().requires_grad_(True) for n in m.norms]
    edge_w = g.w.detach().clone().requires_grad_(True)
    args = (h_s, Wn, nb, wts, bs, gms, bts, slot, sidx, nons, live, g.nodetab, g.pairs, g.rowptr, g.col, g.nodetab_t,
            g.pairs_t, 0.1, EPS, seed, edge_w)
    torch.library.opcheck(torch.ops.leakgnn.gnn_trunk_norm.default, args, {},
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                      "test_aot_dispatch_dynamic"))
    out = torch.ops.leakgnn.gnn_trunk_norm(*args)
    nmask = 661 * ((B + 15) // 16) * 64
    assert len(out) == 2 * 3 + 4 and out[-1].numel() == 3 * nmask and tuple(out[-2].shape) == (4, 661 * B, 2)
    # the heads' input is the last norm of the residual stream, which is the sum of the branches
    assert_close(out[0], F.layer_norm(out[4], (64,), gms[3], bts[3], EPS), what="xn_L")
