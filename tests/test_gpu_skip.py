"""Residual trunk on the GPU: the two skip kernels against the plain ones bit for bit, the skip
detector against a skip restatement of the oracle (eval parity at 2, 4 and 12 layers, fixed and
learned edge weights, the general-width path), train-mode masks, the default's guard, a captured
training step and opcheck of gnn_trunk(skip=True).

The oracle is a test-local subclass of oracle/detector_ref.LeakDetectorRef whose layer loop is
x = x + dropout(relu(conv(x))); it keeps relu_masks and trace.  Under the skip [x_{l+1} > 0] is no
longer a layer's ReLU mask, so the kink decisions come from LeakDetector.capture["fmask"]."""
from __future__ import annotations

import copy
import ctypes
import functools

import pytest
import torch

from helpers import (LTA_INP, RTOL, assert_close, assert_grads_match_truth, check_relu_ties, hip_relu_masks,
                     lta_ids)
from test_gpu_edge_weight import conv_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LW = "edge_log_weight"


# ----------------------------------------------------------------------------- 1. the kernels alone
def _hub_graph(N: int, seed: int) -> torch.Tensor:
    """(2, E) edges of a small random graph: node 0 a hub of in- and out-degree 12 (rows past the
    six inline pairs of a node-table record, in the forward and the transposed CSR), node 1 with
    no edge but its fill loop."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(2, N, (2 * N,), generator=g)
    dst = torch.randint(2, N, (2 * N,), generator=g)
    hub = torch.randperm(N - 2, generator=g)[:12] + 2
    z = torch.zeros(12, dtype=torch.long)
    return torch.stack([torch.cat([src, hub, z]), torch.cat([dst, z, hub])])


@functools.lru_cache(maxsize=None)
def _kernel_graph():
    from models import ops
    N = 41
    gph = ops.GCNGraph.build(_hub_graph(N, 5), N, DEV, add_self_loops=True, normalize=True)
    rp, rpt = gph.rowptr.cpu().long(), gph.rowptr_t.cpu().long()
    deg, degt = rp[1:] - rp[:-1], rpt[1:] - rpt[:-1]
    assert int(deg[0]) > 6 and int(degt[0]) > 6 and int(deg[1]) == 1 and int(degt[1]) == 1
    return gph, N


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B", [16, 20, 48])
@pytest.mark.parametrize("D", [32, 64])
def test_skip_kernels_equal_plain_plus_identity(D, B, p):
    """lg_gcn_fwd_nm_skip / lg_gcn_bwd_nm_skip against lg_gcn_fwd_nm_bits / lg_gcn_bwd_nm_bits, which
    are pinned to their own oracles elsewhere.  B = 16 one full tile per node, 20 a ragged tile, 48
    several tiles per producer; p = 0.1 under a fixed seed and salt.  Everything is torch.equal:
    the skip is one fp32 add after the plain arithmetic.
      forward : y == x + y_plain (torch fp32 sum), ymask == the plain call's ymask ([f > 0]);
      backward: MASK_IN on those bits; dW, db identical; dx == dx_plain + dy without MASK_OUT and
                (dx_plain_unmasked + dy) * scale_out * [x > 0] with it; the same with node_slot /
                dnode_bias (no sensor-rows shortcut) for dx, dW, db."""
    from models import _native as nat
    from models._native import ptr
    gph, N = _kernel_graph()
    lib = nat.load_library()
    st = torch.cuda.current_stream(DEV).cuda_stream
    gen = torch.Generator().manual_seed(100 * D + B)
    x = torch.randn(N, B, D, generator=gen).to(DEV)  # both signs: MASK_OUT's [x > 0] drops about half
    W = (torch.randn(D, D, generator=gen) / D ** 0.5).to(DEV)
    b = (0.1 * torch.randn(D, generator=gen)).to(DEV)
    dy = torch.randn(N, B, D, generator=gen).to(DEV)
    nmask = N * ((B + 15) // 16) * 64
    flags = nat.LG_F_BIAS | nat.LG_F_RELU | (nat.LG_F_DROPOUT if p > 0 else 0)
    seed, salt = 0x1234ABCD5, 3
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0

    def fwd(fn, extra=0, mask=True):
        y = torch.full((N, B, D), float("nan"), device=DEV)
        m = torch.zeros(nmask, dtype=torch.int16, device=DEV)
        rc = getattr(lib, fn)(ptr(gph.nodetab), ptr(gph.pairs), ptr(x), ptr(W), ptr(b), ptr(y), B, N, D, gph.col.numel(),
                              flags | extra, p, seed, salt, st, ptr(m) if mask else None)
        return rc, y, m

    for extra in (0, nat.LG_F_BF16X3):  # the f16x2 transform (default) and the 3-way bf16 split
        rc0, y_plain, m_plain = fwd("lg_gcn_fwd_nm_bits", extra)
        rc1, y_skip, m_skip = fwd("lg_gcn_fwd_nm_skip", extra)
        assert rc0 == 0 and rc1 == 0
        assert torch.equal(m_skip, m_plain)
        assert torch.equal(y_skip, x + y_plain)
        assert int((y_plain > 0).sum()) > 0 and not torch.equal(y_skip, y_plain)
    assert fwd("lg_gcn_fwd_nm_skip", mask=False)[0] == -1  # ymask is required
    for bad in (nat.LG_F_BF16, nat.LG_F_NM3, nat.LG_F_F32_MFMA):
        assert fwd("lg_gcn_fwd_nm_skip", bad)[0] == -2

    ws = torch.empty(int(lib.lg_gcn_bwd_nm_workspace_bytes(D)), dtype=torch.uint8, device=DEV)
    slot = torch.full((N,), -1, dtype=torch.int32)
    slot[torch.arange(0, N, 5)] = torch.arange(len(range(0, N, 5)), dtype=torch.int32)
    slot = slot.to(DEV)

    def bwd(fn, fl, with_slot=False, mask=True):
        dx = torch.full((N, B, D), float("nan"), device=DEV)
        dW, db, dnb = torch.empty(D, D, device=DEV), torch.empty(D, device=DEV), torch.empty(D, device=DEV)
        rc = getattr(lib, fn)(ptr(gph.nodetab_t), ptr(gph.pairs_t), ptr(dy), None, ptr(x), ptr(W), ptr(dx), ptr(dW),
                              ptr(db), ptr(slot) if with_slot else None, ptr(dnb) if with_slot else None, B, N, D, fl,
                              scale, scale, ptr(ws), ws.numel(), st, ptr(m_plain) if mask else None)
        torch.cuda.synchronize()
        return rc, dx, dW, db, dnb

    MI, MO = nat.LG_F_MASK_IN, nat.LG_F_MASK_OUT
    for extra in (0, nat.LG_F_BF16X3):
        rc, dx_p, dW_p, db_p, _ = bwd("lg_gcn_bwd_nm_bits", MI | extra)
        assert rc == 0
        for with_slot in (False, True):
            rc, dx_s, dW_s, db_s, _ = bwd("lg_gcn_bwd_nm_skip", MI | extra, with_slot)
            assert rc == 0
            assert torch.equal(dW_s, dW_p) and torch.equal(db_s, db_p)
            assert torch.equal(dx_s, dx_p + dy)
            rc, dx_m, dW_m, db_m, dnb = bwd("lg_gcn_bwd_nm_skip", MI | MO | extra, with_slot)
            assert rc == 0
            want = torch.where(x > 0, (dx_p + dy) * scale, torch.zeros_like(x))
            assert torch.equal(dx_m, want)
            assert torch.equal(dW_m, dW_p) and torch.equal(db_m, db_p)
            if with_slot:  # dnode_bias: the summed, masked dx over the rows of the nodes without a sensor
                ref = want[slot < 0].double().sum(dim=(0, 1))
                err = (dnb.double() - ref).abs().max().item()
                # an fp32 sum of n terms in any order is within (n - 1) * 2^-24 * sum|terms| of the exact sum
                rows = want[slot < 0]
                lim = rows.numel() / D * 2.0 ** -24 * rows.abs().double().sum(dim=(0, 1)).max().item()
                print(f"D={D} B={B} p={p}: dnode_bias err {err:.3e} (bound {lim:.3e})")
                assert err <= lim
    assert bwd("lg_gcn_bwd_nm_skip", MO)[0] == -1               # MASK_IN is required
    assert bwd("lg_gcn_bwd_nm_skip", MI, mask=False)[0] == -1   # and its bits
    assert bwd("lg_gcn_bwd_nm_skip", MI | nat.LG_F_BF16)[0] == -2


# ----------------------------------------------------------------------------- the skip oracle
@functools.lru_cache(maxsize=None)
def _skip_ref_cls():
    from oracle import gcn_ref, graph_ref
    from oracle.detector_ref import LeakDetectorRef

    class SkipRef(LeakDetectorRef):
        """LeakDetectorRef.forward with the layer loop x = x + dropout(relu(conv(x)))."""

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
                x = x + self.dropout(self._relu(f"conv{i}", conv(x, ei)))
                self.trace[f"conv{i}"] = x
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

    return SkipRef


@functools.lru_cache(maxsize=None)
def _random_sd(layers: int, seed: int = 41, **kw):
    """A random state dict of the `layers`-layer detector (conv biases off zero); shared, read-only."""
    sensors, pipes = lta_ids()
    torch.manual_seed(seed)
    ref = _skip_ref_cls()(LTA_INP, sensors, pipes, gnn_layers=layers, **kw).eval()
    with torch.no_grad():
        for c in ref.convs:
            c.bias.normal_(0, 0.1)
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _oracle(sd, r, tf, dt, dev, layers, up=None, lab=None, masks=None, log_w=None, kw=None):
    """The skip oracle in eval mode: (logits, parameter grads, pre-activations, upstream gradient).
    log_w: link log-weights (a leaf; its gradient under "edge_log_weight"), the convs then run
    conv_ref (PyG's weighted GCNConv in plain torch) as tests/test_gpu_detector_edge_weight.py does."""
    sensors, pipes = lta_ids()
    mr = _skip_ref_cls()(LTA_INP, sensors, pipes, gnn_layers=layers, **(kw or {})).eval()
    mr.load_state_dict(sd)
    mr = mr.to(dt).to(dev)
    mr.sensor_encoder.gru.train()  # MIOpen's RNN backward needs training mode (1 layer: no dropout)
    mr.relu_masks = masks or {}
    lw = None
    if log_w is not None:
        lw = log_w.detach().to(dt).to(dev).requires_grad_(True)
        ew = lw.exp().repeat_interleave(2).repeat(r.shape[0])  # column b * E + e is edge e
        for c in mr.convs:
            c.forward = lambda x, ei, c=c: conv_ref(x, ei, ew, c.lin.weight, c.bias, x.shape[0])
    out = mr(r.to(dt).to(dev), tf.to(dt).to(dev))
    if up is None:
        lo = out.detach().requires_grad_(True)
        torch.nn.functional.cross_entropy(lo, lab).backward()
        up = lo.grad.clone()
    out.backward(up.to(dt).to(dev))
    pre = {k[len("pre_"):]: v.detach() for k, v in mr.trace.items() if k.startswith("pre_")}
    grads = {n: p.grad.detach().cpu() for n, p in mr.named_parameters()}
    if lw is not None:
        grads[LW] = lw.grad.detach().cpu()
    return out.detach().cpu(), grads, pre, up


def _batch(B, seed=42):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 36, 29, generator=gen), torch.randn(B, 36, 9, generator=gen),
            torch.randint(0, 765, (B,), generator=gen))


def _log_w(noise: float = 0.0):
    from models.utils import link_edge_weights
    lw = link_edge_weights(LTA_INP, ("PIPES", "PUMPS", "VALVES"), "inv_length").log()
    if noise:
        lw = lw + noise * torch.randn(lw.shape, generator=torch.Generator().manual_seed(3))
    return lw


def _detector(sd, layers, skip="residual", **kw):
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    m = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=layers, skip=skip, **kw).to(DEV).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"edge_weight", LW}
    return m


def _skip_masks(m, B):
    """The kink decisions of a captured skip forward in the oracle's shapes: helpers.hip_relu_masks
    for the node init, the heads and |h_u - h_v|, the conv sites from capture["fmask"]."""
    N, P = len(m.node_names), len(m.pipe_ids)
    cap = m.capture
    assert cap["node_major"] and len(cap["fmask"]) == len(m.convs)
    masks = hip_relu_masks(cap, B, N, P, m.pipe_ends)
    for l, fm in enumerate(cap["fmask"]):
        assert fm.dtype == torch.bool and tuple(fm.shape) == tuple(cap["xs"][l + 1].shape)
        masks[f"conv{l}"] = fm.permute(1, 0, 2).reshape(B, N, -1).cpu()
    return masks


def _parity(B, layers, log_w=None, learned=False, skip="residual"):
    sd = _random_sd(layers)
    r, tf, lab = _batch(B)
    _, _, pre64, up = _oracle(sd, r, tf, torch.float64, "cpu", layers, lab=lab, log_w=log_w)
    kw = dict(edge_weight=log_w.exp(), learn_edge_weight=learned) if log_w is not None else {}
    m = _detector(sd, layers, skip=skip, **kw)
    m.capture = {}
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.float().to(DEV))
    # (a plain model keeps no fmask: without layers hip_relu_masks alone names every kink)
    masks = (_skip_masks(m, B) if skip == "residual" else
             hip_relu_masks(m.capture, B, len(m.node_names), len(m.pipe_ids), m.pipe_ends))
    ties = check_relu_ties(pre64, masks)
    o64, g64, _, _ = _oracle(sd, r, tf, torch.float64, "cpu", layers, up=up, masks=masks, log_w=log_w)
    o32, g32, _, _ = _oracle(sd, r, tf, torch.float32, "cpu", layers, up=up, masks=masks, log_w=log_w)
    _, g32d, _, _ = _oracle(sd, r, tf, torch.float32, DEV, layers, up=up, masks=masks, log_w=log_w)
    got = {n: p.grad for n, p in m.named_parameters()}
    if not learned:
        for d in (g64, g32, g32d):
            d.pop(LW, None)
    scale = o64.abs().max().item()
    e_gpu = (lg.detach().double().cpu() - o64).abs().max().item()
    e_ref = (o32.double() - o64).abs().max().item()
    print(f"skip L={layers} B={B} weighted={log_w is not None} learned={learned}: logits err vs fp64 {e_gpu:.3e} "
          f"(fp32 oracle's own {e_ref:.3e}, scale {scale:.3e}, RTOL x scale {RTOL * scale:.3e}), "
          f"vs fp32 oracle {(lg.detach().double().cpu() - o32.double()).abs().max().item():.3e}, ties {ties}")
    return m, lg, (o32, o64, e_gpu, e_ref, scale), (got, g32, g64, g32d)


# ----------------------------------------------------------------------------- 2. eval parity
@pytest.mark.parametrize("B", [4, 20, 32])
@pytest.mark.parametrize("layers", [2, 4])
def test_skip_detector_vs_oracle(layers, B):
    """L-TOWN-A, eval, random weights; B = 4 (node-major below 16 windows: the skip takes that
    layout at every B), 20 a ragged tile, 32 two tiles per node.  Logits within RTOL of the fp32
    skip oracle, every parameter gradient against the fp64 skip oracle on the HIP path's side of
    every kink (assert_grads_match_truth)."""
    m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(B, layers)
    m.capture = None  # (a capture alone already takes the unfused route)
    assert not m._fused_encoder(torch.zeros(B, 36, 29, device=DEV), None, B, 661, 64, True)
    assert_close(lg, o32, what=f"L={layers} B={B} logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_skip_detector_12_layers_vs_oracle():
    """gnn_layers = 12, B = 20: every node within reach of a sensor.  The error of 12 chained f16x2
    transforms was not known beforehand, so the logits bar is the yardstick rule: the GPU's error
    against the fp64 oracle within 4x the fp32 CPU oracle's own error against fp64, or within RTOL
    of the logits' scale.  Gradients under assert_grads_match_truth as at 2 and 4 layers.
    Measured on the MI355X: GPU error 2.8e-6, the fp32 CPU oracle's own 3.5e-6, scale 6.9 (RTOL x
    scale 6.9e-5), 4 kink ties."""
    m, lg, (o32, o64, e_gpu, e_ref, scale), (got, g32, g64, g32d) = _parity(20, 12)
    assert e_gpu <= max(4 * e_ref, RTOL * scale), (e_gpu, e_ref, scale)
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


@pytest.mark.parametrize("skip,B", [("residual", 3), ("residual", 16), ("none", 3), ("none", 16)])
def test_no_layers_vs_oracle(skip, B):
    """gnn_layers = 0: the heads read the node init, and gnn_trunk_backward applies the node init's
    mask and sums the non-sensor rows' bias gradient itself (no layer-0 launch does).  Node-major
    under the skip at both B and for the plain model at B = 16, window-major for the plain model
    at B = 3.  Without layers the skip oracle is the plain oracle.  The bars of
    test_skip_detector_vs_oracle."""
    m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(B, 0, skip=skip)
    assert len(m.convs) == 0 and m.capture["node_major"] == (skip == "residual" or B >= 16)
    assert_close(lg, o32, what=f"L=0 skip={skip} B={B} logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_skip_with_fixed_edge_weights_vs_weighted_oracle():
    """edge_weight = inv_length links (a buffer) with the skip, 4 layers, B = 20: logits within RTOL
    of the weighted skip oracle; gradients under the same bar."""
    m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(20, 4, log_w=_log_w())
    assert "edge_weight" in m.state_dict()
    assert_close(lg, o32, what="fixed weights logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_skip_with_learned_edge_weights_grad():
    """learn_edge_weight with the skip, 4 layers, B = 20: every layer's lg_sddmm_nm reads its own
    branch bits; edge_log_weight.grad (and the rest) under the yardstick rule against fp64."""
    m, lg, (o32, *_), (got, g32, g64, g32d) = _parity(20, 4, log_w=_log_w(0.1), learned=True)
    assert float(got[LW].abs().max()) > 0
    e = (got[LW].double().cpu() - g64[LW]).abs().max().item()
    e32 = max((g32[LW].double() - g64[LW]).abs().max().item(), (g32d[LW].double() - g64[LW]).abs().max().item())
    print(f"skip learned weights: edge_log_weight grad err {e:.3e}, fp32 reference err {e32:.3e}, "
          f"scale {g64[LW].abs().max().item():.3e}")
    assert_close(lg, o32, what="learned weights logits")
    assert_grads_match_truth({LW: got[LW]}, {LW: g32[LW]}, {LW: g64[LW]}, ref32={LW: g32d[LW]})
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)


def test_skip_general_widths_vs_oracle():
    """(sensor_hidden, node_hidden) = (48, 40), 3 layers, B = 4: _forward_general's one torch add per
    layer, logits within RTOL of the fp32 skip oracle."""
    kw = dict(sensor_hidden=48, node_hidden=40)
    sd = _random_sd(3, 11, **kw)
    r, tf, lab = _batch(4, seed=12)
    o32, *_ = _oracle(sd, r, tf, torch.float32, "cpu", 3, lab=lab, kw=kw)
    m = _detector(sd, 3, **kw)
    assert not m._widths_tiled()
    with torch.no_grad():
        lg = m(r.to(DEV), tf.to(DEV))
        plain = _detector(sd, 3, skip="none", **kw)(r.to(DEV), tf.to(DEV))
    assert_close(lg, o32, what="logits (48, 40)")
    assert (lg - plain).abs().max().item() > 100 * RTOL * o32.abs().max().item()


# ----------------------------------------------------------------------------- 3. train mode, the default
def _fixed_seed(value: int):
    from models import library
    orig = library.seed_tensor
    library.seed_tensor = lambda device=None: torch.tensor([value], dtype=torch.long)
    return orig


def test_skip_train_mode_masks():
    """Train mode, p = 0.1, B = 32: two forwards with one seed are bit-identical; the dropout
    streams and salts are the plain trunk's, so the skip model's fmask[0] equals the plain model's
    layer-0 mask [x_1 > 0] for the same seed and weights (dense node init on both: layer 0's inputs
    and kernel arithmetic coincide), while deeper masks differ (their inputs do)."""
    from models import library
    sd = _random_sd(3)
    r, tf, _ = (t.to(DEV) for t in _batch(32))
    ms, mp = _detector(sd, 3, dropout=0.1).train(), _detector(sd, 3, skip="none", dropout=0.1).train()
    mp.compress_x0 = False
    orig = _fixed_seed(987654321)
    try:
        with torch.no_grad():
            a = ms(r, tf)
            b = ms(r, tf)
            ms.capture, mp.capture = {}, {}
            c = ms(r, tf)
            mp(r, tf)
    finally:
        library.seed_tensor = orig
    assert torch.equal(a, b) and torch.equal(a, c)
    fm, xs_s, xs_p = ms.capture["fmask"], ms.capture["xs"], mp.capture["xs"]
    assert torch.equal(xs_s[0], xs_p[0])
    assert torch.equal(fm[0], xs_p[1] > 0)
    assert torch.equal(xs_s[1], xs_p[0] + xs_p[1])
    keep = fm[0].float().mean().item()
    assert 0.2 < keep < 0.9 * 0.9 + 0.02  # relu and a 0.9 keep rate
    assert not torch.equal(fm[1], xs_p[2] > 0)
    # the bits are the branch's [f > 0], not [x > 0]: x_2 moves exactly where a unit was kept
    assert not torch.equal(fm[1], xs_s[2] > 0)
    assert bool((xs_s[2] == xs_s[1])[~fm[1]].all())


def test_skip_changes_the_output_and_default_is_untouched():
    """Same weights: the skip model's logits differ from the plain model's by far more than RTOL;
    the plain model built with skip="none" passed explicitly gives bit-identical logits and gradients
    to one built without the argument (B = 32: the fused encoder_trunk op on both)."""
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    sd = _random_sd(2)
    r, tf, lab = (t.to(DEV) for t in _batch(32))
    outs = []
    for kw in ({}, {"skip": "none"}):
        m = LeakDetector(LTA_INP, sensors, pipes, **kw).to(DEV).eval()
        m.load_state_dict(sd)
        assert m._fused_encoder(r, tf, 32, 661, 64, True)
        lg = m(r, tf)
        torch.nn.functional.cross_entropy(lg, lab).backward()
        outs.append((lg.detach(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    with torch.no_grad():
        sk = _detector(sd, 2)(r, tf)
    diff = (sk - outs[0][0]).abs().max().item()
    print(f"skip vs plain logits: max abs diff {diff:.3e} (scale {outs[0][0].abs().max().item():.3e})")
    assert diff > 100 * RTOL * outs[0][0].abs().max().item()


# ----------------------------------------------------------------------------- 4. captured step
def test_captured_step_with_skip_matches_eager():
    """A 4-layer skip model at B = 32, dropout 0: warm-up + 2 replays of a CapturedTrainStep equal
    warm-up + 2 eager steps (tests/test_graph_step.py's bars: loss 1e-6, parameters 1e-5)."""
    from models import library
    from models.detector import LeakDetector
    from models.graph_step import CapturedTrainStep
    sensors, pipes = lta_ids()
    torch.manual_seed(0)
    m1 = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=4, dropout=0.0, skip="residual").to(DEV).train()
    m2 = copy.deepcopy(m1)
    r, tf, lab = (t.to(DEV) for t in _batch(32, seed=1))
    mk = lambda m: torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, fused=True, capturable=True)  # noqa: E731
    o1, o2 = mk(m1), mk(m2)

    def eager():
        o1.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(m1(r, tf), lab)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m1.parameters(), 1.0)
        o1.step()
        return loss

    step = CapturedTrainStep(m2, torch.nn.functional.cross_entropy, o2, (r, tf), lab, clip=1.0, warmup=2)
    for _ in range(2):
        eager()
    for _ in range(2):
        l1, l2 = eager(), step()
    torch.cuda.synchronize()
    assert_close(l2, l1, rtol=1e-6, what="loss")
    for (n, a), b in zip(m2.named_parameters(), m1.parameters()):
        assert bool(torch.isfinite(a).all()), n
        assert_close(a, b, rtol=1e-5, what=n)
    word = ctypes.c_uint32(0)
    assert library.load_library().lg_spin_errors(ctypes.byref(word), 0) == 0 and word.value == 0


# ----------------------------------------------------------------------------- 5. opcheck
@pytest.mark.parametrize("B", [3, 16])
def test_opcheck_gnn_trunk_skip(B):
    """gnn_trunk(skip=True), node-major at both B (3: fewer windows than a tile), three layers, with
    dropout and with edge_w requiring grad (one mask per layer saved and read back)."""
    m = _detector(_random_sd(3), 3, edge_weight=_log_w().exp(), learn_edge_weight=True)
    g, inc, slot, sidx, live, nons = m._device_state(DEV)
    seed = torch.tensor([12345], dtype=torch.long)
    h_s = torch.randn(B, 29, 64, device=DEV, requires_grad=True)
    Wn = torch.randn(64, 65, device=DEV).div_(8).requires_grad_(True)
    nb = torch.randn(64, device=DEV, requires_grad=True)
    wts = [c.lin.weight.detach().clone().requires_grad_(True) for c in m.convs]
    bs = [c.bias.detach().clone().normal_(0, 0.1).requires_grad_(True) for c in m.convs]
    edge_w = g.w.detach().clone().requires_grad_(True)
    args = (h_s, Wn, nb, wts, bs, slot, sidx, nons, live, g.nodetab, g.pairs, g.rowptr, g.col, g.w, g.nodetab_t,
            g.pairs_t, g.rowptr_t, g.col_t, g.w_t, 0.1, True, seed, None, None, None, edge_w)
    torch.library.opcheck(torch.ops.leakgnn.gnn_trunk.default, args, {"bf16": False, "skip": True},
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                      "test_aot_dispatch_dynamic"))
    out = torch.ops.leakgnn.gnn_trunk(*args, skip=True)
    nmask = 661 * ((B + 15) // 16) * 64
    assert out[-2].numel() == 3 * nmask and out[-1].numel() == 0  # a mask per layer, x_0 not compressed
