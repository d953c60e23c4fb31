"""LeakDetector edge weights on the GPU: the lg_sddmm_nm kernel alone, fixed and learned weights
against a weighted restatement of the oracle detector, the in-place table refresh, a captured
training step, and opcheck of the trunk ops with edge_w.

The weighted oracle is oracle/detector_ref.LeakDetectorRef with each convs[i].forward replaced
ON THE INSTANCE by conv_ref of tests/test_gpu_edge_weight.py (PyG's weighted GCNConv in plain
torch), called with the batched weights ew.repeat(B); the link log-weights are a leaf."""
from __future__ import annotations

import copy

import pytest
import torch

from helpers import (LTA_INP, RTOL, assert_close, assert_grads_match_truth, check_relu_ties, hip_relu_masks,
                     lta_ids)
from test_gpu_configs import _random_ref
from test_gpu_edge_weight import conv_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LW = "edge_log_weight"


# ----------------------------------------------------------------------------- 1. the kernel alone
def _hub_graph(N: int, seed: int):
    """(2, E) edges of a random graph with node 0 a hub of in-degree 40 (rows past the six inline
    slots), node 1 with no edge but its fill loop, and an input self-loop edge at node 2."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(2, N, (3 * N,), generator=g)
    dst = torch.randint(2, N, (3 * N,), generator=g)
    hub_src = torch.randperm(N - 2, generator=g)[:40] + 2
    ei = torch.stack([torch.cat([src, hub_src, torch.tensor([2])]),
                      torch.cat([dst, torch.zeros(40, dtype=torch.long), torch.tensor([2])])])
    return ei


def _mask_bits(y: torch.Tensor) -> torch.Tensor:
    """[y > 0] of y (N, B, D) as lg_gcn_fwd_nm_bits' words (include/leakgnn.h): per node and
    16-window tile 64 lanes, bit 4k + i of lane l = row 16g + (64 / (D/4)) k + l // (D/4),
    channel 4 (l % (D/4)) + i."""
    N, B, D = y.shape
    T, lpr = (B + 15) // 16, D // 4
    rpp = 64 // lpr
    yp = torch.zeros(N, T * 16, D, dtype=torch.bool)
    yp[:, :B] = y.cpu() > 0
    yp = yp.view(N, T, 16 // rpp, rpp, lpr, 4)          # [n][g][k][l // lpr][l % lpr][i]
    bit = (1 << (4 * torch.arange(16 // rpp).view(-1, 1) + torch.arange(4).view(1, -1))).long()  # [k][i]
    words = (yp.permute(0, 1, 3, 4, 2, 5).long() * bit).sum(dim=(-1, -2))                        # [n][g][lr][lc]
    words = words.reshape(-1)
    return torch.where(words >= 2 ** 15, words - 2 ** 16, words).to(torch.int16).to(DEV)  # uint16 bits


def _G_formula(rowptr, col, dy, y, W, x, scale, mask):
    """The issue's formula in dy's dtype, on dy's device: da by a masked GEMM, then per slot."""
    N, B, D = dy.shape
    dz = dy * (y > 0) * scale if mask else dy
    da = (dz.reshape(N * B, D) @ W).view(N, B * D)
    rows = torch.repeat_interleave(torch.arange(N, device=dy.device), (rowptr[1:] - rowptr[:-1]).long())
    nnz = int(rowptr[-1])
    G = torch.zeros(col.numel(), dtype=dy.dtype, device=dy.device)
    G[:nnz] = (da[rows] * x.reshape(N, B * D)[col[:nnz].long()]).sum(dim=1)
    return G


@pytest.mark.parametrize("scale", [1.0, 1.0 / 0.9])
@pytest.mark.parametrize("B", [16, 20, 48])
@pytest.mark.parametrize("D", [32, 64])
def test_sddmm_nm_kernel(D, B, scale):
    """library.sddmm_nm against the fp64 formula on the CPU; yardstick: the same formula as fp32
    torch on the GPU (masked GEMM, then lg_sddmm_cols on the [N][B * D] view).  Bar: max abs error
    within 4x the yardstick's, or within RTOL of max|G| (assert_grads_match_truth's rule).  Mask
    from y and from the bit words, and no mask (the inner layers' dz = dy); slots past rowptr[N]
    exactly 0; two runs bit-identical; a short workspace is LG_EINVAL."""
    from models import library, ops
    from models._native import LeakGNNError
    N = 300
    ei = _hub_graph(N, 5)
    gph = ops.GCNGraph.build(ei, N, DEV, add_self_loops=True, normalize=True)
    rp = gph.rowptr.cpu().long()
    deg = rp[1:] - rp[:-1]
    assert int(deg[0]) == 41 and int(deg[1]) == 1 and int(rp[-1]) < gph.col.numel()  # hub, lone loop, spare slots
    gen = torch.Generator().manual_seed(7 + D + B)
    dy = torch.randn(N, B, D, generator=gen)
    y = torch.randn(N, B, D, generator=gen).relu()
    x = torch.randn(N, B, D, generator=gen).relu()
    W = torch.randn(D, D, generator=gen) / D ** 0.5
    dyd, yd, xd, Wd = (t.to(DEV) for t in (dy, y, x, W))
    bits = _mask_bits(y)
    for mask in (True, False):
        truth = _G_formula(rp, gph.col.cpu(), dy.double(), y.double(), W.double(), x.double(), scale, mask)
        dz = (dyd * (yd > 0) * scale) if mask else dyd
        yard = torch.ops.leakgnn.sddmm_cols(gph.rowptr, gph.col, (dz.reshape(N * B, D) @ Wd).view(N, B * D),
                                            xd.reshape(N, B * D))
        e_yard = (yard.double().cpu() - truth).abs().max().item()
        lim = max(4 * e_yard, RTOL * truth.abs().max().item())
        runs = [library.sddmm_nm(gph.rowptr, gph.col, dyd, Wd, xd, y=yd, mask_in=mask, scale=scale)]
        if mask:
            runs.append(library.sddmm_nm(gph.rowptr, gph.col, dyd, Wd, xd, ymask=bits, mask_in=True, scale=scale))
        runs.append(library.sddmm_nm(gph.rowptr, gph.col, dyd, Wd, xd, y=yd, mask_in=mask, scale=scale))
        for G in runs:
            err = (G.double().cpu() - truth).abs().max().item()
            print(f"sddmm_nm D={D} B={B} scale={scale:.3f} mask={mask}: err {err:.3e}, yardstick {e_yard:.3e}, "
                  f"max|G| {truth.abs().max().item():.3e}")
            assert err <= lim, (err, lim, e_yard)
            assert bool((G[int(rp[-1]):] == 0).all())
        assert all(torch.equal(runs[0], G) for G in runs[1:])  # y mask == bit mask; run 1 == run 2
    need = int(library.load_library().lg_sddmm_nm_workspace_bytes(B, gph.col.numel()))
    with pytest.raises(LeakGNNError, match=r"code -1"):
        library.sddmm_nm(gph.rowptr, gph.col, dyd, Wd, xd, ws=torch.empty(need - 16, dtype=torch.uint8, device=DEV))


# ----------------------------------------------------------------------------- the weighted oracle
def _oracle(sd, r, tf, dt, dev, log_w, up=None, lab=None, masks=None, kw=None):
    """oracle_run (tests/helpers.py) of the WEIGHTED detector: link weights exp(log_w), log_w a
    leaf in dt.  Returns (logits, grads incl. "edge_log_weight", pre-activations, upstream)."""
    from oracle.detector_ref import LeakDetectorRef
    sensors, pipes = lta_ids()
    mr = LeakDetectorRef(LTA_INP, sensors, pipes, **(kw or {})).eval()
    mr.load_state_dict(sd)
    mr = mr.to(dt).to(dev)
    mr.sensor_encoder.gru.train()  # MIOpen's RNN backward needs training mode (1 layer: no dropout)
    mr.relu_masks = masks or {}
    B = r.shape[0]
    lw = log_w.detach().to(dt).to(dev).requires_grad_(True)
    ew = lw.exp().repeat_interleave(2).repeat(B)  # column b * E + e is edge e
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
    grads[LW] = lw.grad.detach().cpu()
    return out.detach().cpu(), grads, pre, up


def _batch(B, seed=42):
    sensors, pipes = lta_ids()
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 36, 29, generator=gen), torch.randn(B, 36, 9, generator=gen),
            torch.randint(0, len(pipes) + 1, (B,), generator=gen))


def _log_w(noise: float = 0.0):
    from models.utils import link_edge_weights
    lw = link_edge_weights(LTA_INP, ("PIPES", "PUMPS", "VALVES"), "inv_length").log()
    if noise:
        lw = lw + noise * torch.randn(lw.shape, generator=torch.Generator().manual_seed(3))
    return lw


def _detector(sd, log_w, learned, **kw):
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    m = LeakDetector(LTA_INP, sensors, pipes, edge_weight=log_w.exp(), learn_edge_weight=learned, **kw).to(DEV).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"edge_weight", LW}
    return m


def _parity(B, learned):
    """One case of tests 2 and 3: the HIP detector (capture on: separate encoder + gnn_trunk) against
    the weighted oracle, gradients on the HIP path's side of every kink (as
    test_detector_b256_eval_vs_oracle)."""
    sensors, pipes = lta_ids()
    sd = _random_ref(41)
    r, tf, lab = _batch(B)
    lw = _log_w(0.1 if learned else 0.0)
    _, _, pre64, up = _oracle(sd, r, tf, torch.float64, "cpu", lw, lab=lab)
    m = _detector(sd, lw, learned)
    m.capture = {}
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.float().to(DEV))
    masks = hip_relu_masks(m.capture, B, len(m.node_names), len(pipes), m.pipe_ends)
    check_relu_ties(pre64, masks)
    _, g64, _, _ = _oracle(sd, r, tf, torch.float64, "cpu", lw, up=up, masks=masks)
    o32, g32, _, _ = _oracle(sd, r, tf, torch.float32, "cpu", lw, up=up, masks=masks)
    _, g32d, _, _ = _oracle(sd, r, tf, torch.float32, DEV, lw, up=up, masks=masks)
    got = {n: p.grad for n, p in m.named_parameters()}
    if not learned:
        for d in (g64, g32, g32d):
            d.pop(LW)
    e_fwd = (lg.detach().double().cpu() - o32.double()).abs().max().item() / o32.abs().max().item()
    print(f"B={B} learned={learned}: logits rel err {e_fwd:.3e}")
    if learned:
        e = (got[LW].double().cpu() - g64[LW]).abs().max().item()
        e32 = max((g32[LW].double() - g64[LW]).abs().max().item(), (g32d[LW].double() - g64[LW]).abs().max().item())
        print(f"B={B}: edge_log_weight grad err {e:.3e}, fp32 reference err {e32:.3e}, "
              f"scale {g64[LW].abs().max().item():.3e}")
    assert_close(lg, o32, what=f"B={B} logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)
    return m, sd, r, tf, up, lw


# ----------------------------------------------------------------------------- 2. fixed weights
@pytest.mark.parametrize("B", [4, 20, 32])
def test_fixed_weights_vs_weighted_oracle(B):
    """edge_weight = link_edge_weights(inv_length), eval, random weights; B = 4 window-major, 20 a
    ragged node-major tile, 32 two tiles per slot.  Logits within RTOL of the fp32 weighted oracle,
    every parameter gradient against the fp64 weighted oracle under assert_grads_match_truth."""
    m, *_ = _parity(B, learned=False)
    assert m._reweights == 0 and "edge_weight" in m.state_dict()


@pytest.mark.parametrize("B", [4, 32])
def test_unit_weights_equal_unweighted(B):
    """edge_weight = ones gives the unweighted detector's logits within RTOL.  Whether they are
    bit-identical is printed, not asserted: the weighted gcn_norm (lg_graph_build_w) sums the
    degrees as floats of the weights where lg_graph_build counts edges; with unit weights both
    are exact small integers, so identical bits are expected.  Measured on the MI355X: bit-identical
    at B = 4 and at B = 32 (max abs diff 0)."""
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    sd = _random_ref(41)
    r, tf, _ = _batch(B)
    m0 = LeakDetector(LTA_INP, sensors, pipes).to(DEV).eval()
    m0.load_state_dict(sd)
    m1 = _detector(sd, torch.zeros(m0.edge_index_single.size(1) // 2), learned=False)
    with torch.no_grad():
        a, b = m0(r.to(DEV), tf.to(DEV)), m1(r.to(DEV), tf.to(DEV))
    print(f"unit weights B={B}: bit-identical to unweighted: {torch.equal(a, b)}, "
          f"max abs diff {(a - b).abs().max().item():.3e}")
    assert_close(b, a, what="unit weights")


# ----------------------------------------------------------------------------- 3. learned weights
@pytest.mark.parametrize("B", [4, 20, 32])
def test_learned_weights_grad_vs_weighted_oracle(B):
    """edge_log_weight.grad (and every other gradient) against the fp64 weighted oracle's gradient of
    the same leaf, same bar and kink handling; a second identical run gives torch.equal gradients."""
    m, sd, r, tf, up, lw = _parity(B, learned=True)
    g1 = m.edge_log_weight.grad.clone()
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    m.zero_grad(set_to_none=True)
    m(r.to(DEV), tf.to(DEV)).backward(up.float().to(DEV))
    assert torch.equal(m.edge_log_weight.grad, g1)
    assert m._reweights == 0  # built from these weights: nothing to refresh


def test_learned_weights_fused_equals_separate_ops():
    """Node-major B = 32: encoder_trunk (capture None) and gru_encoder + gnn_trunk
    (fuse_encoder=False) give torch.equal logits and edge_log_weight.grad (the pattern of
    test_encoder_trunk_equals_separate_ops)."""
    sd = _random_ref(41)
    r, tf, _ = _batch(32)
    lw = _log_w(0.1)
    up = torch.randn(32, 765, generator=torch.Generator().manual_seed(9)).to(DEV) / 32
    outs = []
    for fuse in (True, False):
        m = _detector(sd, lw, True)
        m.fuse_encoder = fuse
        assert m._fused_encoder(r.to(DEV), tf.to(DEV), 32, 661, 64, True) == fuse
        lg = m(r.to(DEV), tf.to(DEV))
        lg.backward(up)
        outs.append((lg.detach(), m.edge_log_weight.grad.clone(), m.convs[0].lin.weight.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][1].abs().max()) > 0


def test_learned_weights_general_widths():
    """(sensor_hidden, node_hidden) = (48, 40), B = 4: the general path (GCNConv's own weighted
    autograd over the batched weights) carries the gradient to edge_log_weight, which meets the
    same bar (no kink handling: the general path has no capture hook, as in test_gpu_widths.py)."""
    from oracle.detector_ref import LeakDetectorRef
    sensors, pipes = lta_ids()
    kw = dict(sensor_hidden=48, node_hidden=40)
    torch.manual_seed(11)
    ref = LeakDetectorRef(LTA_INP, sensors, pipes, **kw).eval()
    with torch.no_grad():
        for c in ref.convs:
            c.bias.normal_(0, 0.1)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    r, tf, lab = _batch(4, seed=12)
    lw = _log_w(0.1)
    _, g64, _, up = _oracle(sd, r, tf, torch.float64, "cpu", lw, lab=lab, kw=kw)
    o32, g32, _, _ = _oracle(sd, r, tf, torch.float32, "cpu", lw, up=up, kw=kw)
    m = _detector(sd, lw, True, **kw)
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.float().to(DEV))
    assert_close(lg, o32, what="logits (48, 40)")
    assert float(m.edge_log_weight.grad.abs().max()) > 0
    e, e32 = ((t.double().cpu() - g64[LW]).abs().max().item() for t in (m.edge_log_weight.grad, g32[LW]))
    print(f"(48, 40) B=4: edge_log_weight grad err {e:.3e}, fp32 reference err {e32:.3e}, "
          f"scale {g64[LW].abs().max().item():.3e}")
    # the new gradient under the bar; the other parameters' gradients at these widths are
    # test_gpu_widths.py::test_detector_general_widths_vs_oracle's
    assert_grads_match_truth({LW: m.edge_log_weight.grad}, {LW: g32[LW]}, {LW: g64[LW]})


# ----------------------------------------------------------------------------- 4. stale tables
def test_tables_follow_the_weights_in_place():
    """Forward, edge_log_weight changed in place, forward again at B = 32 (compressed x0): equal
    (torch.equal) to a freshly built detector holding the new values; the sensor-marked tables
    are refreshed into the SAME buffers; a forward without a change launches no reweight."""
    sd = _random_ref(41)
    r, tf, _ = (t.to(DEV) for t in _batch(32))
    lw = _log_w(0.0)
    m = _detector(sd, lw, True)
    with torch.no_grad():
        first = m(r, tf)
    g = m._device_state(DEV)[0]
    assert g.x0marks is not None and m._reweights == 0
    ptrs = (g.x0marks.nodetab_s.data_ptr(), g.x0marks.pairs_s.data_ptr(), g.nodetab.data_ptr(), g.pairs.data_ptr())
    new = lw + 0.3 * torch.randn(lw.shape, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        m.edge_log_weight.copy_(new.to(DEV))
        second = m(r, tf)
    assert m._reweights == 1 and not torch.equal(first, second)
    assert ptrs == (g.x0marks.nodetab_s.data_ptr(), g.x0marks.pairs_s.data_ptr(), g.nodetab.data_ptr(),
                    g.pairs.data_ptr())
    fresh = _detector(sd, lw, True)
    with torch.no_grad():
        fresh.edge_log_weight.copy_(new.to(DEV))  # the new values loaded (not log(exp(new)): other bits)
        want = fresh(r, tf)
        again = m(r, tf)
    assert torch.equal(second, want) and torch.equal(again, want)
    assert m._reweights == 1  # unchanged version: no device work
    m(r, tf).sum().backward()  # nor with autograd on
    assert m._reweights == 1 and m.edge_log_weight.grad is not None


# ----------------------------------------------------------------------------- 5. training step
def test_captured_step_with_learned_weights_matches_eager():
    """Train mode, dropout 0.1, B = 32: three ClipAdamW steps replayed from a CapturedTrainStep and
    three eager ones from the same state with the same dropout seeds (the replays' device seeds
    read back, as test_captured_forward_reads_device_seeds does).  Bar: the captured-step test's
    (tests/test_graph_step.py: loss rtol 1e-6, parameters rtol 1e-5).  All finite,
    edge_log_weight moved, lg_spin_errors zero."""
    import ctypes

    from models import library
    from models.graph_step import CapturedTrainStep
    from models.optim import ClipAdamW
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    torch.manual_seed(0)
    m1 = LeakDetector(LTA_INP, sensors, pipes, dropout=0.1, edge_weight=_log_w().exp(),
                      learn_edge_weight=True).to(DEV).train()
    m2 = copy.deepcopy(m1)
    lw0 = m1.edge_log_weight.detach().clone()
    r, tf, lab = (t.to(DEV) for t in _batch(32, seed=1))
    mk = lambda m: ClipAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, max_norm=1.0)  # noqa: E731
    o1, o2 = mk(m1), mk(m2)
    loss_fn = torch.nn.functional.cross_entropy
    step = CapturedTrainStep(m2, loss_fn, o2, (r, tf), lab, clip=None, warmup=2, preserve_state=True)
    seeds, l2 = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        seeds.append([int(v) for v in step.slots.buf.cpu()])  # the call sites take them in slot order
        l2 = step().clone()
    torch.cuda.synchronize()
    orig, l1 = library.seed_tensor, None
    try:
        for sd in seeds:
            it = iter(sd)
            library.seed_tensor = lambda device=None: torch.tensor([next(it)], dtype=torch.long)
            o1.zero_grad(set_to_none=True)
            l1 = loss_fn(m1(r, tf), lab)
            l1.backward()
            o1.step()
    finally:
        library.seed_tensor = orig
    torch.cuda.synchronize()
    assert_close(l2, l1, rtol=1e-6, what="loss")
    for (n, a), b in zip(m2.named_parameters(), m1.parameters()):
        assert bool(torch.isfinite(a).all()), n
        assert_close(a, b, rtol=1e-5, what=n)
    assert not torch.equal(m2.edge_log_weight.detach(), lw0)
    word = ctypes.c_uint32(0)
    assert library.load_library().lg_spin_errors(ctypes.byref(word), 0) == 0 and word.value == 0
    # the replays moved the weights without moving _version: after invalidate, an eager forward
    # of the captured model equals the eager model's
    m2.invalidate_edge_weights()
    m1.eval(), m2.eval()
    with torch.no_grad():
        assert_close(m2(r, tf), m1(r, tf), rtol=1e-5, what="eval logits after the steps")


# ----------------------------------------------------------------------------- 6. opcheck
def _check(op, args, kwargs=None):
    torch.library.opcheck(op, args, kwargs, test_utils=("test_schema", "test_autograd_registration",
                                                        "test_faketensor", "test_aot_dispatch_dynamic"))


@pytest.mark.parametrize("B", [3, 16])
def test_opcheck_trunk_ops_with_edge_w(B):
    """gnn_trunk (window-major B = 3, node-major B = 16) and encoder_trunk (B = 16) with edge_w
    given and requiring grad (the pattern of tests/test_gpu_library.py)."""
    from models import ops
    m = _detector(_random_ref(41), _log_w(), True)
    g, inc, slot, sidx, live, nons = m._device_state(DEV)
    nm = ops.use_node_major(B, 661, 64)
    seed = torch.tensor([12345], dtype=torch.long)
    h_s = torch.randn(B, 29, 64, device=DEV, requires_grad=True)
    Wn = torch.randn(64, 65, device=DEV).div_(8).requires_grad_(True)
    nb = torch.randn(64, device=DEV, requires_grad=True)
    wts = [c.lin.weight.detach().clone().requires_grad_(True) for c in m.convs]
    bs = [c.bias.detach().clone().normal_(0, 0.1).requires_grad_(True) for c in m.convs]
    edge_w = g.w.detach().clone().requires_grad_(True)
    mk = m._x0marks(g, slot)
    marks = (mk.nodetab_s, mk.pairs_s, mk.pos_slot_t) if nm else (None, None, None)
    _check(torch.ops.leakgnn.gnn_trunk.default,
           (h_s, Wn, nb, wts, bs, slot, sidx, nons, live, g.nodetab, g.pairs, g.rowptr, g.col, g.w, g.nodetab_t,
            g.pairs_t, g.rowptr_t, g.col_t, g.w_t, 0.1 if nm else 0.0, nm, seed, *marks, edge_w), {"bf16": False})
    if not nm:
        return
    r, tf = torch.randn(B, 36, 29, device=DEV), torch.randn(B, 36, 9, device=DEV)
    gru = m.sensor_encoder.gru
    gw = [t.detach().clone().requires_grad_(True) for t in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
                                                              gru.bias_hh_l0)]
    _check(torch.ops.leakgnn.encoder_trunk.default,
           (r, tf, *gw, Wn, nb, wts, bs, slot, sidx, live, g.nodetab, g.pairs, g.nodetab_t, g.pairs_t, mk.nodetab_s,
            mk.pairs_s, mk.pos_slot_t, 0.1, seed, True, edge_w, g.rowptr, g.col), {"bf16": False})


def test_encoder_trunk_edge_w_with_and_without_the_csr():
    """encoder_trunk at B = 16, dropout 0.1, one CPU seed: edge_w, rowptr and col given, defaulted
    from the right one by one, or all left out.  The autograd edge is an anchor only, so the output
    and every parameter gradient are bit-identical in all of them (the bar of
    test_learned_weights_fused_equals_separate_ops), and the backward returns as many gradients as
    autograd saw arguments (autograd checks the count).  dL/dedge_w, where asked for, is non-zero
    and reproducible; asking for it without the CSR is refused."""
    m = _detector(_random_ref(41), _log_w(), True)
    g, inc, slot, sidx, live, nons = m._device_state(DEV)
    B, seed = 16, torch.tensor([12345], dtype=torch.long)
    gen = torch.Generator().manual_seed(5)
    r, tf = torch.randn(B, 36, 29, generator=gen).to(DEV), torch.randn(B, 36, 9, generator=gen).to(DEV)
    up = torch.randn(661, B, 64, generator=gen).to(DEV)
    gru = m.sensor_encoder.gru
    mk = m._x0marks(g, slot)
    leaves = lambda: [t.detach().clone().requires_grad_(True) for t in (  # noqa: E731
        gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, m.sensor_to_node.weight,
        m.sensor_to_node.bias, *(c.lin.weight for c in m.convs), *(c.bias for c in m.convs))]
    nl = len(m.convs)

    def run(*tail):
        p = leaves()
        out = torch.ops.leakgnn.encoder_trunk(r, tf, *p[:6], p[6:6 + nl], p[6 + nl:], slot, sidx, live, g.nodetab,
                                              g.pairs, g.nodetab_t, g.pairs_t, mk.nodetab_s, mk.pairs_s, mk.pos_slot_t,
                                              0.1, seed, True, *tail)
        out[nl - 1].backward(up)
        return [o.detach() for o in out], [t.grad for t in p]

    fixed, learn = g.w.detach().clone(), g.w.detach().clone().requires_grad_(True)
    base = run()
    for tail in ((fixed,), (fixed, g.rowptr), (fixed, g.rowptr, g.col), (learn, g.rowptr, g.col)):
        outs, grads = run(*tail)
        assert all(torch.equal(a, b) for a, b in zip(outs, base[0])), len(tail)
        assert all(a is not None and torch.equal(a, b) for a, b in zip(grads, base[1])), len(tail)
    assert fixed.grad is None and learn.grad is not None and float(learn.grad.abs().max()) > 0
    again = g.w.detach().clone().requires_grad_(True)
    run(again, g.rowptr, g.col)
    assert torch.equal(again.grad, learn.grad)
    with pytest.raises(NotImplementedError, match="needs rowptr / col"):
        run(g.w.detach().clone().requires_grad_(True))
