"""GCNConv with edge_weight (MI355X): the weighted gcn_norm + CSR (lg_graph_build_w /
lg_graph_reweight), the forward on both GCNConv paths, and every gradient including
d edge_weight (lg_sddmm_cols + lg_gcn_norm_bwd).

The reference arithmetic is PyG 2.x's published gcn_norm with edge_weight, restated here in
plain numpy / torch (PyG is not installed): add_remaining_self_loops (input self loops leave the
edge list, one loop per node is appended with weight `fill`, or the weight of the node's LAST
input self loop), deg = scatter_add(weight, dst) in edge order, dis = deg^-1/2 (inf -> 0),
w = (dis[src] * weight) * dis[dst].  fp32 on the CPU for the bit-exact checks, fp64 as the truth.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import RTOL, assert_close, assert_grads_match_truth, load
from oracle import graph_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ----------------------------------------------------------------------------- the restatement
def _self_loop_edges(src, dst, N):
    """loop_eid[n] = the last input edge (n, n) in edge order, -1 if none (numpy int64)."""
    loop_eid = np.full(N, -1, dtype=np.int64)
    for e in np.nonzero(src == dst)[0]:
        loop_eid[src[e]] = e
    return loop_eid


def _edge_list(ei, N, add_loops):
    """(src, dst, eid) of the normalised edge list, numpy: eid = the input edge of each entry
    (appended loops: the supplying self-loop edge or -1)."""
    src, dst = np.asarray(ei[0], dtype=np.int64), np.asarray(ei[1], dtype=np.int64)
    eid = np.arange(src.shape[0], dtype=np.int64)
    if add_loops:
        keep = src != dst
        loops = np.arange(N, dtype=np.int64)
        loop_eid = _self_loop_edges(src, dst, N)
        src, dst, eid = (np.concatenate([src[keep], loops]), np.concatenate([dst[keep], loops]),
                         np.concatenate([eid[keep], loop_eid]))
    return src, dst, eid


def csr_ref(ei, ew, N, add_loops=True, normalize=True, fill=1.0, transpose=False):
    """The weighted gcn_norm as a CSR in fp32 numpy (sequential scatter_add, as a CPU index_add_):
    rowptr int32, col int32, eid int32, w float32; rows in ascending edge order, the loop last."""
    src, dst, eid = _edge_list(ei, N, add_loops)
    ew = np.asarray(ew, dtype=np.float32)
    wt = np.where(eid >= 0, ew[np.maximum(eid, 0)] if ew.size else np.float32(0), np.float32(fill)).astype(np.float32)
    if normalize:
        deg = np.zeros(N, dtype=np.float32)
        np.add.at(deg, dst, wt)
        with np.errstate(divide="ignore"):
            dis = (np.float32(1.0) / np.sqrt(deg)).astype(np.float32)
        dis[np.isinf(dis)] = 0.0
        w = ((dis[src] * wt).astype(np.float32) * dis[dst]).astype(np.float32)
    else:
        w = wt
    key, other = (src, dst) if transpose else (dst, src)
    order = np.argsort(key, kind="stable")
    rowptr = np.zeros(N + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(key, minlength=N))
    return rowptr, other[order].astype(np.int32), eid[order].astype(np.int32), w[order].astype(np.float32)


def conv_ref(x, ei, ew, W, b, N, add_loops=True, normalize=True, fill=1.0):
    """GCNConv.forward(x, edge_index, edge_weight) in plain torch, in x's dtype and on x's device
    (differentiable in x, ew, W, b)."""
    src, dst, eid = _edge_list(ei.cpu().numpy(), N, add_loops)
    src, dst, eid = (torch.from_numpy(a).to(x.device) for a in (src, dst, eid))
    wt = torch.where(eid >= 0, ew[eid.clamp(min=0)] if ew.numel() else ew.new_zeros(()), ew.new_full((), fill))
    if normalize:
        deg = torch.zeros(N, dtype=x.dtype, device=x.device).index_add(0, dst, wt)
        dis = deg.pow(-0.5)
        dis = dis.masked_fill(dis == float("inf"), 0.0)
        w = (dis[src] * wt) * dis[dst]
    else:
        w = wt
    h = x @ W.t()
    y = torch.zeros(N, W.shape[0], dtype=x.dtype, device=x.device).index_add(0, dst, w[:, None] * h[src])
    return y + b if b is not None else y


# ----------------------------------------------------------------------------- graphs
def _rand_graph(N, E, seed, loops=True, dups=True, dst_hi=None):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, dst_hi or N, (E,), generator=g)
    if loops:
        src[: max(1, E // 50)] = dst[: max(1, E // 50)]
    if dups and E > 4:
        src[-2:], dst[-2:] = src[:2].clone(), dst[:2].clone()
    return torch.stack([src, dst])


def _weights(E, seed):
    return torch.empty(E).uniform_(0.1, 2.0, generator=torch.Generator().manual_seed(seed))


def _ltown_a():
    return torch.from_numpy(load("graph_ltown_a.npz")["edge_index"])


def _graph(name):
    if name == "ltown_a_b4":
        return torch.from_numpy(graph_ref.batchify(_ltown_a().numpy(), 661, 4)), 4 * 661
    if name == "random":
        return _rand_graph(3001, 12000, seed=5), 3001
    if name == "small":  # node 299 has no incoming edge
        return _rand_graph(300, 900, seed=1200, dst_hi=299), 300
    raise KeyError(name)


# ----------------------------------------------------------------------------- 1. weighted CSR
def _check_weighted_csr(g, ei, ew, N, add_loops, normalize, fill):
    torch.cuda.synchronize()
    for transpose, (rp, c, e, w) in ((False, (g.rowptr, g.col, g.eid, g.w)), (True, (g.rowptr_t, g.col_t, g.eid_t, g.w_t))):
        rp_o, c_o, e_o, w_o = csr_ref(ei.numpy(), ew.numpy(), N, add_loops, normalize, fill, transpose=transpose)
        rp = rp.cpu().numpy()
        nnz = int(rp[-1])
        np.testing.assert_array_equal(rp, rp_o)
        np.testing.assert_array_equal(c.cpu().numpy()[:nnz], c_o)
        np.testing.assert_array_equal(e.cpu().numpy()[:nnz], e_o)
        np.testing.assert_array_equal(w.detach().cpu().numpy()[:nnz].view(np.uint32), w_o.view(np.uint32))


def _csr_case(name):
    if name == "ltown_a":
        return _ltown_a(), 661, True, True, False
    if name == "empty":
        return torch.zeros(2, 0, dtype=torch.long), 7, True, True, False
    if name == "loops_dups":
        ei = _rand_graph(50, 300, seed=350)
        ei[:, 10] = ei[0, 0]  # a second self loop on edge 0's node: the later one supplies the loop weight
        assert ei[0, 0] == ei[1, 0]
        return ei, 50, True, True, False
    if name == "no_loops":
        return _rand_graph(300, 900, seed=1200, dst_hi=299), 300, False, True, False
    if name == "no_norm":
        return _rand_graph(300, 900, seed=1200, dst_hi=299), 300, True, False, False
    if name == "improved":
        return _rand_graph(1000, 7000, seed=8000), 1000, True, True, True
    raise KeyError(name)


@pytest.mark.parametrize("case", ["ltown_a", "empty", "loops_dups", "no_loops", "no_norm", "improved"])
def test_weighted_csr_bit_exact(case):
    from models.ops import GCNGraph
    ei, N, add_loops, normalize, improved = _csr_case(case)
    E = ei.size(1)
    ew = _weights(E, seed=N + E)
    fill = 2.0 if improved else 1.0
    g = GCNGraph.build(ei, N, DEV, add_self_loops=add_loops, normalize=normalize, improved=improved, edge_weight=ew)
    _check_weighted_csr(g, ei, ew, N, add_loops, normalize, fill)
    if case == "no_loops":
        assert g.dis[299].item() == 0.0  # no incoming edge: deg 0, dis inf -> 0
    # new weights on the same structure (lg_graph_reweight): the same bits as a fresh build
    ew2 = _weights(E, seed=N + E + 1)
    g.reweight(ew2)
    _check_weighted_csr(g, ei, ew2, N, add_loops, normalize, fill)
    nnz = int(g.rowptr[-1])
    assert torch.equal(g.pairs[:nnz, 0], g.col[:nnz]) and torch.equal(g.pairs[:nnz, 1], g.w.view(torch.int32)[:nnz])
    assert torch.equal(g.pairs_t[:nnz, 1], g.w_t.view(torch.int32)[:nnz])


# ----------------------------------------------------------------------------- 2. None unchanged
def test_none_is_unchanged_and_unit_weights_match():
    from models.ops import GCNGraph
    ei = _ltown_a()  # no input self loops
    assert not bool((ei[0] == ei[1]).any())
    g = GCNGraph.build(ei, 661, DEV)
    assert g.eid is None and g.dis is None
    for transpose, (rp, c, w) in ((False, (g.rowptr, g.col, g.w)), (True, (g.rowptr_t, g.col_t, g.w_t))):
        rp_o, c_o, w_o = graph_ref.gcn_csr(ei.numpy(), 661, transpose=transpose)
        nnz = int(rp_o[-1])
        np.testing.assert_array_equal(rp.cpu().numpy(), rp_o)
        np.testing.assert_array_equal(c.cpu().numpy()[:nnz], c_o)
        np.testing.assert_array_equal(w.cpu().numpy()[:nnz].view(np.uint32), w_o.view(np.uint32))
    g1 = GCNGraph.build(ei, 661, DEV, edge_weight=torch.ones(ei.size(1)))
    nnz = int(g.rowptr[-1])
    assert nnz == g.col.numel()  # no dropped loops: every slot is in use
    for name in ("rowptr", "col", "w", "rowptr_t", "col_t", "w_t", "pairs", "pairs_t", "nodetab", "nodetab_t"):
        a, b = (getattr(t, name) for t in (g, g1))
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
        assert torch.equal(a, b), name


# ----------------------------------------------------------------------------- 3./4. forward and gradients
def _run_conv_case(din, dout, ei, N, seed, add_loops=True, normalize=True, improved=False):
    """GCNConv(din, dout) forward + backward on the GPU against the restatement in fp32 (CPU) and
    fp64 (the truth).  Returns the error figures."""
    from models.gcn import GCNConv
    torch.manual_seed(seed)
    conv = GCNConv(din, dout, improved=improved, add_self_loops=add_loops, normalize=normalize).to(DEV)
    with torch.no_grad():
        conv.bias.normal_()
    E = ei.size(1)
    x, gy, ew = torch.randn(N, din), torch.randn(N, dout), _weights(E, seed + 1)
    xg, ewg = x.to(DEV).requires_grad_(True), ew.to(DEV).requires_grad_(True)
    y = conv(xg, ei.to(DEV), ewg)
    assert y.shape == (N, dout)
    y.backward(gy.to(DEV))
    gpu = {"x": xg.grad, "W": conv.lin.weight.grad, "b": conv.bias.grad, "ew": ewg.grad}
    assert all(torch.isfinite(v).all() for v in gpu.values())
    fill = 2.0 if improved else 1.0
    refs = {}
    for dt in (torch.float32, torch.float64):
        leaves = {"x": x, "W": conv.lin.weight, "b": conv.bias, "ew": ew}
        leaves = {k: v.detach().cpu().clone().to(dt).requires_grad_(True) for k, v in leaves.items()}
        yr = conv_ref(leaves["x"], ei, leaves["ew"], leaves["W"], leaves["b"], N, add_loops, normalize, fill)
        yr.backward(gy.to(dt))
        refs[dt] = (yr.detach(), {k: v.grad for k, v in leaves.items()})
    y64, g64 = refs[torch.float64]
    y32, g32 = refs[torch.float32]
    scale = y64.abs().max().item()
    figs = {"fwd": (y.detach().cpu().double() - y64).abs().max().item() / scale}
    for k in g64:
        s = g64[k].abs().max().item()
        figs["d" + k] = ((gpu[k].cpu().double() - g64[k]).abs().max().item() / s,
                         (g32[k].double() - g64[k]).abs().max().item() / s)
    print(f"GCNConv({din},{dout}) N={N} loops={add_loops} norm={normalize} improved={improved}: "
          + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} gpu {v[0]:.2e} / cpu32 {v[1]:.2e}"
                      for k, v in figs.items()))
    assert_close(y, y64, what=f"GCNConv({din},{dout}) weighted fwd")
    assert_grads_match_truth(gpu, g32, g64)
    return figs


@pytest.mark.parametrize("din,dout", [(64, 64), (32, 32), (48, 80), (64, 16), (7, 5)])
@pytest.mark.parametrize("graph", ["ltown_a_b4", "random"])
def test_weighted_gcnconv_fwd_and_all_grads(din, dout, graph):
    """Forward at the project's bar and dx, dW, db, d edge_weight against the fp64 restatement
    (the fp32 restatement's own error is the yardstick, helpers.assert_grads_match_truth), on
    the fused path (in == out in {32, 64}) and the general one."""
    ei, N = _graph(graph)
    _run_conv_case(din, dout, ei, N, seed=din * 1000 + dout)


@pytest.mark.parametrize("din,dout", [(64, 64), (48, 80)])
@pytest.mark.parametrize("mode", ["no_norm", "no_loops", "improved"])
def test_weighted_gcnconv_modes(din, dout, mode):
    ei, N = _graph("small")
    _run_conv_case(din, dout, ei, N, seed=din + dout, add_loops=mode != "no_loops", normalize=mode != "no_norm",
                   improved=mode == "improved")


# ----------------------------------------------------------------------------- 5. lg_sddmm_cols
def test_sddmm_cols_c_abi():
    """lg_sddmm_cols through the C ABI: odd and strided widths, rows with only their self loop,
    out past nnz untouched, N == 0 / C == 0 without a launch."""
    from models import ops
    from models.ops import GCNGraph
    lib = ops.load_library()
    N = 500
    ei = _rand_graph(N - 50, 2000, seed=3)  # nodes 450..499: self loops only
    graph = GCNGraph.build(ei, N, DEV)
    rp, col = graph.rowptr.cpu().long(), graph.col.cpu().long()
    nnz = int(rp[-1])
    row = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    assert int((rp[1:] - rp[:-1])[450:].max()) == 1
    for C, lda, ldb in ((13, 13, 13), (40, 44, 48), (64, 72, 64)):
        a, b = torch.randn(N, lda), torch.randn(N, ldb)
        ad, bd = a.to(DEV), b.to(DEV)
        out = torch.full((graph.col.numel(),), 7.0, device=DEV)
        ops.check(lib.lg_sddmm_cols(ops.ptr(graph.rowptr), ops.ptr(graph.col), ops.ptr(ad), lda, ops.ptr(bd), ldb,
                                    ops.ptr(out), N, C, ops.stream_of(ad)), "lg_sddmm_cols")
        torch.cuda.synchronize()
        ref = (a[row, :C].double() * b[col[:nnz], :C].double()).sum(-1)
        assert_close(out[:nnz], ref, what=f"sddmm_cols C={C} lda={lda} ldb={ldb}")
        assert torch.all(out[nnz:] == 7.0), "elements past nnz untouched"
        out2 = torch.full_like(out, 7.0)
        ops.check(lib.lg_sddmm_cols(ops.ptr(graph.rowptr), ops.ptr(graph.col), ops.ptr(ad), lda, ops.ptr(bd), ldb,
                                    ops.ptr(out2), N, C, ops.stream_of(ad)), "lg_sddmm_cols")
        assert torch.equal(out, out2), "deterministic"
    untouched = torch.full_like(out, 7.0)
    for n_, c_ in ((0, 8), (N, 0)):
        assert lib.lg_sddmm_cols(ops.ptr(graph.rowptr), ops.ptr(graph.col), ops.ptr(ad), 64, ops.ptr(bd), 64,
                                 ops.ptr(untouched), n_, c_, ops.stream_of(ad)) == 0
    torch.cuda.synchronize()
    assert torch.all(untouched == 7.0)


# ----------------------------------------------------------------------------- 6. cache behaviour
@pytest.mark.parametrize("din,dout", [(64, 64), (48, 80)])
def test_weight_cache_follows_the_weights(din, dout):
    from models.gcn import GCNConv
    ei, N = _ltown_a().to(DEV), 661
    E = ei.size(1)
    torch.manual_seed(11)
    conv = GCNConv(din, dout).to(DEV)
    x = torch.randn(N, din, device=DEV)
    ew = _weights(E, 1).to(DEV)
    with torch.no_grad():
        y1 = conv(x, ei, ew)
        assert torch.equal(conv(x, ei, ew), y1), "same object, same version: bit-equal"
        assert torch.equal(conv(x, ei, ew.clone()), y1), "a fresh tensor with equal values: bit-equal"
        new = _weights(E, 2).to(DEV)
        ew.copy_(new)  # in place: the version counter moves, the cache must not be served
        y2 = conv(x, ei, ew)
        fresh = GCNConv(din, dout).to(DEV)
        fresh.load_state_dict(conv.state_dict())
        assert torch.equal(y2, fresh(x, ei, new)), "modified in place: the output follows the new weights"
        assert not torch.equal(y1, y2)
        assert_close(y2, conv_ref(x.cpu().double(), ei.cpu(), new.cpu().double(), conv.lin.weight.detach().cpu().double(),
                                  conv.bias.detach().cpu().double(), N), what="after the in-place change")
        # the unweighted call keeps its own cache and result
        assert torch.equal(conv(x, ei), fresh(x, ei))
    grads = []
    for _ in range(2):  # determinism: identical inputs, bit-identical d edge_weight
        w = new.clone().requires_grad_(True)
        xg = x.clone().requires_grad_(True)
        conv.zero_grad()
        conv(xg, ei, w).square().sum().backward()
        grads.append((w.grad.clone(), xg.grad.clone(), conv.lin.weight.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 7. learned weights train
def test_learned_edge_weights_train():
    """Three SGD steps on edge_weight alone (N = 661) against the same loop on the fp32
    restatement run on the GPU: final weights within RTOL * 10 (three compounding steps)."""
    from models.gcn import GCNConv
    ei, N, D = _ltown_a().to(DEV), 661, 64
    torch.manual_seed(3)
    conv = GCNConv(D, D).to(DEV)
    with torch.no_grad():
        conv.bias.normal_()
    x, gy = torch.randn(N, D, device=DEV), torch.randn(N, D, device=DEV)
    start = _weights(ei.size(1), 9).to(DEV)
    W, b = conv.lin.weight.detach(), conv.bias.detach()
    final = []
    for fwd in (lambda w: conv(x, ei, w), lambda w: conv_ref(x, ei, w, W, b, N)):
        w = torch.nn.Parameter(start.clone())
        opt = torch.optim.SGD([w], lr=1.0)
        for _ in range(3):
            opt.zero_grad()
            ((fwd(w) * gy).sum() / N).backward()
            opt.step()
        final.append(w.detach().clone())
    moved = (final[1] - start).abs().max().item()
    print(f"learned weights: moved up to {moved:.3e}, HIP vs restatement "
          f"{(final[0] - final[1]).abs().max().item() / final[1].abs().max().item():.3e} of max |w|")
    assert moved > 1e-3 and bool((final[1] > 0).all())
    assert_close(final[0], final[1], rtol=RTOL * 10, what="edge weights after 3 SGD steps")
