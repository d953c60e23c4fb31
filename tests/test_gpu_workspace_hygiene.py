"""Workspace hygiene of the workspace-taking entry points: the size `*_workspace_bytes` returns is
enough, the workspace may hold anything on entry, and nothing outside the workspace and the
documented outputs is written.

Every case calls its entry point through _native.load_library() four times: three times inside a
helpers.Arena (the workspace at exactly the promised byte count and every output between guard
bands; the workspace pre-filled with 0x00, 0xFF, or finite junk; the outputs with NaN) and once the
way today's callers do (outputs from torch.full, a roomy torch.empty workspace).  Asserted:
  rc == 0;  every guard byte intact;  no NaN left in an output the header documents as overwritten;
  the four runs bytewise equal on every output (the project's promise: no float atomics, fixed-order
  reductions);  every const input bytewise unchanged;  on the 0xFF run the op's fp64 bar.
References: where an existing module has one it is imported (graph_ref / csr_ref for the builders,
event_truth, test_gpu_step_tail's fp64 AdamW and its bars); elsewhere plain fp64 torch of the same
composition with helpers.assert_close / assert_grads_close at their defaults.

Read before poisoning: each case's docstring records what reading its entry point's host function
and kernels found.  For the entry points run here: the only word a kernel polls across workgroups is
lg_clip_adamw's ticket (step[1], caller state, never poisoned); the index-typed workspace words (the
builders' counts and cursors, loop_e) are initialised by the entry points' hipMemsetAsync; the float
slabs and partials are written by the launch in front of the reduction that reads them.  Entry points
this module does not run are not covered by that statement."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import Arena, assert_close, assert_grads_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("zeros", "ones", "junk", "roomy")


def _lib():
    from models import _native as nat
    return nat.load_library(), nat


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _hygiene(call, ws: dict, outs: dict, consts: dict, ref=None, may_keep_nan=(), setup=None, post=None):
    """call(P) -> rc with P[name] the device address of each workspace / output; ws {name: bytes};
    outs {name: (shape, dtype)}; consts {name: tensor} the call's const inputs; setup(views) writes the
    initial value of in/out arguments; post(outputs) -> the parts of the outputs the call defines (compared
    across the runs and passed on); ref(outputs of the 0xFF run).  Returns the 0xFF run's outputs."""
    for name, n in ws.items():
        assert n >= 0, f"{name}: the size query returned {n}"
    runs = {}
    for mode in MODES:
        if mode == "roomy":
            bufs = {n: torch.empty(b + 4096, dtype=torch.uint8, device=DEV) for n, b in ws.items()}
            views = {n: (torch.full(s, float("nan"), dtype=d, device=DEV) if d.is_floating_point
                         else torch.full(s, -1, dtype=d, device=DEV)) for n, (s, d) in outs.items()}
            P = {**{n: b.data_ptr() for n, b in bufs.items()}, **{n: v.data_ptr() for n, v in views.items()}}
            arena = None
        else:
            arena = Arena(DEV, ws, outs)
            arena.poison(mode, seed=len(runs))
            views = {n: arena.out(n) for n in outs}
            P = {n: arena.ptr(n) for n in list(ws) + list(outs)}
        if setup is not None:
            setup(views)
        before = {n: t.clone() for n, t in consts.items() if t is not None}
        rc = call(P)
        torch.cuda.synchronize()
        assert rc == 0, f"{mode}: rc = {rc}"
        if arena is not None:
            bad = arena.violations()
            assert not bad, f"{mode}: a store outside the promised footprint: {bad}"
        for n, t in before.items():
            assert torch.equal(t.view(torch.uint8), consts[n].view(torch.uint8)), f"{mode}: const input {n} changed"
        for n, v in views.items():
            if v.dtype.is_floating_point and n not in may_keep_nan:
                assert not bool(torch.isnan(v).any()), f"{mode}: output {n} keeps NaN (not every element overwritten, " \
                                                       f"or a stale workspace word reached it)"
        runs[mode] = {n: v.clone() for n, v in views.items()}
        if post is not None:
            runs[mode] = post(runs[mode])
    for mode in MODES[1:]:
        for n in runs["zeros"]:
            a, b = runs["zeros"][n], runs[mode][n]
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
                f"output {n} differs between workspace 'zeros' and '{mode}': the result depends on what the workspace held"
    if ref is not None:
        ref(runs["ones"])
    return runs["ones"]


# ----------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def _graph(kind: str):
    """hub: tests/test_gpu_skip.py's 41-node graph (a row past the six inline pairs in both CSRs, a node
    with only its self loop); edgeless: 17 nodes, self loops only."""
    from models import ops
    from test_gpu_skip import _kernel_graph
    if kind == "hub":
        return _kernel_graph()
    g = ops.GCNGraph.build(torch.zeros(2, 0, dtype=torch.long), 17, DEV, add_self_loops=True, normalize=True)
    return g, 17


def _dense(g, N):
    rp, col, w = g.rowptr.cpu().long(), g.col.cpu().long(), g.w.cpu()
    nnz = int(rp[-1])
    rows = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    A = torch.zeros(N, N, dtype=torch.float64)
    return A.index_put_((rows, col[:nnz]), w[:nnz].double(), accumulate=True)


def _slot5(N):
    """S = 5 sensors, the hub (node 0) included."""
    slot = torch.full((N,), -1, dtype=torch.int32)
    idx = torch.tensor([0, 3, 7, 11, 16])
    slot[idx] = torch.arange(5, dtype=torch.int32)
    return slot.to(DEV), idx


def _trunk_inputs(g, N, B, D, seed):
    lib, nat = _lib()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, B, D, generator=gen).to(DEV)
    W = (torch.randn(D, D, generator=gen) / D ** 0.5).to(DEV)
    b = (0.1 * torch.randn(D, generator=gen)).to(DEV)
    dy = torch.randn(N, B, D, generator=gen).to(DEV)
    y = torch.empty(N, B, D, device=DEV)
    ymask = torch.zeros(N * ((B + 15) // 16) * 64, dtype=torch.int16, device=DEV)
    rc = lib.lg_gcn_fwd_nm_bits(_p(g.nodetab), _p(g.pairs), _p(x), _p(W), _p(b), _p(y), B, N, D, g.col.numel(),
                                nat.LG_F_BIAS | nat.LG_F_RELU, 0.0, 0, 0, _st(), _p(ymask))
    torch.cuda.synchronize()
    assert rc == 0
    return x, W, dy, y, ymask


def _trunk_ref(A, x, W, dy, y, slot, mask_in, mask_out, s_in, s_out, skip):
    """fp64, node-major (N, B, D): the header's formulas for lg_gcn_bwd (dnode_bias: rows without a sensor)."""
    x, W, dy = x.double().cpu(), W.double().cpu(), dy.double().cpu()
    dz = dy * s_in * (y.cpu() > 0) if mask_in else dy
    t = torch.einsum("mn,mbd->nbd", A, dz)
    dx = t @ W + (dy if skip else 0.0)
    if mask_out:
        dx = dx * s_out * (x > 0)
    out = {"dx_out": dx, "dW": torch.einsum("nbo,nbi->oi", t, x), "db": dz.sum(dim=(0, 1))}
    if slot is not None:
        out["dnode_bias"] = dx[slot.cpu() < 0].sum(dim=(0, 1))
    return out


def _check(got: dict, want: dict, what: str):
    for n, r in want.items():
        assert_close(got[n], r.reshape(got[n].shape), what=f"{what} {n}")


NM_CASES = [(e, m, sl) for e in ("lg_gcn_bwd_nm_bits", "lg_gcn_bwd_nm", "lg_gcn_bwd_nm_skip") for m in (False, True)
            for sl in (False, True) if m or not e.endswith("_skip")]


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("kind", ["hub", "edgeless"])
@pytest.mark.parametrize("entry,mask_in,with_slot", NM_CASES)
def test_trunk_backward_node_major(entry, mask_in, with_slot, kind, B, D):
    """lg_gcn_bwd_nm_bits / lg_gcn_bwd_nm / lg_gcn_bwd_nm_skip, with and without LG_F_MASK_IN (the skip
    form requires it: only with) x with and without node_slot / dnode_bias (S = 5, hub included), always
    under LG_F_MASK_OUT.  Workspace: 2 x CUs slab rows of D*D + 2D floats; grid = min(tiles / waves, 2 x
    CUs) <= the rows; every launched workgroup stores its whole row at the kernel's end, no early return
    in k_gcn_bwd_nm3, and the reducer reads `grid` rows: nothing polled, nothing read before written.
    Excluded from the NaN check: nothing (dnode_bias is passed only with node_slot; LG_F_DX_SENSOR_ROWS,
    under which dx rows may stay unwritten, is not set)."""
    lib, nat = _lib()
    g, N = _graph(kind)
    x, W, dy, y, ymask = _trunk_inputs(g, N, B, D, 7 * D + B)
    slot, _ = _slot5(N)
    nws = int(lib.lg_gcn_bwd_nm_workspace_bytes(D))
    s_in, s_out = 1.0 / 0.9, 1.0 / 0.8
    skip, bits = entry.endswith("_skip"), entry != "lg_gcn_bwd_nm"
    flags = nat.LG_F_MASK_OUT | (nat.LG_F_MASK_IN if mask_in else 0)
    outs = {"dx_out": ((N, B, D), torch.float32), "dW": ((D, D), torch.float32), "db": ((D,), torch.float32)}
    if with_slot:
        outs["dnode_bias"] = ((D,), torch.float32)
    use_bits = bits and mask_in

    def call(P):
        args = (_p(g.nodetab_t), _p(g.pairs_t), _p(dy), None if use_bits else _p(y), _p(x), _p(W), P["dx_out"],
                P["dW"], P["db"], _p(slot) if with_slot else None, P.get("dnode_bias"), B, N, D, flags, s_in,
                s_out, P["workspace"], nws, _st())
        return getattr(lib, entry)(*args, _p(ymask) if use_bits else None) if bits else getattr(lib, entry)(*args)

    want = _trunk_ref(_dense(g, N), x, W, dy, y, slot if with_slot else None, mask_in, True, s_in, s_out, skip)
    _hygiene(call, {"workspace": nws}, outs,
             {"dy": dy, "y": y, "x": x, "W": W, "ymask": ymask, "nodetab_t": g.nodetab_t, "pairs_t": g.pairs_t},
             ref=lambda o: _check(o, want, entry))


@pytest.mark.parametrize("with_slot", [False, True])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("kind", ["hub", "edgeless"])
def test_trunk_backward_compressed_x0(kind, B, D, with_slot):
    """lg_gcn_bwd_nm_x0 (layer 0 on the compressed node init: xs0 + x0bits from lg_node_init_bits_fwd, p =
    0.1; no MASK_IN by contract), MASK_OUT, with and without node_slot.  It is nm_bwd with the X0 option:
    the same kernel, grid bound, end-of-kernel slab-row store and reduction as lg_gcn_bwd_nm_bits; the
    workspace holds float slab rows only.  Reference: the header's formulas in fp64 on the dense x0 that
    lg_node_init_proj_fwd writes for the same seed."""
    from models import ops
    lib, nat = _lib()
    g, N = _graph(kind)
    slot, idx = _slot5(N)
    S, p, seed = 5, 0.1, 0x5EED
    gen = torch.Generator().manual_seed(3 * D + B)
    h_s = torch.randn(B, S, D, generator=gen).to(DEV)
    Wp = (torch.randn(D, D + 1, generator=gen) / 8).to(DEV)
    nbias = torch.randn(D, generator=gen).to(DEV)
    W = (torch.randn(D, D, generator=gen) / D ** 0.5).to(DEV)
    dy = torch.randn(N, B, D, generator=gen).to(DEV)
    sidx = idx.to(DEV)
    x0 = torch.empty(N, B, D, device=DEV)
    xs0 = torch.zeros(S, B, D, device=DEV)
    bits = torch.zeros(N * ((B + 15) // 16) * 64, dtype=torch.int16, device=DEV)
    fl = nat.LG_F_DROPOUT
    assert lib.lg_node_init_proj_fwd(_p(slot), _p(sidx), _p(h_s), _p(Wp), _p(nbias), _p(x0), B, N, S, D, D,
                                     fl | nat.LG_F_NODE_MAJOR, p, seed, 0, _st()) == 0
    assert lib.lg_node_init_bits_fwd(_p(slot), _p(sidx), _p(h_s), _p(Wp), _p(nbias), _p(xs0), _p(bits), B, N, S, D, D, fl,
                                     p, seed, 0, _st()) == 0
    mk = ops.SensorMarks.build(g, slot)
    torch.cuda.synchronize()
    nws = int(lib.lg_gcn_bwd_nm_workspace_bytes(D))
    s_out = 1.0 / (1.0 - p)
    outs = {"dx_out": ((N, B, D), torch.float32), "dW": ((D, D), torch.float32), "db": ((D,), torch.float32)}
    if with_slot:
        outs["dnode_bias"] = ((D,), torch.float32)

    def call(P):
        return lib.lg_gcn_bwd_nm_x0(_p(g.nodetab_t), _p(g.pairs_t), _p(mk.pos_slot_t), _p(dy), _p(xs0), _p(bits), _p(nbias),
                                    _p(W), P["dx_out"], P["dW"], P["db"], _p(slot) if with_slot else None,
                                    P.get("dnode_bias"), B, N, S, D, nat.LG_F_MASK_OUT | nat.LG_F_DROPOUT, p, s_out,
                                    P["workspace"], nws, _st())

    want = _trunk_ref(_dense(g, N), x0, W, dy, None, slot if with_slot else None, False, True, 1.0, s_out, False)
    _hygiene(call, {"workspace": nws}, outs, {"dy": dy, "xs0": xs0, "x0bits": bits, "W": W, "node_bias": nbias,
                                              "pos_slot_t": mk.pos_slot_t}, ref=lambda o: _check(o, want, "x0"))


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("kind", ["hub", "edgeless"])
def test_trunk_backward_window_major(kind, B, D):
    """lg_gcn_bwd (window-major [B][N][D]) with MASK_IN | MASK_OUT, with and without node_slot.  Workspace:
    bwd_grid_max() slab rows; k_gcn_bwd stores (first chunk) or adds to (later chunks of a > 4 GiB split,
    not reached here) its own row at the kernel's end; the reducer reads the launched grid's rows.
    General width (7, 5): the entry point serves D in {32, 64} only (the general path composes
    lg_spmm_cols, which takes no workspace); it must refuse with LG_EUNSUPPORTED and write nothing."""
    lib, nat = _lib()
    g, N = _graph(kind)
    xn, W, dyn, yn, _ = _trunk_inputs(g, N, B, D, 11 * D + B)
    x, dy, y = (t.permute(1, 0, 2).contiguous() for t in (xn, dyn, yn))
    A = _dense(g, N)
    slot, _ = _slot5(N)
    nws = int(lib.lg_gcn_bwd_workspace_bytes(D))
    flags = nat.LG_F_MASK_IN | nat.LG_F_MASK_OUT
    for with_slot in (False, True):
        outs = {"dx_out": ((B, N, D), torch.float32), "dW": ((D, D), torch.float32), "db": ((D,), torch.float32)}
        if with_slot:
            outs["dnode_bias"] = ((D,), torch.float32)

        def call(P):
            return lib.lg_gcn_bwd(_p(g.rowptr_t), _p(g.col_t), _p(g.w_t), _p(dy), _p(y), _p(x), _p(W), P["dx_out"], P["dW"],
                                  P["db"], _p(slot) if with_slot else None, P.get("dnode_bias"), B, N, D, g.col.numel(),
                                  flags, 1.25, 0.5, P["workspace"], nws, _st())

        want = _trunk_ref(A, xn, W, dyn, yn, slot if with_slot else None, True, True, 1.25, 0.5, False)
        want["dx_out"] = want["dx_out"].permute(1, 0, 2)
        _hygiene(call, {"workspace": nws}, outs, {"dy": dy, "y": y, "x": x, "W": W, "w_t": g.w_t, "col_t": g.col_t},
                 ref=lambda o: _check(o, want, f"lg_gcn_bwd slot={with_slot}"))
    assert lib.lg_gcn_bwd_workspace_bytes(7) == -2 and lib.lg_gcn_bwd_workspace_bytes(5) == -2
    ar = Arena(DEV, {"workspace": nws}, {"dx_out": ((B, N, 7), torch.float32), "dW": ((5, 7), torch.float32)})
    ar.poison("ones")
    rc = lib.lg_gcn_bwd(_p(g.rowptr_t), _p(g.col_t), _p(g.w_t), _p(dy), None, _p(x), _p(W), ar.ptr("dx_out"), ar.ptr("dW"),
                        None, None, None, B, N, 7, g.col.numel(), 0, 1.0, 1.0, ar.ptr("workspace"), nws, _st())
    torch.cuda.synchronize()
    assert rc == -2 and not ar.violations()
    assert bool(torch.isnan(ar.out("dx_out")).all()) and bool(torch.isnan(ar.out("dW")).all())


@pytest.mark.parametrize("kind", ["hub", "edgeless"])
def test_trunk_backward_rows(kind):
    """lg_gcn_bwd_rows (one graph, x [N][D]); D = 64 is the only width it serves, D = 32 must be refused
    (LG_EUNSUPPORTED) with nothing written.  Workspace lg_gcn_bwd_nm_workspace_bytes(64): grid <= 2 x CUs
    rows, each stored whole at the end of k_gcn_bwd_rows (no early return)."""
    lib, _ = _lib()
    g, N = _graph(kind)
    D = 64
    x, W, dy, _, _ = _trunk_inputs(g, N, 1, D, 99)
    A = _dense(g, N)
    nws = int(lib.lg_gcn_bwd_nm_workspace_bytes(D))
    outs = {"dx": ((N, D), torch.float32), "dW": ((D, D), torch.float32), "db": ((D,), torch.float32)}

    def call(P, D=D):
        return lib.lg_gcn_bwd_rows(_p(g.nodetab_t), _p(g.pairs_t), _p(dy), _p(x), _p(W), P["dx"], P["dW"], P["db"], N, D,
                                   P["workspace"], nws, _st())

    want = _trunk_ref(A, x, W, dy, None, None, False, False, 1.0, 1.0, False)
    want["dx"] = want.pop("dx_out")
    _hygiene(call, {"workspace": nws}, outs, {"dy": dy, "x": x, "W": W}, ref=lambda o: _check(o, want, "lg_gcn_bwd_rows"))
    ar = Arena(DEV, {"workspace": nws}, outs)
    assert call({n: ar.ptr(n) for n in ["workspace", *outs]}, D=32) == -2
    torch.cuda.synchronize()
    assert not ar.violations() and all(bool(torch.isnan(ar.out(n)).all()) for n in outs)


# ----------------------------------------------------------------------------- the GRU encoder's backward
def _gru_case(B, S, L, I, H, seed, dh=None):
    lib, _ = _lib()
    gen = torch.Generator().manual_seed(seed)
    r = torch.randn(B, L, S, generator=gen)
    tf = torch.randn(B, L, 9, generator=gen) if I == 10 else None
    gru = torch.nn.GRU(I, H, batch_first=True)
    with torch.no_grad():
        for p in gru.parameters():
            p.uniform_(-0.3, 0.3, generator=gen)
    dh = torch.randn(B * S, H, generator=gen) if dh is None else dh
    dev = {k: (None if v is None else v.to(DEV)) for k, v in
           dict(r=r, tf=tf, w_ih=gru.weight_ih_l0.detach(), w_hh=gru.weight_hh_l0.detach(), b_ih=gru.bias_ih_l0.detach(),
                b_hh=gru.bias_hh_l0.detach(), dh=dh).items()}
    h_seq = torch.empty(L, B * S, H, device=DEV)
    gates = torch.empty(L, B * S, 4, H, device=DEV)
    h_last = torch.empty(B * S, H, device=DEV)
    rc = lib.lg_gru_fwd(_p(dev["r"]), _p(dev["tf"]), _p(dev["w_ih"]), _p(dev["w_hh"]), _p(dev["b_ih"]), _p(dev["b_hh"]),
                        _p(h_seq), _p(gates), _p(h_last), B, L, S, I, H, _st())
    torch.cuda.synchronize()
    assert rc == 0
    # fp64 truth: nn.GRU on x[q = b*S + s][t] = [residual[b][t][s], tfeat[b][t]]
    g64 = torch.nn.GRU(I, H, batch_first=True).double()
    g64.load_state_dict({k: v.double() for k, v in gru.state_dict().items()})
    xs = r.permute(0, 2, 1).reshape(B * S, L, 1).double()
    if I == 10:
        xs = torch.cat([xs, tf.double()[:, None].expand(B, S, L, 9).reshape(B * S, L, 9)], dim=-1)
    xs.requires_grad_(True)
    _, hL = g64(xs)
    (hL[0] * dh.double()).sum().backward()
    grads = {n: p.grad for n, p in g64.named_parameters()}
    return dev, h_seq, gates, h_last, hL[0].detach(), xs.grad, grads


GRU_CASES = [(B, I, H, dx) for B in (1, 3) for I in (1, 10) for H in (32, 64, 48) for dx in (False, True)] + [(103, 1, 48, False)]


@pytest.mark.parametrize("B,I,H,dx", GRU_CASES)
def test_gru_backward(B, I, H, dx):
    """lg_gru_bwd, S = 5, L = 36; H = 48 the generic kernel, B = 103 its B*S = 515 > 512 slab rows (three
    workgroups take a second sequence).  Workspace: one slab row per workgroup (16 sequences a workgroup
    with dx, 32 without, one sequence a workgroup up to 512 generic); the size query covers the larger
    (with-dx) count; rows are stored by k_gru_bwd / k_gru_bwd2 / k_gru_seq_gen_bwd before reduce_gru_slab
    reads `nb` rows; the memset path is B == 0 only.  Nothing polled.  dx is passed or NULL (optional
    output, absent from the checks when NULL)."""
    lib, _ = _lib()
    S, L = 5, 36
    dev, h_seq, gates, h_last, hL64, dx64, g64 = _gru_case(B, S, L, I, H, 1000 * B + 10 * I + H)
    assert_close(h_last, hL64, what="GRU h_L")
    nws = int(lib.lg_gru_bwd_workspace_bytes(B, S, I, H))
    outs = {"dw_ih": ((3 * H, I), torch.float32), "dw_hh": ((3 * H, H), torch.float32), "db_ih": ((3 * H,), torch.float32),
            "db_hh": ((3 * H,), torch.float32)}
    if dx:
        outs["dx"] = ((B * S, L, I), torch.float32)

    def call(P):
        return lib.lg_gru_bwd(_p(dev["r"]), _p(dev["tf"]), _p(dev["w_ih"]), _p(dev["w_hh"]), _p(h_seq), _p(gates),
                              _p(dev["dh"]), P.get("dx"), P["dw_ih"], P["dw_hh"], P["db_ih"], P["db_hh"], B, L, S, I, H,
                              P["workspace"], nws, _st())

    def ref(o):
        names = {"weight_ih_l0": "dw_ih", "weight_hh_l0": "dw_hh", "bias_ih_l0": "db_ih", "bias_hh_l0": "db_hh"}
        assert_grads_close([(n, o[k]) for n, k in names.items()], g64, prefix="GRU grad ")
        if dx:
            assert_close(o["dx"], dx64, what="GRU dx")

    consts = {k: v for k, v in dev.items() if v is not None}
    consts.update(h_seq=h_seq, gates=gates)
    _hygiene(call, {"workspace": nws}, outs, consts, ref=ref)


# ----------------------------------------------------------------------------- node init backward
@pytest.mark.parametrize("K,M,N", [(3, 64, 32), (250, 32, 64)])
def test_linear_dw(K, M, N):
    """lg_linear_dw: split-K slabs, one row per workgroup of linear_dw_grid(K), each stored by k_linear_dw
    before the reducer reads the same count (memset: K == 0 only).  db is given (not NULL)."""
    lib, _ = _lib()
    gen = torch.Generator().manual_seed(K + M + N)
    dy, x = torch.randn(K, M, generator=gen).to(DEV), torch.randn(K, N, generator=gen).to(DEV)
    nws = int(lib.lg_linear_dw_workspace_bytes(K, M, N))

    def ref(o):
        want = torch.cat([dy.double().t() @ x.double(), dy.double().sum(0, keepdim=True).t()], 1)
        assert_close(o["dw"], want, what="dW")
        assert_close(o["db"], want[:, N], what="db")

    _hygiene(lambda P: lib.lg_linear_dw(_p(dy), _p(x), K, M, N, P["dw"], P["db"], P["workspace"], nws, _st()),
             {"workspace": nws}, {"dw": ((M, N + 1), torch.float32), "db": ((M,), torch.float32)}, {"dy": dy, "x": x}, ref=ref)


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("nm", [False, True])
def test_sensor_proj_backward(nm, B, D):
    """lg_sensor_proj_bwd, S = 5 sensors of the 41-node graph's ids, Ds = D, with dbias_in and live (one
    dead sensor); window-major and LG_F_NODE_MAJOR dx0.  Workspace: ceil(B*S / rows per workgroup) slab
    rows of D*(Ds+1) + D floats, each stored by its workgroup before the reducer reads that count."""
    lib, nat = _lib()
    N, S = 41, 5
    _, idx = _slot5(N)
    gen = torch.Generator().manual_seed(31 * B + D)
    dx0 = torch.randn((N, B, D) if nm else (B, N, D), generator=gen).to(DEV)
    h_s = torch.randn(B, S, D, generator=gen).to(DEV)
    W = (torch.randn(D, D + 1, generator=gen) / 8).to(DEV)
    dbin = torch.randn(D, generator=gen).to(DEV)
    live = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0], device=DEV)
    sidx = idx.to(DEV)
    nws = int(lib.lg_sensor_proj_bwd_workspace_bytes(B, S, D, D))

    def call(P):
        return lib.lg_sensor_proj_bwd(_p(dx0), _p(sidx), _p(live), _p(h_s), _p(W), _p(dbin), P["dh_s"], P["dW"], P["db"], B, N,
                                      S, D, D, nat.LG_F_NODE_MAJOR if nm else 0, P["workspace"], nws, _st())

    def ref(o):
        d = dx0.double().cpu()
        dproj = (d.permute(1, 0, 2) if nm else d)[:, idx] * live.double().cpu()[None, :, None]
        h1 = torch.cat([h_s.double().cpu(), torch.ones(B, S, 1, dtype=torch.float64)], -1)
        assert_close(o["dh_s"], dproj @ W.double().cpu()[:, :D], what="dh_s")
        assert_close(o["dW"], torch.einsum("bso,bsi->oi", dproj, h1), what="dW")
        assert_close(o["db"], dproj.sum(dim=(0, 1)) + dbin.double().cpu(), what="db")

    _hygiene(call, {"workspace": nws}, {"dh_s": ((B, S, D), torch.float32), "dW": ((D, D + 1), torch.float32),
                                        "db": ((D,), torch.float32)},
             {"dx0": dx0, "h_s": h_s, "W": W, "dbias_in": dbin, "live": live, "sensor_idx": sidx}, ref=ref)


# ----------------------------------------------------------------------------- heads
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("B", [1, 17])
def test_pool_head_backward(B, D, train):
    """lg_pool_head_bwd on what lg_pool_head_fwd saved (pooled, hid), eval and train (p = 0.1) flags,
    logits column col = P of ldo = P + 1.  Workspace: pool_bwd_grid(B) float slab rows, rounded up to 256
    bytes, then one fp64 partial per workgroup (db2); both zero-filled only at B == 0, otherwise stored by
    every workgroup of k_pool_head_bwd before the reducer reads that grid.  Nothing polled."""
    lib, nat = _lib()
    N, HID, P = 41, 128, 6
    gen = torch.Generator().manual_seed(5 * B + D + int(train))
    x = torch.randn(B, N, D, generator=gen).to(DEV)
    w1 = (torch.randn(HID, D, generator=gen) / D ** 0.5).to(DEV)
    b1 = (0.1 * torch.randn(HID, generator=gen)).to(DEV)
    w2 = (torch.randn(HID, generator=gen) / HID ** 0.5).to(DEV)
    b2 = torch.randn(1, generator=gen).to(DEV)
    dlog = torch.randn(B, P + 1, generator=gen).to(DEV)
    pooled, hid = torch.empty(B, D, device=DEV), torch.empty(B, HID, device=DEV)
    logits = torch.zeros(B, P + 1, device=DEV)
    flags, p = (nat.LG_F_DROPOUT, 0.1) if train else (0, 0.0)
    rc = lib.lg_pool_head_fwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(pooled), _p(hid), _p(logits), P + 1, P, B, N, D, HID,
                              flags, p, 12345, 7, _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert_close(pooled, x.double().mean(1), what="pooled")
    nws = int(lib.lg_pool_head_bwd_workspace_bytes(B, D, HID))

    def call(P_):
        return lib.lg_pool_head_bwd(_p(pooled), _p(hid), _p(w1), _p(w2), _p(dlog), P + 1, P, P_["dpooled"], P_["dw1"],
                                    P_["db1"], P_["dw2"], P_["db2"], B, D, HID, flags, p, P_["workspace"], nws, _st())

    def ref(o):
        dl = dlog.double().cpu()[:, P]
        h, pl = hid.double().cpu(), pooled.double().cpu()
        dpre = dl[:, None] * w2.double().cpu()[None] * (h > 0) * (1.0 / (1.0 - p))
        want = {"dpooled": dpre @ w1.double().cpu(), "dw1": dpre.t() @ pl, "db1": dpre.sum(0), "dw2": (dl[:, None] * h).sum(0),
                "db2": dl.sum().reshape(1)}
        _check(o, want, "pool head")

    outs = {"dpooled": ((B, D), torch.float32), "dw1": ((HID, D), torch.float32), "db1": ((HID,), torch.float32),
            "dw2": ((HID,), torch.float32), "db2": ((1,), torch.float32)}
    _hygiene(call, {"workspace": nws}, outs, {"pooled": pooled, "hid": hid, "w1": w1, "w2": w2, "dlogits": dlog}, ref=ref)


@pytest.mark.parametrize("B,H,S", [(1, 128, 5), (17, 128, 29)])
def test_head_mse_backward(B, H, S):
    """lg_head_mse_bwd on lg_head_mse_fwd's y_hat.  Workspace: `chunks` rows of S*H + S floats; the
    launch's grid (chunks, column tiles) stores every column of every row before the reducer reads
    `chunks` rows.  Nothing polled in the backward (the forward's counter is not a workspace word)."""
    lib, _ = _lib()
    gen = torch.Generator().manual_seed(B + S)
    h = torch.randn(B, H, generator=gen).to(DEV)
    w = (torch.randn(S, H, generator=gen) / H ** 0.5).to(DEV)
    b = torch.randn(S, generator=gen).to(DEV)
    y = torch.randn(B, S, generator=gen).to(DEV)
    gl = torch.tensor([0.75], device=DEV)
    yhat, rowsq, loss = torch.empty(B, S, device=DEV), torch.empty(B, device=DEV), torch.empty(1, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib.lg_head_mse_fwd(_p(h), _p(w), _p(b), _p(y), B, H, S, _p(yhat), _p(rowsq), _p(loss), _p(counter), _st())
    torch.cuda.synchronize()
    assert rc == 0
    nws = int(lib.lg_head_mse_bwd_workspace_bytes(B, H, S))

    def ref(o):
        d = 2.0 * 0.75 / (B * S) * (yhat.double().cpu() - y.double().cpu())
        _check(o, {"dh": d @ w.double().cpu(), "dweight": d.t() @ h.double().cpu(), "dbias": d.sum(0)}, "head mse")

    _hygiene(lambda P: lib.lg_head_mse_bwd(_p(h), _p(w), _p(y), _p(yhat), _p(gl), B, H, S, P["dh"], P["dweight"], P["dbias"],
                                           P["workspace"], nws, _st()),
             {"workspace": nws}, {"dh": ((B, H), torch.float32), "dweight": ((S, H), torch.float32), "dbias": ((S,), torch.float32)},
             {"h": h, "weight": w, "target": y, "y_hat": yhat, "grad_loss": gl}, ref=ref)


# ----------------------------------------------------------------------------- graph builders
def _edges(N, E, seed):
    """E about 3N random edges with self loops and duplicates (tests/test_gpu_parity.py's generator)."""
    from test_gpu_parity import _rand_graph
    return _rand_graph(N, E, seed) if E else torch.zeros(2, 0, dtype=torch.long)


@pytest.mark.parametrize("dense", [False, True], ids=["E0", "E3N"])
@pytest.mark.parametrize("N", [17, 1023, 1025])
def test_graph_builders(N, dense):
    """lg_graph_build and lg_graph_build_w, outputs carved at exactly E + N slots, against oracle.graph_ref
    .gcn_csr and tests/test_gpu_edge_weight.py's csr_ref bit for bit over the rowptr[N] slots in use (the
    slots of col, w, eid and their transposes past rowptr[N], left by dropped self loops, are documented
    as not written: they are cut off before the run-to-run comparison, and w / w_t are excluded from the NaN
    check, which looks at float outputs only).  Workspace words: counts and cursors (4 N int32) are
    zeroed and loop_e set to -1 by hipMemsetAsync in the entry point; dis / item are written for every
    node / used slot before they are read.  No word is polled."""
    from oracle import graph_ref
    from test_gpu_edge_weight import csr_ref
    lib, _ = _lib()
    E = 3 * N if dense else 0
    ei = _edges(N, E, N + E)
    ew = torch.empty(E).uniform_(0.1, 2.0, generator=torch.Generator().manual_seed(N))
    eid, ewd = ei.to(DEV), ew.to(DEV)
    i32, f32 = torch.int32, torch.float32
    csr = {"rowptr": ((N + 1,), i32), "col": ((E + N,), i32), "w": ((E + N,), f32), "rowptr_t": ((N + 1,), i32),
           "col_t": ((E + N,), i32), "w_t": ((E + N,), f32)}
    partial = ("w", "w_t")  # floats among the outputs whose slots past rowptr[N] are not written

    def used(o):
        """The slots the call defines: col / w / eid and their transposes up to rowptr[N] (the fills behind them
        differ between the arena and a plain tensor only by accident of the fill value)."""
        nnz = {"": int(o["rowptr"][-1]), "_t": int(o["rowptr_t"][-1])}
        return {n: (v[:nnz["_t" if n.endswith("_t") else ""]] if n.split("_")[0] in ("col", "w", "eid") else v)
                for n, v in o.items()}
    nws = int(lib.lg_graph_workspace_bytes(E, N))

    def ref(o):
        for tr, (rp, c, w) in ((False, ("rowptr", "col", "w")), (True, ("rowptr_t", "col_t", "w_t"))):
            rp_o, c_o, w_o = graph_ref.gcn_csr(ei.numpy(), N, True, True, 1.0, transpose=tr)
            nnz = int(rp_o[-1])
            np.testing.assert_array_equal(o[rp].cpu().numpy(), rp_o)
            np.testing.assert_array_equal(o[c].cpu().numpy()[:nnz], c_o)
            np.testing.assert_array_equal(o[w].cpu().numpy()[:nnz].view(np.uint32), w_o.view(np.uint32))

    _hygiene(lambda P: lib.lg_graph_build(_p(eid) if E else None, E, N, 1, 1, 1.0, P["rowptr"], P["col"], P["w"], P["rowptr_t"],
                                          P["col_t"], P["w_t"], P["workspace"], nws, _st()),
             {"workspace": nws}, csr, {"edge_index": eid}, ref=ref, may_keep_nan=partial, post=used)

    outs = dict(csr, eid=((E + N,), i32), eid_t=((E + N,), i32), dis=((N,), f32))
    nws_w = int(lib.lg_graph_build_w_workspace_bytes(E, N))

    def ref_w(o):
        for tr, (rp, c, e, w) in ((False, ("rowptr", "col", "eid", "w")), (True, ("rowptr_t", "col_t", "eid_t", "w_t"))):
            rp_o, c_o, e_o, w_o = csr_ref(ei.numpy(), ew.numpy(), N, True, True, 1.0, transpose=tr)
            nnz = int(rp_o[-1])
            np.testing.assert_array_equal(o[rp].cpu().numpy(), rp_o)
            np.testing.assert_array_equal(o[c].cpu().numpy()[:nnz], c_o)
            np.testing.assert_array_equal(o[e].cpu().numpy()[:nnz], e_o)
            np.testing.assert_array_equal(o[w].cpu().numpy()[:nnz].view(np.uint32), w_o.view(np.uint32))
        assert not bool(torch.isnan(o["dis"]).any())

    order = ("rowptr", "col", "w", "eid", "rowptr_t", "col_t", "w_t", "eid_t", "dis")
    _hygiene(lambda P: lib.lg_graph_build_w(_p(eid) if E else None, _p(ewd) if E else None, E, N, 1, 1, 1.0,
                                            *[P[n] for n in order], P["workspace"], nws_w, _st()),
             {"workspace": nws_w}, outs, {"edge_index": eid, "edge_weight": ewd}, ref=ref_w, may_keep_nan=partial, post=used)


@pytest.mark.parametrize("dense", [False, True], ids=["P0", "P3N"])
@pytest.mark.parametrize("N", [17, 1023, 1025])
def test_incidence_build(N, dense):
    """lg_incidence_build against oracle.graph_ref.incidence_csr, bit for bit; inc_item at exactly 2P slots.
    Workspace: counts and cursors (2 N int32), zeroed by the entry point's hipMemsetAsync."""
    from oracle import graph_ref
    lib, _ = _lib()
    Pn = 3 * N if dense else 0
    ends = _edges(N, Pn, 7 * N).t().contiguous()  # (P, 2)
    endd = ends.to(DEV)
    nws = int(lib.lg_incidence_workspace_bytes(Pn, N))

    def ref(o):
        rp, it = graph_ref.incidence_csr(ends.numpy().reshape(Pn, 2), N)
        np.testing.assert_array_equal(o["inc_rowptr"].cpu().numpy(), rp)
        np.testing.assert_array_equal(o["inc_item"].cpu().numpy(), it)

    _hygiene(lambda P: lib.lg_incidence_build(_p(endd) if Pn else None, Pn, N, P["inc_rowptr"], P["inc_item"] if Pn else None,
                                              P["workspace"], nws, _st()),
             {"workspace": nws}, {"inc_rowptr": ((N + 1,), torch.int32), "inc_item": ((2 * Pn,), torch.int32)},
             {"ends": endd}, ref=ref)


# ----------------------------------------------------------------------------- evaluator and optimizer tails
@pytest.mark.parametrize("W", [1, 37])
def test_event_decide(W):
    """lg_event_decide against tests/test_window_metrics_host.py's event_truth (out exactly, summed bit for
    bit).  Workspace: W int32 alarm words, each written by k_event_alarm before k_event_decide (the next
    launch on the stream) reads them as booleans; none is an index or a polled word."""
    from test_window_metrics_host import event_truth
    lib, _ = _lib()
    rng = np.random.default_rng(W)
    C, noleak, step = 13, 12, 300 * 10 ** 9
    x = rng.standard_normal((W, C)).astype(np.float32)
    x[:, noleak] += 30.0
    x[W // 3, 4] = 99.0  # the trigger
    end_ns = (np.arange(W, dtype=np.int64) * 300 + 11) * 10 ** 9
    xd, ed = torch.from_numpy(x).to(DEV), torch.from_numpy(end_ns).to(DEV)
    nws = int(lib.lg_event_decide_workspace_bytes(W))
    assert nws == 4 * W

    def ref(o):
        trig, stop, pred, s = event_truth(x, end_ns, 5 * step, noleak)
        assert o["out"].cpu().tolist() == [trig, stop, pred] and trig == W // 3
        assert np.array_equal(o["summed"].cpu().numpy().view(np.uint32), s.view(np.uint32))

    _hygiene(lambda P: lib.lg_event_decide(_p(xd), _p(ed), W, C, C, 5 * step, noleak, P["out"], P["summed"], P["workspace"],
                                           nws, _st()),
             {"workspace": nws}, {"out": ((3,), torch.int64), "summed": ((C,), torch.float32)}, {"logits": xd, "end_ns": ed},
             ref=ref)


@pytest.mark.parametrize("max_norm", [0.5, 0.0])
def test_clip_adamw(max_norm):
    """lg_clip_adamw over T = 3 tensors of 1, 1000 and 70001 elements (70 slices: the one-launch form),
    against tests/test_gpu_step_tail.py's fp64 AdamW under its bars.  step is caller state by contract:
    zeros at creation (step[1], the ticket the launch spins on, is NOT in the workspace and is never
    poisoned); the workspace holds one fp64 partial per slice, stored by each workgroup before its
    arrival and read after the (bounded) barrier.  param, grad and both moments are updated in place:
    they are carved as outputs and set to the same initial state before every run.  max_norm = 0 with a
    norm output is still the one-launch form."""
    from test_gpu_step_tail import _adam_bars, _adam_state, _cat, _ref_adamw, _torch_step
    lib, _ = _lib()
    sizes = [1, 1000, 70001]
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
    P0, G0, M0, V0 = _adam_state(sizes, 3, moments=True)
    csz = (ctypes.c_int64 * 3)(*sizes)
    nws = int(lib.lg_clip_adamw_workspace_bytes(ctypes.addressof(csz), 3))
    assert nws == 8 * ((sum(sizes) + 1023) // 1024)  # one fp64 partial per 1024-element slice
    outs = {f"{k}{t}": ((n,), torch.float32) for t, n in enumerate(sizes) for k in "pgmv"}
    outs["step"] = ((4,), torch.float32)
    outs["norm"] = ((1,), torch.float32)

    def setup(v):
        for t in range(3):
            for k, L in zip("pgmv", (P0, G0, M0, V0)):
                v[f"{k}{t}"].copy_(L[t])
        v["step"].zero_()
        v["step"][0] = 4.0

    def call(P):
        table = (ctypes.c_int64 * 12)(*[P[f"{k}{t}"] for t in range(3) for k in "pgmv"])
        return lib.lg_clip_adamw(ctypes.addressof(table), ctypes.addressof(csz), 3, P["step"], hp["lr"], hp["b1"], hp["b2"],
                                 hp["eps"], hp["wd"], max_norm, P["norm"], P["workspace"], nws, _st())

    def ref(o):
        assert (o["step"][0].item(), *o["step"][1:3].view(torch.int32).tolist()) == (5.0, 0, 0)
        got = {k: _cat([o[f"{c}{t}"] for t in range(3)]) for k, c in (("p", "p"), ("g", "g"), ("m", "m"), ("v", "v"))}
        got["update"] = got["p"] - _cat(P0)
        got["norm"] = o["norm"][0].double().cpu()
        _adam_bars(got, _torch_step(P0, G0, M0, V0, 4, hp, max_norm), _ref_adamw(P0, G0, M0, V0, 4, hp, max_norm),
                   f"hygiene max_norm={max_norm}")

    _hygiene(call, {"workspace": nws}, outs, {}, ref=ref, setup=setup)


# ----------------------------------------------------------------------------- GRU: fused node init, stacked layers
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("I", [1, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_gru_node_init_backward(B, I, H):
    """lg_gru_node_init_bwd on what lg_gru_node_init_fwd saved (its private lane-order h_seq / gates), S = 5
    sensors of a 41-node graph, L = 36, live with one dead sensor, dbias_in given.  Workspace:
    ceil(B*S / 32) slab rows of the six gradients; k_gru_bwd2 stores its row before reduce_gru_slab reads
    that count; the memset path is B == 0 only; nothing polled.  Reference: nn.GRU in fp64 driven by dh_last =
    dproj W[:, :H], dproj = dx0[sensor rows] * live; dproj_w = dproj^T [h_L, 1]; dproj_b = sum dproj + dbias_in."""
    lib, _ = _lib()
    S, L, N = 5, 36, 41
    slot, idx = _slot5(N)
    sidx = idx.to(DEV)
    gen = torch.Generator().manual_seed(17 * B + I + H)
    dx0 = torch.randn(N, B, H, generator=gen)
    Wp = torch.randn(H, H + 1, generator=gen) / 8
    nbias, dbin = torch.randn(H, generator=gen), torch.randn(H, generator=gen)
    live = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0])
    dproj = dx0.double()[idx].permute(1, 0, 2) * live.double()[None, :, None]          # (B, S, H)
    dh = (dproj @ Wp.double()[:, :H]).reshape(B * S, H)
    dev, _, _, _, hL64, _, g64 = _gru_case(B, S, L, I, H, 1000 * B + 10 * I + H, dh=dh.float())
    nb16 = (B * S + 15) // 16
    h_seq = torch.empty(L * nb16 * 16 * H, device=DEV)
    gates = torch.empty(4 * L * nb16 * 16 * H, device=DEV)
    h_last = torch.empty(B * S, H, device=DEV)
    xs0 = torch.empty(S, B, H, device=DEV)
    bits = torch.zeros(N * ((B + 15) // 16) * 64, dtype=torch.int16, device=DEV)
    d = {k: v.to(DEV) for k, v in dict(dx0=dx0, Wp=Wp, nbias=nbias, dbin=dbin, live=live).items()}
    rc = lib.lg_gru_node_init_fwd(_p(dev["r"]), _p(dev["tf"]), _p(dev["w_ih"]), _p(dev["w_hh"]), _p(dev["b_ih"]),
                                  _p(dev["b_hh"]), _p(h_seq), _p(gates), _p(h_last), _p(slot), _p(sidx), _p(d["Wp"]),
                                  _p(d["nbias"]), _p(xs0), _p(bits), B, L, S, I, H, N, 0, 0.0, 0, 0, _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert_close(h_last, hL64, what="GRU h_L")
    nws = int(lib.lg_gru_node_init_bwd_workspace_bytes(B, S, I, H))
    outs = {"dw_ih": ((3 * H, I), torch.float32), "dw_hh": ((3 * H, H), torch.float32), "db_ih": ((3 * H,), torch.float32),
            "db_hh": ((3 * H,), torch.float32), "dproj_w": ((H, H + 1), torch.float32), "dproj_b": ((H,), torch.float32)}

    def call(P):
        return lib.lg_gru_node_init_bwd(_p(dev["r"]), _p(dev["tf"]), _p(dev["w_ih"]), _p(dev["w_hh"]), _p(h_seq), _p(gates),
                                        _p(d["dx0"]), _p(sidx), _p(d["live"]), _p(d["Wp"]), _p(d["dbin"]), P["dw_ih"],
                                        P["dw_hh"], P["db_ih"], P["db_hh"], P["dproj_w"], P["dproj_b"], B, L, S, I, H, N,
                                        P["workspace"], nws, _st())

    def ref(o):
        h1 = torch.cat([hL64.reshape(B, S, H), torch.ones(B, S, 1, dtype=torch.float64)], -1)
        want = dict(g64, dproj_w=torch.einsum("bso,bsi->oi", dproj, h1), dproj_b=dproj.sum(dim=(0, 1)) + dbin.double())
        names = {"weight_ih_l0": "dw_ih", "weight_hh_l0": "dw_hh", "bias_ih_l0": "db_ih", "bias_hh_l0": "db_hh",
                 "dproj_w": "dproj_w", "dproj_b": "dproj_b"}
        assert_grads_close([(n, o[k]) for n, k in names.items()], want, prefix="GRU+node init grad ")

    consts = {k: v for k, v in dev.items() if v is not None}
    consts.update(d, h_seq=h_seq, gates=gates)
    _hygiene(call, {"workspace": nws}, outs, consts, ref=ref)


SEQ_CASES = [(n, i, h, 5) for n in (1, 17) for i in (10, 64) for h in (64, 128)] + [(17, 10, 128, 1)]


@pytest.mark.parametrize("Nseq,I,H,L", SEQ_CASES)
def test_gru_seq_backward(Nseq, I, H, L):
    """lg_gru_seq_bwd, dense input, with dh_seq, dh_last and dx: (I, H) = (64, 64) the MFMA kernel, (10, 64)
    the generic one, H = 128 the tiled layers of csrc/gru128.hip (lg_gru_seq_tiled).  Workspace at H = 128:
    min(32, ceil(Nseq / 8)) slab rows, the dh carry [Nseq][H] and dG for a pass of steps; one pass here, so
    the carry is written and never read; k_gru128_bwd_rec writes dG before k_gru128_dw / k_gru128_dx read
    it, and every (row block, gate tile) workgroup of k_gru128_dw stores its slab segment (no early return;
    L = 1 at Nseq = 17 leaves the third row block without rows: it stores zeros).  Elsewhere: one slab row
    per workgroup, stored before reduce_gru_slab; memset only at Nseq == 0.  Nothing polled."""
    lib, _ = _lib()
    assert lib.lg_gru_seq_tiled(I, H, 1) == int((I, H) != (10, 64))
    gen = torch.Generator().manual_seed(Nseq + I + H + L)
    gru = torch.nn.GRU(I, H)
    with torch.no_grad():
        for p in gru.parameters():
            p.uniform_(-0.3, 0.3, generator=gen)
    x = torch.randn(L, Nseq, I, generator=gen)
    dhs, dhl = torch.randn(L, Nseq, H, generator=gen), torch.randn(Nseq, H, generator=gen)
    w = {k: v.detach().to(DEV) for k, v in dict(w_ih=gru.weight_ih_l0, w_hh=gru.weight_hh_l0, b_ih=gru.bias_ih_l0,
                                                b_hh=gru.bias_hh_l0).items()}
    xd, dhsd, dhld = x.to(DEV), dhs.to(DEV), dhl.to(DEV)
    h_seq, gates = torch.empty(L, Nseq, H, device=DEV), torch.empty(L, Nseq, 4, H, device=DEV)
    rc = lib.lg_gru_seq_fwd(_p(xd), _p(w["w_ih"]), _p(w["w_hh"]), _p(w["b_ih"]), _p(w["b_hh"]), _p(h_seq), _p(gates), Nseq, L,
                            I, H, 0, 0.0, 0, 0, _st())
    torch.cuda.synchronize()
    assert rc == 0
    g64 = torch.nn.GRU(I, H).double()
    g64.load_state_dict({k: v.double() for k, v in gru.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    out, hL = g64(x64)
    ((out * dhs.double()).sum() + (hL[0] * dhl.double()).sum()).backward()
    assert_close(h_seq, out.detach(), what="h_seq")
    nws = int(lib.lg_gru_seq_bwd_workspace_bytes(Nseq, I, H))
    outs = {"dx": ((L, Nseq, I), torch.float32), "dw_ih": ((3 * H, I), torch.float32), "dw_hh": ((3 * H, H), torch.float32),
            "db_ih": ((3 * H,), torch.float32), "db_hh": ((3 * H,), torch.float32)}

    def call(P):
        return lib.lg_gru_seq_bwd(_p(xd), None, None, _p(w["w_ih"]), _p(w["w_hh"]), _p(h_seq), _p(gates), _p(dhsd), _p(dhld),
                                  P["dx"], P["dw_ih"], P["dw_hh"], P["db_ih"], P["db_hh"], 0, 0, Nseq, L, I, H, 0, 0.0, 0, 0,
                                  P["workspace"], nws, _st())

    def ref(o):
        names = {"weight_ih_l0": "dw_ih", "weight_hh_l0": "dw_hh", "bias_ih_l0": "db_ih", "bias_hh_l0": "db_hh"}
        assert_grads_close([(n, o[k]) for n, k in names.items()], {n: p.grad for n, p in g64.named_parameters()},
                           prefix="GRU layer grad ")
        assert_close(o["dx"], x64.grad, what="dx")

    _hygiene(call, {"workspace": nws}, outs, dict(w, x=xd, h_seq=h_seq, gates=gates, dh_seq=dhsd, dh_last=dhld), ref=ref)


# ----------------------------------------------------------------------------- EdgeHead and both heads
def _pipes(kind):
    """hub: one pipe per distinct unordered edge of the hub graph (P about 2N); six: P = 6."""
    from test_gpu_skip import _hub_graph
    if kind == "six":
        return torch.tensor([[0, 3], [3, 7], [7, 0], [11, 16], [16, 2], [5, 9]])
    e = _hub_graph(41, 5).t()
    e = torch.unique(torch.sort(e, dim=1).values, dim=0)
    return e[e[:, 0] != e[:, 1]].contiguous()


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


EDGE_CASES = [(e, pk, B, D, tr, sc) for e in ("lg_edge_head_bwd", "lg_edge_head_bwd_scatter", "lg_heads_bwd_scatter")
              for pk in ("hub", "six") for B in (1, 17) for D in (32, 64) for tr in (False, True)
              for sc in ((False,) if e == "lg_edge_head_bwd" else (False, True))]
EDGE_CASES += [(e, "hub", 0, 32, True, sc) for e in ("lg_edge_head_bwd_scatter", "lg_heads_bwd_scatter") for sc in (False, True)]


@pytest.mark.parametrize("entry,pkind,B,D,train,sched", EDGE_CASES)
def test_edge_and_heads_backward(entry, pkind, B, D, train, sched):
    """lg_edge_head_bwd, lg_edge_head_bwd_scatter and lg_heads_bwd_scatter on what the two forward entry
    points saved; N = 41, eval and train (p = 0.1), without and with a pipe schedule.  B = 0 in the list
    stands for B = the CU count, where the scatter entry points take their one-workgroup-per-window forms
    (streamed with a schedule, per-window without); at B = 1 and 17 (fewer windows than CUs) they run the
    two launches.  Workspace: `grid` slab rows (dW1, db1, dw2, padded) rounded up to 256 bytes, then one
    fp64 per workgroup; every workgroup of k_edge_bwd (all three forms) stores its row and its fp64 at the
    kernel's end, no early return; zero-fill only at B*P == 0.  The NoLeakHead's workspace in the fused
    form: one row per edge workgroup, written in the prologue.  No word is polled; the schedule and the
    incidence CSR are inputs.  Excluded from the NaN check: dpipe in the streamed form (documented as
    untouched there).  dpool is an input of lg_edge_head_bwd_scatter and an output of lg_heads_bwd_scatter."""
    from models import ops
    lib, nat = _lib()
    N, HID = 41, 128
    B = B or _cus()
    ends = _pipes(pkind)
    P = ends.shape[0]
    inc = ops.Incidence.build(ends, N, DEV, schedule=sched)
    sc, hdr = inc.schedule(D) if sched else (None, [])
    chdr = (ctypes.c_int32 * 16)(*hdr) if sched else None
    gen = torch.Generator().manual_seed(B + D + P + int(train))
    h = torch.randn(B, N, D, generator=gen).to(DEV)
    w1 = (torch.randn(HID, 3 * D, generator=gen) / (3 * D) ** 0.5).to(DEV)
    b1 = (0.1 * torch.randn(HID, generator=gen)).to(DEV)
    w2 = (torch.randn(HID, generator=gen) / HID ** 0.5).to(DEV)
    b2 = torch.randn(1, generator=gen).to(DEV)
    nw1 = (torch.randn(HID, D, generator=gen) / D ** 0.5).to(DEV)
    nb1 = (0.1 * torch.randn(HID, generator=gen)).to(DEV)
    nw2 = (torch.randn(HID, generator=gen) / HID ** 0.5).to(DEV)
    dlog = torch.randn(B, P + 1, generator=gen).to(DEV)
    dpool_in = torch.randn(B, D, generator=gen).to(DEV)
    flags, p = (nat.LG_F_DROPOUT, 0.1) if train else (0, 0.0)
    logits = torch.zeros(B, P + 1, device=DEV)
    hid = torch.empty(B * P, HID, device=DEV)
    pooled, nhid = torch.empty(B, D, device=DEV), torch.empty(B, HID, device=DEV)
    assert lib.lg_edge_head_fwd(_p(inc.ends), _p(h), _p(w1), _p(b1), _p(w2), _p(b2), _p(logits), P + 1, _p(hid), B, N, P, D, HID,
                                flags, p, 777, 3, _st()) == 0
    assert lib.lg_pool_head_fwd(_p(h), _p(nw1), _p(nb1), _p(nw2), _p(b2), _p(pooled), _p(nhid), _p(logits), P + 1, P, B, N, D,
                                HID, flags, p, 777, 4, _st()) == 0
    torch.cuda.synchronize()
    nws = int(lib.lg_edge_head_bwd_workspace_bytes(B, P, D, HID))
    nnws = int(lib.lg_pool_head_bwd_workspace_bytes(B, D, HID))
    f32 = torch.float32
    outs = {"dpipe": ((B, P, 2, D), f32), "dw1": ((HID, 3 * D), f32), "db1": ((HID,), f32), "dw2": ((HID,), f32), "db2": ((1,), f32)}
    ws = {"workspace": nws}
    heads = entry == "lg_heads_bwd_scatter"
    if entry != "lg_edge_head_bwd":
        outs["dh"] = ((B, N, D), f32)
    if heads:
        outs.update(dpool=((B, D), f32), ndw1=((HID, D), f32), ndb1=((HID,), f32), ndw2=((HID,), f32), ndb2=((1,), f32))
        ws["nworkspace"] = nnws
    streamed = sched and entry != "lg_edge_head_bwd" and B >= _cus()

    def call(P_):
        edge = (_p(inc.ends), _p(h), _p(w1), _p(w2), _p(hid), _p(dlog), P + 1, P_["dpipe"], P_["dw1"], P_["db1"], P_["dw2"], P_["db2"])
        tail = (B, N, P, D, HID, flags, p, P_["workspace"], nws, _st())
        if entry == "lg_edge_head_bwd":
            return lib.lg_edge_head_bwd(*edge, *tail)
        scat = (_p(inc.rowptr), _p(inc.item), _p(sc), chdr)
        if not heads:
            return lib.lg_edge_head_bwd_scatter(*edge, *scat, _p(dpool_in), P_["dh"], *tail)
        return lib.lg_heads_bwd_scatter(_p(pooled), _p(nhid), _p(nw1), _p(nw2), P_["ndw1"], P_["ndb1"], P_["ndw2"], P_["ndb2"],
                                        flags, p, P_["nworkspace"], nnws, *edge, *scat, P_["dpool"], P_["dh"], *tail)

    def ref(o):
        sc_ = 1.0 / (1.0 - p)
        h64, e = h.double().cpu(), ends
        hu, hv = h64[:, e[:, 0]], h64[:, e[:, 1]]
        feat = torch.cat([hu, hv, (hu - hv).abs()], -1)                                  # (B, P, 3D)
        dl = dlog.double().cpu()
        hd = hid.double().cpu().reshape(B, P, HID)
        dpre = dl[:, :P, None] * w2.double().cpu() * (hd > 0) * sc_
        dfeat = dpre @ w1.double().cpu()
        sg = torch.sign(hu - hv)
        dpipe = torch.stack([dfeat[..., :D] + sg * dfeat[..., 2 * D:], dfeat[..., D:2 * D] - sg * dfeat[..., 2 * D:]], 2)
        want = {"dw1": torch.einsum("bpo,bpi->oi", dpre, feat), "db1": dpre.sum(dim=(0, 1)),
                "dw2": (dl[:, :P, None] * hd).sum(dim=(0, 1)), "db2": dl[:, :P].sum().reshape(1)}
        if not streamed:
            want["dpipe"] = dpipe
        if heads:
            nh, pl = nhid.double().cpu(), pooled.double().cpu()
            npre = dl[:, P, None] * nw2.double().cpu() * (nh > 0) * sc_
            want.update(dpool=npre @ nw1.double().cpu(), ndw1=npre.t() @ pl, ndb1=npre.sum(0),
                        ndw2=(dl[:, P, None] * nh).sum(0), ndb2=dl[:, P].sum().reshape(1))
        if "dh" in o:
            dpool = want["dpool"] if heads else dpool_in.double().cpu()
            dh = (dpool / N)[:, None, :].expand(B, N, D).clone()
            dh.index_add_(1, e[:, 0], dpipe[:, :, 0])
            dh.index_add_(1, e[:, 1], dpipe[:, :, 1])
            want["dh"] = dh
        _check(o, want, entry)

    consts = {"h": h, "w1": w1, "w2": w2, "hid": hid, "dlogits": dlog, "inc_item": inc.item, "inc_rowptr": inc.rowptr,
              "pooled": pooled, "nhid": nhid, "sched": sc}
    if not heads:
        consts["dpool"] = dpool_in
    _hygiene(call, ws, outs, consts, ref=ref, may_keep_nan=("dpipe",) if streamed else ())


# ----------------------------------------------------------------------------- learned edge weights
@functools.lru_cache(maxsize=None)
def _weighted_graph():
    """The hub graph plus an input self-loop edge on node 7 and two on node 3 (the later one supplies the
    loop weight, the earlier one is dropped), weighted."""
    from models import ops
    from test_gpu_skip import _hub_graph
    ei = torch.cat([_hub_graph(41, 5), torch.tensor([[7, 3, 3], [7, 3, 3]])], 1)
    ew = torch.empty(ei.shape[1]).uniform_(0.1, 2.0, generator=torch.Generator().manual_seed(9))
    return ei, ew


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("mask_in", [False, True])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("B", [1, 17])
def test_sddmm_and_norm_backward(B, D, mask_in, normalize):
    """lg_sddmm_nm, then lg_gcn_norm_bwd on its G.  sddmm workspace: ceil(B/16) x nnz_cap float partials;
    every (node, window tile) has a tile whose wave stores the partial of each slot of its row, so all
    (tile, slot < rowptr[N]) words are written before k_sddmm_nm_reduce reads exactly those; slots past
    rowptr[N] are written as 0 without a read.  norm_bwd workspace: E floats Ge; k_route_edges stores Ge[e]
    for every edge that owns a forward slot, and k_norm_bwd reads Ge[e] only through eid_t, whose edges all
    own a forward slot; dedge_weight is zeroed by the entry point (dropped self loops keep 0).  No polls,
    no index words.  References: fp64 of the header's formulas; dL/d edge_weight by autograd of the
    weighted gcn_norm in fp64 (tests/test_gpu_edge_weight.py's _edge_list order)."""
    from models import ops
    from test_gpu_edge_weight import _edge_list
    lib, nat = _lib()
    N = 41
    ei, ew = _weighted_graph()
    E = ei.shape[1]
    g = ops.GCNGraph.build(ei, N, DEV, add_self_loops=True, normalize=normalize, edge_weight=ew)
    cap = E + N
    x, W, dy, y, ymask = _trunk_inputs(g, N, B, D, 5 * D + B)
    scale = 1.0 / 0.9
    nws = int(lib.lg_sddmm_nm_workspace_bytes(B, cap))
    assert nws == (B + 15) // 16 * cap * 4
    nnz = int(g.rowptr[-1])

    def ref(o):
        dz = dy.double().cpu() * ((y.cpu() > 0) * scale if mask_in else 1.0)
        da = dz @ W.double().cpu()
        rp, col = g.rowptr.cpu().long(), g.col.cpu().long()[:nnz]
        rows = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
        want = torch.zeros(cap, dtype=torch.float64)
        want[:nnz] = (da[rows] * x.double().cpu()[col]).sum(dim=(1, 2))
        assert_close(o["G"], want, what="sddmm G")

    G = _hygiene(lambda P: lib.lg_sddmm_nm(_p(g.rowptr), _p(g.col), _p(dy), _p(y), None, _p(W), _p(x), P["G"], B, N, D, cap,
                                           nat.LG_F_MASK_IN if mask_in else 0, scale, P["workspace"], nws, _st()),
                 {"workspace": nws}, {"G": ((cap,), torch.float32)}, {"dy": dy, "y": y, "W": W, "x": x, "col": g.col}, ref=ref)["G"]
    nws2 = int(lib.lg_gcn_norm_bwd_workspace_bytes(E, N))
    ewd = g.edge_weight

    def ref2(o):
        src, dst, eid = (torch.from_numpy(a) for a in _edge_list(ei.numpy(), N, True))
        w64 = ew.double().requires_grad_(True)
        wt = torch.where(eid >= 0, w64[eid.clamp(min=0)], torch.ones((), dtype=torch.float64))
        if normalize:
            dis = torch.zeros(N, dtype=torch.float64).index_add(0, dst, wt).pow(-0.5)
            wn = dis[src] * wt * dis[dst]
        else:
            wn = wt
        order = torch.argsort(dst, stable=True)
        (wn[order] * G.double().cpu()[:nnz]).sum().backward()
        assert_close(o["dedge_weight"], w64.grad, what="d edge_weight")

    _hygiene(lambda P: lib.lg_gcn_norm_bwd(_p(G), _p(g.rowptr), _p(g.col), _p(g.eid), _p(g.rowptr_t), _p(g.col_t), _p(g.eid_t),
                                           _p(g.dis), _p(ewd), E, N, int(normalize), 1.0, P["dedge_weight"], P["workspace"],
                                           nws2, _st()),
             {"workspace": nws2}, {"dedge_weight": ((E,), torch.float32)}, {"G": G, "dis": g.dis, "edge_weight": ewd, "eid": g.eid},
             ref=ref2)


# ----------------------------------------------------------------------------- TCN stage backward
@pytest.mark.parametrize("nseg,rows", [(1, 1), (1, 17), (7, 5)])
@pytest.mark.parametrize("residual", [False, True])
def test_tcn_conv_backward(nseg, rows, residual):
    """lg_tcn_conv_bwd on lg_tcn_conv_train_fwd's saves (tests/test_gpu_tcn_train.py's smallest plan, a
    single longer segment, and several segments), dilation 1, p = 0.25, conv1 form (dres into dx) and conv2
    form (forward residual), with dx.  Workspace: one row of 3 x 128 floats per k_tcn_ln_bwd workgroup
    (dgamma, dbeta, db partials), rounded up to 256 bytes, then one row of 128 x 128 x 3 floats per
    k_tcn_dw row block; each launched workgroup stores its row and the two reductions read the launched
    counts; float words only, nothing polled.  Reference and bar: that module's _stage_ref in fp64 / fp32
    under assert_grads_match_truth on the kernel's own keep decisions."""
    from helpers import assert_grads_match_truth
    from models.ops import TCN_SALT
    from models.tcn_plan import train_tables
    from test_gpu_tcn_train import C, _rand_stage, _stage_gpu, _stage_ref
    lib, _ = _lib()
    gen = torch.Generator().manual_seed(100 * nseg + rows + int(residual))
    fwd, tr = train_tables(rows, (1,))
    table, table_t = torch.from_numpy(fwd[int(residual)]), torch.from_numpy(tr[int(residual)])
    p, seed, salt = 0.25, 1235, TCN_SALT + 5
    rows_blk = rows if residual else 0
    t = _rand_stage(gen, nseg, rows, rows_blk, table)
    dy = torch.randn(nseg * rows, C, generator=gen)
    dres = None if residual else torch.randn(nseg * rows, C, generator=gen)
    f, _ = _stage_gpu(t, p, seed, salt, nseg, rows, rows_blk, rows)
    d = {k: v.to(DEV) for k, v in dict(x=t["x"], w=t["w"], lw=t["lw"], table=table, table_t=table_t, dy=dy).items()}
    dresd = None if dres is None else dres.to(DEV)
    pkt = torch.empty(int(lib.lg_tcn_packed_weight_floats(C)), device=DEV)
    assert lib.lg_tcn_pack_weight_t(_p(d["w"]), _p(pkt), C, _st()) == 0
    torch.cuda.synchronize()
    nws = int(lib.lg_tcn_conv_bwd_workspace_bytes(nseg, rows, C))
    R = nseg * rows
    f32 = torch.float32
    outs = {"dz": ((R, C), f32), "dx": ((R, C), f32), "dw": ((C, C, 3), f32), "db": ((C,), f32), "dgamma": ((C,), f32),
            "dbeta": ((C,), f32)}

    def call(P):
        return lib.lg_tcn_conv_bwd(_p(d["dy"]), _p(f["s"]), _p(f["xhat"]), _p(f["rstd"]), _p(d["x"]), _p(dresd), _p(d["table"]),
                                   _p(d["table_t"]), _p(pkt), _p(d["lw"]), p, P["dz"], P["dx"], P["dw"], P["db"], P["dgamma"],
                                   P["dbeta"], nseg, rows, rows if dres is not None else 0, rows, C, P["workspace"], nws, _st())

    def ref(o):
        mask, scale = (f["s"] > 0).cpu(), 1.0 / (1.0 - p)
        _, g64 = _stage_ref(t, torch.float64, mask, scale, nseg, rows, rows_blk, dy, dres, table_t, rows)
        _, g32 = _stage_ref(t, torch.float32, mask, scale, nseg, rows, rows_blk, dy, dres, table_t, rows)
        assert_grads_match_truth(o, g32, g64)

    _hygiene(call, {"workspace": nws}, outs, dict(d, s=f["s"], xhat=f["xhat"], rstd=f["rstd"], pkt=pkt), ref=ref)
