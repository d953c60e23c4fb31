"""The transform flags of the node-major trunk select different kernels, and each selects the right
one: on the fp32 tier the default (2-way f16 split) and LG_F_BF16X3 (3-way bf16 split) both stay
inside the bars the other trunk tests hold them to AND differ from each other in at least one
element; LG_F_BF16 (one bf16 product) differs from both.  Both fp32-tier transforms sit inside the
same 1e-6 bars, so without the "differ" half a dispatch line that swapped them would pass every
other test.  Checked for the dense forward (k_gcn_fwd_pc, and k_gcn_fwd_nm3's two forms), the
compressed layer-0 forward (X0), the residual forward (SKIP) and the backward (dx and dW).

Shapes: a connected random graph of N = 300 nodes with one hub of degree > 8 in the forward and the
transposed CSR (a row past the six inline pairs of a node-table record), S = 5 sensors (the hub
among them), D in {32, 64}, B in {3, 17}: one ragged tile per node, and two window groups with a
ragged second one.  600 tiles at B = 17 make many workgroups on several XCD chunks; the inputs are
continuous random numbers, so two transforms that round differently cannot agree everywhere."""
from __future__ import annotations

import functools

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, S = 300, 5
P_DROP, SEED, SALT = 0.1, 0x5EED1234, 2


@functools.lru_cache(maxsize=None)
def _graph():
    """(graph, marks, slot): a random spanning tree (connected) plus N / 2 random edges plus a hub
    (node 0) with 12 more neighbours, every edge in both directions; sensors at 5 nodes."""
    from models import ops
    g = torch.Generator().manual_seed(17)
    child = torch.arange(1, N)
    parent = (torch.rand(N - 1, generator=g) * child).long()  # parent < child: a tree rooted at 0
    a, b = torch.randint(1, N, (N // 2,), generator=g), torch.randint(1, N, (N // 2,), generator=g)
    hub = torch.randperm(N - 1, generator=g)[:12] + 1
    src = torch.cat([child, a, hub])
    dst = torch.cat([parent, b, torch.zeros(12, dtype=torch.long)])
    ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    gph = ops.GCNGraph.build(ei, N, DEV)
    rp, rpt = gph.rowptr.cpu().long(), gph.rowptr_t.cpu().long()
    assert int(rp[1] - rp[0]) > 8 and int(rpt[1] - rpt[0]) > 8
    slot = torch.full((N,), -1, dtype=torch.int32)
    slot[torch.tensor([0, 7, 100, 200, 299])] = torch.arange(S, dtype=torch.int32)
    slot = slot.to(DEV)
    return gph, ops.SensorMarks.build(gph, slot), slot


def _differ(a, b, what):
    assert not torch.equal(a, b), f"{what}: bit-identical results, the flags selected the same transform"


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("D", [32, 64])
def test_transform_flags_select_distinct_kernels(D, B):
    from models import _native as nat
    from models import ops
    from models.library import expand_x0
    from models._native import ptr
    gph, mk, slot = _graph()
    lib = nat.load_library()
    gen = torch.Generator().manual_seed(1000 * D + B)
    x = torch.randn(N, B, D, generator=gen).relu().to(DEV)  # trunk inputs are post-ReLU
    W = (torch.randn(D, D, generator=gen) / 8).to(DEV)
    b = (torch.randn(D, generator=gen) / 4).to(DEV)
    st = ops.stream_of(x)
    flags = nat.LG_F_BIAS | nat.LG_F_RELU | nat.LG_F_DROPOUT
    X3, BF, PC, NM3, F32 = nat.LG_F_BF16X3, nat.LG_F_BF16, nat.LG_F_PC, nat.LG_F_NM3, nat.LG_F_F32_MFMA
    nmask = N * ((B + 15) // 16) * 64

    # ---- dense forward: every transform against the exact-fp32 form, 1e-6 of the output scale
    def fwd(extra, fn="lg_gcn_fwd_nm_bits", xin=None):
        y = torch.full((N, B, D), float("nan"), device=DEV)
        m = torch.zeros(nmask, dtype=torch.int16, device=DEV)
        ops.check(getattr(lib, fn)(ptr(gph.nodetab), ptr(gph.pairs), ptr(x if xin is None else xin), ptr(W), ptr(b),
                                   ptr(y), B, N, D, gph.nnz_cap, flags | extra, P_DROP, SEED, SALT, st, ptr(m)),
                  f"{fn} {extra:#x}")
        return y

    y_ref = fwd(F32)
    scale = y_ref.abs().max().item()
    y = {name: fwd(fl) for name, fl in (("f16x2", 0), ("bf16x3", X3), ("nm3", NM3), ("bf16 pc", BF | PC), ("bf16 nm3", BF))}
    for name in ("f16x2", "bf16x3"):
        err = (y[name].double() - y_ref.double()).abs().max().item()
        print(f"D={D} B={B} fwd {name}: err {err:.3e} (bar {1e-6 * scale:.3e})")
        assert err <= 1e-6 * scale, f"fwd {name}: off by {err:.3e} (scale {scale:.3e})"
    assert torch.equal(y["nm3"], y["bf16x3"]), "pc and nm3 run the same 3-way split"
    _differ(y["f16x2"], y["bf16x3"], "fwd default vs LG_F_BF16X3")
    _differ(y["nm3"], y_ref, "fwd LG_F_NM3 vs LG_F_F32_MFMA")
    for name in ("bf16 pc", "bf16 nm3"):
        for other in ("f16x2", "bf16x3"):
            _differ(y[name], y[other], f"fwd {name} vs {other}")

    # ---- layer 0 on the compressed input: each transform against the dense call on the same one
    xs0 = torch.randn(S, B, D, generator=gen).relu().to(DEV)
    bits = torch.randint(-2 ** 15, 2 ** 15, (nmask,), generator=gen, dtype=torch.int16).to(DEV)
    nbias = torch.randn(D, generator=gen).to(DEV)
    x0 = expand_x0(xs0, bits, slot, nbias, N, P_DROP)

    def fwd_x0(extra):
        out = torch.full((N, B, D), float("nan"), device=DEV)
        ops.check(lib.lg_gcn_fwd_nm_x0(ptr(mk.nodetab_s), ptr(mk.pairs_s), ptr(xs0), ptr(bits), ptr(nbias), ptr(W), ptr(b),
                                       ptr(out), B, N, S, D, flags | extra, P_DROP, SEED, SALT, st), f"fwd x0 {extra:#x}")
        return out

    yx = {name: fwd_x0(fl) for name, fl in (("f16x2", 0), ("bf16x3", X3), ("bf16", BF | PC))}
    for name, fl in (("f16x2", 0), ("bf16x3", X3)):
        dense = fwd(fl, xin=x0)
        sc = dense.abs().max().item()
        err = (yx[name] - dense).abs().max().item()
        print(f"D={D} B={B} x0 fwd {name}: err {err:.3e} (bar {1e-6 * sc:.3e})")
        assert err <= 1e-6 * sc, f"x0 fwd {name}: off the dense call by {err:.3e} (scale {sc:.3e})"
    _differ(yx["f16x2"], yx["bf16x3"], "x0 fwd default vs LG_F_BF16X3")
    _differ(yx["bf16"], yx["f16x2"], "x0 fwd LG_F_BF16 vs default")
    _differ(yx["bf16"], yx["bf16x3"], "x0 fwd LG_F_BF16 vs LG_F_BF16X3")

    # ---- residual forward: x + the plain call's result on the same transform, bit for bit
    ys = {name: fwd(fl, "lg_gcn_fwd_nm_skip") for name, fl in (("f16x2", 0), ("bf16x3", X3))}
    for name in ys:
        assert torch.equal(ys[name], x + y[name]), f"skip fwd {name} != x + plain {name}"
    _differ(ys["f16x2"], ys["bf16x3"], "skip fwd default vs LG_F_BF16X3")

    # ---- backward: dx and dW against the window-major fp32 kernels (RTOL of the scale, as
    # test_gcn_node_major_matches_window_major), MASK_IN from y, MASK_OUT, the node-bias sum
    dy = torch.randn(N, B, D, generator=gen).to(DEV)
    sc = 1.0 / (1.0 - P_DROP)
    bflags = nat.LG_F_MASK_IN | nat.LG_F_MASK_OUT

    def outs():
        return (torch.full((N, B, D), float("nan"), device=DEV), torch.empty(D, D, device=DEV),
                torch.empty(D, device=DEV), torch.empty(D, device=DEV))

    dx_w, dW_w, db_w, dnb_w = outs()
    xw, yw, dyw = (t.transpose(0, 1).contiguous() for t in (x, y_ref, dy))
    ws = torch.empty(int(lib.lg_gcn_bwd_workspace_bytes(D)), device=DEV, dtype=torch.uint8)
    ops.check(lib.lg_gcn_bwd(ptr(gph.rowptr_t), ptr(gph.col_t), ptr(gph.w_t), ptr(dyw), ptr(yw), ptr(xw), ptr(W), ptr(dx_w),
                             ptr(dW_w), ptr(db_w), ptr(slot), ptr(dnb_w), B, N, D, gph.nnz_cap, bflags, sc, sc, ptr(ws),
                             ws.numel(), st), "lg_gcn_bwd")
    dx_w = dx_w.view(B, N, D).transpose(0, 1)
    wsn = torch.empty(int(lib.lg_gcn_bwd_nm_workspace_bytes(D)), device=DEV, dtype=torch.uint8)

    def bwd(extra):
        dx, dW, db, dnb = outs()
        ops.check(lib.lg_gcn_bwd_nm(ptr(gph.nodetab_t), ptr(gph.pairs_t), ptr(dy), ptr(y_ref), ptr(x), ptr(W), ptr(dx),
                                    ptr(dW), ptr(db), ptr(slot), ptr(dnb), B, N, D, bflags | extra, sc, sc, ptr(wsn),
                                    wsn.numel(), st), f"lg_gcn_bwd_nm {extra:#x}")
        return dx, dW

    g = {name: bwd(fl) for name, fl in (("f16x2", 0), ("bf16x3", X3), ("bf16", BF))}
    for name in ("f16x2", "bf16x3"):
        for got, ref, what in zip(g[name], (dx_w, dW_w), ("dx", "dW")):
            err = (got.double() - ref.double()).abs().max().item()
            print(f"D={D} B={B} bwd {name} {what}: err {err:.3e} (scale {ref.abs().max().item():.3e})")
            assert_close(got, ref, what=f"bwd {name} {what}")
    for i, what in enumerate(("dx", "dW")):
        _differ(g["f16x2"][i], g["bf16x3"][i], f"bwd {what} default vs LG_F_BF16X3")
        _differ(g["bf16"][i], g["f16x2"][i], f"bwd {what} LG_F_BF16 vs default")
        _differ(g["bf16"][i], g["bf16x3"][i], f"bwd {what} LG_F_BF16 vs LG_F_BF16X3")
    torch.cuda.synchronize()
