"""Host side of the edge-weight entry points (no GPU): argument validation of the C ABI
(LG_EINVAL before any HIP call, with stand-in device pointers) and of GCNConv's edge_weight."""
from __future__ import annotations

import pytest
import torch


def _lib():
    from models import _native
    return _native.load_library()


def test_workspace_queries():
    lib = _lib()
    for fn in (lib.lg_graph_build_w_workspace_bytes, lib.lg_gcn_norm_bwd_workspace_bytes):
        assert fn(-1, 5) == -1 and fn(5, -1) == -1
        assert fn(0, 0) > 0
    assert lib.lg_graph_build_w_workspace_bytes(1532, 661) >= 4 * 5 * 661
    assert lib.lg_gcn_norm_bwd_workspace_bytes(1532, 661) >= 4 * 1532


def test_entry_points_reject_null_and_short_workspace():
    lib = _lib()
    F = 16  # a non-NULL stand-in device pointer (never dereferenced on these paths)
    E, N = 1532, 661
    wsb = lib.lg_graph_build_w_workspace_bytes(E, N)
    build = [F, F, E, N, 1, 1, 1.0, F, F, F, F, F, F, F, F, F, F, wsb, None]
    for i in (0, 1, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16):  # every pointer in turn
        args = list(build)
        args[i] = None
        assert lib.lg_graph_build_w(*args) == -1, i
    short = list(build)
    short[17] = wsb - 1
    assert lib.lg_graph_build_w(*short) == -1
    assert lib.lg_graph_build_w(*(build[:3] + [0] + build[4:])) == -1   # N == 0
    assert lib.lg_graph_build_w(*(build[:2] + [-1] + build[3:])) == -1  # E < 0

    rew = [F, F, F, F, F, F, F, E, N, 1, 1.0, F, F, F, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 11, 12, 13):
        args = list(rew)
        args[i] = None
        assert lib.lg_graph_reweight(*args) == -1, i
    assert lib.lg_graph_reweight(*(rew[:8] + [0] + rew[9:])) == -1

    wsn = lib.lg_gcn_norm_bwd_workspace_bytes(E, N)
    bwd = [F, F, F, F, F, F, F, F, F, E, N, 1, 1.0, F, F, wsn, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
        args = list(bwd)
        args[i] = None
        assert lib.lg_gcn_norm_bwd(*args) == -1, i
    short = list(bwd)
    short[15] = wsn - 1
    assert lib.lg_gcn_norm_bwd(*short) == -1

    sd = [F, F, F, 64, F, 64, F, N, 64, None]
    for i in (0, 1, 2, 4, 6):
        args = list(sd)
        args[i] = None
        assert lib.lg_sddmm_cols(*args) == -1, i
    assert lib.lg_sddmm_cols(F, F, F, 63, F, 64, F, N, 64, None) == -1  # lda < C
    assert lib.lg_sddmm_cols(F, F, F, 64, F, 63, F, N, 64, None) == -1  # ldb < C
    assert lib.lg_sddmm_cols(F, F, F, 64, F, 64, F, -1, 64, None) == -1
    assert lib.lg_sddmm_cols(None, None, None, 64, None, 64, None, 0, 64, None) == 0  # nothing to do, no launch
    assert lib.lg_sddmm_cols(None, None, None, 64, None, 64, None, N, 0, None) == 0


def test_gcnconv_rejects_bad_edge_weight_before_the_device():
    from models.gcn import GCNConv
    conv = GCNConv(8, 8)
    x, ei = torch.zeros(5, 8), torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(ValueError):
        conv(x, ei, torch.ones(4))
    with pytest.raises(ValueError):
        conv(x, ei, torch.ones(3, 1))
    with pytest.raises(TypeError):
        conv(x, ei, torch.ones(3, dtype=torch.long))
    with pytest.raises(TypeError):
        conv(x, ei, [1.0, 1.0, 1.0])
    assert conv._wgraph is None  # nothing was built
