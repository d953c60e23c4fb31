"""NormalPredictorGRU on the library: the parts that need no GPU (module tree, CPU forward, the new
entry points' bindings, argument checks, fast-path eligibility)."""
from __future__ import annotations

import pytest
import torch
import torch.nn as nn


def _lib():
    from models import _native
    return _native.load_library()


def test_state_dict_and_cpu_forward():
    from models.predictor import NormalPredictorGRU
    torch.manual_seed(0)
    m = NormalPredictorGRU(29, 9).eval()
    keys = [f"gru.{n}_l{l}" for l in range(2) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    assert list(m.state_dict()) == keys + ["head.weight", "head.bias"]
    gru = nn.GRU(38, 128, num_layers=2, batch_first=True, dropout=0.1).eval()
    head = nn.Linear(128, 29)
    gru.load_state_dict(m.gru.state_dict())
    head.load_state_dict(m.head.state_dict())
    x, tf = torch.randn(3, 7, 29), torch.randn(3, 7, 9)
    with torch.no_grad():
        want = head(gru(torch.cat([x, tf], -1))[0][:, -1])
        got = m(x, tf)
    assert torch.equal(got, want)


def test_entry_points_exposed():
    from models import _native, library  # noqa: F401
    lib = _lib()
    for name in ("lg_gru_seq_tiled", "lg_gru_seq_infer", "lg_gru_win_fwd"):
        assert name in _native.SIGNATURES
        assert getattr(lib, name) is not None
    assert hasattr(torch.ops.leakgnn, "gru_predictor") and hasattr(torch.ops.leakgnn, "gru_predictor_backward")
    assert lib.lg_abi_version() == _native.ABI_VERSION


def test_tiled_predicate_and_validation():
    lib = _lib()
    for I in (1, 38, 128, 1024):
        for d in (0, 1):
            assert lib.lg_gru_seq_tiled(I, 128, d) == 1
    assert lib.lg_gru_seq_tiled(38, 64, 0) == 0 and lib.lg_gru_seq_tiled(1025, 128, 0) == 0
    assert lib.lg_gru_seq_tiled(32, 32, 0) == 1 and lib.lg_gru_seq_tiled(64, 64, 1) == 1
    F = 64  # a non-null address that is never read: every call below is rejected before a launch
    EINVAL, EUNSUP = -1, -2
    assert lib.lg_gru_seq_infer(F, F, F, F, F, None, None, 4, 3, 38, 128, 0, 0.0, 0, 0, None) == EINVAL
    assert lib.lg_gru_seq_infer(F, F, F, F, F, F, F, 4, 3, 38, 64, 0, 0.0, 0, 0, None) == EUNSUP
    assert lib.lg_gru_seq_infer(F, F, F, F, F, F, F, 4, 0, 38, 128, 0, 0.0, 0, 0, None) == EINVAL
    assert lib.lg_gru_win_fwd(F, F, F, F, F, 2, 8, 5, 4, 64, None) == EUNSUP
    assert lib.lg_gru_win_fwd(F, F, F, F, F, 2, 7, 5, 4, 128, None) == EINVAL     # T < l_pred + n_win - 1
    assert lib.lg_gru_win_fwd(F, F, F, None, None, 2, 9, 5, 4, 128, None) == EINVAL
    # the backward's workspace covers the slab rows, the dh carry and at least one step of dG
    ws = lib.lg_gru_seq_bwd_workspace_bytes(40, 38, 128)
    assert ws >= 4 * (5 * (384 * (128 + 38) + 768) + 40 * 128 + 40 * 512)
    assert lib.lg_gru_seq_bwd(F, None, None, F, F, F, F, F, None, None, F, F, F, F, 0, 0, 40, 3, 38, 128, 0, 0.0, 0, 0,
                              F, 4 * (5 * (384 * (128 + 38) + 768) + 40 * 128), None) == EINVAL


def test_op_shape_checks():
    from models import library
    H, I = 128, 38
    x = torch.zeros(2, 5, I)
    good = dict(w_ih=[torch.zeros(3 * H, I), torch.zeros(3 * H, H)], w_hh=[torch.zeros(3 * H, H)] * 2,
                b_ih=[torch.zeros(3 * H)] * 2, b_hh=[torch.zeros(3 * H)] * 2)
    assert library._predictor_dims(x, **good) == (2, 5, I, H, 2)
    for key, bad in (("w_ih", [torch.zeros(3 * H, I), torch.zeros(3 * H, I)]), ("w_hh", [torch.zeros(3 * H, H)]),
                     ("b_hh", [torch.zeros(3 * H), torch.zeros(H)]), ("w_ih", [torch.zeros(2 * H, I), torch.zeros(3 * H, H)])):
        with pytest.raises(ValueError):
            library._predictor_dims(x, **{**good, key: bad})
    with pytest.raises(ValueError):
        library._predictor_dims(torch.zeros(2, 5), **good)


def test_fast_path_eligibility():
    from models import gru_plan, tcn_plan
    from models.predictor import NormalPredictorGRU, NormalPredictorTCN
    assert gru_plan.fast_path_eligible(NormalPredictorGRU(29, 9).eval())
    assert gru_plan.fast_path_eligible(NormalPredictorGRU(33, 9, hidden_size=128).eval())
    assert gru_plan.fast_path_eligible(NormalPredictorGRU(29, 9, num_layers=1).eval())
    assert not gru_plan.fast_path_eligible(NormalPredictorGRU(29, 9).train())
    assert not gru_plan.fast_path_eligible(NormalPredictorGRU(29, 9, hidden_size=64).eval())
    bi = NormalPredictorGRU(29, 9).eval()
    bi.gru = nn.GRU(38, 128, num_layers=2, batch_first=True, bidirectional=True)
    assert not gru_plan.fast_path_eligible(bi.eval())
    assert not gru_plan.fast_path_eligible(NormalPredictorTCN(29, 9).eval())
    assert not tcn_plan.fast_path_eligible(NormalPredictorGRU(29, 9).eval())
