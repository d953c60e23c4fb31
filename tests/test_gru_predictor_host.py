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
    bads = (("w_ih", [torch.zeros(3 * H, I), torch.zeros(3 * H, I)]), ("w_hh", [torch.zeros(3 * H, H)]),
            ("b_hh", [torch.zeros(3 * H), torch.zeros(H)]), ("w_ih", [torch.zeros(2 * H, I), torch.zeros(3 * H, H)]))
    # the one validator under gru_predictor (dense x) and gru_stack (residual, I from w_ih[0])
    for op, inp, dense in (("gru_predictor", x, True), ("gru_stack", torch.zeros(2, 5, 7), False)):
        assert library._gru_dims(op, inp, dense, **good) == (I, H, 2)
        assert library._gru_dims(op, inp, dense, good["w_ih"], good["w_hh"]) == (I, H, 2)  # the backward ops: no biases
        for key, bad in bads:
            with pytest.raises(ValueError, match=f"^{op}: "):
                library._gru_dims(op, inp, dense, **{**good, key: bad})
        with pytest.raises(ValueError, match=f"^{op}: "):
            library._gru_dims(op, torch.zeros(2, 5), dense, **good)
        with pytest.raises(ValueError, match=f"^{op}: dropout p"):
            library._gru_dims(op, inp, dense, **good, p=1.0)
    with pytest.raises(ValueError, match="I, H in 1..1024"):
        library._gru_dims("gru_predictor", torch.zeros(2, 5, 1025), True, [torch.zeros(3 * H, 1025)], [torch.zeros(3 * H, H)])


def test_split_runs():
    from models import library
    ts = [torch.zeros(i) for i in range(6)]
    (a,), b, c = library._split(ts, 1, 2, 3)
    assert a is ts[0] and b == ts[1:3] and c == ts[3:] and library._split(tuple(ts), 6, 0) == [ts, []]
    with pytest.raises(ValueError):
        library._split(ts, 2, 3)


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
