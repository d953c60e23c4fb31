"""Pre-norm trunk, host side: the constructor's rules, the state dict, the checkpoint / CLI plumbing
and the argument checks of the two new C entry points (no GPU needed: the checks return before any
launch, with stand-in device pointers as in tests/test_host.py)."""
from __future__ import annotations

import pytest

from helpers import LTA_INP, lta_ids


def _detector(**kw):
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    return LeakDetector(LTA_INP, sensors, pipes, **kw)


# ----------------------------------------------------------------------------- module rules
def test_norm_value_is_checked():
    with pytest.raises(ValueError, match="norm"):
        _detector(skip="residual", norm="bogus")


def test_norm_needs_the_skip():
    with pytest.raises(ValueError, match="skip"):
        _detector(norm="layer")
    with pytest.raises(ValueError, match="skip"):
        _detector(norm="layer", skip="none")


def test_norm_refuses_the_bf16_tier():
    with pytest.raises(NotImplementedError, match="fp32"):
        _detector(skip="residual", norm="layer", mlp_dtype="bf16")


# ----------------------------------------------------------------------------- state dict, call sites
def test_default_has_no_norm_state():
    """norm="none", passed or not, is the module as before: same keys, no `norms` attribute."""
    plain = _detector(gnn_layers=4, skip="residual")
    same = _detector(gnn_layers=4, skip="residual", norm="none")
    assert list(plain.state_dict()) == list(same.state_dict())
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in same.named_modules()]
    assert not hasattr(same, "norms") and same.norm == "none" and _detector().norm == "none"
    assert not any(k.startswith("norms") for k in same.state_dict())


def test_norm_adds_exactly_its_layernorms():
    import torch
    plain = _detector(gnn_layers=4, skip="residual")
    m = _detector(gnn_layers=4, skip="residual", norm="layer")
    want = {f"norms.{l}.{w}" for l in range(5) for w in ("weight", "bias")}
    assert set(m.state_dict()) - set(plain.state_dict()) == want
    assert set(plain.state_dict()) - set(m.state_dict()) == set()
    assert len(m.norms) == 5
    for n in m.norms:  # stock modules, default eps
        assert type(n) is torch.nn.LayerNorm and n.eps == 1e-5 and tuple(n.normalized_shape) == (64,)
    m2 = _detector(gnn_layers=4, skip="residual", norm="layer", sensor_hidden=48, node_hidden=40)
    assert tuple(m2.norms[0].normalized_shape) == (40,)
    # the fused encoder_trunk route is off, as for the skip
    assert not m._fused_encoder(torch.zeros(32, 36, 29), None, 32, 661, 64, True)


def test_detector_from_args_reads_norm():
    from models.detector import detector_from_args, detector_from_checkpoint
    sensors, pipes = lta_ids()
    deep = detector_from_args(LTA_INP, sensors, pipes, {"gnn_layers": 4, "skip": "residual", "norm": "layer"})
    assert len(deep.convs) == 4 and deep.norm == "layer" and len(deep.norms) == 5
    for args in ({"gnn_layers": 4, "skip": "residual"}, {"gnn_layers": 4, "skip": "residual", "norm": "none"}, {}):
        old = detector_from_args(LTA_INP, sensors, pipes, args)
        assert old.norm == "none" and not hasattr(old, "norms")
    ck = {"sensor_ids": sensors, "pipe_ids_in_order": pipes, "detector_state": deep.state_dict(),
          "args": {"gnn_layers": 4, "skip": "residual", "norm": "layer"}}
    back = detector_from_checkpoint(ck, LTA_INP)  # strict load: the norms' keys are expected
    assert back.norm == "layer" and len(back.norms) == 5
    ck_old = {"sensor_ids": sensors, "pipe_ids_in_order": pipes, "detector_state": old.state_dict(), "args": {}}
    assert detector_from_checkpoint(ck_old, LTA_INP).norm == "none"


def test_cli_accepts_norm():
    from models import train_detector
    base = ["--leak_root", "x", "--inp_path", "y", "--predictor_ckpt", "z", "--out_dir", "o"]
    a = train_detector.main(base + ["--gnn_layers", "8", "--skip", "residual", "--norm", "layer"], parse_only=True)
    assert a.norm == "layer" and vars(a)["norm"] == "layer"  # what the checkpoint's "args" stores
    assert train_detector.main(base, parse_only=True).norm == "none"
    with pytest.raises(SystemExit):
        train_detector.main(base + ["--norm", "batch"], parse_only=True)


# ----------------------------------------------------------------------------- C ABI argument checks
F = 16  # a non-NULL stand-in device pointer (never dereferenced on these paths)
EINVAL, EUNSUPPORTED = -1, -2


def test_layernorm_entry_points_exported():
    from models import _native
    lib = _native.load_library()
    assert lib.lg_abi_version() == 26 == _native.ABI_VERSION  # additions only
    for name in ("lg_add_layernorm_fwd", "lg_layernorm_bwd", "lg_layernorm_bwd_workspace_bytes"):
        assert hasattr(lib, name) and name in _native.SIGNATURES


def test_add_layernorm_fwd_argument_checks():
    from models import _native
    lib = _native.load_library()
    fwd = lib.lg_add_layernorm_fwd
    #          x  f  gamma beta xsum xn stats rows D  eps   stream
    assert fwd(None, F, F, F, F, F, F, 100, 64, 1e-5, None) == EINVAL
    assert fwd(F, F, F, F, F, None, F, 100, 64, 1e-5, None) == EINVAL
    assert fwd(F, F, None, F, F, F, F, 100, 64, 1e-5, None) == EINVAL
    assert fwd(F, F, F, None, F, F, F, 100, 64, 1e-5, None) == EINVAL
    assert fwd(F, F, F, F, None, F, F, 100, 64, 1e-5, None) == EINVAL      # f without xsum
    assert fwd(F, None, F, F, F, F, F, 100, 64, 1e-5, None) == EINVAL      # xsum without f
    assert fwd(F, F, F, F, F, F, F, -1, 64, 1e-5, None) == EINVAL
    assert fwd(F, F, F, F, F, F, F, 100, 64, -1.0, None) == EINVAL
    assert fwd(F, F, F, F, F, F, F, 100, 48, 1e-5, None) == EUNSUPPORTED
    assert fwd(F, None, F, F, None, F, None, 100, 48, 1e-5, None) == EUNSUPPORTED
    assert fwd(F, F, F, F, F, F, F, 2 ** 31, 64, 1e-5, None) == EUNSUPPORTED
    assert fwd(F, None, F, F, None, F, None, 0, 64, 1e-5, None) == 0       # no rows: nothing to launch


def test_layernorm_bwd_argument_checks():
    from models import _native
    lib = _native.load_library()
    bwd = lib.lg_layernorm_bwd
    assert lib.lg_layernorm_bwd_workspace_bytes(48) == EUNSUPPORTED
    for D in (32, 64):
        need = lib.lg_layernorm_bwd_workspace_bytes(D)
        assert need > 0 and need % 16 == 0
        #          dxn x stats gamma carry dx dgamma dbeta rows D flags scale ws bytes stream
        assert bwd(F, F, F, F, F, F, F, F, 100, D, 0, 1.0, F, need - 1, None) == EINVAL   # workspace too small
        assert bwd(F, F, F, F, None, F, F, F, 100, D, 0x10, 1.0, F, 0, None) == EINVAL
        assert bwd(F, F, F, F, F, F, F, F, 100, D, 0, 1.0, None, need, None) == EINVAL
        for hole in (0, 1, 2, 3, 5, 6, 7):  # every required pointer (carry, index 4, may be NULL)
            ptrs = [F] * 8
            ptrs[hole] = None
            assert bwd(*ptrs, 100, D, 0, 1.0, F, need, None) == EINVAL, hole
        assert bwd(F, F, F, F, F, F, F, F, 100, D, 0x08, 1.0, F, need, None) == EUNSUPPORTED  # only LG_F_MASK_OUT
    assert bwd(F, F, F, F, F, F, F, F, 100, 48, 0, 1.0, F, 1 << 30, None) == EUNSUPPORTED
