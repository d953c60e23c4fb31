"""K-hop diffusion of the node init, host side: the constructor's checks, the state dict, the
checkpoint / CLI plumbing, the reach line, the output layouts and the entry points' host-side checks
(no GPU needed)."""
from __future__ import annotations

import argparse

import pytest
import torch

from helpers import LTA_INP, lta_ids


def _detector(**kw):
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    return LeakDetector(LTA_INP, sensors, pipes, **kw)


@pytest.mark.parametrize("kw", [{"diffuse_hops": -1}, {"diffuse_hops": 65}, {"diffuse_hops": 2.5},
                                {"diffuse_hops": 2, "diffuse_alpha": -0.1}, {"diffuse_hops": 2, "diffuse_alpha": 1.5},
                                {"diffuse_alpha": float("nan")}])
def test_constructor_checks_hops_and_alpha(kw):
    with pytest.raises(ValueError, match="diffuse_"):
        _detector(**kw)


def test_constructor_refuses_bf16_and_learned_weights():
    with pytest.raises(NotImplementedError, match="fp32"):
        _detector(diffuse_hops=2, mlp_dtype="bf16")
    with pytest.raises(NotImplementedError, match="fixed edge weights"):
        _detector(diffuse_hops=2, learn_edge_weight=True)
    # neither refusal touches the detector without hops
    assert _detector(mlp_dtype="bf16").diffuse_hops == 0
    assert _detector(learn_edge_weight=True, diffuse_alpha=0.3).diffuse_hops == 0


def test_hops_add_no_state():
    plain, hops = _detector(), _detector(diffuse_hops=10, diffuse_alpha=0.2)
    assert list(plain.state_dict()) == list(hops.state_dict())
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in hops.named_parameters()]
    assert (hops.diffuse_hops, hops.diffuse_alpha) == (10, 0.2) and (plain.diffuse_hops, plain.diffuse_alpha) == (0, 0.1)
    hops.load_state_dict(plain.state_dict(), strict=True)
    # the stage is not folded into the fused encoder op
    assert not hops._fused_encoder(torch.zeros(32, 36, 29), None, 32, 661, 64, True)


def test_detector_from_args_and_checkpoint_round_trip():
    from models.detector import detector_from_args, detector_from_checkpoint
    sensors, pipes = lta_ids()
    d = detector_from_args(LTA_INP, sensors, pipes, {"diffuse_hops": 10, "diffuse_alpha": 0.25})
    assert (d.diffuse_hops, d.diffuse_alpha, len(d.convs)) == (10, 0.25, 2)
    assert detector_from_args(LTA_INP, sensors, pipes, {"diffuse_hops": 4}).diffuse_alpha == 0.1
    old = detector_from_args(LTA_INP, sensors, pipes, {})
    assert old.diffuse_hops == 0 and list(old.state_dict()) == list(_detector().state_dict())
    ck = {"sensor_ids": sensors, "pipe_ids_in_order": pipes, "detector_state": d.state_dict(),
          "args": {"gnn_layers": 2, "diffuse_hops": 10, "diffuse_alpha": 0.25}}
    back = detector_from_checkpoint(ck, LTA_INP)
    assert (back.diffuse_hops, back.diffuse_alpha) == (10, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), d.state_dict().values()))
    # a checkpoint from before the flags has neither key: hops 0
    ck_old = dict(ck, args={"gnn_layers": 2})
    assert detector_from_checkpoint(ck_old, LTA_INP).diffuse_hops == 0
    assert detector_from_checkpoint(dict(ck, args=None), LTA_INP).diffuse_hops == 0


def test_cli_accepts_the_flags():
    from models import train_detector
    base = ["--leak_root", "x", "--inp_path", "y", "--predictor_ckpt", "z", "--out_dir", "o"]
    a = train_detector.main(base + ["--diffuse_hops", "10", "--diffuse_alpha", "0.2"], parse_only=True)
    assert a.diffuse_hops == 10 and a.diffuse_alpha == 0.2
    d = train_detector.main(base, parse_only=True)
    assert d.diffuse_hops == 0 and d.diffuse_alpha == 0.1
    assert vars(a)["diffuse_hops"] == 10 and vars(a)["diffuse_alpha"] == 0.2  # what the checkpoint's "args" stores
    with pytest.raises(SystemExit):
        train_detector.main(base + ["--diffuse_hops", "many"], parse_only=True)


@pytest.mark.parametrize("layers,hops,nodes,pipes", [(2, 0, 473, 475), (2, 2, 237, 208), (2, 6, 22, 13), (2, 10, 0, 0)])
def test_reach_line_counts_layers_plus_hops(layers, hops, nodes, pipes):
    """The start-up line reports reach gnn_layers + diffuse_hops: the counts of utils.sensor_reach at
    that depth (tests/test_skip_host.py pins them for 2, 4, 8 and 12)."""
    from models import train_detector
    det = _detector(gnn_layers=layers, diffuse_hops=hops)
    args = argparse.Namespace(gnn_layers=layers, skip="none", norm="none", diffuse_hops=hops)
    line = train_detector.reach_line(det, args)
    assert f"diffuse_hops={hops}: {nodes}/661 nodes and {pipes}/" in line and f"gnn_layers={layers}" in line


def test_layouts_gain_z_only_with_hops():
    from models import library
    for L in (0, 2, 4):
        plain = library._gnn_trunk_layout(L, 4, 661, 29, 64)
        hops = library._gnn_trunk_layout(L, 4, 661, 29, 64, diffuse=True)
        assert hops[0][:-1] == plain[0] and hops[0][-1] == ((661, 4, 64), torch.float32)
        assert "z" not in plain[1] and hops[1]["z"] == len(plain[0])
        assert hops[1]["h"] == (plain[1]["h"] if L else hops[1]["z"])  # without layers the heads read z
        assert library._positions("gnn_trunk", len(hops[0]), True) == hops[1]
        assert library._positions("gnn_trunk", len(plain[0])) == plain[1]
        pn, hn = library._gnn_trunk_norm_layout(L, 4, 661, 64), library._gnn_trunk_norm_layout(L, 4, 661, 64, diffuse=True)
        assert hn[0][:-1] == pn[0] and hn[1]["z"] == len(pn[0]) and hn[1]["h"] == pn[1]["h"] == 0
        assert library._positions("gnn_trunk_norm", len(hn[0]), True) == hn[1]
    f = library.trunk_fields("gnn_trunk", list(range(6)), True)
    assert f.xs == [0, 1, 2] and f.z == 5 and f.h == 2
    assert library.trunk_fields("gnn_trunk", list(range(5))).z is None


def test_op_schemas_carry_the_keywords():
    from models import library  # noqa: F401
    s = str(torch.ops.leakgnn.gnn_trunk.default._schema)
    assert "Int hops=0" in s and "float alpha=0." in s and s.index("*") < s.index("Int hops=0")
    assert "Int hops=0" in str(torch.ops.leakgnn.gnn_trunk_norm.default._schema)
    assert "Int hops=0" in str(torch.ops.leakgnn.gnn_trunk_backward.default._schema)
    d = str(torch.ops.leakgnn.diffuse.default._schema)
    assert "Int hops" in d and "float alpha" in d
    with pytest.raises(ValueError):
        library.check_diffuse(0, 0.1)
    library.check_diffuse(0, 0.1, zero_ok=True)
    with pytest.raises(ValueError):
        library.check_diffuse(3, 1.01)


def test_entry_points_exported_and_checked_on_the_host():
    """The ABI number stays; the fit rule, the workspace sizes and the refusals that need no device."""
    from models import _native
    lib = _native.load_library()
    assert lib.lg_abi_version() == 26 == _native.ABI_VERSION
    for name in ("lg_diffuse_fwd", "lg_diffuse_bwd", "lg_diffuse_slice", "lg_diffuse_workspace_bytes"):
        assert hasattr(lib, name) and name in _native.SIGNATURES
    # the widest slice whose rows fit: 32 floats up to 768 nodes, 16 to 1536, 8 to 3072
    assert [lib.lg_diffuse_slice(n, 64) for n in (1, 661, 768, 769, 1536, 1537, 3072, 3073)] == [32, 32, 32, 16, 16, 8, 8, 0]
    assert lib.lg_diffuse_slice(661, 32) == 32 and lib.lg_diffuse_slice(661, 48) == -2 and lib.lg_diffuse_slice(0, 64) == -1
    hw = _native.LG_F_DIFFUSE_HOPWISE
    assert lib.lg_diffuse_workspace_bytes(256, 661, 64, 12, 0, 0) == 0 == lib.lg_diffuse_workspace_bytes(256, 661, 64, 12, 0, 1)
    act = 256 * 661 * 64 * 4
    assert lib.lg_diffuse_workspace_bytes(256, 661, 64, 12, hw, 0) == act
    assert lib.lg_diffuse_workspace_bytes(256, 661, 64, 12, hw, 1) == 2 * act
    assert lib.lg_diffuse_workspace_bytes(256, 661, 64, 1, hw, 1) == 0
    assert lib.lg_diffuse_workspace_bytes(2, 4000, 64, 3, 0, 0) == 2 * 4000 * 64 * 4
    assert lib.lg_diffuse_workspace_bytes(2, 661, 64, 0, 0, 0) == -1 and lib.lg_diffuse_workspace_bytes(2, 661, 16, 2, 0, 0) == -2
    # refusals decided before any HIP call (the pointers are never followed)
    a, b = 4096, 8192
    fwd = lambda **k: lib.lg_diffuse_fwd(*[{**dict(t=a, p=a, x=a, z=b, B=2, N=41, D=64, h=2, al=0.1, f=0, w=None, nb=0, s=None),  # noqa: E731
                                            **k}[q] for q in ("t", "p", "x", "z", "B", "N", "D", "h", "al", "f", "w", "nb", "s")])
    assert fwd(D=48) == -2 and fwd(h=0) == -1 and fwd(h=65) == -1 and fwd(al=1.5) == -1 and fwd(al=float("nan")) == -1
    assert fwd(z=a) == -1 and fwd(x=None) == -1 and fwd(B=-1) == -1 and fwd(f=_native.LG_F_RELU) == -2
    assert fwd(f=hw) == -1 and fwd(B=0) == 0
    assert lib.lg_diffuse_bwd(a, a, a, None, b, 2, 41, 64, 2, 0.1, _native.LG_F_MASK_OUT, 1.0, None, 0, None) == -1
    assert lib.lg_diffuse_bwd(a, a, a, None, b, 0, 41, 64, 2, 0.1, 0, 1.0, None, 0, None) == 0
