"""Residual trunk, host side: the reach helper, the constructor's refusals, the state dict, the
checkpoint / CLI plumbing and the two new C entry points (no GPU needed)."""
from __future__ import annotations

import pytest
import torch

from helpers import LTA_INP, load, lta_ids


def _detector(**kw):
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    return LeakDetector(LTA_INP, sensors, pipes, **kw)


@pytest.mark.parametrize("layers,nodes,pipes", [(2, 473, 475), (4, 237, 208), (8, 22, 13), (12, 0, 0)])
def test_sensor_reach_ltown_a(layers, nodes, pipes):
    """L-TOWN-A with the 29 fixture sensors: nodes farther than `layers` hops from every sensor, and
    pipes with both ends among them (the farthest node is 11 hops away)."""
    from models.utils import sensor_reach
    g = load("graph_ltown_a.npz")
    got = sensor_reach(torch.from_numpy(g["edge_index"]), len(g["node_names"]), torch.from_numpy(g["sensor_node_idx"]),
                       torch.from_numpy(g["pipe_ends"]), layers)
    assert got == (nodes, pipes)
    # numpy inputs, and the detector's own graph, give the same counts
    assert sensor_reach(g["edge_index"], len(g["node_names"]), g["sensor_node_idx"], g["pipe_ends"], layers) == got


def test_sensor_reach_small_graph():
    """A path 0-1-2-3-4 with the sensor at 0, pipes = its edges: 0 layers leave all but the sensor
    out; each layer brings one node in; a pipe counts only when BOTH ends are out."""
    from models.utils import sensor_reach
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])
    ends = ei.t()
    assert [sensor_reach(ei, 5, [0], ends, k) for k in range(5)] == [(4, 3), (3, 2), (2, 1), (1, 0), (0, 0)]


def test_skip_value_is_checked():
    with pytest.raises(ValueError, match="skip"):
        _detector(skip="bogus")


def test_skip_refuses_the_bf16_tier():
    with pytest.raises(NotImplementedError, match="fp32"):
        _detector(skip="residual", mlp_dtype="bf16")


def test_skip_adds_no_state():
    plain, skip = _detector(gnn_layers=3), _detector(gnn_layers=3, skip="residual")
    assert list(plain.state_dict()) == list(skip.state_dict())
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in skip.named_parameters()]
    assert skip.skip == "residual" and plain.skip == "none" and _detector().skip == "none"
    skip.load_state_dict(plain.state_dict(), strict=True)


def test_detector_from_args_reads_depth_and_skip():
    from models.detector import detector_from_args, detector_from_checkpoint
    sensors, pipes = lta_ids()
    deep = detector_from_args(LTA_INP, sensors, pipes, {"gnn_layers": 4, "skip": "residual"})
    assert len(deep.convs) == 4 and deep.skip == "residual"
    old = detector_from_args(LTA_INP, sensors, pipes, {})
    assert len(old.convs) == 2 and old.skip == "none"
    assert list(old.state_dict()) == list(_detector().state_dict())
    # a checkpoint carries both in its args; one from before the flags has neither
    ck = {"sensor_ids": sensors, "pipe_ids_in_order": pipes, "detector_state": deep.state_dict(),
          "args": {"gnn_layers": 4, "skip": "residual"}}
    back = detector_from_checkpoint(ck, LTA_INP)
    assert len(back.convs) == 4 and back.skip == "residual"
    ck_old = {"sensor_ids": sensors, "pipe_ids_in_order": pipes, "detector_state": old.state_dict(), "args": {}}
    assert len(detector_from_checkpoint(ck_old, LTA_INP).convs) == 2


def test_cli_accepts_the_flags():
    from models import train_detector
    base = ["--leak_root", "x", "--inp_path", "y", "--predictor_ckpt", "z", "--out_dir", "o"]
    a = train_detector.main(base + ["--gnn_layers", "8", "--skip", "residual"], parse_only=True)
    assert a.gnn_layers == 8 and a.skip == "residual"
    d = train_detector.main(base, parse_only=True)
    assert d.gnn_layers == 2 and d.skip == "none"
    assert vars(a)["skip"] == "residual"  # what the checkpoint's "args" stores
    with pytest.raises(SystemExit):
        train_detector.main(base + ["--skip", "dense"], parse_only=True)


def test_skip_entry_points_exported():
    from models import _native
    lib = _native.load_library()
    assert lib.lg_abi_version() == 26 == _native.ABI_VERSION
    for name in ("lg_gcn_fwd_nm_skip", "lg_gcn_bwd_nm_skip"):
        assert hasattr(lib, name) and name in _native.SIGNATURES
    # the skip forms take the arguments of the bits forms
    assert _native.SIGNATURES["lg_gcn_fwd_nm_skip"] == _native.SIGNATURES["lg_gcn_fwd_nm_bits"]
    assert _native.SIGNATURES["lg_gcn_bwd_nm_skip"] == _native.SIGNATURES["lg_gcn_bwd_nm_bits"]


def test_unpack_mask_inverts_the_bit_layout():
    """detector._unpack_mask (the capture hook's fmask) against the layout include/leakgnn.h states,
    packed here independently, at a ragged B and both widths."""
    from models.detector import _unpack_mask
    for D, B, N in ((64, 20, 3), (32, 16, 2), (32, 5, 2)):
        g = torch.Generator().manual_seed(D + B)
        m = torch.rand(N, B, D, generator=g) > 0.5
        T, lpr = (B + 15) // 16, D // 4
        rpp = 64 // lpr
        words = torch.zeros(N, T, 64, dtype=torch.int32)
        for n in range(N):
            for b in range(B):
                for c in range(D):
                    if m[n, b, c]:
                        r = b % 16
                        lane = (r % rpp) * lpr + c // 4
                        words[n, b // 16, lane] |= 1 << (4 * (r // rpp) + c % 4)
        w16 = torch.where(words >= 2 ** 15, words - 2 ** 16, words).to(torch.int16).reshape(-1)
        assert torch.equal(_unpack_mask(w16, N, B, D), m)
