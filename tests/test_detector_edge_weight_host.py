"""LeakDetector edge weights, host side (no GPU): utils.link_edge_weights, the constructor's
state-dict contract and argument checks, and the checkpoint constructor path of the evaluator."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import GOLD, LTA_INP, load, lta_ids

MODES = ("ones", "length", "inv_length", "conductance")


def _golden_keys() -> list:
    """The reference's state-dict keys, from the golden detector fixture (as
    test_host.py::test_detector_boundary_state_dict reads them; tests/golden/meta.json records
    how oracle/make_golden.py wrote that fixture)."""
    return sorted(k[len("param."):] for k in load("detector_b2.npz") if k.startswith("param."))


def _n_links() -> int:
    return int(np.load(GOLD / "graph_ltown_a.npz")["edge_index"].shape[1]) // 2


def test_link_edge_weights_length_matches_window_evaluator():
    """"length" is the length column window_evaluator._parse_links_with_length reads (pumps and
    valves at its eps), divided by the mean, in link-table order."""
    from models.utils import link_edge_weights
    from models.window_evaluator import _parse_links_with_length
    links = _parse_links_with_length(LTA_INP, 0.1)
    lengths = np.array([v[2] for v in links.values()], dtype=np.float64)
    w = link_edge_weights(LTA_INP, ("PIPES", "PUMPS", "VALVES"), "length")
    assert w.dtype == torch.float32 and tuple(w.shape) == (_n_links(),)
    np.testing.assert_array_equal(w.numpy(), (lengths / lengths.mean()).astype(np.float32))


@pytest.mark.parametrize("mode", MODES)
def test_link_edge_weights_modes(mode):
    from models.utils import link_edge_weights
    w = link_edge_weights(LTA_INP, ("PIPES", "PUMPS", "VALVES"), mode)
    assert tuple(w.shape) == (_n_links(),) and bool((w > 0).all()) and bool(torch.isfinite(w).all())
    assert abs(float(w.double().mean()) - 1.0) < 1e-6
    if mode == "ones":
        assert bool((w == 1).all())
    with pytest.raises(ValueError):
        link_edge_weights(LTA_INP, ("PIPES",), "diameter")


def test_state_dict_keys_default_fixed_learned():
    """Defaults: today's keys (the golden fixture's, as test_detector_boundary_state_dict);
    fixed weights add only `edge_weight`, learned ones only `edge_log_weight`."""
    from models.detector import LeakDetector
    from models.utils import link_edge_weights
    sensors, pipes = lta_ids()
    meta = {"state_dict_keys": _golden_keys()}
    base = LeakDetector(LTA_INP, sensors, pipes)
    assert sorted(base.state_dict().keys()) == meta["state_dict_keys"]
    assert not base.weighted and base._link_weight_source() is None
    w = link_edge_weights(LTA_INP, mode="inv_length")
    fixed = LeakDetector(LTA_INP, sensors, pipes, edge_weight=w)
    assert set(fixed.state_dict()) - set(meta["state_dict_keys"]) == {"edge_weight"}
    assert set(meta["state_dict_keys"]) <= set(fixed.state_dict())
    assert torch.equal(fixed.state_dict()["edge_weight"], w)
    assert [n for n, _ in fixed.named_parameters()] == [n for n, _ in base.named_parameters()]
    learned = LeakDetector(LTA_INP, sensors, pipes, edge_weight=w, learn_edge_weight=True)
    assert set(learned.state_dict()) - set(meta["state_dict_keys"]) == {"edge_log_weight"}
    assert torch.equal(learned.edge_log_weight.detach(), w.log()) and learned.edge_log_weight.requires_grad
    from_one = LeakDetector(LTA_INP, sensors, pipes, learn_edge_weight=True)
    assert bool((from_one.edge_log_weight == 0).all()) and tuple(from_one.edge_log_weight.shape) == (_n_links(),)
    # the new parameter belongs to the trunk side of the gradient split
    assert all(p is not learned.edge_log_weight for p in learned.overlap_split())
    # link j is the directed edges 2j, 2j + 1
    pe = fixed._per_edge_weights(torch.device("cpu"))
    assert torch.equal(pe, w.repeat_interleave(2)) and pe.numel() == fixed.edge_index_single.size(1)
    ei = fixed.edge_index_single
    assert torch.equal(ei[0, 0::2], ei[1, 1::2]) and torch.equal(ei[1, 0::2], ei[0, 1::2])


def test_bad_edge_weight_raises():
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    n = _n_links()
    with pytest.raises(ValueError, match=rf"\({n},\)"):
        LeakDetector(LTA_INP, sensors, pipes, edge_weight=torch.ones(n + 1))
    with pytest.raises(ValueError, match="positive"):
        LeakDetector(LTA_INP, sensors, pipes, edge_weight=torch.ones(n).index_fill_(0, torch.tensor([3]), -1.0))
    with pytest.raises(TypeError):
        LeakDetector(LTA_INP, sensors, pipes, edge_weight=torch.ones(n, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        LeakDetector(LTA_INP, sensors, pipes, learn_edge_weight=True, mlp_dtype="bf16")


@pytest.mark.parametrize("args,extra", [(None, set()), ({"lr": 1e-3}, set()),
                                        ({"edge_weight": "inv_length", "learn_edge_weight": False}, {"edge_weight"}),
                                        ({"edge_weight": "length", "learn_edge_weight": True}, {"edge_log_weight"}),
                                        ({"edge_weight": "none", "learn_edge_weight": True}, {"edge_log_weight"})])
def test_checkpoint_constructor_path(args, extra):
    """A checkpoint dict as train_detector writes it rebuilds the same module keys through the
    evaluator's constructor path and loads strictly; a checkpoint without the new args (or
    without args at all) is the unweighted detector."""
    from models.detector import detector_from_args, detector_from_checkpoint
    sensors, pipes = lta_ids()
    meta = {"state_dict_keys": _golden_keys()}
    torch.manual_seed(3)
    src = detector_from_args(LTA_INP, sensors, pipes, args)
    assert set(src.state_dict()) - set(meta["state_dict_keys"]) == extra
    if "edge_log_weight" in extra:
        with torch.no_grad():
            src.edge_log_weight.add_(0.25)
    ckpt = {"detector_state": src.state_dict(), "sensor_ids": sensors, "pipe_ids_in_order": pipes}
    if args is not None:
        ckpt["args"] = args
    det = detector_from_checkpoint(ckpt, LTA_INP)
    assert list(det.state_dict().keys()) == list(src.state_dict().keys())
    for k, v in src.state_dict().items():
        assert torch.equal(det.state_dict()[k], v), k
    if extra:  # a weighted state does not load into the unweighted module
        with pytest.raises(RuntimeError):
            detector_from_checkpoint({**ckpt, "args": {}}, LTA_INP)


def test_train_detector_cli_has_edge_weight_flags():
    import inspect

    from models import event_evaluator, train_detector
    src = inspect.getsource(train_detector.main)
    assert '"--edge_weight"' in src and '"--learn_edge_weight"' in src
    assert "detector_from_checkpoint" in inspect.getsource(event_evaluator.main)
