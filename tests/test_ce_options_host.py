"""Host side of the cross entropy options (CPU): loss.distance_smoothing, CrossEntropyLoss's
constructor validation and torch route, loss_from_args / check_loss_args and the training CLI's
three flags, and the argument validation of lg_cross_entropy_opt_fwd / _bwd (LG_EINVAL before any
HIP call)."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from helpers import LTA_INP

P = 0x1000  # any non-null address: a call that fails its argument checks never reads it
INF = float("inf")
# four pipes on a line, 100 m apart, the fourth cut off from the rest
DIST = np.array([[0, 100, 200, INF], [100, 0, 100, INF], [200, 100, 0, INF], [INF, INF, INF, 0]], dtype=np.float32)


def test_distance_smoothing_table():
    from models.loss import distance_smoothing
    u = distance_smoothing(DIST, 50.0, 5)
    assert u.dtype == torch.float32 and tuple(u.shape) == (5, 5) and u.device.type == "cpu"
    e = np.exp(-DIST.astype(np.float64) / 50.0)
    want = np.zeros((5, 5))
    want[:4, :4] = e / e.sum(axis=1, keepdims=True)
    want[4, 4] = 1.0
    assert np.abs(want.sum(axis=1) - 1.0).max() < 1e-15           # fp64 rows sum to 1 before the cast
    assert torch.equal(u, torch.from_numpy(want.astype(np.float32)))
    assert float(u[0, 3]) == 0.0 and float(u[3, 0]) == 0.0        # the unreachable pair
    assert float(u[3, 3]) == 1.0                                  # all of pipe 3's mass stays on it
    assert torch.equal(u[4], torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0]))  # the no-leak row is one-hot
    assert not (u[:4, 4] != 0).any()                              # pipe rows: 0 in the no-leak column
    assert float(u[0, 1]) > float(u[0, 2]) > 0.0                  # nearer pipes take more
    assert torch.equal(distance_smoothing(DIST, 1e-3, 5), torch.eye(5))  # a tiny sigma tends to the identity
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_m"):
            distance_smoothing(DIST, bad, 5)
    with pytest.raises(ValueError, match="does not fit"):
        distance_smoothing(DIST, 50.0, 4)


def test_constructor_validation():
    from models.loss import CrossEntropyLoss, distance_smoothing
    u = distance_smoothing(DIST, 50.0, 5)
    m = CrossEntropyLoss(label_smoothing=0.1, smoothing=u, weight=torch.ones(5))
    assert torch.equal(m.smoothing, u) and "smoothing" not in m.state_dict()
    assert CrossEntropyLoss().smoothing is None
    with pytest.raises(ValueError, match=r"\(C, C\)"):
        CrossEntropyLoss(label_smoothing=0.1, smoothing=u[:, :4])
    with pytest.raises(ValueError, match=r"\(C, C\)"):
        CrossEntropyLoss(label_smoothing=0.1, smoothing=u[0])
    neg = u.clone()
    neg[0, 0], neg[0, 1] = neg[0, 0] + 2 * neg[0, 1], -neg[0, 1]  # the row still sums to 1
    with pytest.raises(ValueError, match="negative"):
        CrossEntropyLoss(label_smoothing=0.1, smoothing=neg)
    off = u.clone()
    off[2, 2] += 1e-4
    with pytest.raises(ValueError, match="sum to 1"):
        CrossEntropyLoss(label_smoothing=0.1, smoothing=off)
    nan = u.clone()
    nan[1, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        CrossEntropyLoss(label_smoothing=0.1, smoothing=nan)
    with pytest.raises(ValueError, match="label_smoothing > 0"):
        CrossEntropyLoss(smoothing=u)
    with pytest.raises(ValueError, match="number of classes"):
        CrossEntropyLoss(label_smoothing=0.1, smoothing=u, weight=torch.ones(4))


@pytest.mark.parametrize("kw", [{"weight": True}, {"label_smoothing": 0.15}, {"reduction": "sum"},
                                {"reduction": "none"}, {"weight": True, "label_smoothing": 0.15, "reduction": "sum"},
                                {"ignore_index": 2}, {}])
def test_module_on_cpu_is_torch(kw):
    """CPU tensors take torch's route: the same bits as torch.nn.CrossEntropyLoss, loss and gradient."""
    from models.loss import CrossEntropyLoss
    g = torch.Generator().manual_seed(0)
    kw = dict(kw)
    if kw.get("weight"):
        kw["weight"] = torch.rand(7, generator=g) + 0.5
    x = torch.randn(6, 7, generator=g)
    ign = kw.get("ignore_index", -100)
    t = torch.tensor([0, 6, 2, ign, 3, 2])
    outs = []
    for cls in (CrossEntropyLoss, torch.nn.CrossEntropyLoss):
        xx = x.clone().requires_grad_(True)
        out = cls(**kw)(xx, t)
        out.sum().backward()
        outs.append((out.detach(), xx.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_table_on_cpu_raises():
    from models.loss import CrossEntropyLoss, distance_smoothing
    m = CrossEntropyLoss(label_smoothing=0.1, smoothing=distance_smoothing(DIST, 50.0, 5))
    with pytest.raises(NotImplementedError, match="smoothing table"):
        m(torch.zeros(3, 5), torch.tensor([0, 1, 4]))


def _args(*extra):
    from models import train_detector
    return train_detector.main(["--leak_root", "d", "--inp_path", str(LTA_INP), "--predictor_ckpt", "p",
                                "--out_dir", "o", *extra], parse_only=True)


def test_loss_from_args_and_cli_flags():
    from models.loss import CrossEntropyLoss, loss_from_args
    pipes = ["p1", "p2", "p3"]
    a = _args()
    assert (a.label_smoothing, a.smooth_sigma_m, a.noleak_weight) == (0.0, 0.0, 1.0)
    assert {"label_smoothing", "smooth_sigma_m", "noleak_weight"} <= set(vars(a))  # what ckpt["args"] keeps
    for src in (a, vars(a), {}):  # the namespace, its vars(), a checkpoint written before the flags
        m = loss_from_args(src, LTA_INP, pipes)
        assert type(m) is CrossEntropyLoss
        assert m.weight is None and m.label_smoothing == 0.0 and m.reduction == "mean" and m.smoothing is None
        assert m.ignore_index == -100
    m = loss_from_args(_args("--label_smoothing", "0.1"), LTA_INP, pipes)
    assert m.label_smoothing == 0.1 and m.weight is None and m.smoothing is None
    m = loss_from_args(_args("--noleak_weight", "0.25"), LTA_INP, pipes)
    assert torch.equal(m.weight, torch.tensor([1.0, 1.0, 1.0, 0.25])) and m.label_smoothing == 0.0
    assert m.smoothing is None
    with pytest.raises(ValueError, match="label_smoothing"):
        loss_from_args(_args("--smooth_sigma_m", "200"), LTA_INP, pipes)
    with pytest.raises(ValueError, match="noleak_weight"):
        loss_from_args(_args("--noleak_weight", "-1"), LTA_INP, pipes)


def test_loss_from_args_distance_table():
    """--smooth_sigma_m builds the table from the network's own pipe distances."""
    from helpers import lta_ids
    from models.loss import distance_smoothing, loss_from_args
    from models.window_evaluator import PipeDistanceOracle
    _, pipes = lta_ids()
    pipes = pipes[:40]
    m = loss_from_args(_args("--label_smoothing", "0.1", "--smooth_sigma_m", "200", "--noleak_weight", "0.5"),
                       LTA_INP, pipes)
    C = len(pipes) + 1
    oracle = PipeDistanceOracle.build(LTA_INP, pipes)
    oracle.ensure_pipe_matrix()
    assert torch.equal(m.smoothing, distance_smoothing(oracle.pipe_dist, 200.0, C))
    assert tuple(m.smoothing.shape) == (C, C) and float(m.weight[C - 1]) == 0.5 and m.label_smoothing == 0.1
    assert (m.smoothing.double().sum(dim=1) - 1.0).abs().max().item() < 1e-5
    assert torch.equal(m.smoothing.argmax(dim=1), torch.arange(C))  # a pipe is nearest to itself


def test_check_loss_args_refusals():
    from models.loss import check_loss_args
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    check_loss_args(_args(), 8, gpu)
    check_loss_args(_args("--noleak_weight", "0.5"), 1, cpu)
    check_loss_args(_args("--label_smoothing", "0.1"), 8, cpu)
    check_loss_args(_args("--label_smoothing", "0.1", "--smooth_sigma_m", "200"), 8, gpu)
    check_loss_args({}, 8, cpu)
    with pytest.raises(ValueError, match="data parallel"):
        check_loss_args(_args("--noleak_weight", "0.5"), 2, gpu)
    with pytest.raises(ValueError, match="--device cuda"):
        check_loss_args(_args("--label_smoothing", "0.1", "--smooth_sigma_m", "200"), 1, cpu)


def test_train_detector_refuses_before_loading_anything(monkeypatch, tmp_path):
    """The refusals come at start-up: before the predictor checkpoint (which does not exist here) is read."""
    from models import train_detector
    base = ["--leak_root", str(tmp_path), "--inp_path", str(LTA_INP), "--predictor_ckpt", str(tmp_path / "none.ckpt"),
            "--out_dir", str(tmp_path / "out"), "--device", "cpu"]
    with pytest.raises(ValueError, match="--device cuda"):
        train_detector.main(base + ["--label_smoothing", "0.1", "--smooth_sigma_m", "200"])
    monkeypatch.setattr(train_detector, "dist_env", lambda: (0, 0, 2))
    monkeypatch.setattr(train_detector, "init_distributed", lambda backend: None)
    with pytest.raises(ValueError, match="data parallel"):
        train_detector.main(base + ["--noleak_weight", "0.5"])


def test_ce_opt_c_abi_validation():
    """Both entry points return LG_EINVAL (-1) for each bad argument, with no GPU and no device memory."""
    from models import _native
    lib = _native.load_library()
    # logits, target, B, C, ldx, ignore, weight, smoothing, ldu, eps, reduction, loss, lse, rowloss, rowsum,
    # denom, counter, stream
    fwd_ok = [P, P, 4, 5, 5, -100, P, P, 5, 0.1, 0, P, P, P, P, P, P, None]
    # logits, target, lse, rowsum, denom, grad, B, C, ldx, ignore, weight, smoothing, ldu, eps, reduction,
    # dlogits, ldd, stream
    bwd_ok = [P, P, P, P, P, P, 4, 5, 5, -100, P, P, 5, 0.1, 0, P, 5, None]
    bad_fwd = {2: [-1], 3: [0, -3], 4: [4], 8: [4, 0], 9: [1.0, -0.01, 1.5, math.nan, math.inf], 10: [3, -1],
               0: [None], 1: [None], 11: [None], 12: [None], 13: [None], 14: [None], 15: [None], 16: [None]}
    for i, vals in bad_fwd.items():
        for v in vals:
            a = list(fwd_ok)
            a[i] = v
            assert lib.lg_cross_entropy_opt_fwd(*a) == -1, f"fwd: argument {i} = {v}"
    bad_bwd = {6: [-1], 7: [0, -3], 8: [4], 12: [4, 0], 13: [1.0, -0.01, 1.5, math.nan, math.inf], 14: [3, -1], 16: [4],
               0: [None], 1: [None], 2: [None], 3: [None], 4: [None], 5: [None], 15: [None]}
    for i, vals in bad_bwd.items():
        for v in vals:
            a = list(bwd_ok)
            a[i] = v
            assert lib.lg_cross_entropy_opt_bwd(*a) == -1, f"bwd: argument {i} = {v}"
    # B == 0 still checks the scalars it would write (mean, sum); the sum's backward needs no denom but a grad
    for red in (0, 1):
        for i in (11, 15, 16):
            a = list(fwd_ok)
            a[2], a[10], a[i] = 0, red, None
            assert lib.lg_cross_entropy_opt_fwd(*a) == -1, f"fwd, B = 0, reduction {red}: null argument {i}"
    a = list(bwd_ok)
    a[6], a[14], a[5] = 0, 1, None
    assert lib.lg_cross_entropy_opt_bwd(*a) == -1
    # ldu is not looked at without a table; none with B == 0 has nothing to do and touches nothing
    a = list(fwd_ok)
    a[2], a[7], a[8], a[10] = 0, None, 0, 2
    a[11] = a[15] = a[16] = None
    assert lib.lg_cross_entropy_opt_fwd(*a) == 0
    a = list(bwd_ok)
    a[6], a[11], a[12], a[14], a[4] = 0, None, 0, 2, None
    assert lib.lg_cross_entropy_opt_bwd(*a) == 0
