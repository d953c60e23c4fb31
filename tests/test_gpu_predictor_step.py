"""The predictor's training step on the GPU: the fused tail (head + MSE, ClipAdamW) eagerly and
as one captured HIP graph (train_predictor.CapturedPredictorStep), and the TCN's packed conv
weights under capture and after replays (library._tcn_packed, tcn_plan._packed_weights).

Shapes are small: TCN B = 4, L = 12, S = 3, 2 blocks; GRU B = 4, L = 6, S = 3, 2 layers at
hidden 128 (the tiled kernels) and 20 (the generic ones); dropout 0 unless stated.  The bars for
captured against eager are tests/test_graph_step.py's: losses rtol 1e-6, parameters rtol 1e-5."""
from __future__ import annotations

import copy
import json
import re

import pytest
import torch

from helpers import GOLD, assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, TD, B = 3, 9, 4
ARCHS = ["tcn", "gru128", "gru20"]


def _model(arch: str, dropout: float = 0.0, seed: int = 0, blocks: int = 2):
    from models.predictor import NormalPredictorGRU, NormalPredictorTCN
    torch.manual_seed(seed)
    if arch == "tcn":
        m = NormalPredictorTCN(S, TD, num_blocks=blocks, dropout=dropout)
    else:
        m = NormalPredictorGRU(S, TD, hidden_size=int(arch[3:]), num_layers=2, dropout=dropout)
    return m.to(DEV).train()


def _batches(arch: str, n: int, seed: int = 1):
    L = 12 if arch == "tcn" else 6
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, L, S, generator=g).to(DEV), torch.randn(B, L, TD, generator=g).to(DEV),
             torch.randn(B, S, generator=g).to(DEV)) for _ in range(n)]


def _opt(m, lr: float = 1e-3, wd: float = 1e-4):
    from models.optim import ClipAdamW
    return ClipAdamW(m.parameters(), lr=lr, weight_decay=wd, max_norm=1.0)


def _eager_step(m, opt, x, xt, y):
    from models.train_predictor import head_loss_fn
    opt.zero_grad(set_to_none=True)
    loss = head_loss_fn(m)(m.features(x, xt), y)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def _error_word(opt) -> int:
    return int(opt.param_groups[0]["step_t"][2:3].view(torch.int32).item())


def _run_pair(arch: str, blocks: int = 2, before_replays=None):
    """(eager model, captured model, their optimizers) after 4 steps on 4 different batches, one
    stepped eagerly and its deep copy by graph replays; losses compared on the way."""
    from models.train_predictor import CapturedPredictorStep
    bs = _batches(arch, 4)
    m1 = _model(arch, blocks=blocks)
    m2 = copy.deepcopy(m1)
    o1, o2 = _opt(m1), _opt(m2)
    step = CapturedPredictorStep(m2, o2, *bs[0])
    if before_replays is not None:
        before_replays(m2)
    for x, xt, y in bs:  # the batches differ: with one repeated batch a stale weight pack would not show
        l1 = _eager_step(m1, o1, x, xt, y)
        l2 = step(x, xt, y)
        assert_close(l2, l1, rtol=1e-6, what=f"{arch} loss")
    torch.cuda.synchronize()
    assert _error_word(o1) == 0 and _error_word(o2) == 0
    return m1, m2, o1, o2


@pytest.mark.parametrize("arch", ARCHS)
def test_captured_step_matches_eager_step(arch):
    m1, m2, _, _ = _run_pair(arch)
    for (n, a), b in zip(m2.named_parameters(), m1.parameters()):
        assert_close(a, b, rtol=1e-5, what=f"{arch} {n}")


def _tcn_op_args(m, h):
    stages = [(c.conv, n) for blk in m.tcn for c, n in ((blk.conv1, blk.norm1), (blk.conv2, blk.norm2))]
    return (h, [c.weight for c, _ in stages], [c.bias for c, _ in stages], [n.weight for _, n in stages],
            [n.bias for _, n in stages], float(m.tcn[0].norm1.eps), 0.0, torch.zeros(1, dtype=torch.int64), False)


def test_tcn_pack_is_recorded_in_the_graph():
    """A capture of leakgnn::tcn_predictor after an eager call has filled the pack cache still
    records the pack launches: a replay after an in-place weight change convolves with the new
    weights.  (With a cache hit during capture the graph would keep the weights of capture time.)"""
    from models import library
    m = _model("tcn")
    h = torch.randn(B, 12, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        args = _tcn_op_args(m, h)
        first = torch.ops.leakgnn.tcn_predictor(*args)[0].clone()   # fills the cache
        w = m.tcn[0].conv2.conv.weight
        assert library._TCN_PACK_CACHE[w.data_ptr()][0] == w._version
        def entries():
            return {k: (v[0], id(v[2]), id(v[3])) for k, v in library._TCN_PACK_CACHE.items()}
        cached = entries()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = torch.ops.leakgnn.tcn_predictor(*args)[0]
        assert entries() == cached, "a capture must not touch the pack cache"
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)
        w.mul_(2.0)
        g.replay()
        ref = torch.ops.leakgnn.tcn_predictor(*_tcn_op_args(m, h))[0]
        torch.cuda.synchronize()
    assert not torch.equal(ref, first)
    assert_close(out, ref, what="replay at the new weights")


def test_no_stale_pack_after_replays_train_forward_backward():
    """After the replays an eager train-mode forward + backward on the captured copy equals the
    eager copy's: the packs an eager call made BEFORE the replays (same _version as now) are gone."""
    from models import library
    from models.train_predictor import head_loss_fn
    x, xt, y = _batches("tcn", 1, seed=9)[0]

    def prime(m2):  # an eager call between the capture and the replays: its packs carry the current versions
        with torch.no_grad():
            m2.features(x, xt)
        w = m2.tcn[0].conv1.conv.weight
        assert library._TCN_PACK_CACHE[w.data_ptr()][0] == w._version

    m1, m2, _, _ = _run_pair("tcn", before_replays=prime)
    w = m2.tcn[0].conv1.conv.weight
    assert w.data_ptr() not in library._TCN_PACK_CACHE  # CapturedPredictorStep dropped it
    outs = []
    for m in (m1, m2):
        m.zero_grad(set_to_none=True)
        loss = head_loss_fn(m)(m.features(x, xt), y)
        loss.backward()
        outs.append((loss.detach(), {n: p.grad for n, p in m.named_parameters()}))
    torch.cuda.synchronize()
    assert_close(outs[1][0], outs[0][0], rtol=1e-6, what="loss after replays")
    for n, g in outs[1][1].items():
        assert_close(g, outs[0][1][n], rtol=1e-5, what=f"grad {n} after replays")


def test_no_stale_pack_after_replays_tcn_residual():
    """tcn_plan.tcn_residual on a default-shape TCN (4 blocks) over the smallest segment
    (l_pred = l_det = 1): called before the replays, so its module-level packs exist, and again
    after them on both copies."""
    from models.tcn_plan import tcn_residual
    g = torch.Generator().manual_seed(4)
    seg, tseg = torch.randn(B, 2, S, generator=g).to(DEV), torch.randn(B, 2, TD, generator=g).to(DEV)
    before = {}

    def prime(m2):
        before["r"] = tcn_residual(m2.eval(), seg, tseg, 1, 1).clone()
        assert getattr(m2, "_lg_tcn_packed", None) is not None
        m2.train()

    m1, m2, _, _ = _run_pair("tcn", blocks=4, before_replays=prime)
    r1 = tcn_residual(m1.eval(), seg, tseg, 1, 1)
    r2 = tcn_residual(m2.eval(), seg, tseg, 1, 1)
    torch.cuda.synchronize()
    assert not torch.equal(r2, before["r"]), "four steps must move the residual"
    assert_close(r2, r1, rtol=1e-5, what="tcn_residual after replays")


@pytest.mark.parametrize("arch", ["tcn", "gru128"])
def test_dropout_under_capture(arch):
    """p = 0.1 inside the captured step: with lr = 0 (the weights stay put) two replays on the same
    input differ (each replay draws new masks), and with a real lr the loss falls over 30 replays
    on one fixed batch."""
    from models.train_predictor import CapturedPredictorStep
    x, xt, y = _batches(arch, 1, seed=5)[0]
    m = _model(arch, dropout=0.1)
    frozen = CapturedPredictorStep(m, _opt(m, lr=0.0, wd=0.0), x, xt, y)
    a = frozen().clone()
    b = frozen().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a) and torch.isfinite(b) and a.item() != b.item()
    opt = _opt(m, lr=3e-3)
    step = CapturedPredictorStep(m, opt, x, xt, y)
    losses = torch.stack([step().clone() for _ in range(30)]).cpu()
    assert torch.isfinite(losses).all()
    assert losses[-5:].mean() < losses[:5].mean(), losses.tolist()
    assert _error_word(opt) == 0


@pytest.fixture(scope="module")
def normal_set(tmp_path_factory):
    from models.synth import write_synthetic_normal_set
    sensors = json.loads((GOLD / "harness.json").read_text())["sensors"]
    d = tmp_path_factory.mktemp("synth_pred_step") / "normal"
    write_synthetic_normal_set(d, sensors, n_windows=12, T=577, seed=0)
    return d


@pytest.mark.parametrize("arch", ["tcn", "gru"])
def test_train_predictor_cli_capture_on(normal_set, tmp_path, capsys, monkeypatch, arch):
    """--capture on end to end: 19 steps in batches of 8 = two replayed batches and an eager tail of
    3; the checkpoint keeps its keys, the loss is finite and ClipAdamW's error word is 0."""
    from models import train_predictor
    words = []
    real = train_predictor.check_optimizer_errors

    def spy(opt):
        words.append(_error_word(opt))
        real(opt)
    monkeypatch.setattr(train_predictor, "check_optimizer_errors", spy)
    out = tmp_path / "out"
    train_predictor.main(["--normal_root", str(normal_set), "--out_dir", str(out), "--epochs", "1",
                          "--steps_per_epoch", "19", "--val_steps", "8", "--test_steps", "8", "--batch_size", "8",
                          "--device", "cuda", "--log_every", "1", "--arch", arch, "--capture", "on"])
    ck = torch.load(out / "predictor_last.ckpt", weights_only=True)
    assert set(ck) == {"epoch", "arch", "model_state", "standardizer_mean", "standardizer_std", "sensor_ids", "args"}
    assert ck["arch"] == arch and ck["args"]["capture"] == "on"
    assert all(torch.isfinite(v).all() for v in ck["model_state"].values())
    log = capsys.readouterr().out
    steps = [float(v) for v in re.findall(r"step \d+/\d+ loss=([0-9.eE+-]+|nan|inf)", log)]
    assert len(steps) == 3 and all(v == v and v < float("inf") for v in steps), log
    assert words == [0]
