"""leakgnn::window_metrics and leakgnn::event_decide (csrc/metrics.hip) on the GPU against the
brute-force statement of the row order in tests/test_window_metrics_host.py.  Every comparison is
`==` on integers, on float64 values taken from a table and on fp32 bit patterns: nothing is
rounded, so there is no tolerance anywhere in this file."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest
import torch

from helpers import GOLD, LTA_INP
from test_window_metrics_host import event_truth, window_truth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF, NAN = math.inf, math.nan
PAD = 3  # extra columns behind a row when the logits are a sliced view (ldx = C + PAD)


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _sliced(x: np.ndarray) -> torch.Tensor:
    """The logits as a (B, C) view of a wider matrix whose other columns would win every comparison."""
    B, C = x.shape
    wide = np.full((B, C + PAD), 3.0e38, dtype=np.float32)
    wide[:, :C] = x
    v = _dev(wide)[:, :C]
    assert v.stride(0) == C + PAD or B == 1
    return v


def _run(x, label, nlc, topk=5, bucket=None, dist=None, inv_rank=None, radii=(), acc_is=(), counters=None, view=False):
    from models import ops
    xd = _sliced(x) if view else _dev(x)
    cnt = ops.window_counters(DEV) if counters is None else counters
    rank, atd = ops.window_metrics(xd, _dev(label, torch.int64), nlc, cnt, topk=topk, bucket=_dev(bucket, torch.int32),
                                   dist=_dev(dist, torch.float64), inv_rank=_dev(inv_rank, torch.int32),
                                   radii=radii, acc_is=acc_is)
    return cnt, rank, atd


def _check(x, label, nlc, topk=5, bucket=None, dist=None, inv_rank=None, radii=(), acc_is=(), view=False, what=""):
    from models.ops import WINDOW_COUNTERS
    cnt, rank, atd = _run(x, label, nlc, topk, bucket, dist, inv_rank, radii, acc_is, view=view)
    c, rank_ref, atd_ref = window_truth(x, label, nlc, topk, bucket, dist, inv_rank, radii, acc_is)
    got = dict(zip(WINDOW_COUNTERS, cnt.cpu().tolist()))
    assert got == c, (what, {k: (got[k], c[k]) for k in c if got[k] != c[k]})
    assert rank.dtype == torch.int32 and np.array_equal(rank.cpu().numpy(), rank_ref), what
    if dist is None:
        assert atd is None
    else:  # float64 values out of the table, +inf and NaN: compared as bit patterns
        assert atd.dtype == torch.float64
        assert np.array_equal(atd.cpu().numpy().view(np.int64), atd_ref.view(np.int64)), what
    return got


def _tables(nlc: int, rng):
    dist = np.round(rng.random((nlc, nlc)) * 400.0, 1)
    np.fill_diagonal(dist, 0.0)
    order = np.argsort(dist.astype(np.float32), axis=1, kind="stable")
    inv = np.empty_like(order)
    np.put_along_axis(inv, order, np.broadcast_to(np.arange(nlc), order.shape), axis=1)
    return dist.astype(np.float64), inv.astype(np.int32)


@pytest.mark.parametrize("C", [2, 63, 65, 765])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_window_metrics_equals_brute_force(B, C):
    """B: a partial workgroup (1), a partial last wave set (5), several workgroups (67).  C: the
    smallest row, one short of / one past a wave's width, the L-TOWN width.  Half of the rows are
    quantised to 1/4 so that ties are everywhere; a NaN, a +inf and a -inf are sprinkled in."""
    rng = np.random.default_rng(1000 * B + C)
    nlc = C - 1
    x = rng.standard_normal((B, C)).astype(np.float32) * 2.0
    x[::2] = np.round(x[::2] * 4.0) / 4.0
    if B >= 5:
        x[1, rng.integers(C)] = NAN
        x[2, rng.integers(C)] = INF
        x[3, rng.integers(C)] = -INF
        x[4, :] = 0.0
        x[4, ::2] = -0.0
    label = rng.integers(0, C, B)
    label[::4] = nlc
    bucket = rng.integers(-1, 4, B)
    dist, inv = _tables(nlc, rng)
    radii8 = (0.0, 50.0, 100.0, 150.0, 200.0, 300.0, 399.9, INF)
    acc8 = (0, 1, 2, 5, 10, 20, nlc, 10**12)
    for view in (False, True):
        for use_b, use_d, use_i, n in [(0, 0, 0, 0), (1, 1, 1, 8), (1, 0, 0, 8), (0, 1, 0, 8), (0, 1, 1, 0), (1, 1, 1, 3)]:
            _check(x, label, nlc, topk=5, bucket=bucket if use_b else None, dist=dist if use_d else None,
                   inv_rank=inv if use_i else None, radii=radii8[:n] if use_d else (),
                   acc_is=acc8[:n] if use_i else (), view=view, what=(view, use_b, use_d, use_i, n))
    _check(x, label, nlc, topk=1, what="topk 1")
    _check(x, label, nlc, topk=C + 5, what="topk past C")


def test_constructed_rows():
    """Rows whose answer is decided by the tie rule, with the expected numbers written out."""
    C, nlc = 6, 5
    x = np.array([
        [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],    # 0: all equal, label 3: first entry 0, label at position 3, rank 4
        [0.5, 2.0, 0.0, 2.0, -1.0, 0.0],   # 1: label 3 tied with the LOWER index 1: position 1, rank 2, pred1 = 1
        [0.5, 2.0, 0.0, 2.0, -1.0, 0.0],   # 2: label 1 tied with the HIGHER index 3: position 0, pred1 = 1
        [0.0, 3.0, 1.0, 0.0, 0.0, 3.0],    # 3: no-leak tied with the best pipe: the pipe (lower index) is first
        [0.0, INF, 1.0, NAN, 0.0, 2.0],    # 4: NaN above +inf: pred1 = 3; label 1 at position 1
        [0.0, NAN, 1.0, NAN, 0.0, 2.0],    # 5: two NaNs: the lower index first; label 5 (no-leak) at position 2
    ], dtype=np.float32)
    label = np.array([3, 3, 1, 5, 1, 5])
    got = _check(x, label, nlc, topk=2, what="constructed")
    cnt, rank, _ = _run(x, label, nlc, topk=2)
    assert rank.cpu().tolist() == [4, 2, 1, 0, 2, 0]
    # hit1: rows 2 only (row 3 predicts pipe 1 for a no-leak label); hitk (positions 3, 1, 0, 1, 1, 2 < 2): rows 1-4
    assert got["correct1"] == 1 and got["correctk"] == 4
    assert (got["tp"], got["fp"], got["fn"], got["tn"]) == (4, 2, 0, 0)
    assert got["nl_total"] == 2 and got["nl_correct"] == 0 and got["leak_correct1"] == 1 and got["leak_correctk"] == 3
    # the same rows with the no-leak entry alone on top: now it wins
    x[3, 5] = 3.5
    assert _check(x, label, nlc, topk=2)["tn"] == 1


@pytest.mark.parametrize("kind", ["noleak", "leak"])
def test_all_labels_one_kind(kind):
    rng = np.random.default_rng(7)
    B, C = 9, 65
    nlc = C - 1
    x = rng.standard_normal((B, C)).astype(np.float32)
    label = np.full(B, nlc) if kind == "noleak" else rng.integers(0, nlc, B)
    dist, inv = _tables(nlc, rng)
    got = _check(x, label, nlc, bucket=rng.integers(0, 4, B), dist=dist, inv_rank=inv, radii=(100.0, INF), acc_is=(1, 5))
    assert got["nl_total" if kind == "noleak" else "leak_total"] == B
    assert got["leak_total" if kind == "noleak" else "nl_total"] == 0


@pytest.mark.parametrize("bad", [-1, 65, 2**40, -2**40])
def test_out_of_range_label_touches_bad_label_only(bad):
    from models.ops import WINDOW_COUNTERS
    rng = np.random.default_rng(11)
    B, C = 6, 65
    nlc = C - 1
    x = rng.standard_normal((B, C)).astype(np.float32)
    label = rng.integers(0, C, B)
    bucket = rng.integers(0, 4, B)
    dist, inv = _tables(nlc, rng)
    kw = dict(dist=dist, inv_rank=inv, radii=(100.0, INF), acc_is=(1, 5))
    label[2] = bad
    got = _check(x, label, nlc, bucket=bucket, **kw)
    keep = np.arange(B) != 2
    rest = _check(x[keep], label[keep], nlc, bucket=bucket[keep], **kw)
    assert got["bad_label"] == 1 and rest["bad_label"] == 0
    assert all(got[k] == rest[k] for k in WINDOW_COUNTERS if k != "bad_label")


def test_accumulates_in_place_and_repeats():
    """Two calls into one counter tensor == the sum of two separate calls; a repeated call gives
    the same integers (integer atomics: nothing depends on scheduling)."""
    rng = np.random.default_rng(13)
    C = 765
    nlc = C - 1
    dist, inv = _tables(nlc, rng)
    kw = dict(dist=dist, inv_rank=inv, radii=(50.0, 100.0, 300.0), acc_is=(1, 5, 10, 20))
    xs = [np.round(rng.standard_normal((B, C)) * 8.0).astype(np.float32) / 8.0 for B in (67, 5)]
    labels = [rng.integers(0, C, x.shape[0]) for x in xs]
    buckets = [rng.integers(-1, 4, x.shape[0]) for x in xs]
    one = [_run(x, l, nlc, bucket=b, **kw)[0] for x, l, b in zip(xs, labels, buckets)]
    both, _, _ = _run(xs[0], labels[0], nlc, bucket=buckets[0], **kw)
    _run(xs[1], labels[1], nlc, bucket=buckets[1], counters=both, **kw)
    assert torch.equal(both, one[0] + one[1]) and int(both[0]) == 72
    again = [_run(x, l, nlc, bucket=b, **kw) for x, l, b in zip(xs, labels, buckets)]
    assert all(torch.equal(a[0], o) for a, o in zip(again, one))


def test_window_metrics_does_not_synchronise():
    from models import ops
    rng = np.random.default_rng(17)
    B, C = 67, 765
    nlc = C - 1
    dist, inv = _tables(nlc, rng)
    x, label = _dev(rng.standard_normal((B, C)).astype(np.float32)), _dev(rng.integers(0, C, B), torch.int64)
    bucket, distd, invd = _dev(rng.integers(-1, 4, B), torch.int32), _dev(dist), _dev(inv)
    cnt = ops.window_counters(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            rank, atd = ops.window_metrics(x, label, nlc, cnt, topk=5, bucket=bucket, dist=distd, inv_rank=invd,
                                           radii=(50.0, 100.0, 300.0), acc_is=(1, 5, 10, 20))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(cnt[0]) == 2 * B and rank.shape == (B,) and atd.shape == (B,)


def test_window_metrics_refuses_what_it_cannot_read():
    from models import ops
    x = torch.zeros(4, 6, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    cnt = ops.window_counters(DEV)
    with pytest.raises(ValueError, match="float32"):
        ops.window_metrics(x.double(), lab, 5, cnt)
    with pytest.raises(ValueError, match="column stride"):
        ops.window_metrics(torch.zeros(6, 4, device=DEV).t(), lab, 5, cnt)
    with pytest.raises(ValueError, match="label"):
        ops.window_metrics(x, lab.int(), 5, cnt)
    with pytest.raises(ValueError, match="counters"):
        ops.window_metrics(x, lab, 5, cnt[:-1])
    with pytest.raises(Exception, match="invalid|LG_EINVAL|argument"):
        ops.window_metrics(x, lab, 6, cnt)  # nlc outside 1 .. C - 1: LG_EINVAL from the library
    rank, atd = ops.window_metrics(x[:0], lab[:0], 5, cnt)  # an empty batch: no launch
    assert rank.numel() == 0 and atd is None and int(cnt.sum()) == 0


# ------------------------------------------------------------------ event_decide
def _event_check(x: np.ndarray, end_ns: np.ndarray, agg_ns: int, noleak: int, view: bool = False, what=""):
    import pandas as pd
    from models import ops
    from models.event_evaluator import first_alarm, sum_logits_from
    xd = _sliced(x) if view else _dev(x)
    out, summed = ops.event_decide(xd, _dev(end_ns, torch.int64), agg_ns, noleak, want_sum=True)
    out2, none = ops.event_decide(xd, _dev(end_ns, torch.int64), agg_ns, noleak)
    assert none is None and torch.equal(out, out2)
    trig, stop, pred, s = event_truth(x, end_ns, agg_ns, noleak)
    assert out.dtype == torch.int64 and out.cpu().tolist() == [trig, stop, pred], what
    assert np.array_equal(summed.cpu().numpy().view(np.uint32), s.view(np.uint32)), what
    host = xd.cpu()  # the host copy the CPU route works on
    assert (first_alarm(host, noleak) if host.numel() else None) == (None if trig < 0 else trig)
    if trig >= 0:
        ref = sum_logits_from(host, end_ns, trig, pd.Timedelta(agg_ns, unit="ns"))
        assert np.array_equal(summed.cpu().numpy().view(np.uint32), ref.numpy().view(np.uint32)), what
    return trig, stop, pred


@pytest.mark.parametrize("W", [1, 40])
def test_event_decide(W):
    """No alarm at all, an alarm in the last row, agg_ns = 0, a window that reaches W, a window
    that ends inside; the summed row has the bits of sum_logits_from on the host copy."""
    rng = np.random.default_rng(100 + W)
    C = 765
    noleak = C - 1
    step = 300 * 10**9
    end_ns = (np.arange(W, dtype=np.int64) * 300 + 11) * 10**9
    quiet = rng.standard_normal((W, C)).astype(np.float32)
    quiet[:, noleak] = 9.0
    assert _event_check(quiet, end_ns, 12 * step, noleak, what="no alarm") == (-1, -1, -1)
    tie = quiet.copy()
    tie[:, 5] = 9.0  # a pipe ties with no-leak in every row: the pipe (lower index) is first, so row 0 alarms
    assert _event_check(tie, end_ns, 0, noleak, what="tie")[:2] == (0, 1)
    last = quiet.copy()
    last[W - 1, 17] = 9.5
    assert _event_check(last, end_ns, 12 * step, noleak, what="last row") == (W - 1, W, 17)
    if W == 1:
        return
    x = rng.standard_normal((W, C)).astype(np.float32) * 3.0
    x[:, noleak] += 4.0
    x[:9, noleak] = 50.0
    x[9, 123] = 60.0  # the trigger; the rows after it decide the sum
    for agg, stop in [(0, 10), (1, 10), (step, 10), (step + 1, 11), (12 * step, 21), (31 * step, 40), (10**15, 40)]:
        for view in (False, True):
            trig, got_stop, _ = _event_check(x, end_ns, agg, noleak, view=view, what=(agg, view))
            assert (trig, got_stop) == (9, stop), agg
    x[20, 3] = NAN  # from row 20 on the sum's column 3 is NaN, and NaN is first
    assert _event_check(x, end_ns, 12 * step, noleak, what="nan")[2] == 3
    narrow = x[:, :2].copy()  # C = 2
    narrow[:, 1] = 0.0
    narrow[:, 0] = -1.0
    narrow[30, 0] = 1.0
    assert _event_check(narrow, end_ns, 3 * step, 1, what="C = 2") == (30, 33, 1)


def test_event_decide_empty_scenario():
    from models import ops
    out, summed = ops.event_decide(torch.zeros(0, 9, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV),
                                   10**9, 8, want_sum=True)
    assert out.cpu().tolist() == [-1, -1, -1] and not summed.cpu().any()


# ------------------------------------------------------------------ the evaluator, end to end
GROUPS = ("basic", "binary", "bucket", "atd", "success", "accuracy_i")


@pytest.fixture(scope="module")
def leak_set(tmp_path_factory):
    from models.datasets import AbruptLeakDetectorDataset, SensorStandardizer
    from models.synth import write_synthetic_leak_set
    info = json.loads((GOLD / "harness.json").read_text())
    arrs = np.load(GOLD / "harness.npz")
    d = tmp_path_factory.mktemp("synthds_wm") / "leak"
    write_synthetic_leak_set(d, info["sensors"], info["pipes"], scenes_per_pipe=2, n_noleak=6, T=400, seed=0)
    st = SensorStandardizer(arrs["std_mean"], arrs["std_std"])
    eds = AbruptLeakDetectorDataset(d, steps_per_epoch=48, seed=7, standardizer=st, sensor_ids=info["sensors"])
    return info, arrs, eds


@pytest.mark.parametrize("loader_kind", ["dataloader", "device"])
def test_evaluator_fused_equals_torch_route(leak_set, loader_kind):
    """DetectorEvaluator(fused=True) == DetectorEvaluator(fused=False), dict against dict, on the
    synthetic leak set and the stand-in detector of tests/test_harness.py, all six metric groups;
    and fused=None takes the kernel route for these logits."""
    from torch.utils.data import DataLoader
    from models.datasets import DeviceBatchLoader
    from models.window_evaluator import DetectorEvaluator
    from test_harness import _fixed_detector, _tcn
    info, arrs, eds = leak_set
    seen = []

    class Recording(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = _fixed_detector(arrs)

        def forward(self, residual, tfeat):
            out = self.inner(residual, tfeat)
            seen.append(out.detach().clone())
            return out

    def run(fused):
        seen.clear()
        ev = DetectorEvaluator(_tcn().to(DEV), Recording(), DEV, l_pred=36, l_det=36, topk=5, metric_groups=GROUPS,
                               inp_path=LTA_INP, pipe_ids_in_order=info["pipe_ids_in_order"], fused=fused)
        loader = DataLoader(eds, batch_size=16) if loader_kind == "dataloader" else DeviceBatchLoader(eds, 16, DEV)
        return ev.evaluate(loader), torch.cat(seen)

    torch_route, logits = run(False)
    # a condition on the input: the torch route is defined only without ties
    assert logits.dtype == torch.float32 and logits.shape == (48, len(info["pipes"]) + 1)
    assert all(len(set(row.tolist())) == row.numel() for row in logits.cpu()) and bool(torch.isfinite(logits).all())
    fused, logits_f = run(True)
    assert torch.equal(logits, logits_f)
    assert set(fused) == set(torch_route)
    assert fused == torch_route, {k: (fused[k], torch_route[k]) for k in fused if fused[k] != torch_route[k]}
    assert fused["n_total"] == 48.0 and fused["n_leak"] > 0 and fused["n_noleak"] > 0 and fused["atd_n"] > 0
    default, _ = run(None)
    assert default == fused


def test_evaluator_fused_raises_on_bad_label(leak_set):
    from models.window_evaluator import DetectorEvaluator
    from test_harness import _fixed_detector, _tcn
    info, arrs, eds = leak_set
    batch = {k: (torch.as_tensor(np.stack([np.asarray(eds[i][k]) for i in range(4)])) if k in ("noisy_seg", "time_seg")
                 else [eds[i][k] for i in range(4)]) for k in ("noisy_seg", "time_seg", "label", "bucket")}
    ev = DetectorEvaluator(_tcn().to(DEV), _fixed_detector(arrs), DEV, l_pred=36, l_det=36, fused=True)
    assert ev.evaluate([batch])["n_total"] == 4.0
    batch["label"][1] = len(info["pipes"]) + 1
    with pytest.raises(ValueError, match="label outside"):
        ev.evaluate([batch])
