"""Host side of the evaluator kernels (CPU): the argument checks of lg_window_metrics /
lg_event_decide through the C ABI with no device, the counter layout, and the brute-force numpy
statement of the row order that tests/test_gpu_window_metrics.py holds the kernels to.

The order (include/leakgnn.h): entry a precedes entry b when a's value is greater, NaN counting as
greater than +inf, or the values are equal and a's index is lower.  `row_order` below writes it out
as a sort by (-value, index) with NaN first; `window_truth` / `event_truth` derive every output of
the two entry points from it, row by row, in plain Python."""
from __future__ import annotations

import inspect
import math
import re

import numpy as np
import torch

P = 0x1000  # any non-null address: a call that fails its argument checks never reads it
BUCKETS = ("early", "late", "pre", "noleak")


# ------------------------------------------------------------------ the truth (shared with the GPU tests)
def row_order(row: np.ndarray) -> list:
    """Indices of one row, first entry first: sorted by (-value, index), NaN before everything."""
    def key(i):
        v = float(row[i])
        return (0, 0.0, i) if math.isnan(v) else (1, -v, i)  # -0.0 == 0.0 under tuple comparison
    return sorted(range(len(row)), key=key)


def window_truth(logits: np.ndarray, label, nlc: int, topk: int, bucket=None, dist=None, inv_rank=None,
                 radii=(), acc_is=()):
    """(counters by name, rank_out, atd_out) of lg_window_metrics, from row_order alone."""
    from models.ops import WINDOW_COUNTERS
    B, C = logits.shape
    c = {name: 0 for name in WINDOW_COUNTERS}
    rank_out = np.zeros(B, dtype=np.int32)
    atd_out = np.full(B, np.nan, dtype=np.float64)
    for b in range(B):
        y = int(label[b])
        if not 0 <= y < C:
            c["bad_label"] += 1
            continue
        order = row_order(logits[b])
        pred1 = order[0]
        hit1 = pred1 == y
        hitk = order.index(y) < min(topk, C)
        is_nl = y == nlc
        pred_nl = pred1 == nlc
        c["total"] += 1
        c["correct1"] += hit1
        c["correctk"] += hitk
        c["nl_total"] += is_nl
        c["nl_correct"] += hit1 and is_nl
        c["leak_total"] += not is_nl
        c["leak_correct1"] += hit1 and not is_nl
        c["leak_correctk"] += hitk and not is_nl
        c["tp"] += (not pred_nl) and (not is_nl)
        c["fp"] += (not pred_nl) and is_nl
        c["fn"] += pred_nl and not is_nl
        c["tn"] += pred_nl and is_nl
        if bucket is not None:
            bc = int(bucket[b])
            if 0 <= bc < 4:
                name = BUCKETS[bc]
                c[f"b_total_{name}"] += 1
                c[f"b_correct1_{name}"] += hit1
                c[f"b_correctk_{name}"] += hitk
                c[f"b_pred_nl_{name}"] += pred_nl
            c["pre_false_alarm"] += is_nl and (not pred_nl) and bc == 2
            c["noleak_false_alarm"] += is_nl and (not pred_nl) and bc == 3
        if is_nl:
            continue
        pipes = [i for i in order if i < nlc]
        rank_out[b] = 1 + pipes.index(min(y, nlc - 1))
        if dist is None:
            continue
        look = (not pred_nl) and y < nlc
        pc = min(pred1, nlc - 1)
        d = float(dist[y, pc]) if look else math.inf
        atd_out[b] = d
        for r, rad in enumerate(radii):
            c[f"success[{r}]"] += d <= rad
        if inv_rank is not None and look:
            pos = int(inv_rank[pc, y])
            for i, ii in enumerate(acc_is):
                c[f"acc_i[{i}]"] += pos < ii and ii > 0
    return {k: int(v) for k, v in c.items()}, rank_out, (atd_out if dist is not None else None)


def event_truth(logits: np.ndarray, end_ns: np.ndarray, agg_ns: int, noleak: int):
    """(trig, stop, pred, summed) of lg_event_decide from row_order; (-1, -1, -1, zeros) without an alarm."""
    W, C = logits.shape
    trig = next((i for i in range(W) if row_order(logits[i])[0] != noleak), -1)
    if trig < 0:
        return -1, -1, -1, np.zeros(C, dtype=np.float32)
    stop = next((i for i in range(trig, W) if int(end_ns[i]) - int(end_ns[trig]) >= agg_ns), W)
    stop = max(stop, trig + 1)
    s = logits[trig].astype(np.float32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(trig + 1, stop):
            s = (s + logits[i]).astype(np.float32)
    return trig, stop, row_order(s)[0], s


# ------------------------------------------------------------------ tests
def test_row_order_statement():
    inf, nan = math.inf, math.nan
    assert row_order(np.array([1.0, 3.0, 2.0], dtype=np.float32)) == [1, 2, 0]
    assert row_order(np.array([2.0, 2.0, 2.0], dtype=np.float32)) == [0, 1, 2]          # ties: the lower index
    assert row_order(np.array([1.0, inf, nan, -inf, nan], dtype=np.float32)) == [2, 4, 1, 0, 3]  # NaN above +inf
    assert row_order(np.array([-0.0, 0.0, -1.0], dtype=np.float32)) == [0, 1, 2]          # -0 == +0


def test_truth_agrees_with_torch_route_on_tie_free_rows():
    """On rows without a repeated value the order gives what the evaluator's torch code computes
    (argmax, topk membership, the stable descending argsort's rank), run here on the CPU."""
    g = torch.Generator().manual_seed(3)
    B, C, nlc, topk = 37, 21, 20, 5
    x = torch.randn(B, C, generator=g)
    assert all(len(set(r.tolist())) == C for r in x)
    label = torch.randint(0, C, (B,), generator=g)
    label[:6] = nlc
    dist = torch.rand(nlc, nlc, generator=g, dtype=torch.float64) * 400.0
    rank_tab = torch.argsort(dist.float(), dim=1)
    inv = torch.empty_like(rank_tab)
    inv.scatter_(1, rank_tab, torch.arange(nlc).expand_as(rank_tab))
    radii, acc_is = (50.0, 100.0, 300.0), (1, 5, 10, 0)
    c, rank_out, atd_out = window_truth(x.numpy(), label.numpy(), nlc, topk, None, dist.numpy(), inv.numpy(),
                                        radii, acc_is)
    # the torch route of DetectorEvaluator.evaluate, statement by statement
    pred1 = x.argmax(dim=-1)
    hitk = (x.topk(k=topk, dim=-1).indices == label.unsqueeze(1)).any(dim=1)
    hit1 = pred1 == label
    is_nl = label == nlc
    is_leak = ~is_nl
    order = torch.argsort(x[:, :nlc], dim=1, descending=True)
    invo = torch.empty_like(order)
    invo.scatter_(1, order, torch.arange(nlc).unsqueeze(0).expand(B, -1))
    ranks = invo.gather(1, label.clamp_max(nlc - 1).unsqueeze(1)).squeeze(1) + 1
    assert c["total"] == B and c["correct1"] == int(hit1.sum()) and c["correctk"] == int(hitk.sum())
    assert c["nl_correct"] == int((hit1 & is_nl).sum()) and c["leak_correctk"] == int((hitk & is_leak).sum())
    pred_leak = pred1 != nlc
    assert (c["tp"], c["fp"], c["fn"], c["tn"]) == tuple(int(v.sum()) for v in (
        pred_leak & is_leak, pred_leak & is_nl, ~pred_leak & is_leak, ~pred_leak & is_nl))
    assert np.array_equal(rank_out[is_leak.numpy()], ranks[is_leak].numpy())
    assert not rank_out[is_nl.numpy()].any()
    y, p = label[is_leak], pred1[is_leak]
    missed = p == nlc
    d = torch.where(missed, torch.full_like(y, 0, dtype=torch.float64), dist[y, p.clamp_max(nlc - 1)])
    d = torch.where(missed, torch.full_like(d, float("inf")), d)
    assert np.array_equal(atd_out[is_leak.numpy()], d.numpy()) and np.isnan(atd_out[is_nl.numpy()]).all()
    for r, rad in enumerate(radii):
        assert c[f"success[{r}]"] == int((d <= rad).sum())
    pos = inv[p.clamp_max(nlc - 1), y]
    for i, ii in enumerate(acc_is):
        assert c[f"acc_i[{i}]"] == int(((~missed) & (pos < ii) & (ii > 0)).sum())


def test_event_truth_agrees_with_host_helpers():
    import pandas as pd
    from models.event_evaluator import first_alarm, sum_logits_from
    g = torch.Generator().manual_seed(5)
    W, C = 40, 9
    x = torch.randn(W, C, generator=g)
    x[:, C - 1] += 1.5
    x[:7, C - 1] = 10.0  # the first seven windows stay no-leak
    end_ns = (np.arange(W, dtype=np.int64) * 300 + 7) * 10**9
    for agg_s in (0, 300, 1500, 10**6):
        trig, stop, pred, s = event_truth(x.numpy(), end_ns, agg_s * 10**9, C - 1)
        assert trig == first_alarm(x, C - 1) and trig >= 7
        ref = sum_logits_from(x, end_ns, trig, pd.Timedelta(seconds=agg_s))
        assert np.array_equal(s.view(np.uint32), ref.numpy().view(np.uint32)) and pred == int(torch.argmax(ref))
        assert stop == (W if agg_s == 10**6 else trig + max(1, agg_s // 300))


def test_window_counters_cover_evaluate():
    """ops.WINDOW_COUNTERS (with its two aliases) has a slot for every name evaluate() accumulates
    under, in the order include/leakgnn.h documents, plus bad_label."""
    from models import ops, window_evaluator
    names = ops.WINDOW_COUNTERS
    assert len(names) == len(set(names)) == 47 and names[-1] == "bad_label"
    assert ops.WINDOW_BUCKETS == window_evaluator._BUCKETS == BUCKETS and ops.WINDOW_MAX_LIST == 8
    assert names[:12] == ("total", "correct1", "correctk", "nl_total", "nl_correct", "leak_total", "leak_correct1",
                          "leak_correctk", "tp", "fp", "fn", "tn")
    assert names[12:16] == ("b_total_early", "b_correct1_early", "b_correctk_early", "b_pred_nl_early")
    assert names[28:30] == ("pre_false_alarm", "noleak_false_alarm")
    assert names[30] == "success[0]" and names[37] == "success[7]" and names[38] == "acc_i[0]" and names[45] == "acc_i[7]"
    src = inspect.getsource(window_evaluator.DetectorEvaluator.evaluate)
    used = set(re.findall(r'add\(f?"([^"]+)"', src))
    assert {"total", "tp", "b_total_{b}", "success_{r}", "acc_i_{ii}", "pre_total"} <= used  # the pattern finds them
    for name in used:
        if name == "success_{r}":
            want = ["success[0]"]
        elif name == "acc_i_{ii}":
            want = ["acc_i[0]"]
        elif "{b}" in name:
            want = [name.replace("{b}", b) for b in BUCKETS]
        else:
            want = [ops.WINDOW_COUNTER_ALIASES.get(name, name)]
        assert set(want) <= set(names), name


# logits, label, B, C, ldx, nlc, topk, bucket, dist, inv_rank, radii_host, R, acc_is_host, I, counters, n_counters,
# rank_out, atd_out, stream
WM_OK = [P, P, 4, 5, 6, 4, 5, P, P, P, P, 3, P, 4, P, 47, P, P, None]


def test_window_metrics_c_abi_validation():
    """LG_EINVAL (-1) for each bad argument, with no GPU and no device memory; B == 0 is LG_OK."""
    from models import _native
    lib = _native.load_library()
    bad = {0: [None], 1: [None], 14: [None],          # null logits, label, counters
           2: [-1],                                   # B < 0
           3: [1, 0, -2],                             # C < 2 (nlc = 4 is then out of range as well)
           4: [4, 0],                                 # ldx < C
           5: [0, 5, -1, 9],                          # nlc outside 1 .. C - 1
           6: [0, -3],                                # topk < 1
           11: [-1, 9], 13: [-1, 9],                  # R, I outside 0 .. 8
           8: [None],                                 # inv_rank without dist
           15: [46, 48, 0],                           # a counter tensor of another layout
           16: [None], 17: [None],                    # outputs the call would write
           10: [None], 12: [None]}                    # R > 0 / I > 0 without the host array
    for i, vals in bad.items():
        for v in vals:
            a = list(WM_OK)
            a[i] = v
            assert lib.lg_window_metrics(*a) == -1, f"argument {i} = {v}"
    a = list(WM_OK)
    a[3], a[4], a[5] = 1, 1, 1  # C < 2 on its own
    assert lib.lg_window_metrics(*a) == -1
    # the optional inputs absent, lists empty: still checked before any HIP call; B == 0 returns LG_OK
    a = list(WM_OK)
    a[2] = 0
    assert lib.lg_window_metrics(*a) == 0
    a[7] = a[8] = a[9] = a[10] = a[12] = a[17] = None
    a[11] = a[13] = 0
    assert lib.lg_window_metrics(*a) == 0
    a[0] = a[1] = a[16] = None  # an empty batch has no rows to point at
    assert lib.lg_window_metrics(*a) == 0
    a[14] = None                # but the counters are checked even then
    assert lib.lg_window_metrics(*a) == -1


def test_event_decide_c_abi_validation():
    from models import _native
    lib = _native.load_library()
    assert lib.lg_event_decide_workspace_bytes(40) == 160 and lib.lg_event_decide_workspace_bytes(0) == 0
    # logits, end_ns, W, C, ldx, agg_ns, noleak, out, summed, workspace, workspace_bytes, stream
    ok = [P, P, 40, 9, 9, 10**9, 8, P, P, P, 160, None]
    bad = {0: [None], 1: [None], 2: [-1], 3: [0, -1], 4: [8], 6: [-1, 9], 7: [None], 9: [None], 10: [159, 0]}
    for i, vals in bad.items():
        for v in vals:
            a = list(ok)
            a[i] = v
            assert lib.lg_event_decide(*a) == -1, f"argument {i} = {v}"


def test_evaluator_fused_flag_on_cpu():
    """fused=None resolves to the torch route for CPU logits; fused=True refuses them."""
    import pytest
    from models.window_evaluator import DetectorEvaluator
    none = torch.nn.Identity()
    x = torch.zeros(2, 5)
    ev = DetectorEvaluator(none, none, torch.device("cpu"), l_pred=1, l_det=1)
    assert ev.fused is None and ev._fused_for(x) is False
    assert DetectorEvaluator(none, none, torch.device("cpu"), l_pred=1, l_det=1, fused=False)._fused_for(x) is False
    with pytest.raises(ValueError, match="fused=True"):
        DetectorEvaluator(none, none, torch.device("cpu"), l_pred=1, l_det=1, fused=True)._fused_for(x)
