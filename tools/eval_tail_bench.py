"""Time of the evaluator tails on the GPU: the torch route against the HIP kernels.

  python tools/eval_tail_bench.py [--B 256] [--P 764] [--iters 300] [--W 2000] [--out FILE]

Window evaluator: DetectorEvaluator.evaluate over `iters` identical batches whose "detector" hands
back one fixed (B, P+1) logits tensor and whose residual builder does nothing, so that what is
timed is the tail alone: from the logits to the accumulated counters, all six metric groups, the
batch dict shaped as datasets.DeviceBatchLoader writes it.  The loader records a device event
before it yields each batch; a batch's time is the gap between two consecutive events, reported as
the median over the warmed batches, next to the wall time per batch of the whole call.
fused=False is the parent route (torch ops), fused=True the one launch of leakgnn::window_metrics;
the two are run alternately, `rounds` times.

Event evaluator: one scenario of W windows, alarm at W / 4, a 12 h aggregation window at 5 min
steps.  Host route: the logits' copy to the host, first_alarm, sum_logits_from and the argmax
(what evaluate_dataset_event_level did on every device); kernel route: leakgnn::event_decide and
the copy of its three integers.  Wall time around work that ends in a synchronising copy, median
over `iters // 3` warmed repeats.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "leak-det-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GROUPS = ("basic", "binary", "bucket", "atd", "success", "accuracy_i")
WARM = 20


def window_leg(B: int, P: int, iters: int, rounds: int, dev: torch.device) -> dict:
    import pandas as pd  # noqa: F401  (the evaluators' own import, paid before any timing)
    from models.window_evaluator import _BUCKETS, DetectorEvaluator
    g = torch.Generator().manual_seed(0)
    C = P + 1
    base = torch.linspace(-4.0, 4.0, C)  # every row a permutation of C distinct values: no ties, so the
    logits = torch.stack([base[torch.randperm(C, generator=g)] for _ in range(B)])  # torch route is defined
    logits[: B // 3, P] = 10.0  # a third of the rows predict no-leak
    logits = logits.to(dev)
    label = torch.randint(0, C, (B,), generator=g)
    label[::5] = P
    seg = torch.zeros(B, 2, 1, device=dev)
    batch = {"noisy_seg": seg, "time_seg": seg, "label": label.to(dev),
             "bucket": [_BUCKETS[i % 4] for i in range(B)],
             "num_classes": torch.full((B,), C, dtype=torch.long, device=dev)}

    class Fixed(torch.nn.Module):
        def forward(self, residual, tfeat):
            return logits

    def make(fused: bool) -> DetectorEvaluator:
        ev = DetectorEvaluator(torch.nn.Identity(), Fixed(), dev, l_pred=1, l_det=1, topk=5, metric_groups=GROUPS,
                               inp_path=REPO / "leak-det-gnn_amd" / "data" / "L-TOWN-A.inp", pipe_ids_in_order=PIPES[:P],
                               fused=fused)
        ev.residual_builder = lambda predictor, noisy, tseg, **kw: noisy
        return ev

    def timed(ev: DetectorEvaluator) -> tuple:
        marks = []

        def loader():
            for _ in range(WARM + iters):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)
                yield batch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.evaluate(loader())
        wall = (time.perf_counter() - t0) / (WARM + iters)
        torch.cuda.synchronize()
        gaps = [marks[i].elapsed_time(marks[i + 1]) * 1e3 for i in range(WARM, WARM + iters - 1)]
        return out, statistics.median(gaps), wall * 1e6

    evs = {"torch": make(False), "hip": make(True)}
    res = {k: {"event_gap_us": [], "wall_us": []} for k in evs}
    outs = {}
    for _ in range(rounds):
        for k, ev in evs.items():
            outs[k], gap, wall = timed(ev)
            res[k]["event_gap_us"].append(round(gap, 1))
            res[k]["wall_us"].append(round(wall, 1))
    assert outs["torch"] == outs["hip"], "the two routes disagree on tie-free logits"
    return {"B": B, "C": C, "batches": iters, **res}


def event_leg(W: int, C: int, reps: int, rounds: int, dev: torch.device) -> dict:
    import pandas as pd
    from models import ops
    from models.event_evaluator import first_alarm, sum_logits_from
    g = torch.Generator().manual_seed(1)
    x = torch.randn(W, C, generator=g)
    x[:, C - 1] += 2.0
    x[: W // 4, C - 1] = 20.0
    x[W // 4, 7] = 30.0
    end_ns = (np.arange(W, dtype=np.int64) * 300) * 10**9
    agg = pd.Timedelta(hours=12.0)
    xd, ed = x.to(dev), torch.from_numpy(end_ns).to(dev)

    def host():
        lg = xd.cpu()
        trig = first_alarm(lg, C - 1)
        return trig, int(torch.argmax(sum_logits_from(lg, end_ns, trig, agg)))

    def hip():
        out, _ = ops.event_decide(xd, ed, int(agg.value), C - 1)
        trig, _, pred = out.tolist()
        return trig, pred

    assert host() == hip() == (W // 4, host()[1])
    res = {"torch_host": [], "hip": []}
    for _ in range(rounds):
        for name, fn in (("torch_host", host), ("hip", hip)):
            ts = []
            for i in range(5 + reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e6)
            res[name].append(round(statistics.median(ts[5:]), 1))
    return {"W": W, "C": C, "agg_rows": 144, "wall_us": res}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--P", type=int, default=764)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--W", type=int, default=2000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_tail_bench: needs a ROCm GPU; a CPU run measures nothing")
    with np.load(REPO / "tests" / "golden" / "graph_ltown_a.npz") as z:
        PIPES = [str(p) for p in z["pipe_ids"]]
    dev = torch.device("cuda:0")
    result = {"window": window_leg(args.B, args.P, args.iters, args.rounds, dev),
              "event": event_leg(args.W, args.P + 1, max(10, args.iters // 3), args.rounds, dev)}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
