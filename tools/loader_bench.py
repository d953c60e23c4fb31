"""Time of one full iteration of DeviceBatchLoader in its two draw modes.

  python tools/loader_bench.py [--batch 256] [--batches 100] [--pipes 250] [--scenes_per_pipe 4]
                               [--rounds 3] [--data DIR] [--out FILE]

A synthetic abrupt-leak set from models/synth.py (pipes x scenes_per_pipe leak scenes, T = 240 at
29 sensors) is written once, loaded into HBM once per mode, and the loader is iterated over
`batches` batches of `batch` windows with nothing consuming them, so what is timed is the loader
alone: draw="host" makes the per-sample numpy draws on the CPU, draw="device" in a HIP kernel.  A
batch counts as done at a device event recorded on the loader's stream after the batch was
yielded, i.e. after its tensors are ready; the iteration's time runs from before iter() to the last
event (the device mode's up-front draw launch and its final error-word read included in the wall
figure).  Reported per mode and round: ms per batch (wall / batches), batches/s, and the median gap
between consecutive batch events.  The modes alternate, `rounds` times.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "leak-det-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_iteration(loader) -> dict:
    marks = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in loader:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)
    marks[-1].synchronize()
    wall = time.perf_counter() - t0
    torch.cuda.synchronize()
    gaps = [a.elapsed_time(b) for a, b in zip(marks[1:-1], marks[2:])]
    n = len(marks)
    return {"ms_per_batch": round(wall * 1e3 / n, 4), "batches_per_s": round(n / wall, 1),
            "event_gap_ms_median": round(statistics.median(gaps), 4) if gaps else None}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--pipes", type=int, default=250)
    ap.add_argument("--scenes_per_pipe", type=int, default=4)
    ap.add_argument("--noleak", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--data", type=str, default=None, help="directory for the synthetic set (default: a temp dir)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench: needs a ROCm GPU; a CPU run measures nothing")
    from models.datasets import AbruptLeakDetectorDataset, DeviceBatchLoader
    from models.synth import write_synthetic_leak_set
    dev = torch.device("cuda:0")
    sensors = [f"n{i}" for i in range(29)]
    pipes = [f"p{i}" for i in range(args.pipes)]
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(args.data or tmp) / "leak"
        if not (root / "manifest.jsonl").is_file():
            write_synthetic_leak_set(root, sensors, pipes, scenes_per_pipe=args.scenes_per_pipe, n_noleak=args.noleak,
                                     T=240, seed=0)
        ds = AbruptLeakDetectorDataset(root, steps_per_epoch=args.batch * args.batches, seed=123, sensor_ids=sensors,
                                       cache_size=1 << 20)
        loaders = {m: DeviceBatchLoader(ds, args.batch, dev, draw=m) for m in ("host", "device")}
        for ld in loaders.values():  # warm-up: allocator, kernel load, numpy's first calls
            for i, _ in enumerate(DeviceBatchLoader(ds, args.batch, dev, draw=ld.draw)):
                if i == 2:
                    break
        res = {m: [] for m in loaders}
        for _ in range(args.rounds):
            for m, ld in loaders.items():
                res[m].append(timed_iteration(ld))
        result = {"batch": args.batch, "batches": args.batches, "leak_scenes": len(ds.leak_scene_ids),
                  "noleak_scenes": len(ds.noleak_scene_ids), "seg_len": ds.seg_len, **res}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
