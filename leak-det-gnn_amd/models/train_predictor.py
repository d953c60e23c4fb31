"""Train + evaluate the normal-state predictor on no-leak data (reference
models/train_predictor.py): same CLI flags (:95-109), split (:46-56), loop order
(:196-222) and checkpoint schema (:236-244).

  python -m models.train_predictor --normal_root DATA --out_dir OUT [--arch tcn|gru] ...

Differences that do not change results: batches come from datasets.DeviceBatchLoader
(scenes resident in HBM, one gather per batch; --loader torch restores the
DataLoader path), and checkpoints store the standardizer as plain lists of floats: they
load with torch.load(weights_only=True), and the reference's loaders
(train_detector.py / event_evaluator.py: np.asarray(std_mean, dtype=np.float32) after a
load with map_location=cuda) accept them on any device.

On a ROCm GPU the step's tail is fused: the head and the loss are one op
(loss.head_mse_loss over model.features(...), one launch each way) and clip_grad_norm_ + AdamW one
launch (optim.ClipAdamW, whose error word is read once per epoch).  --capture on replays every
full-size batch's step as one captured HIP graph (models/graph_step.py) and runs the tail batch
eagerly; --capture auto (the default) captures for the archs where the captured step measured
faster than the eager one on every round (CAPTURE_AUTO below).  --device cpu keeps
torch's AdamW and nn.MSELoss.
"""
from __future__ import annotations

import argparse
import json
import math
import random
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from .datasets import DeviceBatchLoader, NormalPredictorDataset, ShardBatchSampler, compute_sensor_stats_from_normal
from .predictor import NormalPredictorGRU, NormalPredictorTCN
from .utils import now


# --capture auto: the archs whose captured step's slowest round was below the parent step's fastest
# (tools/kbench.py --which predictor_step)
CAPTURE_AUTO = {"tcn": True, "gru": True}


class PredictorFeatures(nn.Module):
    """What graph_step.CapturedTrainStep trains: forward is the predictor's `features`, and the
    parameters are the whole predictor's, head included (the loss function applies the head)."""

    def __init__(self, predictor: nn.Module) -> None:
        super().__init__()
        self.predictor = predictor

    def forward(self, x: torch.Tensor, x_time: torch.Tensor) -> torch.Tensor:
        return self.predictor.features(x, x_time)


def head_loss_fn(predictor: nn.Module):
    """loss_fn(features, y) = head_mse_loss with `predictor.head`'s weight and bias."""
    from .loss import head_mse_loss
    head = predictor.head

    def loss_fn(feat: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return head_mse_loss(feat, head.weight, head.bias, y)
    return loss_fn


class CapturedPredictorStep:
    """One training step of a predictor (features, head + MSE, backward, ClipAdamW with its own
    clipping) as one replayed HIP graph: graph_step.CapturedTrainStep over PredictorFeatures,
    built on the first batch without disturbing the parameters, the optimizer state or torch's
    generator.  A call with (x, x_time, y) copies a batch of the same shape into the static inputs,
    replays, and returns the (static) loss.  A replay updates the weights on the device without
    moving their version counters, so every call ends by dropping the cached weight packs
    (library.invalidate_weight_packs): no eager call after it reads a pack older than the weights."""

    def __init__(self, predictor: nn.Module, opt, x: torch.Tensor, x_time: torch.Tensor, y: torch.Tensor,
                 warmup: int = 2) -> None:
        from .graph_step import CapturedTrainStep
        self.step = CapturedTrainStep(PredictorFeatures(predictor), head_loss_fn(predictor), opt,
                                      (x.contiguous().clone(), x_time.contiguous().clone()), y.contiguous().clone(),
                                      clip=None, warmup=warmup, preserve_state=True)

    def __call__(self, x=None, x_time=None, y=None) -> torch.Tensor:
        from . import library
        if x is not None:
            self.step.inputs[0].copy_(x)
            self.step.inputs[1].copy_(x_time)
            self.step.label.copy_(y)
        loss = self.step()
        library.invalidate_weight_packs()
        return loss


def check_optimizer_errors(opt) -> None:
    """Raise if a ClipAdamW launch of this optimizer set its error word (step_t[2]: a grid-barrier
    wait timed out and that step's update is invalid)."""
    for group in opt.param_groups:
        st = group.get("step_t")
        if torch.is_tensor(st) and int(st[2:3].view(torch.int32).item()) != 0:
            raise RuntimeError("ClipAdamW reported a grid-barrier timeout (error word "
                               f"{int(st[2:3].view(torch.int32).item())}); the parameters are invalid")


def set_seed(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def pick_device(device: str) -> torch.device:
    if device == "auto":
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return torch.device(device)


def split_ids(ids: List[str], seed: int, ratios=(0.8, 0.1, 0.1)) -> Tuple[List[str], List[str], List[str]]:
    """train_predictor.py:46-56."""
    assert abs(sum(ratios) - 1.0) < 1e-6
    rng = random.Random(seed)
    ids = list(ids)
    rng.shuffle(ids)
    n = len(ids)
    n_train, n_val = int(n * ratios[0]), int(n * ratios[1])
    return ids[:n_train], ids[n_train:n_train + n_val], ids[n_train + n_val:]


def make_loader(ds, batch_size: int, device: torch.device, kind: str, num_workers: int = 0,
                shard: Tuple[int, int] = (0, 1)):
    """Batches of `batch_size` samples in index order; with shard = (rank, world) each rank
    gets its contiguous slice of every global batch (data parallelism)."""
    if kind == "device_draw":  # the per-sample draws on the device as well (datasets.DeviceBatchLoader, draw="device")
        if device.type != "cuda":
            raise ValueError("--loader device_draw needs the GPU path (--device cuda)")
        return DeviceBatchLoader(ds, batch_size, device, shard=shard, draw="device")
    if kind == "device" and device.type == "cuda":
        return DeviceBatchLoader(ds, batch_size, device, shard=shard)
    if shard[1] > 1:
        return DataLoader(ds, batch_sampler=ShardBatchSampler(len(ds), batch_size, *shard), num_workers=num_workers,
                          pin_memory=(device.type == "cuda"))
    return DataLoader(ds, batch_size=batch_size, num_workers=num_workers, pin_memory=(device.type == "cuda"))


@torch.no_grad()
def evaluate_predictor(model: nn.Module, loader, device: torch.device, standardizer_mean: torch.Tensor,
                       standardizer_std: torch.Tensor) -> Dict[str, float]:
    """MAE / RMSE in original units (train_predictor.py:58-92), sums kept on the device."""
    model.eval()
    mae_sum = torch.zeros((), dtype=torch.float64, device=device)
    mse_sum = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    for batch in loader:
        x, x_time = batch["x"].to(device), batch["x_time"].to(device)
        y = batch["y"].to(device)[:, 0, :]
        y_hat = model(x, x_time)
        err = (y_hat * standardizer_std + standardizer_mean) - (y * standardizer_std + standardizer_mean)
        mae_sum += err.abs().sum().double()
        mse_sum += (err * err).sum().double()
        n += y.numel()
    return {"mae": float(mae_sum.item() / max(n, 1)), "rmse": float(math.sqrt(mse_sum.item() / max(n, 1)))}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--normal_root", type=str, required=True, help="Path to normal dataset root")
    ap.add_argument("--out_dir", type=str, required=True, help="Output directory for checkpoints/logs")
    ap.add_argument("--arch", type=str, default="tcn", choices=["tcn", "gru"])
    ap.add_argument("--epochs", type=int, default=15)
    ap.add_argument("--steps_per_epoch", type=int, default=100000)
    ap.add_argument("--val_steps", type=int, default=8000)
    ap.add_argument("--test_steps", type=int, default=8000)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight_decay", type=float, default=1e-4)
    ap.add_argument("--grad_clip", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", type=str, default="auto", help="auto|cuda|cpu|cuda:0 ...")
    ap.add_argument("--num_workers", type=int, default=0)
    ap.add_argument("--log_every", type=int, default=50)
    ap.add_argument("--loader", type=str, default="device", choices=["device", "device_draw", "torch"],
                    help="device: scenes in HBM, samples drawn on the host; device_draw: drawn by a HIP kernel as "
                         "well (same batches, no host work per sample); torch: the reference's DataLoader")
    ap.add_argument("--capture", type=str, default="auto", choices=["auto", "on", "off"],
                    help="replay each full-size training batch's step as one captured HIP graph "
                         "(models/graph_step.py; auto = on for the GPU path where it measured faster); "
                         "the tail batch runs eagerly")
    ap.add_argument("--profile", type=int, default=0,
                    help="torch.profiler over this many training steps (after one warm-up step): "
                         "<out_dir>/predictor_trace.json + predictor_ops.txt (models/profiling.py)")
    args = ap.parse_args(argv)

    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    set_seed(args.seed)
    device = pick_device(args.device)
    fused_step = device.type == "cuda"  # head + MSE as one op, clip_grad_norm_ + AdamW as one launch
    use_graph = args.capture == "on" or (args.capture == "auto" and fused_step and CAPTURE_AUTO[args.arch])
    if use_graph and not fused_step:
        raise ValueError("--capture on needs the GPU path (--device cuda)")
    print(f"{now()} [predictor] device={device} seed={args.seed}")
    print(f"{now()} [predictor] loading normal data from: {args.normal_root}")

    stdzr = compute_sensor_stats_from_normal(Path(args.normal_root))
    mean = torch.tensor(stdzr.mean, dtype=torch.float32, device=device)
    std = torch.tensor(stdzr.std, dtype=torch.float32, device=device)
    base_ds = NormalPredictorDataset(normal_root=args.normal_root, steps_per_epoch=1, seed=args.seed,
                                     standardizer=stdzr)
    sensor_ids = base_ds.get_sensor_node_ids()
    train_ids, val_ids, test_ids = split_ids(base_ds.scene_ids, args.seed, ratios=(0.8, 0.1, 0.1))
    print(f"{now()} [predictor] scenes: total={len(base_ds.scene_ids)} train={len(train_ids)} "
          f"val={len(val_ids)} test={len(test_ids)}")

    def mk(steps, seed, ids):
        ds = NormalPredictorDataset(normal_root=args.normal_root, l_in_steps=36, horizon_steps=1,
                                    steps_per_epoch=steps, seed=seed, sensor_ids=sensor_ids, standardizer=stdzr,
                                    cache_size=1024)
        ds.scene_ids = ids
        return make_loader(ds, args.batch_size, device, args.loader, args.num_workers)

    train_loader = mk(args.steps_per_epoch, args.seed, train_ids)
    val_loader = mk(args.val_steps, args.seed + 1, val_ids)
    test_loader = mk(args.test_steps, args.seed + 2, test_ids)

    S = len(sensor_ids)
    model = (NormalPredictorTCN(num_sensors=S, time_dim=9) if args.arch == "tcn"
             else NormalPredictorGRU(num_sensors=S, time_dim=9)).to(device)
    clip = args.grad_clip if args.grad_clip and args.grad_clip > 0 else None
    if fused_step:
        from .optim import ClipAdamW
        opt = ClipAdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_norm=clip)
        feat_loss = head_loss_fn(model)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
        loss_fn = nn.MSELoss()
    cstep = None  # CapturedPredictorStep, built at the first full-size batch
    best_rmse = float("inf")
    best_path, last_path = out_dir / "predictor_best.ckpt", out_dir / "predictor_last.ckpt"
    meta = {"arch": args.arch, "num_sensors": S, "time_dim": 9, "l_in_steps": 36, "horizon_steps": 1,
            "sensor_ids": sensor_ids, "standardizer": {"mean": stdzr.mean.tolist(), "std": stdzr.std.tolist()},
            "split": {"train_ids": train_ids, "val_ids": val_ids, "test_ids": test_ids}}
    (out_dir / "predictor_meta.json").write_text(json.dumps(meta, indent=2, ensure_ascii=False), encoding="utf-8")

    print(f"{now()} [predictor] start training: epochs={args.epochs}, steps/epoch={args.steps_per_epoch}, "
          f"batch={args.batch_size}")
    from .profiling import StepProfiler
    prof = StepProfiler(out_dir, "predictor", args.profile, device)
    for epoch in range(1, args.epochs + 1):
        model.train()
        running = torch.zeros((), dtype=torch.float64, device=device)
        seen = 0
        for it, batch in enumerate(train_loader, start=1):
            x, x_time = batch["x"].to(device), batch["x_time"].to(device)
            y = batch["y"].to(device)[:, 0, :]
            if use_graph and x.size(0) == args.batch_size:
                # full-size batch: the whole step (features, head + MSE, backward, clip + AdamW) as
                # one graph replay on static inputs; the same arithmetic as the eager branch below
                if cstep is None:
                    cstep = CapturedPredictorStep(model, opt, x, x_time, y)
                    loss = cstep()
                else:
                    loss = cstep(x, x_time, y)
            elif fused_step:
                loss = feat_loss(model.features(x, x_time), y)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            else:
                loss = loss_fn(model(x, x_time), y)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                if clip is not None:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
                opt.step()
            running += loss.detach().double() * x.size(0)
            seen += x.size(0)
            prof.step()
            if (it % args.log_every) == 0:
                print(f"{now()} [predictor][epoch {epoch:02d}] step {it:05d}/{len(train_loader):05d} "
                      f"loss={running.item() / max(seen, 1):.6f}")
        train_loss = running.item() / max(seen, 1)
        if fused_step:
            check_optimizer_errors(opt)
        val_metrics = evaluate_predictor(model, val_loader, device, mean, std)
        print(f"{now()} [predictor][epoch {epoch:02d}] done. train_loss={train_loss:.6f} "
              f"val_mae={val_metrics['mae']:.4f} val_rmse={val_metrics['rmse']:.4f}")
        ckpt = {"epoch": epoch, "arch": args.arch, "model_state": model.state_dict(),
                "standardizer_mean": [float(v) for v in stdzr.mean],
                "standardizer_std": [float(v) for v in stdzr.std],
                "sensor_ids": sensor_ids, "args": vars(args)}
        torch.save(ckpt, last_path)
        if val_metrics["rmse"] < best_rmse:
            best_rmse = val_metrics["rmse"]
            torch.save(ckpt, best_path)
            print(f"{now()} [predictor] new best: rmse={best_rmse:.4f} -> {best_path.name}")

    prof.close()
    best_ckpt = torch.load(best_path, map_location=device, weights_only=True)
    model.load_state_dict(best_ckpt["model_state"])
    test_metrics = evaluate_predictor(model, test_loader, device, mean, std)
    print(f"{now()} [predictor] TEST: mae={test_metrics['mae']:.4f} rmse={test_metrics['rmse']:.4f}")
    print(f"{now()} [predictor] saved: {best_path.name}, {last_path.name}, meta.json")


if __name__ == "__main__":
    main()
