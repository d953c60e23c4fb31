"""The training loss, nn.CrossEntropyLoss() (reference train_detector.py:235, 311), as a
registered op on one HIP launch each way (csrc/loss.hip: lg_cross_entropy_fwd / _bwd).

torch's cross_entropy is six launches per step here (log_softmax, nll forward, two fills,
nll backward, log_softmax backward).  `CrossEntropyLoss` is a drop-in for the reference's
default-constructed module — mean reduction, ignore_index -100, no class weights, no label
smoothing, (B, C) fp32 logits with int64 targets on the GPU.  Class weights, label smoothing
(torch's uniform one, or a (C, C) table such as `distance_smoothing`'s) and the sum / none
reductions run on a second op pair, leakgnn::cross_entropy_opt (lg_cross_entropy_opt_fwd / _bwd),
one launch each way as well; bf16 logits, probability targets, other ranks and CPU tensors are
handed to torch's own implementation unchanged.  `loss_from_args` builds the module from the
training CLI's flags.

The predictor's loss, nn.MSELoss() over head = nn.Linear(H, S) of the last hidden state
(reference train_predictor.py), is `head_mse_loss`: leakgnn::head_mse, one launch forward
(csrc/head_mse.hip: lg_head_mse_fwd) and one kernel plus the slab reduction backward
(lg_head_mse_bwd), in place of torch's eight or so; CPU tensors, other dtypes and shapes outside
the kernels' range go to F.mse_loss(F.linear(...)).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ._native import check, load_library, ptr, stream_of

NS = "leakgnn"
_POOL_SLOTS = 256
_POOLS: dict = {}   # device -> int32 [_POOL_SLOTS] of completion counters, zeros at rest
_SLOTS: dict = {}   # (device, stream handle) -> index into the device's pool


def _counter(dev: torch.device, stream: int) -> Tensor:
    """lg_cross_entropy_fwd's completion counter for launches on `stream` (include/leakgnn.h:
    one per stream that may run the loss concurrently; the launch leaves it at 0).  Counters are
    slots of one per-device pool allocated (zeroed) on the first call, so a stream first seen
    while a HIP graph is being captured takes a slot without a captured fill; the graph keeps
    that slot's address for every replay (a shared per-device counter let an eager
    loss on one stream and a replayed step on another interleave their tickets)."""
    key = (dev, stream)
    i = _SLOTS.get(key)
    pool = _POOLS.get(dev)
    if pool is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("leakgnn cross_entropy: run the loss once eagerly before capturing it "
                               "(its counter pool is allocated on the first call)")
        pool = _POOLS[dev] = torch.zeros(_POOL_SLOTS, dtype=torch.int32, device=dev)
    if i is None:
        i = len([k for k in _SLOTS if k[0] == dev])
        if i >= _POOL_SLOTS:
            raise RuntimeError(f"leakgnn cross_entropy: more than {_POOL_SLOTS} streams on {dev}")
        _SLOTS[key] = i
    return pool[i:i + 1]


@torch.library.custom_op(f"{NS}::cross_entropy", mutates_args=(), device_types="cuda")
def cross_entropy(logits: Tensor, target: Tensor, ignore_index: int) -> Tuple[Tensor, Tensor]:
    """(mean loss, per-row logsumexp).  The row losses are summed in row order by the last
    workgroup to finish (deterministic)."""
    lib = load_library()
    x, t = logits.contiguous(), target.contiguous()
    B, C = x.shape
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    lse = torch.empty(B, device=x.device, dtype=torch.float32)
    rowloss = torch.empty(B, device=x.device, dtype=torch.float32)
    st = stream_of(x)
    check(lib.lg_cross_entropy_fwd(ptr(x), ptr(t), B, C, C, ignore_index, ptr(loss), ptr(lse), ptr(rowloss),
                                   ptr(_counter(x.device, st)), st), "lg_cross_entropy_fwd")
    return loss, lse


@cross_entropy.register_fake
def _(logits, target, ignore_index):
    return logits.new_empty(()), logits.new_empty(logits.shape[0])


@torch.library.custom_op(f"{NS}::cross_entropy_backward", mutates_args=(), device_types="cuda")
def cross_entropy_backward(grad: Tensor, logits: Tensor, target: Tensor, lse: Tensor, ignore_index: int) -> Tensor:
    lib = load_library()
    x, t, g = logits.contiguous(), target.contiguous(), grad.contiguous().float()
    B, C = x.shape
    dx = torch.empty_like(x)
    check(lib.lg_cross_entropy_bwd(ptr(x), ptr(t), ptr(lse), ptr(g), B, C, C, ignore_index, ptr(dx), C,
                                   stream_of(x)), "lg_cross_entropy_bwd")
    return dx


@cross_entropy_backward.register_fake
def _(grad, logits, target, lse, ignore_index):
    return torch.empty_like(logits)


def _ce_setup(ctx, inputs, output):
    logits, target, ignore_index = inputs
    ctx.ignore_index = ignore_index
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(logits, target, output[1])


def _ce_bwd(ctx, g, _glse):
    if g is None:
        return None, None, None
    logits, target, lse = ctx.saved_tensors
    return torch.ops.leakgnn.cross_entropy_backward(g, logits, target, lse, ctx.ignore_index), None, None


cross_entropy.register_autograd(_ce_bwd, setup_context=_ce_setup)


# ---------------------------------------------------------------------------- the options
_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


def _table(smoothing: Optional[Tensor]) -> Tuple[Optional[Tensor], int]:
    """The table as lg_cross_entropy_opt_* take it: unit column stride, and its row stride."""
    if smoothing is None:
        return None, 0
    u = smoothing if smoothing.stride(1) == 1 else smoothing.contiguous()
    return u, u.stride(0)


@torch.library.custom_op(f"{NS}::cross_entropy_opt", mutates_args=(), device_types="cuda")
def cross_entropy_opt(logits: Tensor, target: Tensor, weight: Optional[Tensor], smoothing: Optional[Tensor],
                      ignore_index: int, eps: float, reduction: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(loss, lse, rowsum, denom) of lg_cross_entropy_opt_fwd (include/leakgnn.h has the formula):
    class weights (C,), label smoothing eps over the (C, C) table `smoothing` (None: uniform),
    reduction 0 mean / 1 sum (loss a scalar) / 2 none (loss (B,)).  One launch; deterministic."""
    lib = load_library()
    x, t = logits.contiguous(), target.contiguous()
    w = None if weight is None else weight.contiguous()
    u, ldu = _table(smoothing)
    B, C = x.shape
    if (w is not None and tuple(w.shape) != (C,)) or (u is not None and tuple(u.shape) != (C, C)):
        raise ValueError(f"cross_entropy_opt: weight {None if w is None else tuple(w.shape)} / smoothing "
                         f"{None if u is None else tuple(u.shape)} do not fit {C} classes")
    lse = torch.empty(B, device=x.device, dtype=torch.float32)
    rowloss = torch.empty(B, device=x.device, dtype=torch.float32)
    rowsum = torch.empty(B, device=x.device, dtype=torch.float32)
    denom = torch.empty((), device=x.device, dtype=torch.float32)
    loss = rowloss if reduction == 2 else torch.empty((), device=x.device, dtype=torch.float32)
    st = stream_of(x)
    check(lib.lg_cross_entropy_opt_fwd(ptr(x), ptr(t), B, C, C, ignore_index, ptr(w), ptr(u), ldu, eps, reduction,
                                       ptr(loss), ptr(lse), ptr(rowloss), ptr(rowsum), ptr(denom),
                                       ptr(_counter(x.device, st)), st), "lg_cross_entropy_opt_fwd")
    return loss, lse, rowsum, denom


@cross_entropy_opt.register_fake
def _(logits, target, weight, smoothing, ignore_index, eps, reduction):
    B = logits.shape[0]
    return (logits.new_empty((B,) if reduction == 2 else ()), logits.new_empty(B), logits.new_empty(B),
            logits.new_empty(()))


@torch.library.custom_op(f"{NS}::cross_entropy_opt_backward", mutates_args=(), device_types="cuda")
def cross_entropy_opt_backward(grad: Tensor, logits: Tensor, target: Tensor, lse: Tensor, rowsum: Tensor,
                               denom: Tensor, weight: Optional[Tensor], smoothing: Optional[Tensor],
                               ignore_index: int, eps: float, reduction: int) -> Tensor:
    """dlogits for the upstream gradient `grad`: a scalar (mean, sum) or (B,) (none).  One launch."""
    lib = load_library()
    x, t, g = logits.contiguous(), target.contiguous(), grad.contiguous().float()
    w = None if weight is None else weight.contiguous()
    u, ldu = _table(smoothing)
    B, C = x.shape
    if g.numel() != (B if reduction == 2 else 1):
        raise ValueError(f"cross_entropy_opt_backward: grad has {g.numel()} elements for reduction {reduction}, B = {B}")
    dx = torch.empty_like(x)
    check(lib.lg_cross_entropy_opt_bwd(ptr(x), ptr(t), ptr(lse), ptr(rowsum), ptr(denom), ptr(g), B, C, C,
                                       ignore_index, ptr(w), ptr(u), ldu, eps, reduction, ptr(dx), C, stream_of(x)),
          "lg_cross_entropy_opt_bwd")
    return dx


@cross_entropy_opt_backward.register_fake
def _(grad, logits, target, lse, rowsum, denom, weight, smoothing, ignore_index, eps, reduction):
    return torch.empty_like(logits)


def _ceo_setup(ctx, inputs, output):
    logits, target, weight, smoothing, ctx.ignore_index, ctx.eps, ctx.reduction = inputs
    ctx.mark_non_differentiable(*output[1:])
    ctx.set_materialize_grads(False)
    ctx.has = (weight is not None, smoothing is not None)
    ctx.save_for_backward(logits, target, *output[1:], *[t for t in (weight, smoothing) if t is not None])


def _ceo_bwd(ctx, g, *_unused):
    if g is None:
        return (None,) * 7
    logits, target, lse, rowsum, denom, *rest = ctx.saved_tensors
    weight = rest.pop(0) if ctx.has[0] else None
    smoothing = rest.pop(0) if ctx.has[1] else None
    dx = torch.ops.leakgnn.cross_entropy_opt_backward(g, logits, target, lse, rowsum, denom, weight, smoothing,
                                                      ctx.ignore_index, ctx.eps, ctx.reduction)
    return (dx,) + (None,) * 6  # no gradient to weight or smoothing


cross_entropy_opt.register_autograd(_ceo_bwd, setup_context=_ceo_setup)


def _check_smoothing(smoothing: Tensor, weight: Optional[Tensor], label_smoothing: float) -> Tensor:
    """Host-side validation of a smoothing table, once at construction: (C, C), finite,
    non-negative, rows summing to 1 within 1e-5, C that of `weight`; fp32 on return."""
    if not torch.is_tensor(smoothing) or smoothing.dim() != 2 or smoothing.shape[0] != smoothing.shape[1]:
        raise ValueError(f"smoothing must be a (C, C) tensor, got "
                         f"{tuple(smoothing.shape) if torch.is_tensor(smoothing) else type(smoothing).__name__}")
    if not label_smoothing > 0.0:
        raise ValueError("smoothing needs label_smoothing > 0 (the table spreads the label_smoothing mass)")
    if weight is not None and tuple(weight.shape) != (smoothing.shape[0],):
        raise ValueError(f"weight {tuple(weight.shape)} and smoothing {tuple(smoothing.shape)} disagree on the "
                         f"number of classes")
    u = smoothing.detach().double().cpu()
    if not torch.isfinite(u).all():
        raise ValueError("smoothing has non-finite entries")
    if (u < 0).any():
        raise ValueError("smoothing has negative entries")
    dev = (u.sum(dim=1) - 1.0).abs().max().item() if u.numel() else 0.0
    if dev > 1e-5:
        raise ValueError(f"smoothing rows must sum to 1 within 1e-5 (worst row is off by {dev:.3e})")
    return smoothing.detach().to(torch.float32)


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss on the fused HIP ops for (B, C) fp32 GPU logits with (B,) int64 targets:
    the default configuration on leakgnn::cross_entropy, class weights, label smoothing and the
    sum / none reductions on leakgnn::cross_entropy_opt.  `smoothing`: a (C, C) table whose row y
    is the distribution the label_smoothing mass of a row labelled y is spread over (None: torch's
    uniform 1 / C; `distance_smoothing` builds one from pipe distances); it has no torch route.
    bf16 logits, probability targets, other ranks and CPU tensors go to torch."""

    def __init__(self, weight: Optional[Tensor] = None, size_average=None, ignore_index: int = -100, reduce=None,
                 reduction: str = "mean", label_smoothing: float = 0.0, *,
                 smoothing: Optional[Tensor] = None) -> None:
        super().__init__(weight, size_average, ignore_index, reduce, reduction, label_smoothing)
        if smoothing is not None:
            smoothing = _check_smoothing(smoothing, self.weight, float(label_smoothing))
        self.register_buffer("smoothing", smoothing, persistent=False)

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        if (input.is_cuda and input.dim() == 2 and input.dtype == torch.float32 and target.dtype == torch.int64
                and target.dim() == 1 and self.reduction in _REDUCTIONS and 0.0 <= self.label_smoothing < 1.0
                and (self.weight is None or (self.weight.dtype == torch.float32
                                             and self.weight.device == input.device))):
            if (self.weight is None and self.reduction == "mean" and self.label_smoothing == 0.0
                    and self.smoothing is None):
                return torch.ops.leakgnn.cross_entropy(input, target, int(self.ignore_index))[0]
            if self.smoothing is not None and self.smoothing.device != input.device:
                raise RuntimeError(f"CrossEntropyLoss: smoothing is on {self.smoothing.device}, the logits on "
                                   f"{input.device}; move the module with .to(device)")
            return torch.ops.leakgnn.cross_entropy_opt(input, target, self.weight, self.smoothing,
                                                       int(self.ignore_index), float(self.label_smoothing),
                                                       _REDUCTIONS[self.reduction])[0]
        if self.smoothing is not None:
            raise NotImplementedError("CrossEntropyLoss: a smoothing table runs only on the HIP op ((B, C) fp32 GPU "
                                      "logits, (B,) int64 targets); torch's cross_entropy has no such option")
        return super().forward(input, target)


def distance_smoothing(dist, sigma_m: float, num_classes: int) -> Tensor:
    """The smoothing table that follows the pipe distances the evaluator scores by (dist: the (P, P)
    matrix of window_evaluator.PipeDistanceOracle.ensure_pipe_matrix(), metres; num_classes = P + 1,
    the last class no-leak).  Pipe row y: U[y, c] = exp(-dist[y, c] / sigma_m) / Z_y over the pipe
    classes (an infinite distance gives 0), 0 in the no-leak column; the no-leak row is one-hot on
    itself.  Computed in numpy float64; returns a CPU float32 (C, C) tensor."""
    import numpy as np
    if not sigma_m > 0:
        raise ValueError(f"distance_smoothing: sigma_m must be > 0, got {sigma_m}")
    d = np.asarray(dist, dtype=np.float64)
    P = int(num_classes) - 1
    if d.shape != (P, P):
        raise ValueError(f"distance_smoothing: dist {d.shape} does not fit {num_classes} classes (P = {P} pipes)")
    if np.isnan(d).any() or (d < 0).any():
        raise ValueError("distance_smoothing: distances must be >= 0 (inf for unreachable pairs)")
    u = np.zeros((P + 1, P + 1), dtype=np.float64)
    if P:
        e = np.exp(-d / float(sigma_m))  # exp(-inf) = 0; the diagonal (distance 0) keeps Z_y >= 1
        z = e.sum(axis=1, keepdims=True)
        if not (z > 0).all():
            raise ValueError("distance_smoothing: a pipe row has no reachable class (its own distance must be 0)")
        u[:P, :P] = e / z
    u[P, P] = 1.0
    return torch.from_numpy(u.astype(np.float32))


def loss_from_args(args, inp_path, pipe_ids_in_order) -> CrossEntropyLoss:
    """The loss of the training CLI from its flags (`args`: the namespace, its vars(), or a
    checkpoint's ckpt["args"]; a missing key is the default): "label_smoothing" eps, "smooth_sigma_m"
    (> 0: the eps mass follows distance_smoothing of the network's pipe distances; 0: uniform) and
    "noleak_weight" (the weight of class P, pipes keep 1).  All defaults: CrossEntropyLoss()."""
    a = args if isinstance(args, dict) else vars(args)
    eps = float(a.get("label_smoothing") or 0.0)
    sigma = float(a.get("smooth_sigma_m") or 0.0)
    w_nl = float(1.0 if a.get("noleak_weight") is None else a.get("noleak_weight"))
    C = len(pipe_ids_in_order) + 1
    if sigma < 0 or (sigma > 0 and not eps > 0):
        raise ValueError("--smooth_sigma_m must be >= 0 and needs --label_smoothing > 0")
    weight = None
    if w_nl != 1.0:
        if not w_nl >= 0:
            raise ValueError(f"--noleak_weight must be >= 0, got {w_nl}")
        weight = torch.ones(C, dtype=torch.float32)
        weight[C - 1] = w_nl
    table = None
    if sigma > 0:
        from .window_evaluator import PipeDistanceOracle
        oracle = PipeDistanceOracle.build(inp_path, pipe_ids_in_order)
        oracle.ensure_pipe_matrix()
        table = distance_smoothing(oracle.pipe_dist, sigma, C)
    return CrossEntropyLoss(weight=weight, label_smoothing=eps, smoothing=table)


def check_loss_args(args, world: int, device: torch.device) -> None:
    """Start-up refusals of the loss flags: a no-leak weight under data parallel (the per-rank
    rescale n_local * world / n_glob assumes an unweighted mean), a distance table on the CPU."""
    a = args if isinstance(args, dict) else vars(args)
    w_nl = 1.0 if a.get("noleak_weight") is None else float(a.get("noleak_weight"))
    if world > 1 and w_nl != 1.0:
        raise ValueError("--noleak_weight != 1 is not supported with data parallel (world > 1): the per-rank "
                         "loss rescale assumes an unweighted mean")
    if torch.device(device).type != "cuda" and float(a.get("smooth_sigma_m") or 0.0) > 0:
        raise ValueError("--smooth_sigma_m > 0 needs the GPU path (--device cuda): the distance smoothing table "
                         "has no torch route")


# ============================================================================ head + MSE
HEAD_MSE_MAX_DIM = 1024  # lg_head_mse_fwd: 1 <= H, S <= 1024, B * max(H, S) * 4 < 2 GiB


@torch.library.custom_op(f"{NS}::head_mse", mutates_args=(), device_types="cuda")
def head_mse(h: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    """(loss, y_hat): y_hat = h weight^T + bias (B, S), loss = mean((y_hat - target)^2).  The row
    sums are added in row order by the last workgroup to finish (deterministic)."""
    lib = load_library()
    h, w, b, y = h.contiguous(), weight.contiguous(), bias.contiguous(), target.contiguous()
    B, H = h.shape
    S = w.shape[0]
    if tuple(w.shape) != (S, H) or tuple(b.shape) != (S,) or tuple(y.shape) != (B, S):
        raise ValueError(f"head_mse: h {tuple(h.shape)}, weight {tuple(w.shape)}, bias {tuple(b.shape)}, "
                         f"target {tuple(y.shape)} do not fit (B, H), (S, H), (S,), (B, S)")
    loss = torch.empty((), device=h.device, dtype=torch.float32)
    y_hat = torch.empty(B, S, device=h.device, dtype=torch.float32)
    rowsq = torch.empty(B, device=h.device, dtype=torch.float32)
    st = stream_of(h)
    check(lib.lg_head_mse_fwd(ptr(h), ptr(w), ptr(b), ptr(y), B, H, S, ptr(y_hat), ptr(rowsq), ptr(loss),
                              ptr(_counter(h.device, st)), st), "lg_head_mse_fwd")
    return loss, y_hat


@head_mse.register_fake
def _(h, weight, bias, target):
    return h.new_empty(()), h.new_empty(h.shape[0], weight.shape[0])


@torch.library.custom_op(f"{NS}::head_mse_backward", mutates_args=(), device_types="cuda")
def head_mse_backward(grad: Tensor, h: Tensor, weight: Tensor, target: Tensor,
                      y_hat: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(dh, dweight, dbias) for the upstream scalar gradient `grad`; all three overwritten."""
    lib = load_library()
    h, w, y, g = h.contiguous(), weight.contiguous(), target.contiguous(), grad.contiguous().float()
    B, H = h.shape
    S = w.shape[0]
    dh, dw = torch.empty_like(h), torch.empty_like(w)
    db = torch.empty(S, device=h.device, dtype=torch.float32)
    ws = torch.empty(int(lib.lg_head_mse_bwd_workspace_bytes(B, H, S)), device=h.device, dtype=torch.uint8)
    check(lib.lg_head_mse_bwd(ptr(h), ptr(w), ptr(y), ptr(y_hat), ptr(g), B, H, S, ptr(dh), ptr(dw), ptr(db), ptr(ws),
                              ws.numel(), stream_of(h)), "lg_head_mse_bwd")
    return dh, dw, db


@head_mse_backward.register_fake
def _(grad, h, weight, target, y_hat):
    return torch.empty_like(h), torch.empty_like(weight), weight.new_empty(weight.shape[0])


def _hm_setup(ctx, inputs, output):
    h, weight, _, target = inputs
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(h, weight, target, output[1])


def _hm_bwd(ctx, g, _gy):
    if g is None:
        return None, None, None, None
    h, weight, target, y_hat = ctx.saved_tensors
    dh, dw, db = torch.ops.leakgnn.head_mse_backward(g, h, weight, target, y_hat)
    return dh, dw, db, None


head_mse.register_autograd(_hm_bwd, setup_context=_hm_setup)


def head_mse_supported(h: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> bool:
    """Whether leakgnn::head_mse takes these tensors: fp32 on the GPU, h (B, H), weight (S, H), bias
    (S,), target (B, S), within lg_head_mse_fwd's range."""
    ts = (h, weight, bias, target)
    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts) or h.dim() != 2 or weight.dim() != 2:
        return False
    (B, H), S = h.shape, weight.shape[0]
    return (tuple(weight.shape) == (S, H) and tuple(bias.shape) == (S,) and tuple(target.shape) == (B, S)
            and B >= 1 and 1 <= H <= HEAD_MSE_MAX_DIM and 1 <= S <= HEAD_MSE_MAX_DIM
            and B * max(H, S) * 4 < 2 ** 31)


def head_mse_loss(h: Tensor, weight: Tensor, bias: Tensor, target: Tensor) -> Tensor:
    """F.mse_loss(F.linear(h, weight, bias), target): the fused HIP op for fp32 GPU tensors in its
    range, torch's own ops for everything else (CPU tensors, other dtypes or shapes)."""
    if head_mse_supported(h, weight, bias, target):
        return torch.ops.leakgnn.head_mse(h, weight, bias, target)[0]
    return F.mse_loss(F.linear(h, weight, bias), target)
