"""The training loss, nn.CrossEntropyLoss() (reference train_detector.py:235, 311), as a
registered op on one HIP launch each way (csrc/loss.hip: lg_cross_entropy_fwd / _bwd).

torch's cross_entropy is six launches per step here (log_softmax, nll forward, two fills,
nll backward, log_softmax backward).  `CrossEntropyLoss` is a drop-in for the reference's
default-constructed module — mean reduction, ignore_index -100, no class weights, no label
smoothing, (B, C) fp32 logits with int64 targets on the GPU; anything else is handed to
torch's own implementation unchanged.

The predictor's loss, nn.MSELoss() over head = nn.Linear(H, S) of the last hidden state
(reference train_predictor.py), is `head_mse_loss`: leakgnn::head_mse, one launch forward
(csrc/head_mse.hip: lg_head_mse_fwd) and one kernel plus the slab reduction backward
(lg_head_mse_bwd), in place of torch's eight or so; CPU tensors, other dtypes and shapes outside
the kernels' range go to F.mse_loss(F.linear(...)).
"""
from __future__ import annotations

from typing import Tuple

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


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss with the default configuration on the fused HIP op; any other
    configuration or input falls through to torch."""

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        if (self.weight is None and self.reduction == "mean" and self.label_smoothing == 0.0 and input.is_cuda
                and input.dim() == 2 and input.dtype == torch.float32 and target.dtype == torch.int64
                and target.dim() == 1):
            return torch.ops.leakgnn.cross_entropy(input, target, int(self.ignore_index))[0]
        return super().forward(input, target)


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
