"""torch.library registration of the libleakgnn operators (namespace ``leakgnn``).

SURVEY §8(b): the hot path sits behind registered PyTorch operators whose bodies call
the C ABI (include/leakgnn.h) on torch's current HIP stream, with autograd formulas in
Python, so torch.compile / torch.export / any dispatcher-level caller sees them as
ordinary ops (fake / meta implementations give output shapes without running kernels).

  leakgnn::gcn_conv            PyG GCNConv.forward (detector.py:163,199): Ahat (x W^T) + b
  leakgnn::spmm_cols           the propagate of GCNConv's general path (any width)
  leakgnn::gcn_edge_norm       PyG gcn_norm with edge_weight over a built structure (w, w_t, dis)
  leakgnn::sddmm_cols          dL/dw of a propagate (no autograd of its own)
  sddmm_nm (plain function)    dL/dw of one node-major trunk layer (lg_sddmm_nm)
  leakgnn::mean_pool           PyG global_mean_pool over B equal windows (detector.py:215)
  leakgnn::sensor_proj         sensor_to_node on the sensor rows (detector.py:184-189)
  leakgnn::gru_encoder         SharedSensorGRUEncoder's GRU (detector.py:60-73)
  leakgnn::gru_stack           the same with num_layers > 1 (dense-input upper layers, inter-layer dropout)
  leakgnn::gru_predictor       NormalPredictorGRU's nn.GRU over a dense (B, L, I) input (MFMA layers at H = 128)
  leakgnn::tcn_predictor       NormalPredictorTCN's conv stack over the projected (B, L, 128) input, for training
  leakgnn::diffuse             K-hop personalised-PageRank propagation of a node-major tensor (lg_diffuse_fwd)
  leakgnn::gnn_trunk           node init + L x [GCNConv, ReLU, Dropout] (detector.py:178-201); skip=True: identity skips;
                               hops > 0: leakgnn::diffuse's stage between the node init and layer 0
  leakgnn::gnn_trunk_norm      the same with a LayerNorm before every residual branch and before the heads
  leakgnn::encoder_trunk       gru_encoder + gnn_trunk as one op (node-major, compressed node init)
  leakgnn::detector_heads      pipe gather + EdgeHead + mean pool + NoLeakHead
                               (detector.py:76-102, 206-218)
  leakgnn::window_metrics      DetectorEvaluator.evaluate's per-batch tail (window_evaluator.py:227-483); no autograd
  leakgnn::event_decide        the event evaluator's trigger + aggregation (event_evaluator.py:327-342); no autograd
and one ``*_backward`` op per differentiable op (registered autograd formulas call them).

Every op takes plain tensors (the graph CSR and its node tables are inputs, not Python
objects) and fp32 CUDA tensors; there is no CPU kernel, so a CPU call raises.  Dropout
seeds are a 1-element int64 tensor: a CPU tensor's value, or - under HIP-graph capture -
a device tensor whose ADDRESS the kernels read at launch (LG_SALT_SEED_PTR), so replays
draw fresh masks.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import functools
import inspect

from collections import OrderedDict, namedtuple
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _native as nat
from ._native import check, load_library, ptr, stream_of
from .ops import (EDGE_HEAD_SALT, GCN_BWD_NM_EXTRA_FLAGS, GCN_FWD_DENSE_EXTRA_FLAGS, GCN_FWD_NM_EXTRA_FLAGS,
                  GRU_PRED_SALT, GRU_STACK_SALT, NM_MAX_BYTES, NOLEAK_HEAD_SALT, TCN_SALT, WINDOW_COUNTERS,
                  WINDOW_MAX_LIST, _check_d, _timed)

NS = "leakgnn"


def _seed_args(seed: Tensor) -> Tuple[int, int]:
    """(seed value or device address, salt bits) of a dropout seed tensor."""
    if seed.is_cuda:
        return seed.data_ptr(), nat.LG_SALT_SEED_PTR
    return int(seed.item()), 0


def _req(*ts: Optional[Tensor]) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("leakgnn ops run only on a ROCm GPU (tensor on %s); there is no CPU path" % t.device)
        if t.is_floating_point() and t.dtype != torch.float32:
            raise TypeError(f"leakgnn ops compute in fp32, got {t.dtype} (cast the inputs with .float())")


def _c(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.contiguous()


# ============================================================================ gcn_conv
# GCNConv's single-graph kernels at D = 64: True (default) = the node-table row tiles
# lg_gcn_{fwd,bwd}_rows (split-bf16 MFMA, fp32-level accuracy; at C5 17.7 / 40.4 us against
# 26.7 / 50.5 us, profiles/r03/r03ac), False = window-major lg_gcn_fwd / lg_gcn_bwd (exact
# fp32 MFMA, and the D = 32 path)
_ROWS = True


def _use_rows(Ntot: int, D: int) -> bool:
    """The row-tile kernels take the graph only when its node-major activation fits one launch's
    32-bit buffer offsets (N * D * 4 <= ops.NM_MAX_BYTES, ~8.4M nodes at D = 64); larger graphs
    go to lg_gcn_fwd / lg_gcn_bwd (window-major, up to kLgMaxRows rows)."""
    return D == 64 and _ROWS and Ntot * D * 4 <= NM_MAX_BYTES

@torch.library.custom_op(f"{NS}::gcn_conv", mutates_args=(), device_types="cuda")
def gcn_conv(x: Tensor, weight: Tensor, bias: Optional[Tensor], rowptr: Tensor, col: Tensor, w: Tensor,
             rowptr_t: Tensor, col_t: Tensor, w_t: Tensor, nodetab: Tensor, pairs: Tensor, nodetab_t: Tensor,
             pairs_t: Tensor) -> Tensor:
    """y = Ahat (x W^T) + b on one graph: lg_gcn_fwd_rows (D = 64: 16-node tiles off the node
    table nodetab / pairs of GCNGraph) or lg_gcn_fwd (D = 32, or `_ROWS = False`: exact fp32
    MFMA over the gcn_norm'ed CSR rowptr / col / w of lg_graph_build)."""
    lib = load_library()
    x, weight, bias = _c(x), _c(weight), _c(bias)
    _req(x, weight, bias)
    Ntot, D = x.shape
    _check_d(D)
    if weight.shape != (D, D):
        raise NotImplementedError("GCNConv kernels need in_channels == out_channels")
    y = torch.empty_like(x)
    flags = nat.LG_F_BIAS if bias is not None else 0
    with _timed("gcn_fwd", x.device):
        if _use_rows(Ntot, D):
            check(lib.lg_gcn_fwd_rows(ptr(nodetab), ptr(pairs), ptr(x), ptr(weight), ptr(bias), ptr(y), Ntot, D, flags,
                                      stream_of(x)), "lg_gcn_fwd_rows")
        else:
            check(lib.lg_gcn_fwd(ptr(rowptr), ptr(col), ptr(w), ptr(x), ptr(weight), ptr(bias), ptr(y), 1, Ntot, D,
                                 col.numel(), flags, 0.0, 0, 0, stream_of(x)), "lg_gcn_fwd")
    return y


@gcn_conv.register_fake
def _(x, weight, bias, rowptr, col, w, rowptr_t, col_t, w_t, nodetab, pairs, nodetab_t, pairs_t):
    return torch.empty_like(x)


@torch.library.custom_op(f"{NS}::gcn_conv_backward", mutates_args=(), device_types="cuda")
def gcn_conv_backward(dy: Tensor, x: Tensor, weight: Tensor, rowptr_t: Tensor, col_t: Tensor,
                      w_t: Tensor, nodetab_t: Tensor, pairs_t: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dW, db) of gcn_conv (lg_gcn_bwd over the transposed CSR; lg_gcn_bwd_rows over the
    transposed node table when the row-tile kernels are selected)."""
    lib = load_library()
    dy, x, weight = _c(dy), _c(x), _c(weight)
    _req(dy, x, weight)
    Ntot, D = x.shape
    dx = torch.empty_like(x)
    dW = torch.empty_like(weight)
    db = torch.empty(D, device=x.device, dtype=x.dtype)
    with _timed("gcn_bwd", x.device):
        if _use_rows(Ntot, D):
            ws = torch.empty(int(lib.lg_gcn_bwd_nm_workspace_bytes(D)), device=x.device, dtype=torch.uint8)
            check(lib.lg_gcn_bwd_rows(ptr(nodetab_t), ptr(pairs_t), ptr(dy), ptr(x), ptr(weight), ptr(dx), ptr(dW),
                                      ptr(db), Ntot, D, ptr(ws), ws.numel(), stream_of(x)), "lg_gcn_bwd_rows")
        else:
            ws = torch.empty(int(lib.lg_gcn_bwd_workspace_bytes(D)), device=x.device, dtype=torch.uint8)
            check(lib.lg_gcn_bwd(ptr(rowptr_t), ptr(col_t), ptr(w_t), ptr(dy), None, ptr(x), ptr(weight), ptr(dx),
                                 ptr(dW), ptr(db), None, None, 1, Ntot, D, col_t.numel(), 0, 1.0, 1.0, ptr(ws), ws.numel(),
                                 stream_of(x)), "lg_gcn_bwd")
    return dx, dW, db


@gcn_conv_backward.register_fake
def _(dy, x, weight, rowptr_t, col_t, w_t, nodetab_t, pairs_t):
    return torch.empty_like(x), torch.empty_like(weight), x.new_empty(x.shape[1])


def _gcn_conv_setup(ctx, inputs, output):
    x, weight, bias, rowptr, col, _, rowptr_t, col_t, w_t, _, _, nodetab_t, pairs_t = inputs
    ctx.has_bias = bias is not None
    ctx.w_grad = bool(ctx.needs_input_grad[5])  # w: learned edge weights (leakgnn::gcn_edge_norm)
    ctx.save_for_backward(x, weight, rowptr_t, col_t, w_t, nodetab_t, pairs_t, *((rowptr, col) if ctx.w_grad else ()))


def _gcn_conv_bwd(ctx, dy):
    x, weight, rowptr_t, col_t, w_t, nodetab_t, pairs_t = ctx.saved_tensors[:7]
    dx, dW, db = torch.ops.leakgnn.gcn_conv_backward(dy, x, weight, rowptr_t, col_t, w_t, nodetab_t, pairs_t)
    dw = None
    if ctx.w_grad:  # dL/dw[k] = dy[n] . (x W^T)[col k]: one library GEMM, then the SDDMM over the CSR
        rowptr, col = ctx.saved_tensors[7:]
        with torch.autocast("cuda", enabled=False):
            z = x @ weight.t()
        dw = torch.ops.leakgnn.sddmm_cols(rowptr, col, dy, z)
    return (dx, dW, (db if ctx.has_bias else None), None, None, dw) + (None,) * 7


gcn_conv.register_autograd(_gcn_conv_bwd, setup_context=_gcn_conv_setup)


# ============================================================================ spmm_cols
# GCNConv's general path (models/gcn.py): widths other than the fused kernels' 32 / 64, or
# in_channels != out_channels.  The propagate runs on lg_spmm_cols (any column count, bias
# fused), the transform on a library GEMM.
@torch.library.custom_op(f"{NS}::spmm_cols", mutates_args=(), device_types="cuda")
def spmm_cols(x: Tensor, bias: Optional[Tensor], rowptr: Tensor, col: Tensor, w: Tensor, rowptr_t: Tensor,
              col_t: Tensor, w_t: Tensor) -> Tensor:
    """y = Ahat x (+ bias) for x [N][C], any C (lg_spmm_cols over the gcn_norm'ed CSR)."""
    lib = load_library()
    x, bias = _c(x), _c(bias)
    _req(x, bias)
    N, C = x.shape
    y = torch.empty_like(x)
    with _timed("spmm_cols", x.device):
        check(lib.lg_spmm_cols(ptr(rowptr), ptr(col), ptr(w), ptr(x), C, ptr(bias), ptr(y), C, N, C, stream_of(x)),
              "lg_spmm_cols")
    return y


@spmm_cols.register_fake
def _(x, bias, rowptr, col, w, rowptr_t, col_t, w_t):
    return torch.empty_like(x)


def _spmm_cols_setup(ctx, inputs, output):
    x, bias, rowptr, col, _, rowptr_t, col_t, w_t = inputs
    ctx.has_bias = bias is not None
    ctx.w_grad = bool(ctx.needs_input_grad[4])  # w: learned edge weights (leakgnn::gcn_edge_norm)
    ctx.save_for_backward(rowptr_t, col_t, w_t, *((x, rowptr, col) if ctx.w_grad else ()))


def _spmm_cols_bwd(ctx, dy):
    rowptr_t, col_t, w_t = ctx.saved_tensors[:3]
    # dx = Ahat^T dy: the same propagate over the transposed CSR (its rows are the columns of Ahat)
    dx = torch.ops.leakgnn.spmm_cols(dy, None, rowptr_t, col_t, w_t, rowptr_t, col_t, w_t)
    dw = None
    if ctx.w_grad:  # dL/dw[k] = dy[n] . x[col k]
        x, rowptr, col = ctx.saved_tensors[3:]
        dw = torch.ops.leakgnn.sddmm_cols(rowptr, col, dy, x)
    return dx, (dy.sum(0) if ctx.has_bias else None), None, None, dw, None, None, None


spmm_cols.register_autograd(_spmm_cols_bwd, setup_context=_spmm_cols_setup)


# ============================================================================ edge weights
# PyG GCNConv.forward(x, edge_index, edge_weight): the weighted gcn_norm as a differentiable op
# over the structure of a weighted GCNGraph (ops.GCNGraph.build(..., edge_weight=...)), and the
# sampled dense-dense product the propagates' dL/dw is made of.
@torch.library.custom_op(f"{NS}::sddmm_cols", mutates_args=(), device_types="cuda")
def sddmm_cols(rowptr: Tensor, col: Tensor, a: Tensor, b: Tensor) -> Tensor:
    """out[k] = a[row(k)] . b[col[k]] for every CSR slot k (lg_sddmm_cols); a, b [N][C], any C.
    out has col's length, zero past rowptr[N].  No autograd: it is what the backwards of
    gcn_conv and spmm_cols return as dL/dw."""
    lib = load_library()
    a, b = _c(a), _c(b)
    _req(a, b)
    N, C = a.shape
    if b.shape != a.shape or rowptr.numel() != N + 1:
        raise ValueError(f"sddmm_cols: a {tuple(a.shape)}, b {tuple(b.shape)}, rowptr {tuple(rowptr.shape)}")
    out = torch.zeros(col.numel(), device=a.device, dtype=torch.float32)
    with _timed("sddmm_cols", a.device):
        check(lib.lg_sddmm_cols(ptr(rowptr), ptr(col), ptr(a), C, ptr(b), C, ptr(out), N, C, stream_of(a)),
              "lg_sddmm_cols")
    return out


@sddmm_cols.register_fake
def _(rowptr, col, a, b):
    return a.new_empty(col.shape[0])


def sddmm_nm(rowptr: Tensor, col: Tensor, dy: Tensor, weight: Tensor, x: Tensor, *, y: Optional[Tensor] = None,
             ymask: Optional[Tensor] = None, mask_in: bool = False, scale: float = 1.0,
             ws: Optional[Tensor] = None) -> Tensor:
    """dL/dw of one node-major trunk layer (lg_sddmm_nm): G[k] = sum_b (dz W)[n, b] . x[col k, b] for
    every slot k of row n of the forward CSR, dz = dy * scale * [y > 0] under mask_in (the mask
    from y, or from the bit words ymask of lg_gcn_fwd_nm_bits), else dy.  dy, x, y: (N, B, D).
    G has col's length, zero past rowptr[N].  Deterministic.  ws: the caller's workspace (uint8),
    allocated here when None.  A plain function with no autograd of its own, as sddmm_cols: it is
    what the trunk ops' backward returns as the gradient of edge_w."""
    lib = load_library()
    dy, weight, x, y = _c(dy), _c(weight), _c(x), _c(y)
    _req(dy, weight, x, y)
    N, B, D = dy.shape
    _check_d(D)
    if x.shape != dy.shape or tuple(weight.shape) != (D, D) or rowptr.numel() != N + 1:
        raise ValueError(f"sddmm_nm: dy {tuple(dy.shape)}, x {tuple(x.shape)}, weight {tuple(weight.shape)}, "
                         f"rowptr {tuple(rowptr.shape)}")
    if mask_in and y is None and ymask is None:
        raise ValueError("sddmm_nm: mask_in needs y or ymask")
    cap = col.numel()
    if ws is None:
        ws = torch.empty(int(lib.lg_sddmm_nm_workspace_bytes(B, cap)), device=dy.device, dtype=torch.uint8)
    G = torch.empty(cap, device=dy.device, dtype=torch.float32)
    with _timed("sddmm_nm", dy.device):
        check(lib.lg_sddmm_nm(ptr(rowptr), ptr(col), ptr(dy), ptr(y), ptr(ymask), ptr(weight), ptr(x), ptr(G), B, N, D,
                              cap, nat.LG_F_MASK_IN if mask_in else 0, scale, ptr(ws), ws.numel(), stream_of(dy)),
              "lg_sddmm_nm")
    return G


@torch.library.custom_op(f"{NS}::gcn_edge_norm", mutates_args=(), device_types="cuda")
def gcn_edge_norm(edge_weight: Tensor, rowptr: Tensor, col: Tensor, eid: Tensor, rowptr_t: Tensor, col_t: Tensor,
                  eid_t: Tensor, normalize: bool, fill: float) -> Tuple[Tensor, Tensor, Tensor]:
    """(w, w_t, dis) of PyG's weighted gcn_norm over a built structure (lg_graph_reweight):
    deg summed per row in edge order, dis = deg^-1/2, w = (dis[src] * weight) * dis[dst]; a loop
    slot takes its supplying self-loop edge's weight or `fill` (eid = -1).  Kernel launches
    only.  The gradient flows through w (w_t holds the same numbers in the other order)."""
    lib = load_library()
    edge_weight = _c(edge_weight)
    _req(edge_weight)
    E, N, cap = edge_weight.numel(), rowptr.numel() - 1, col.numel()
    w = torch.zeros(cap, device=col.device, dtype=torch.float32)
    w_t = torch.zeros(cap, device=col.device, dtype=torch.float32)
    dis = torch.empty(N, device=col.device, dtype=torch.float32)
    check(lib.lg_graph_reweight(ptr(rowptr), ptr(col), ptr(eid), ptr(rowptr_t), ptr(col_t), ptr(eid_t),
                                ptr(edge_weight) if E else None, E, N, int(normalize), fill, ptr(dis), ptr(w), ptr(w_t),
                                stream_of(col)), "lg_graph_reweight")
    return w, w_t, dis


@gcn_edge_norm.register_fake
def _(edge_weight, rowptr, col, eid, rowptr_t, col_t, eid_t, normalize, fill):
    return (edge_weight.new_empty(col.shape[0]), edge_weight.new_empty(col.shape[0]),
            edge_weight.new_empty(rowptr.shape[0] - 1))


@torch.library.custom_op(f"{NS}::gcn_edge_norm_backward", mutates_args=(), device_types="cuda")
def gcn_edge_norm_backward(dw: Tensor, edge_weight: Tensor, dis: Tensor, rowptr: Tensor, col: Tensor, eid: Tensor,
                           rowptr_t: Tensor, col_t: Tensor, eid_t: Tensor, normalize: bool, fill: float) -> Tensor:
    """dL/d edge_weight from dw = dL/dw in CSR order (lg_gcn_norm_bwd: deterministic, no float
    atomics)."""
    lib = load_library()
    dw, edge_weight = _c(dw), _c(edge_weight)
    _req(dw, edge_weight, dis)
    E, N = edge_weight.numel(), rowptr.numel() - 1
    dv = torch.empty(E, device=dw.device, dtype=torch.float32)
    ws = torch.empty(int(lib.lg_gcn_norm_bwd_workspace_bytes(E, N)), device=dw.device, dtype=torch.uint8)
    check(lib.lg_gcn_norm_bwd(ptr(dw), ptr(rowptr), ptr(col), ptr(eid), ptr(rowptr_t), ptr(col_t), ptr(eid_t), ptr(dis),
                              ptr(edge_weight) if E else None, E, N, int(normalize), fill, ptr(dv) if E else None,
                              ptr(ws), ws.numel(), stream_of(dw)), "lg_gcn_norm_bwd")
    return dv


@gcn_edge_norm_backward.register_fake
def _(dw, edge_weight, dis, rowptr, col, eid, rowptr_t, col_t, eid_t, normalize, fill):
    return torch.empty_like(edge_weight)


def _edge_norm_setup(ctx, inputs, output):
    edge_weight, rowptr, col, eid, rowptr_t, col_t, eid_t, normalize, fill = inputs
    w, w_t, dis = output
    ctx.mark_non_differentiable(w_t, dis)
    ctx.set_materialize_grads(False)
    ctx.norm = (normalize, fill)
    ctx.save_for_backward(edge_weight, dis, rowptr, col, eid, rowptr_t, col_t, eid_t)


def _edge_norm_bwd(ctx, dw, _dw_t, _ddis):
    if dw is None:
        return (None,) * 9
    dv = torch.ops.leakgnn.gcn_edge_norm_backward(dw, *ctx.saved_tensors, *ctx.norm)
    return (dv,) + (None,) * 8


gcn_edge_norm.register_autograd(_edge_norm_bwd, setup_context=_edge_norm_setup)


# ============================================================================ mean_pool
@torch.library.custom_op(f"{NS}::mean_pool", mutates_args=(), device_types="cuda")
def mean_pool(x: Tensor, B: int, N: int) -> Tensor:
    """global_mean_pool for batch = arange(B).repeat_interleave(N) (lg_mean_pool_fwd)."""
    lib = load_library()
    x = _c(x)
    _req(x)
    D = x.shape[-1]
    _check_d(D)
    out = torch.empty(B, D, device=x.device, dtype=torch.float32)
    check(lib.lg_mean_pool_fwd(ptr(x), ptr(out), B, N, D, stream_of(x)), "lg_mean_pool_fwd")
    return out


@mean_pool.register_fake
def _(x, B, N):
    return x.new_empty(B, x.shape[-1])


def _mean_pool_setup(ctx, inputs, output):
    ctx.BN = (inputs[1], inputs[2])


def _mean_pool_bwd(ctx, dout):
    B, N = ctx.BN
    return (dout / float(N)).unsqueeze(1).expand(B, N, dout.shape[-1]).reshape(B * N, -1), None, None


mean_pool.register_autograd(_mean_pool_bwd, setup_context=_mean_pool_setup)


# ============================================================================ sensor_proj
@torch.library.custom_op(f"{NS}::sensor_proj", mutates_args=(), device_types="cuda")
def sensor_proj(h_s: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """sensor_to_node on the rows that carry a sensor (detector.py:160, 184-189): their
    Linear input is [h_s, 1], so proj = h_s W[:, :Ds]^T + (W[:, Ds] + b), one GEMM."""
    _req(h_s, weight, bias)
    B, S, Ds = h_s.shape
    D = weight.shape[0]
    with torch.autocast("cuda", enabled=False):
        return torch.addmm(weight[:, Ds] + bias, h_s.reshape(B * S, Ds), weight[:, :Ds].t()).view(B, S, D)


@sensor_proj.register_fake
def _(h_s, weight, bias):
    return h_s.new_empty(h_s.shape[0], h_s.shape[1], weight.shape[0])


@torch.library.custom_op(f"{NS}::sensor_proj_backward", mutates_args=(), device_types="cuda")
def sensor_proj_backward(dproj: Tensor, h_s: Tensor, weight: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """dh_s = dproj W[:, :Ds] (GEMM); dW (incl. the mask column) and db in one split-K
    MFMA kernel (lg_linear_dw) instead of a skinny-K (K = B*S) GEMM."""
    lib = load_library()
    dproj, h_s, weight = _c(dproj), _c(h_s), _c(weight)
    _req(dproj, h_s, weight)
    B, S, Ds = h_s.shape
    D = weight.shape[0]
    K = B * S
    d2, h2 = dproj.view(K, D), h_s.view(K, Ds)
    with torch.autocast("cuda", enabled=False):
        dh = (d2 @ weight[:, :Ds]).view(B, S, Ds)
    dW = torch.empty(D, Ds + 1, device=d2.device, dtype=torch.float32)
    db = torch.empty(D, device=d2.device, dtype=torch.float32)
    ws = torch.empty(int(lib.lg_linear_dw_workspace_bytes(K, D, Ds)), device=d2.device, dtype=torch.uint8)
    with _timed("linear_dw", d2.device):
        check(lib.lg_linear_dw(ptr(d2), ptr(h2), K, D, Ds, ptr(dW), ptr(db), ptr(ws), ws.numel(), stream_of(d2)), "lg_linear_dw")
    return dh, dW, db


@sensor_proj_backward.register_fake
def _(dproj, h_s, weight):
    return torch.empty_like(h_s), weight.new_empty(weight.shape), weight.new_empty(weight.shape[0])


def _sensor_proj_setup(ctx, inputs, output):
    h_s, weight, _ = inputs
    ctx.save_for_backward(h_s, weight)


def _sensor_proj_bwd(ctx, dproj):
    h_s, weight = ctx.saved_tensors
    dh, dW, db = torch.ops.leakgnn.sensor_proj_backward(dproj, h_s, weight)
    return (dh if ctx.needs_input_grad[0] else None), dW, db


sensor_proj.register_autograd(_sensor_proj_bwd, setup_context=_sensor_proj_setup)


# ============================================================================ GRU ops: shared drivers
# gru_encoder, gru_stack and gru_predictor are one layer loop (_gru_forward) and one BPTT loop
# (_gru_bptt) over the C entry points.  What differs between the ops is passed in:
#   layer-0 input       enc = (residual, tfeat) read in place (lg_gru_fwd), or a dense time-major xt
#                       through lg_gru_seq_fwd / lg_gru_seq_bwd like every upper layer (gru_predictor)
#   layer-0 backward    under enc, lg_gru_bwd (gru_encoder: own_l0) or lg_gru_seq_bwd's encoder form
#   dropout salts       salt0 + boundary (GRU_STACK_SALT / GRU_PRED_SALT)
#   top h_seq, no save  dropped where the layer can write h_last alone (keep_h False)
#   workspace           each entry's query, plus ws_extra bytes (gru_predictor's one-pass dG at H = 128)
def _split(ts, *lens: int) -> List[List[Tensor]]:
    """A flat tensor sequence cut into consecutive runs of the given lengths (a + b + ... undone)."""
    if sum(lens) != len(ts):
        raise ValueError(f"expected {sum(lens)} tensors in runs of {lens}, got {len(ts)}")
    runs, i = [], 0
    for n in lens:
        runs.append(list(ts[i:i + n]))
        i += n
    return runs


def _gru_dims(op: str, x: Tensor, dense: bool, w_ih: List[Tensor], w_hh: List[Tensor],
              b_ih: Optional[List[Tensor]] = None, b_hh: Optional[List[Tensor]] = None, p: float = 0.0
              ) -> Tuple[int, int, int]:
    """(I, H, layers) of a GRU op's per-layer weight lists, every shape checked.  x is the dense
    (B, L, I) input or, not dense, residual (B, L, S) with I taken from w_ih[0]; the bias lists are
    checked where given (the backward ops take none)."""
    if x.dim() != 3:
        raise ValueError(f"{op}: {'x must be (B, L, I)' if dense else 'residual must be (B, L, S)'}, "
                         f"got {tuple(x.shape)}")
    nl = len(w_hh)
    if nl < 1 or any(ts is not None and len(ts) != nl for ts in (w_ih, b_ih, b_hh)):
        raise ValueError(f"{op}: one (w_ih, w_hh, b_ih, b_hh) per layer")
    if w_hh[0].dim() != 2 or w_ih[0].dim() != 2:
        raise ValueError(f"{op}: w_hh must be (3H, H), got {tuple(w_hh[0].shape)}")
    H = w_hh[0].shape[1]
    I = x.shape[2] if dense else w_ih[0].shape[1]
    if dense and (x.shape[1] < 1 or not (1 <= I <= 1024 and 1 <= H <= 1024)):
        raise ValueError(f"{op}: L >= 1 and I, H in 1..1024, got L {x.shape[1]}, I {I}, H {H}")
    for l in range(nl):
        want = (3 * H, I if l == 0 else H)
        if (tuple(w_ih[l].shape) != want or tuple(w_hh[l].shape) != (3 * H, H)
                or any(b is not None and tuple(b[l].shape) != (3 * H,) for b in (b_ih, b_hh))):
            raise ValueError(f"{op}: layer {l} weights {tuple(w_ih[l].shape)}, {tuple(w_hh[l].shape)}, biases "
                             f"{[tuple(b[l].shape) for b in (b_ih, b_hh) if b is not None]}; expected {want}, "
                             f"{(3 * H, H)}, {(3 * H,)}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{op}: dropout p must be in [0, 1), got {p}")
    return I, H, nl


def _layer_drop(l: int, p: float, seed: Tensor, salt0: int) -> Tuple[int, float, int, int]:
    """(flags, p, seed, salt) of the dropout layer l reads its input through: boundary l - 1 of the
    stack (salt0 + l - 1) for l > 0 and p > 0, none otherwise."""
    if l == 0 or not p > 0.0:
        return 0, 0.0, 0, 0
    seed_v, sbit = _seed_args(seed)
    return nat.LG_F_DROPOUT, p, seed_v, (salt0 + l - 1) | sbit


def _gru_forward(lib, enc: Optional[Tuple[Tensor, Optional[Tensor]]], xt: Optional[Tensor], w_ih: List[Tensor],
                 w_hh: List[Tensor], b_ih: List[Tensor], b_hh: List[Tensor], h_last: Tensor, L: int, I: int, p: float,
                 seed: Optional[Tensor], salt0: int, save: bool, keep_h: bool) -> Tuple[List[Tensor], List[Tensor]]:
    """The layer loop: (h_seqs, gates), one of each per layer, and h_last (Nseq * H elements, any
    shape) filled with the top layer's last step.  Layer 0 reads enc or xt (L, Nseq, I), layer
    l > 0 the h_seq below it through dropout boundary l - 1.  Tensors not produced are empty:
    gates without save, and without save the top layer's h_seq unless keep_h - the top layer
    then writes h_last alone (lg_gru_fwd, or lg_gru_seq_infer on a dense input)."""
    H, nl = w_hh[0].shape[1], len(w_hh)
    nseq = h_last.numel() // H
    dev = h_last.device
    st = stream_of(h_last)
    if enc is not None:
        residual, tfeat = enc
        B, _, S = residual.shape
        if tfeat is not None and tuple(tfeat.shape) != (B, L, 9):
            raise ValueError(f"tfeat must be (B, L, 9), got {tuple(tfeat.shape)}")
    h_seqs: List[Tensor] = []
    gates: List[Tensor] = []
    src = xt
    for l in range(nl):
        top = l == nl - 1
        w = (ptr(w_ih[l]), ptr(w_hh[l]), ptr(b_ih[l]), ptr(b_hh[l]))
        hs = torch.empty(L, nseq, H, device=dev) if (save or keep_h or not top) else None
        g = torch.empty(L, nseq, 4, H, device=dev) if save else None
        if l == 0 and enc is not None:
            with _timed("gru_fwd", dev):
                check(lib.lg_gru_fwd(ptr(residual), ptr(tfeat), *w, ptr(hs), ptr(g), ptr(h_last), B, L, S, I, H, st),
                      "lg_gru_fwd")
        elif hs is None:
            with _timed("gru_seq_infer", dev):
                check(lib.lg_gru_seq_infer(ptr(src), *w, None, ptr(h_last), nseq, L, I if l == 0 else H, H,
                                           *_layer_drop(l, p, seed, salt0), st), "lg_gru_seq_infer")
        else:
            with _timed("gru_seq_fwd", dev):
                check(lib.lg_gru_seq_fwd(ptr(src), *w, ptr(hs), ptr(g), nseq, L, I if l == 0 else H, H,
                                         *_layer_drop(l, p, seed, salt0), st), "lg_gru_seq_fwd")
            if top:
                h_last.copy_(hs[L - 1].view(h_last.shape))
        h_seqs.append(hs if hs is not None else torch.empty(0, device=dev))
        gates.append(g if g is not None else torch.empty(0, device=dev))
        src = hs
    return h_seqs, gates


def _gru_bptt(lib, label: str, enc: Optional[Tuple[Tensor, Optional[Tensor]]], xt: Optional[Tensor],
              w_ih: List[Tensor], w_hh: List[Tensor], h_seqs: List[Tensor], gates: List[Tensor], dh: Tensor, L: int,
              I: int, p: float, seed: Optional[Tensor], salt0: int, need_dx: bool, own_l0: bool = False,
              ws_extra: int = 0) -> List[Tensor]:
    """BPTT down the layers: [dx or empty, dW_ih_0 .., dW_hh_0 .., db_ih_0 .., db_hh_0 ..].  The top
    layer takes dh (the gradient of h_L) alone, each layer's dx is the layer below's per-step
    gradient.  Layer 0 reads enc in place and writes dx (Nseq, L, I) - through lg_gru_bwd if
    own_l0 (one layer only), else lg_gru_seq_bwd's encoder form - or reads the dense xt and
    writes dx time-major (L, Nseq, I).  All slab reductions are one batch."""
    H, nl = w_hh[0].shape[1], len(w_hh)
    nseq = dh.numel() // H
    dev = dh.device
    st = stream_of(dh)
    if enc is not None:
        residual, tfeat = enc
        B, _, S = residual.shape
    dw_ih, dw_hh = [torch.empty_like(t) for t in w_ih], [torch.empty_like(t) for t in w_hh]
    db_ih = [torch.empty(3 * H, device=dev) for _ in range(nl)]
    db_hh = [torch.empty(3 * H, device=dev) for _ in range(nl)]
    dx_shape = (nseq, L, I) if enc is not None else (L, nseq, I)
    dx = torch.empty(dx_shape if need_dx else 0, device=dev)
    wss = [torch.empty(int(lib.lg_gru_bwd_workspace_bytes(B, S, I, H)) if own_l0 else
                       int(lib.lg_gru_seq_bwd_workspace_bytes(nseq, I if l == 0 else H, H)) + ws_extra,
                       device=dev, dtype=torch.uint8) for l in range(nl)]
    dh_seq: Optional[Tensor] = None  # the layer above's dx
    with _reduce_batch(lib, st), _timed(label, dev):
        for l in range(nl - 1, -1, -1):
            dh_l = ptr(dh) if l == nl - 1 else None
            dxl = dx if l == 0 else torch.empty(L, nseq, H, device=dev)
            dxp = ptr(dxl) if (l > 0 or need_dx) else None
            w = (ptr(w_ih[l]), ptr(w_hh[l]), ptr(h_seqs[l]), ptr(gates[l]))
            dw = (ptr(dw_ih[l]), ptr(dw_hh[l]), ptr(db_ih[l]), ptr(db_hh[l]))
            if l > 0 or enc is None:
                check(lib.lg_gru_seq_bwd(ptr(xt if l == 0 else h_seqs[l - 1]), None, None, *w, ptr(dh_seq), dh_l, dxp,
                                         *dw, 0, 0, nseq, L, I if l == 0 else H, H, *_layer_drop(l, p, seed, salt0),
                                         ptr(wss[l]), wss[l].numel(), st), "lg_gru_seq_bwd")
            elif own_l0:
                check(lib.lg_gru_bwd(ptr(residual), ptr(tfeat), *w, dh_l, dxp, *dw, B, L, S, I, H, ptr(wss[0]),
                                     wss[0].numel(), st), "lg_gru_bwd")
            else:
                check(lib.lg_gru_seq_bwd(None, ptr(residual), ptr(tfeat), *w, ptr(dh_seq), dh_l, dxp, *dw, B, S, nseq,
                                         L, I, H, 0, 0.0, 0, 0, ptr(wss[0]), wss[0].numel(), st), "lg_gru_seq_bwd")
            dh_seq = dxl
    return [dx] + dw_ih + dw_hh + db_ih + db_hh


def _gru_bptt_fake(dx: Tensor, w_ih: List[Tensor], w_hh: List[Tensor]) -> List[Tensor]:
    H = w_hh[0].shape[1]
    return ([dx] + [torch.empty_like(t) for t in w_ih] + [torch.empty_like(t) for t in w_hh]
            + [dx.new_empty(3 * H) for _ in range(2 * len(w_hh))])


def _unfold_dx(dx: Tensor, residual: Tensor, need_res: bool, need_tf: bool) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(d residual (B, L, S), d tfeat (B, L, I - 1)) of the encoder input's dx (B*S, L, I): column 0 is
    the sensor's residual, the others the window's time features, shared by its S sequences."""
    B, L, S = residual.shape
    dres = dx[..., 0].reshape(B, S, L).transpose(1, 2) if need_res else None
    dtf = dx[..., 1:].reshape(B, S, L, dx.shape[-1] - 1).sum(dim=1) if need_tf else None
    return dres, dtf


# ============================================================================ gru_encoder
@torch.library.custom_op(f"{NS}::gru_encoder", mutates_args=(), device_types="cuda")
def gru_encoder(residual: Tensor, tfeat: Optional[Tensor], w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor,
                save: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """(h_L (B, S, H), h_seq, gates): nn.GRU over the B*S sensor sequences, x_t =
    [residual[b, t, s], tfeat[b, t, :]] read in place (lg_gru_fwd).  save: keep h_t and
    the gate values of every step for the backward (else both are empty)."""
    lib = load_library()
    residual, tfeat, w_ih, w_hh, b_ih, b_hh = (_c(t) for t in (residual, tfeat, w_ih, w_hh, b_ih, b_hh))
    _req(residual, tfeat, w_ih, w_hh, b_ih, b_hh)
    B, L, S = residual.shape
    h_last = torch.empty(B, S, w_hh.shape[1], device=residual.device)
    h_seqs, gates = _gru_forward(lib, (residual, tfeat), None, [w_ih], [w_hh], [b_ih], [b_hh], h_last, L,
                                 w_ih.shape[1], 0.0, None, 0, save, keep_h=False)
    return h_last, h_seqs[0], gates[0]


@gru_encoder.register_fake
def _(residual, tfeat, w_ih, w_hh, b_ih, b_hh, save):
    B, L, S = residual.shape
    H = w_hh.shape[1]
    if save:
        return (residual.new_empty(B, S, H), residual.new_empty(L, B * S, H), residual.new_empty(L, B * S, 4, H))
    return residual.new_empty(B, S, H), residual.new_empty(0), residual.new_empty(0)


@torch.library.custom_op(f"{NS}::gru_encoder_backward", mutates_args=(), device_types="cuda")
def gru_encoder_backward(dh: Tensor, residual: Tensor, tfeat: Optional[Tensor], w_ih: Tensor, w_hh: Tensor,
                         h_seq: Tensor, gates: Tensor, need_dx: bool
                         ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(dx (B*S, L, I) or empty, dW_ih, dW_hh, db_ih, db_hh) by BPTT over the saved gates
    (lg_gru_bwd)."""
    lib = load_library()
    dh, residual, tfeat, w_ih, w_hh = (_c(t) for t in (dh, residual, tfeat, w_ih, w_hh))
    _req(dh, residual, tfeat, w_ih, w_hh)
    if h_seq.numel() == 0 or gates.numel() == 0:
        raise RuntimeError("gru_encoder was run with save=False; no backward")
    dx, dw_ih, dw_hh, db_ih, db_hh = _gru_bptt(lib, "gru_bwd", (residual, tfeat), None, [w_ih], [w_hh], [h_seq], [gates],
                                               dh, residual.shape[1], w_ih.shape[1], 0.0, None, 0, need_dx, own_l0=True)
    return dx, dw_ih, dw_hh, db_ih, db_hh


@gru_encoder_backward.register_fake
def _(dh, residual, tfeat, w_ih, w_hh, h_seq, gates, need_dx):
    B, L, S = residual.shape
    dx = residual.new_empty(B * S, L, w_ih.shape[1]) if need_dx else residual.new_empty(0)
    return tuple(_gru_bptt_fake(dx, [w_ih], [w_hh]))


def _gru_setup(ctx, inputs, output):
    residual, tfeat, w_ih, w_hh, _, _, _ = inputs
    _, h_seq, gates = output
    ctx.mark_non_differentiable(h_seq, gates)
    ctx.set_materialize_grads(False)  # no zero-filled (L, B*S, 4H) gradients for the saved tensors
    ctx.has_tfeat = tfeat is not None
    ctx.save_for_backward(residual, tfeat, w_ih, w_hh, h_seq, gates)


def _gru_bwd(ctx, dh, _dhseq, _dgates):
    if dh is None:
        return (None,) * 7
    residual, tfeat, w_ih, w_hh, h_seq, gates = ctx.saved_tensors
    need_dx = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    dx, dw_ih, dw_hh, db_ih, db_hh = torch.ops.leakgnn.gru_encoder_backward(
        dh.contiguous(), residual, tfeat if ctx.has_tfeat else None, w_ih, w_hh, h_seq, gates, need_dx)
    dres, dtf = _unfold_dx(dx, residual, ctx.needs_input_grad[0], ctx.has_tfeat and ctx.needs_input_grad[1])
    return dres, dtf, dw_ih, dw_hh, db_ih, db_hh, None


gru_encoder.register_autograd(_gru_bwd, setup_context=_gru_setup)


# ============================================================================ gru_stack
# nn.GRU(num_layers > 1) of the sensor encoder: layer 0 through lg_gru_fwd exactly as
# gru_encoder runs it, every upper layer through lg_gru_seq_fwd on the h_seq the layer below
# saved (no copy), inter-layer dropout applied on read (GRU_STACK_SALT + boundary).
@torch.library.custom_op(f"{NS}::gru_stack", mutates_args=(), device_types="cuda")
def gru_stack(residual: Tensor, tfeat: Optional[Tensor], w_ih: List[Tensor], w_hh: List[Tensor], b_ih: List[Tensor],
              b_hh: List[Tensor], p: float, seed: Tensor, save: bool) -> List[Tensor]:
    """[h_L (B, S, H) of the top layer, h_seq_0 .. h_seq_{n-1}, gates_0 .. gates_{n-1}]: the stacked
    GRU over the B*S sensor sequences.  p > 0: dropout between layers (train mode), mask of
    boundary l (between layers l and l + 1) from (seed, GRU_STACK_SALT + l) over element index
    (t * B*S + seq) * H + i.  save: keep every layer's gates for the backward (else they are
    empty; every layer's h_seq is kept either way)."""
    lib = load_library()
    residual, tfeat = _c(residual), _c(tfeat)
    w_ih, w_hh, b_ih, b_hh = ([_c(t) for t in ts] for ts in (w_ih, w_hh, b_ih, b_hh))
    _req(residual, tfeat, *w_ih, *w_hh, *b_ih, *b_hh)
    I, H, _ = _gru_dims("gru_stack", residual, False, w_ih, w_hh, b_ih, b_hh, p)
    B, L, S = residual.shape
    h_last = torch.empty(B, S, H, device=residual.device)
    h_seqs, gates = _gru_forward(lib, (residual, tfeat), None, w_ih, w_hh, b_ih, b_hh, h_last, L, I, p, seed,
                                 GRU_STACK_SALT, save, keep_h=True)
    return [h_last] + h_seqs + gates


@gru_stack.register_fake
def _(residual, tfeat, w_ih, w_hh, b_ih, b_hh, p, seed, save):
    B, L, S = residual.shape
    H = w_hh[0].shape[1]
    nl = len(w_hh)
    return ([residual.new_empty(B, S, H)] + [residual.new_empty(L, B * S, H) for _ in range(nl)]
            + [residual.new_empty(L, B * S, 4, H) if save else residual.new_empty(0) for _ in range(nl)])


@torch.library.custom_op(f"{NS}::gru_stack_backward", mutates_args=(), device_types="cuda")
def gru_stack_backward(dh: Tensor, residual: Tensor, tfeat: Optional[Tensor], w_ih: List[Tensor], w_hh: List[Tensor],
                       h_seqs: List[Tensor], gates: List[Tensor], p: float, seed: Tensor, need_dx: bool
                       ) -> List[Tensor]:
    """[dx (B*S, L, I) or empty, dW_ih_0 .., dW_hh_0 .., db_ih_0 .., db_hh_0 ..]: BPTT down the stack
    (lg_gru_seq_bwd at every layer, layer 0 in its encoder form reading (residual, tfeat) in place)."""
    lib = load_library()
    dh, residual, tfeat = _c(dh), _c(residual), _c(tfeat)
    w_ih, w_hh = [_c(t) for t in w_ih], [_c(t) for t in w_hh]
    _req(dh, residual, tfeat, *w_ih, *w_hh)
    if any(g.numel() == 0 for g in gates):
        raise RuntimeError("gru_stack was run with save=False; no backward")
    I, _, _ = _gru_dims("gru_stack", residual, False, w_ih, w_hh)
    return _gru_bptt(lib, "gru_bwd", (residual, tfeat), None, w_ih, w_hh, h_seqs, gates, dh, residual.shape[1], I, p,
                     seed, GRU_STACK_SALT, need_dx)


@gru_stack_backward.register_fake
def _(dh, residual, tfeat, w_ih, w_hh, h_seqs, gates, p, seed, need_dx):
    B, L, S = residual.shape
    return _gru_bptt_fake(residual.new_empty(B * S, L, w_ih[0].shape[1]) if need_dx else residual.new_empty(0), w_ih, w_hh)


def _gru_stack_setup(ctx, inputs, output):
    residual, tfeat, w_ih, w_hh, _, _, p, seed, _ = inputs
    ctx.nl, ctx.p, ctx.has_tfeat = len(w_hh), p, tfeat is not None
    ctx.mark_non_differentiable(*output[1:])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(residual, tfeat if tfeat is not None else residual, seed, *w_ih, *w_hh, *output[1:])


def _gru_stack_bwd(ctx, grads):
    dh = grads[0]
    if dh is None:
        return (None,) * 9
    nl = ctx.nl
    (residual, tfeat, seed), w_ih, w_hh, h_seqs, gates = _split(ctx.saved_tensors, 3, nl, nl, nl, nl)
    need_tf = ctx.has_tfeat and ctx.needs_input_grad[1]
    out = torch.ops.leakgnn.gru_stack_backward(dh.contiguous(), residual, tfeat if ctx.has_tfeat else None, w_ih, w_hh,
                                               h_seqs, gates, ctx.p, seed, ctx.needs_input_grad[0] or need_tf)
    (dx,), *dws = _split(out, 1, nl, nl, nl, nl)
    return (*_unfold_dx(dx, residual, ctx.needs_input_grad[0], need_tf), *dws, None, None, None)


gru_stack.register_autograd(_gru_stack_bwd, setup_context=_gru_stack_setup)


# ============================================================================ gru_predictor
# NormalPredictorGRU's nn.GRU (reference models/predictor.py:84-111) over a dense (B, L, I)
# input: every layer through lg_gru_seq_fwd / lg_gru_seq_bwd (MFMA kernels at H = 128, the
# generic kernels at other widths), the input copied once to time-major, inter-layer dropout
# applied on read (GRU_PRED_SALT + boundary).
@torch.library.custom_op(f"{NS}::gru_predictor", mutates_args=(), device_types="cuda")
def gru_predictor(x: Tensor, w_ih: List[Tensor], w_hh: List[Tensor], b_ih: List[Tensor], b_hh: List[Tensor],
                  p: float, seed: Tensor, save: bool) -> List[Tensor]:
    """[h_L (B, H) of the top layer, x time-major (L, B, I), h_seq_0 .. h_seq_{n-1}, gates_0 ..
    gates_{n-1}].  p > 0: dropout between layers, mask of boundary l from (seed, GRU_PRED_SALT + l)
    over element index (t * B + b) * H + i.  save=False (inference): no gates, and at H = 128 the
    top layer writes h_L alone (lg_gru_seq_infer); the tensors not produced are empty."""
    lib = load_library()
    x = _c(x)
    w_ih, w_hh, b_ih, b_hh = ([_c(t) for t in ts] for ts in (w_ih, w_hh, b_ih, b_hh))
    _req(x, *w_ih, *w_hh, *b_ih, *b_hh)
    I, H, _ = _gru_dims("gru_predictor", x, True, w_ih, w_hh, b_ih, b_hh, p)
    B, L, _ = x.shape
    xt = x.transpose(0, 1).clone(memory_format=torch.contiguous_format)  # never a view of x
    h_last = torch.empty(B, H, device=x.device)
    h_seqs, gates = _gru_forward(lib, None, xt, w_ih, w_hh, b_ih, b_hh, h_last, L, I, p, seed, GRU_PRED_SALT, save,
                                 keep_h=H != 128)
    return [h_last, xt if save else torch.empty(0, device=x.device)] + h_seqs + gates


@gru_predictor.register_fake
def _(x, w_ih, w_hh, b_ih, b_hh, p, seed, save):
    B, L, I = x.shape
    H = w_hh[0].shape[1]
    nl = len(w_hh)
    hs = [x.new_empty(L, B, H) for _ in range(nl)]
    if not save and H == 128:
        hs[-1] = x.new_empty(0)
    return ([x.new_empty(B, H), x.new_empty(L, B, I) if save else x.new_empty(0)] + hs
            + [x.new_empty(L, B, 4, H) if save else x.new_empty(0) for _ in range(nl)])


@torch.library.custom_op(f"{NS}::gru_predictor_backward", mutates_args=(), device_types="cuda")
def gru_predictor_backward(dh: Tensor, xt: Tensor, w_ih: List[Tensor], w_hh: List[Tensor], h_seqs: List[Tensor],
                           gates: List[Tensor], p: float, seed: Tensor, need_dx: bool) -> List[Tensor]:
    """[dx (B, L, I) or empty, dW_ih_0 .., dW_hh_0 .., db_ih_0 .., db_hh_0 ..]: BPTT down the stack
    (lg_gru_seq_bwd), dx transposed back from time-major."""
    lib = load_library()
    dh = _c(dh)
    w_ih, w_hh = [_c(t) for t in w_ih], [_c(t) for t in w_hh]
    _req(dh, xt, *w_ih, *w_hh)
    if xt.numel() == 0 or any(g.numel() == 0 for g in gates):
        raise RuntimeError("gru_predictor was run with save=False; no backward")
    L, B, I = xt.shape
    H = w_hh[0].shape[1]
    # the H = 128 backward takes its dG a pass of steps at a time: room for all L steps makes it one pass
    out = _gru_bptt(lib, "gru_seq_bwd", None, xt, w_ih, w_hh, h_seqs, gates, dh, L, I, p, seed, GRU_PRED_SALT, need_dx,
                    ws_extra=L * B * 4 * H * 4 if H == 128 else 0)
    if need_dx:
        out[0] = out[0].transpose(0, 1).contiguous()
    return out


@gru_predictor_backward.register_fake
def _(dh, xt, w_ih, w_hh, h_seqs, gates, p, seed, need_dx):
    L, B, I = xt.shape
    return _gru_bptt_fake(xt.new_empty(B, L, I) if need_dx else xt.new_empty(0), w_ih, w_hh)


def _gru_predictor_setup(ctx, inputs, output):
    _, w_ih, w_hh, _, _, p, seed, _ = inputs
    ctx.nl, ctx.p = len(w_hh), p
    ctx.mark_non_differentiable(*output[1:])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(seed, *w_ih, *w_hh, *output[1:])


def _gru_predictor_bwd(ctx, grads):
    dh = grads[0]
    if dh is None:
        return (None,) * 8
    nl = ctx.nl
    (seed,), w_ih, w_hh, (xt,), h_seqs, gates = _split(ctx.saved_tensors, 1, nl, nl, 1, nl, nl)
    need_dx = ctx.needs_input_grad[0]
    out = torch.ops.leakgnn.gru_predictor_backward(dh.contiguous(), xt, w_ih, w_hh, h_seqs, gates, ctx.p, seed, need_dx)
    (dx,), *dws = _split(out, 1, nl, nl, nl, nl)
    return (dx if need_dx else None, *dws, None, None, None)


gru_predictor.register_autograd(_gru_predictor_bwd, setup_context=_gru_predictor_setup)


# ============================================================================ tcn_predictor
# NormalPredictorTCN's conv stack (reference models/predictor.py:31-81) over the output of the input
# projection: every [conv -> LayerNorm -> ReLU -> Dropout] stage is one lg_tcn_conv_train_fwd launch
# (the residual add fused into conv2) and one lg_tcn_conv_bwd call (elementwise / LayerNorm backward,
# dx as the conv kernel over the transposed table, dW as an MFMA GEMM over all rows).  Dropout mask of
# conv i: (seed, TCN_SALT + i) over element index (b * L + t) * 128 + c.
_TCN_PACK_CACHE: "OrderedDict[int, tuple]" = OrderedDict()
_TCN_PACK_MAX = 64


def _tcn_packed(w: Tensor, transposed: bool) -> Tensor:
    """The packed (forward) or transposed-packed (backward dx) form of a Conv1d weight
    (lg_tcn_pack_weight / _t).  Eagerly both are made together and cached per parameter
    (data_ptr, _version) as tcn_plan._packed_weights does: an in-place optimizer step bumps the
    version and so invalidates the entry.  An entry keeps its weight tensor alive, so its address
    cannot be handed to another tensor while the entry exists; the oldest entries are dropped.
    While the stream is capturing, the cache is neither read nor written: the one pack launch the
    caller needs is recorded in the graph, so every replay packs the weights it finds (a replayed
    optimizer step changes them on the device without moving _version).  For the same reason
    whoever replays such a graph calls invalidate_weight_packs() before the next eager call."""
    lib = load_library()
    st = stream_of(w)
    if torch.cuda.is_current_stream_capturing():
        out = torch.empty(int(lib.lg_tcn_packed_weight_floats(128)), device=w.device)
        if transposed:
            check(lib.lg_tcn_pack_weight_t(ptr(w), ptr(out), 128, st), "lg_tcn_pack_weight_t")
        else:
            check(lib.lg_tcn_pack_weight(ptr(w), ptr(out), 128, st), "lg_tcn_pack_weight")
        return out
    try:
        stamp = (w.data_ptr(), w._version)
    except RuntimeError:  # an inference tensor has no version counter: not cached
        stamp = None
    if stamp is not None:
        hit = _TCN_PACK_CACHE.get(stamp[0])
        if hit is not None and hit[0] == stamp[1]:
            _TCN_PACK_CACHE.move_to_end(stamp[0])
            return hit[3] if transposed else hit[2]
    n = int(lib.lg_tcn_packed_weight_floats(128))
    pk, pkt = torch.empty(n, device=w.device), torch.empty(n, device=w.device)
    check(lib.lg_tcn_pack_weight(ptr(w), ptr(pk), 128, st), "lg_tcn_pack_weight")
    check(lib.lg_tcn_pack_weight_t(ptr(w), ptr(pkt), 128, st), "lg_tcn_pack_weight_t")
    if stamp is not None:
        _TCN_PACK_CACHE[stamp[0]] = (stamp[1], w, pk, pkt)
        _TCN_PACK_CACHE.move_to_end(stamp[0])
        while len(_TCN_PACK_CACHE) > _TCN_PACK_MAX:
            _TCN_PACK_CACHE.popitem(last=False)
    return pkt if transposed else pk


def invalidate_weight_packs() -> None:
    """Forget every cached packed weight (this module's and tcn_plan's).  A replayed HIP graph
    that holds an optimizer step updates the weights without moving their _version, so the
    captured predictor step calls this after each replay; the next eager call packs again.  A dict
    clear and a counter bump, no device work."""
    from . import tcn_plan
    _TCN_PACK_CACHE.clear()
    tcn_plan.invalidate_packed_weights()


def _tcn_dims(x: Tensor, conv_w: List[Tensor], conv_b: List[Tensor], ln_w: List[Tensor], ln_b: List[Tensor]
              ) -> Tuple[int, int, int]:
    if x.dim() != 3 or x.shape[2] != 128:
        raise ValueError(f"tcn_predictor: x must be (B, L, 128), got {tuple(x.shape)}")
    B, L, C = x.shape
    n = len(conv_w)
    if n < 2 or n % 2 or not (len(conv_b) == len(ln_w) == len(ln_b) == n):
        raise ValueError("tcn_predictor: two (conv weight, conv bias, LayerNorm weight, LayerNorm bias) per block")
    if not 1 <= L <= 2048:
        raise ValueError(f"tcn_predictor: L must be in 1..2048, got {L}")
    if B * L * C * 4 >= 2 ** 31:
        raise ValueError(f"tcn_predictor: B * L * 512 bytes must stay below 2 GiB, got B {B}, L {L}")
    for i in range(n):
        if tuple(conv_w[i].shape) != (C, C, 3) or any(tuple(t[i].shape) != (C,) for t in (conv_b, ln_w, ln_b)):
            raise ValueError(f"tcn_predictor: conv {i} needs a (128, 128, 3) weight and (128,) bias / LayerNorm "
                             f"vectors, got {tuple(conv_w[i].shape)}")
    return B, L, n


@torch.library.custom_op(f"{NS}::tcn_predictor", mutates_args=(), device_types="cuda")
def tcn_predictor(x: Tensor, conv_w: List[Tensor], conv_b: List[Tensor], ln_w: List[Tensor], ln_b: List[Tensor],
                  eps: float, p: float, seed: Tensor, save: bool) -> List[Tensor]:
    """[h_last (B, 128) = the last block's output at t = L - 1, s_0 .. s_{n-1}, xhat_0 .., rstd_0 ..,
    block outputs 0 .. n/2 - 1] for x (B, L, 128), the input projection's output, and n = 2 * blocks
    conv stages with dilation 2 ** (i // 2).  s_i (B * L, 128) is stage i's output before the residual
    add, xhat_i / rstd_i its normalised conv output and 1 / sqrt(var + eps) (the LayerNorm backward's
    inputs).  save=False (no backward): only h_last, the other tensors are empty."""
    from .tcn_plan import train_tables
    lib = load_library()
    x = _c(x)
    conv_w, conv_b, ln_w, ln_b = ([_c(t) for t in ts] for ts in (conv_w, conv_b, ln_w, ln_b))
    _req(x, *conv_w, *conv_b, *ln_w, *ln_b)
    B, L, n = _tcn_dims(x, conv_w, conv_b, ln_w, ln_b)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"tcn_predictor: dropout p must be in [0, 1), got {p}")
    C = 128
    dev = x.device
    st = stream_of(x)
    seed_v, sbit = _seed_args(seed) if p > 0.0 else (0, 0)
    tabs, _ = train_tables(L, [2 ** b for b in range(n // 2)], dev)
    none = torch.empty(0, device=dev)
    ss, xhs, rss, outs = [], [], [], []
    blk_in = x.view(B * L, C)
    src = blk_in
    with _timed("tcn_train_fwd", dev):
        for i in range(n):
            conv2 = i % 2 == 1
            pk = _tcn_packed(conv_w[i], False)
            s = torch.empty(B * L, C, device=dev) if (save or p > 0.0 or not conv2) else None
            out = torch.empty(B * L, C, device=dev) if conv2 else None
            xh = torch.empty(B * L, C, device=dev) if save else None
            rs = torch.empty(B * L, device=dev) if save else None
            check(lib.lg_tcn_conv_train_fwd(ptr(src), ptr(blk_in) if conv2 else None, ptr(tabs[i]), ptr(pk),
                                            ptr(conv_b[i]), ptr(ln_w[i]), ptr(ln_b[i]), eps, p, seed_v,
                                            ((TCN_SALT + i) | sbit) if p > 0.0 else 0, ptr(s), ptr(out), ptr(xh),
                                            ptr(rs), B, L, L if conv2 else 0, L, C, st), "lg_tcn_conv_train_fwd")
            if save:
                ss.append(s)
                xhs.append(xh)
                rss.append(rs)
            if conv2:
                if save:
                    outs.append(out)
                blk_in = src = out
            else:
                src = s
    h_last = blk_in.view(B, L, C)[:, L - 1].clone(memory_format=torch.contiguous_format)
    if not save:
        return [h_last] + [none.clone() for _ in range(3 * n + n // 2)]
    return [h_last] + ss + xhs + rss + outs


@tcn_predictor.register_fake
def _(x, conv_w, conv_b, ln_w, ln_b, eps, p, seed, save):
    B, L, C = x.shape
    n = len(conv_w)
    if not save:
        return [x.new_empty(B, C)] + [x.new_empty(0) for _ in range(3 * n + n // 2)]
    return ([x.new_empty(B, C)] + [x.new_empty(B * L, C) for _ in range(2 * n)] + [x.new_empty(B * L) for _ in range(n)]
            + [x.new_empty(B * L, C) for _ in range(n // 2)])


@torch.library.custom_op(f"{NS}::tcn_predictor_backward", mutates_args=(), device_types="cuda")
def tcn_predictor_backward(dh: Tensor, x: Tensor, conv_w: List[Tensor], ln_w: List[Tensor], s: List[Tensor],
                           xhat: List[Tensor], rstd: List[Tensor], outs: List[Tensor], p: float,
                           need_dx: bool) -> List[Tensor]:
    """[dx (B, L, 128) or empty, dW_0 .., db_0 .., dgamma_0 .., dbeta_0 ..] for dh, the gradient of
    h_last: lg_tcn_conv_bwd down the stages.  Every gradient is overwritten, none accumulated into."""
    from .tcn_plan import train_tables
    lib = load_library()
    dh, x = _c(dh), _c(x)
    conv_w, ln_w = [_c(t) for t in conv_w], [_c(t) for t in ln_w]
    _req(dh, x, *conv_w, *ln_w)
    n = len(conv_w)
    if len(s) != n or any(t.numel() == 0 for t in s):
        raise RuntimeError("tcn_predictor was run with save=False; no backward")
    B, L, C = x.shape
    dev = x.device
    st = stream_of(x)
    tabs, tabs_t = train_tables(L, [2 ** b for b in range(n // 2)], dev)
    dws = [torch.empty(C, C, 3, device=dev) for _ in range(n)]
    dbs, dgs, dbts = ([torch.empty(C, device=dev) for _ in range(n)] for _ in range(3))
    ws = torch.empty(int(lib.lg_tcn_conv_bwd_workspace_bytes(B, L, C)), device=dev, dtype=torch.uint8)
    dz = torch.empty(B * L, C, device=dev)
    dy = torch.zeros(B, L, C, device=dev)
    dy[:, L - 1] = dh
    dy = dy.view(B * L, C)

    def stage(i, dy_i, src, dres, dx):
        pkt = _tcn_packed(conv_w[i], True)
        check(lib.lg_tcn_conv_bwd(ptr(dy_i), ptr(s[i]), ptr(xhat[i]), ptr(rstd[i]), ptr(src), ptr(dres), ptr(tabs[i]),
                                  ptr(tabs_t[i]), ptr(pkt), ptr(ln_w[i]), p, ptr(dz), ptr(dx), ptr(dws[i]), ptr(dbs[i]),
                                  ptr(dgs[i]), ptr(dbts[i]), B, L, L if dres is not None else 0, L, C, ptr(ws),
                                  ws.numel(), st), "lg_tcn_conv_bwd")

    with _timed("tcn_train_bwd", dev):
        for b in range(n // 2 - 1, -1, -1):
            blk_in = x.view(B * L, C) if b == 0 else outs[b - 1]
            ds1 = torch.empty(B * L, C, device=dev)
            stage(2 * b + 1, dy, s[2 * b], None, ds1)            # conv2: its input is conv1's output
            want_dx = b > 0 or need_dx
            dprev = torch.empty(B * L, C, device=dev) if want_dx else None
            stage(2 * b, ds1, blk_in, dy if want_dx else None, dprev)  # conv1: + the residual's pass-through
            dy = dprev
    dx = dy.view(B, L, C) if need_dx else torch.empty(0, device=dev)
    return [dx] + dws + dbs + dgs + dbts


@tcn_predictor_backward.register_fake
def _(dh, x, conv_w, ln_w, s, xhat, rstd, outs, p, need_dx):
    n = len(conv_w)
    return ([torch.empty_like(x) if need_dx else x.new_empty(0)] + [torch.empty_like(t) for t in conv_w]
            + [x.new_empty(128) for _ in range(3 * n)])


def _tcn_predictor_setup(ctx, inputs, output):
    x, conv_w, _, ln_w, _, _, p, _, _ = inputs
    ctx.n, ctx.p = len(conv_w), p
    ctx.mark_non_differentiable(*output[1:])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(x, *conv_w, *ln_w, *output[1:])


def _tcn_predictor_bwd(ctx, grads):
    dh = grads[0]
    if dh is None:
        return (None,) * 9
    n = ctx.n
    (x,), conv_w, ln_w, s, xhat, rstd, outs = _split(ctx.saved_tensors, 1, n, n, n, n, n, n // 2)
    need_dx = ctx.needs_input_grad[0]
    out = torch.ops.leakgnn.tcn_predictor_backward(dh.contiguous(), x, conv_w, ln_w, s, xhat, rstd, outs, ctx.p, need_dx)
    (dx,), *dws = _split(out, 1, n, n, n, n)
    return (dx if need_dx else None, *dws, None, None, None, None)


tcn_predictor.register_autograd(_tcn_predictor_bwd, setup_context=_tcn_predictor_setup)


REDUCE_BATCH = True  # tests switch it off to compare with one reduction launch per op


@contextlib.contextmanager
def _reduce_batch(lib, st):
    """All slab reductions of the enclosed backward launches as one launch at the end
    (lg_reduce_batch_begin / _flush, include/leakgnn.h).  The enclosed code keeps every
    workspace it passes alive until the flush (the caller's locals).  A batch per backward pass
    instead of per op was measured (+0.7 %) and dropped: autograd reads or copies an op's
    gradients (AccumulateGrad into an existing .grad, a clone when another reference is held)
    before an end-of-pass flush would have written them."""
    if not REDUCE_BATCH:
        yield
        return
    check(lib.lg_reduce_batch_begin(), "lg_reduce_batch_begin")
    try:
        yield
    finally:
        check(lib.lg_reduce_batch_flush(st), "lg_reduce_batch_flush")


def expand_x0(xs0: Tensor, x0bits: Tensor, sensor_slot: Tensor, node_bias: Tensor, N: int, p: float) -> Tensor:
    """x_0 (N, B, D) materialised from the compressed node init (lg_node_init_expand):
    diagnostics and tests only (LeakDetector.capture)."""
    lib = load_library()
    S, B, D = xs0.shape
    x0 = torch.empty(N, B, D, device=xs0.device, dtype=torch.float32)
    check(lib.lg_node_init_expand(ptr(sensor_slot), ptr(xs0), ptr(x0bits), ptr(node_bias), ptr(x0), B, N, D,
                                  nat.LG_F_DROPOUT if p > 0.0 else 0, p, stream_of(xs0)), "lg_node_init_expand")
    return x0


# ============================================================================ diffuse
# APPNP's propagation (Gasteiger et al. 2019) of a node-major tensor: z_0 = x, z_{k+1} = (1 - alpha)
# Ahat z_k + alpha x.  No parameter; the backward is the adjoint recurrence over the transposed
# tables and saves nothing but them.
def check_diffuse(hops: int, alpha: float, zero_ok: bool = False) -> None:
    if not (0 if zero_ok else 1) <= int(hops) <= 64:
        raise ValueError(f"diffuse hops must be in {0 if zero_ok else 1}..64, got {hops}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"diffuse alpha must be in [0, 1], got {alpha}")


def _diffuse_launch(lib, tab: Tensor, pairs: Tensor, src: Tensor, out: Tensor, hops: int, alpha: float, *,
                    backward: bool, x0: Optional[Tensor] = None, scale_out: float = 1.0, flags: int = 0) -> None:
    """lg_diffuse_fwd (src = x_0) or lg_diffuse_bwd (src = g; x0: apply the node init's mask
    [x0 > 0] * scale_out) on (N, B, D) tensors, with the hop-wise form's workspace when it runs."""
    N, B, D = src.shape
    st = stream_of(src)
    flags |= nat.LG_F_MASK_OUT if x0 is not None else 0
    nb = int(lib.lg_diffuse_workspace_bytes(B, N, D, hops, flags, int(backward)))
    if nb < 0:
        check(nb, "lg_diffuse_workspace_bytes")
    ws = torch.empty(nb, device=src.device, dtype=torch.uint8) if nb else None
    with _timed("diffuse_bwd" if backward else "diffuse_fwd", src.device):
        if backward:
            check(lib.lg_diffuse_bwd(ptr(tab), ptr(pairs), ptr(src), ptr(x0), ptr(out), B, N, D, hops, alpha, flags,
                                     scale_out, ptr(ws), nb, st), "lg_diffuse_bwd")
        else:
            check(lib.lg_diffuse_fwd(ptr(tab), ptr(pairs), ptr(src), ptr(out), B, N, D, hops, alpha, flags, ptr(ws),
                                     nb, st), "lg_diffuse_fwd")


@torch.library.custom_op(f"{NS}::diffuse", mutates_args=(), device_types="cuda")
def diffuse(x: Tensor, nodetab: Tensor, pairs: Tensor, nodetab_t: Tensor, pairs_t: Tensor, hops: int,
            alpha: float) -> Tensor:
    """z_hops of z_0 = x, z_{k+1} = (1 - alpha) Ahat z_k + alpha x, for node-major x (N, B, D), D in
    {32, 64}; Ahat from GCNGraph's node tables (edge weights included).  hops in 1..64, alpha in [0, 1]."""
    lib = load_library()
    x = _c(x)
    _req(x)
    if x.dim() != 3:
        raise ValueError(f"diffuse: x must be node-major (N, B, D), got {tuple(x.shape)}")
    _check_d(x.shape[2])
    check_diffuse(hops, alpha)
    z = torch.empty_like(x)
    _diffuse_launch(lib, nodetab, pairs, x, z, hops, alpha, backward=False)
    return z


@diffuse.register_fake
def _(x, nodetab, pairs, nodetab_t, pairs_t, hops, alpha):
    return torch.empty_like(x)


@torch.library.custom_op(f"{NS}::diffuse_backward", mutates_args=(), device_types="cuda")
def diffuse_backward(g: Tensor, nodetab_t: Tensor, pairs_t: Tensor, hops: int, alpha: float) -> Tensor:
    """dx of diffuse: u = g, acc = 0; hops times acc += alpha u, u = (1 - alpha) Ahat^T u; u + acc."""
    lib = load_library()
    g = _c(g)
    _req(g)
    dx = torch.empty_like(g)
    _diffuse_launch(lib, nodetab_t, pairs_t, g, dx, hops, alpha, backward=True)
    return dx


@diffuse_backward.register_fake
def _(g, nodetab_t, pairs_t, hops, alpha):
    return torch.empty_like(g)


def _diffuse_setup(ctx, inputs, output):
    _, _, _, nodetab_t, pairs_t, ctx.hops, ctx.alpha = inputs
    ctx.save_for_backward(nodetab_t, pairs_t)


def _diffuse_bwd(ctx, g):
    nodetab_t, pairs_t = ctx.saved_tensors
    return (torch.ops.leakgnn.diffuse_backward(g, nodetab_t, pairs_t, ctx.hops, ctx.alpha),) + (None,) * 6


diffuse.register_autograd(_diffuse_bwd, setup_context=_diffuse_setup)


# ============================================================================ trunk ops: shared drivers
# gnn_trunk, gnn_trunk_norm and encoder_trunk are one forward layer launch (_layer_forward) and one
# backward layer launch (_layer_backward) over the C entry points, each op call described once by a
# _Trunk.  What differs between the ops is passed in: the layer's input (x_l, its compressed form
# under x0bits, the norm route's xn_l), the mask words it writes or reads, the forward flag rule
# (branch) and the backward's masks.  Each op has one output layout (_*_layout: the real and the
# fake body allocate from it, the autograd setup and trunk_fields read its positions), and the
# autograd glue names what it saves (_save_named / _saved_named: the *_backward op's arguments by
# keyword) and what it returns (_named_grads over the op's own parameter names).
def mask_words(N: int, B: int) -> int:
    """int16 words of one activation's [x > 0] bits (the layout of lg_gcn_fwd_nm_bits,
    include/leakgnn.h): 64 lanes per node and 16-window tile."""
    return N * ((B + 15) // 16) * 64


def _layer_words(ymask: Tensor, l: int, L: int) -> Tensor:  # of a ymask with one mask per layer (skip, norm)
    n = ymask.numel() // L
    return ymask[l * n:(l + 1) * n]


# One call of a trunk op (forward or backward): sizes, layout and tier, the dropout triple drop =
# (dflag, seed_v, sbit), and the tables the call was given (None otherwise): the node tables, the
# CSR triple where window-major needs it, their transposes in a backward, the sensor marks.
_Trunk = dataclasses.make_dataclass("_Trunk", (
    ["lib", "st", "dev", "B", "N", "S", "D", "L", "p", "scale", "drop"]
    + [("node_major", bool, True), ("bf16", bool, False), ("skip", bool, False), ("nnz", int, 0),
       ("hops", int, 0), ("alpha", float, 0.0)]
    + [(k, Optional[Tensor], None) for k in (
        "nodetab", "pairs", "rowptr", "col", "w", "nodetab_t", "pairs_t", "rowptr_t", "col_t", "w_t",
        "nodetab_s", "pairs_s", "pos_slot_t", "sensor_slot", "node_bias")]))


def _trunk(lib, ref: Tensor, B: int, N: int, S: int, D: int, L: int, p: float, seed: Optional[Tensor] = None, **kw):
    """The _Trunk of a call on ref's device and stream.  seed: a forward's (a backward draws nothing)."""
    drop = p > 0.0
    seed_v, sbit = _seed_args(seed) if (drop and seed is not None) else (0, 0)
    return _Trunk(lib=lib, st=stream_of(ref), dev=ref.device, B=B, N=N, S=S, D=D, L=L, p=p,
                  scale=1.0 / (1.0 - p) if drop else 1.0, drop=(nat.LG_F_DROPOUT if drop else 0, seed_v, sbit), **kw)


def _check_trunk_diffuse(op: str, hops: int, alpha: float, node_major: bool = True, bf16: bool = False) -> None:
    check_diffuse(hops, alpha, zero_ok=True)
    if hops > 0 and (bf16 or not node_major):
        raise ValueError(f"{op}: hops > 0 runs on the node-major fp32 tier only")


def _trunk_diffuse_forward(t: _Trunk, x0: Tensor, z: Tensor) -> None:
    """The diffusion stage of a trunk op (t.hops > 0), between the node init and layer 0: z = z_K of
    the dense node-major node init x0."""
    _diffuse_launch(t.lib, t.nodetab, t.pairs, x0, z, t.hops, t.alpha, backward=False)


def _trunk_diffuse_backward(t: _Trunk, dz: Tensor, x0: Tensor, nonsensor_idx: Tensor) -> Tuple[Tensor, Tensor]:
    """(dx0, dbias_ns) from dL/dz: the adjoint hops, then the node init's ReLU / dropout mask from the
    saved x0 inside the same launch (LG_F_MASK_OUT); dbias_ns: the non-sensor rows' bias sum."""
    dx0 = torch.empty_like(dz)
    _diffuse_launch(t.lib, t.nodetab_t, t.pairs_t, dz, dx0, t.hops, t.alpha, backward=True, x0=x0, scale_out=t.scale)
    return dx0, dx0.index_select(0, nonsensor_idx).sum(dim=(0, 1))


def _layer_forward(t: _Trunk, l: int, x: Tensor, W: Tensor, b: Tensor, y: Tensor, words: Optional[Tensor] = None, *,
                   x0bits: Optional[Tensor] = None, branch: bool = False) -> None:
    """y = dropout(relu(Ahat x W^T + b)) of layer l (salt l + 1), [y > 0] into `words` where given.
    x0bits: x is the compressed node init's sensor rows (S, B, D), read through the marked table
    (lg_gcn_fwd_nm_x0).  branch: the layer is a residual branch, lg_gcn_fwd_nm_skip (y = x + f,
    t.skip) or the norm route's lg_gcn_fwd_nm_bits on xn_l; otherwise node-major
    lg_gcn_fwd_nm_bits, window-major lg_gcn_fwd."""
    lib, (dflag, seed_v, sbit) = t.lib, t.drop
    flags = nat.LG_F_BIAS | nat.LG_F_RELU | dflag | (nat.LG_F_BF16 if t.bf16 else 0)
    salt = (l + 1) | sbit
    with _timed("gcn_fwd_l0" if x0bits is not None else "gcn_fwd", t.dev):
        if x0bits is not None:
            # the x0 kernel takes the trunk-forward flags alone (it has no dense-layer variants)
            check(lib.lg_gcn_fwd_nm_x0(ptr(t.nodetab_s), ptr(t.pairs_s), ptr(x), ptr(x0bits), ptr(t.node_bias), ptr(W),
                                       ptr(b), ptr(y), t.B, t.N, t.S, t.D, flags | GCN_FWD_NM_EXTRA_FLAGS, t.p, seed_v,
                                       salt, t.st), "lg_gcn_fwd_nm_x0")
        elif t.node_major:
            if branch:  # its input is signed (the stream, or its norm): only the split-bf16 product applies
                flags |= GCN_FWD_NM_EXTRA_FLAGS & nat.LG_F_BF16X3
            else:       # the dense layers' own flags belong to the fp32 tier (bf16: one product, LG_F_BF16)
                flags |= GCN_FWD_NM_EXTRA_FLAGS | (GCN_FWD_DENSE_EXTRA_FLAGS if not t.bf16 else 0)
            fn, name = ((lib.lg_gcn_fwd_nm_skip, "lg_gcn_fwd_nm_skip") if t.skip else
                        (lib.lg_gcn_fwd_nm_bits, "lg_gcn_fwd_nm_bits"))
            check(fn(ptr(t.nodetab), ptr(t.pairs), ptr(x), ptr(W), ptr(b), ptr(y), t.B, t.N, t.D, t.nnz, flags, t.p,
                     seed_v, salt, t.st, ptr(words)), name)
        else:
            check(lib.lg_gcn_fwd(ptr(t.rowptr), ptr(t.col), ptr(t.w), ptr(x), ptr(W), ptr(b), ptr(y), t.B, t.N, t.D,
                                 t.nnz, flags, t.p, seed_v, salt, t.st), "lg_gcn_fwd")


class _WGrad:
    """dL/dw of the trunk's layers, collected by _layer_backward when the edge coefficients
    learn (rowptr, col given: the forward CSR): G = sum over the layers of _layer_dw, added in the
    order the backward visits them (last layer first), over the CSR's slots.  Otherwise empty."""

    def __init__(self, rowptr: Optional[Tensor], col: Optional[Tensor]):
        self.rowptr, self.col, self.G, self.on = rowptr, col, None, rowptr is not None

    def add(self, G: Tensor) -> None:
        self.G = G if self.G is None else self.G + G

    def total(self, dev) -> Tensor:
        return self.G if self.G is not None else torch.zeros(self.col.numel() if self.on else 0, device=dev)


def _layer_dw(t: _Trunk, dy: Tensor, x: Tensor, y: Optional[Tensor], W: Tensor, words: Optional[Tensor],
              mask_in: bool, x0bits: Optional[Tensor], rowptr: Tensor, col: Tensor) -> Tensor:
    """One layer's share of dL/dw: G[k] = sum_b (dz W)[n, b] . x[col k, b] for every slot k of row n,
    with dz = dy * scale * [f > 0] under mask_in (the last plain layer, every skip / norm branch:
    the mask from the layer's bit words, else from its output y) and dz = dy otherwise (that dy is
    the layer above's dx, which that launch already masked: LG_F_MASK_OUT), exactly the dz of the
    layer's own backward launch.  Node-major: lg_sddmm_nm; the compressed node init is
    materialised for layer 0 (lg_node_init_expand; a compressed-x0 form of the kernel is left for
    later).  Window-major: da on a library GEMM, then ONE lg_sddmm_cols over the [N][B * D]
    transposes.  Deterministic."""
    if t.node_major:
        if x0bits is not None:
            x = expand_x0(x, x0bits, t.sensor_slot, t.node_bias, t.N, t.p)
        return sddmm_nm(rowptr, col, dy, W, x, y=y if (mask_in and words is None) else None, ymask=words,
                        mask_in=mask_in, scale=t.scale)
    B, N, D = dy.shape
    dz = dy * (y > 0) * t.scale if mask_in else dy
    with torch.autocast("cuda", enabled=False):
        da = (dz.reshape(B * N, D) @ W).view(B, N, D)
    return torch.ops.leakgnn.sddmm_cols(rowptr, col, da.transpose(0, 1).reshape(N, B * D),
                                        x.transpose(0, 1).reshape(N, B * D))


def _layer_backward(t: _Trunk, l: int, dy: Tensor, x: Tensor, y: Optional[Tensor], W: Tensor, words: Optional[Tensor],
                    ws: Tensor, *, mask_in: bool, mask_out: bool, scale_out: float, dbias_ns: Optional[Tensor] = None,
                    x0bits: Optional[Tensor] = None, wgrad: Optional[_WGrad] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dW, db) of layer l from dy, ONE fused launch: dz = dy * scale * [f > 0] under mask_in
    (from `words`, else from the layer's output y), dx masked by the input's own ReLU / dropout
    under mask_out and scaled by scale_out.  x: the layer's input (x_l; the norm route's xn_l, no
    ReLU output: scale_out 1.0, no mask_out; under x0bits the compressed node init's sensor rows).
    dbias_ns (layer 0 in front of the node init): the launch also sums dx's non-sensor rows into it
    and writes dx for the sensor rows only (all lg_sensor_proj_bwd reads).  t.skip: dx = dy + the
    branch's (lg_gcn_bwd_nm_skip).  wgrad: the layer's dL/dw is added first (_layer_dw)."""
    lib, B, N, D = t.lib, t.B, t.N, t.D
    flags = ((nat.LG_F_MASK_IN if mask_in else 0) | (nat.LG_F_MASK_OUT if mask_out else 0)
             | (nat.LG_F_BF16 if t.bf16 else 0) | (GCN_BWD_NM_EXTRA_FLAGS if t.node_major and not t.bf16 else 0)
             | (nat.LG_F_DX_SENSOR_ROWS if dbias_ns is not None else 0))
    slot_p, dbias_p = (ptr(t.sensor_slot), ptr(dbias_ns)) if dbias_ns is not None else (None, None)
    dx = torch.empty_like(dy)
    dW, db = torch.empty(D, D, device=t.dev, dtype=torch.float32), torch.empty(D, device=t.dev, dtype=torch.float32)
    if wgrad is not None and wgrad.on:
        wgrad.add(_layer_dw(t, dy, x, y, W, words, mask_in, x0bits, wgrad.rowptr, wgrad.col))
    with _timed("gcn_bwd" if l == t.L - 1 else f"gcn_bwd_l{l}", t.dev):
        if x0bits is not None:
            check(lib.lg_gcn_bwd_nm_x0(ptr(t.nodetab_t), ptr(t.pairs_t), ptr(t.pos_slot_t), ptr(dy), ptr(x), ptr(x0bits),
                                       ptr(t.node_bias), ptr(W), ptr(dx), ptr(dW), ptr(db), slot_p, dbias_p, B, N, t.S,
                                       D, flags | t.drop[0], t.p, t.scale, ptr(ws), ws.numel(), t.st),
                  "lg_gcn_bwd_nm_x0")
        elif t.node_major:
            fn, name = ((lib.lg_gcn_bwd_nm_skip, "lg_gcn_bwd_nm_skip") if t.skip else
                        (lib.lg_gcn_bwd_nm_bits, "lg_gcn_bwd_nm_bits"))
            check(fn(ptr(t.nodetab_t), ptr(t.pairs_t), ptr(dy), ptr(y), ptr(x), ptr(W), ptr(dx), ptr(dW), ptr(db), slot_p,
                     dbias_p, B, N, D, flags, t.scale, scale_out, ptr(ws), ws.numel(), t.st, ptr(words)), name)
        else:
            check(lib.lg_gcn_bwd(ptr(t.rowptr_t), ptr(t.col_t), ptr(t.w_t), ptr(dy), ptr(y), ptr(x), ptr(W), ptr(dx),
                                 ptr(dW), ptr(db), slot_p, dbias_p, B, N, D, t.col_t.numel(), flags, t.scale, scale_out,
                                 ptr(ws), ws.numel(), t.st), "lg_gcn_bwd")
    return dx, dW, db


def _trunk_layer_launches(t: _Trunk, dy: Tensor, xs, ymask: Tensor, weights, x0bits: Optional[Tensor], wgrad: _WGrad,
                          z: Optional[Tensor] = None):
    """The GCN layers' backward of gnn_trunk and encoder_trunk, last first: (dx0, [dW_l], [db_l],
    dbias_ns, workspaces).  dx0: the node init's pre-activation gradient (layer 0's dx: masked by
    the node init's ReLU / dropout; under x0bits the sensor nodes' rows only); dbias_ns: its
    non-sensor rows' sum.  Plain: the last layer masks its output ([x_L > 0], from ymask's bits
    where the forward wrote them), every layer its input.  t.skip: x_{l+1} = x_l + f_l, so
    dx_l = dx_{l+1} + (branch); every layer applies its own mask (LG_F_MASK_IN on its bit words)
    and only layer 0 a LG_F_MASK_OUT, the node init's.  z (t.hops > 0): layer 0's input is the
    diffused z_K, no ReLU output: its launch runs without LG_F_MASK_OUT, node_slot and dnode_bias and
    returns dL/dz in full (_trunk_diffuse_backward applies the node init's mask)."""
    L, D, lib = t.L, t.D, t.lib
    wsb = lib.lg_gcn_bwd_nm_workspace_bytes(D) if t.node_major else lib.lg_gcn_bwd_workspace_bytes(D)
    # one workspace per layer: the layers' slab reductions run together at the batch flush
    wss = [torch.empty(int(wsb), device=t.dev, dtype=torch.uint8) for _ in range(L)]
    dWs, dbs = [dy] * L, [dy] * L
    dbias_ns = torch.empty(D, device=t.dev, dtype=torch.float32)
    for l in range(L - 1, -1, -1):
        last = l == L - 1
        words = (_layer_words(ymask, l, L) if t.skip else  # else [x_L > 0] as bits
                 ymask if (t.node_major and last and ymask.numel() > 0) else None)
        at_z = l == 0 and z is not None
        dy, dWs[l], dbs[l] = _layer_backward(
            t, l, dy, z if at_z else xs[l], None if t.skip else xs[l + 1], weights[l], words, wss[l],
            mask_in=last or t.skip, mask_out=(l == 0 or not t.skip) and not at_z, scale_out=t.scale,
            dbias_ns=dbias_ns if (l == 0 and not at_z) else None,
            x0bits=x0bits if l == 0 else None, wgrad=wgrad)  # dx: already masked by the previous op's relu/dropout
    return dy, dWs, dbs, dbias_ns, wss


def _sensor_proj_backward(t: _Trunk, dy, h_s, proj_weight, sensor_idx, slot_live, dbias_ns, wss):
    """(dh_s, dproj_weight, dnode_bias) from the node init's pre-activation gradient dy (ONE
    lg_sensor_proj_bwd) and the non-sensor rows' bias sum dbias_ns.  The workspace joins wss."""
    lib, dev, B, D = t.lib, t.dev, t.B, t.D
    S, Ds = h_s.shape[1], h_s.shape[2]
    dh_s, dbp = torch.empty(B, S, Ds, device=dev, dtype=torch.float32), torch.empty(D, device=dev, dtype=torch.float32)
    dWp = torch.empty(D, Ds + 1, device=dev, dtype=torch.float32)
    wsp = torch.empty(int(lib.lg_sensor_proj_bwd_workspace_bytes(B, S, Ds, D)), device=dev, dtype=torch.uint8)
    wss.append(wsp)  # held by the caller until the reduce batch is flushed
    with _timed("linear_dw", dev):
        check(lib.lg_sensor_proj_bwd(ptr(dy), ptr(sensor_idx), ptr(slot_live), ptr(h_s), ptr(proj_weight),
                                     ptr(dbias_ns), ptr(dh_s), ptr(dWp), ptr(dbp), B, t.N, S, Ds, D,
                                     nat.LG_F_NODE_MAJOR if t.node_major else 0, ptr(wsp), wsp.numel(), t.st),
              "lg_sensor_proj_bwd")
    return dh_s, dWp, dbp


# ---------------------------------------------------------------------------- output layouts
# An op's output list: (entries, pos), one (shape, dtype) per entry and the named positions, each an index, a
# list of indices or None (the op has no such output).  Sizes default to 0: the positions need L alone.
_F32, _I16 = torch.float32, torch.int16


def _alloc(lay, like: Tensor) -> List[Tensor]:
    return [like.new_empty(shape, dtype=dt) for shape, dt in lay[0]]  # (a fake tensor gives fake ones)


def _gnn_trunk_layout(L, B=0, N=0, S=0, D=0, node_major=True, skip=False, x0c=False, diffuse=False):
    """[x_0, ..., x_L, ymask, x0bits]; x_L is the heads' input.  x0c: x_0 is its sensor rows.
    diffuse (hops > 0): one more entry, z = z_K, layer 0's input (the heads' at L == 0)."""
    act = (N, B, D) if node_major else (B, N, D)
    nmask = mask_words(N, B) if (node_major and L > 0) else 0
    return ([((S, B, D) if x0c else act, _F32)] + [(act, _F32)] * L
            + [((nmask * (L if skip else 1),), _I16), ((nmask if x0c else 0,), _I16)] + [(act, _F32)] * bool(diffuse),
            dict(xs=list(range(L + 1)), xns=None, ymask=L + 1, x0bits=L + 2, h=L if (L or not diffuse) else L + 3,
                 **(dict(z=L + 3) if diffuse else {})))


def _gnn_trunk_norm_layout(L, B=0, N=0, D=0, diffuse=False):
    """[xn_L, x_0 .. x_L, xn_0 .. xn_{L-1}, stats, ymask]; xn_L is the heads' input.  diffuse (hops >
    0): one more entry, z = z_K, the residual stream's start (x_1 = z + f_0; x_0 stays the node init)."""
    return ([((N, B, D), _F32)] * (2 * L + 2) + [((L + 1, N * B, 2), _F32), ((mask_words(N, B) * L,), _I16)]
            + [((N, B, D), _F32)] * bool(diffuse),
            dict(xs=list(range(1, L + 2)), xns=list(range(L + 2, 2 * L + 2)) + [0], ymask=2 * L + 3, x0bits=None, h=0,
                 stats=2 * L + 2, **(dict(z=2 * L + 4) if diffuse else {})))


def _encoder_trunk_layout(L, B=0, N=0, S=0, D=0, Lw=0, H=0, save=False):
    """[x_1, ..., x_L, ymask, xs0, x0bits, h_seq, gates]; x_L is the heads' input.  h_seq / gates: the
    fused GRU pair's saved steps, in 16-sequence blocks (empty unless save)."""
    nmask, rows = mask_words(N, B), _gru_ni_rows(B * S)
    return ([((N, B, D), _F32)] * L + [((nmask,), _I16), ((S, B, D), _F32), ((nmask,), _I16),
                                       ((Lw, rows, H) if save else (0,), _F32), ((Lw, rows, 4, H) if save else (0,), _F32)],
            dict(xs=[L + 1] + list(range(L)), xns=None, ymask=L, x0bits=L + 2, h=L - 1, h_seq=L + 3, gates=L + 4))


# op -> (layout, L of an output count; diffuse: the count includes z)
_LAYOUTS = {"gnn_trunk": (_gnn_trunk_layout, lambda n, diffuse=False: n - 3 - diffuse),
            "gnn_trunk_norm": (_gnn_trunk_norm_layout, lambda n, diffuse=False: (n - 4 - diffuse) // 2),
            "encoder_trunk": (_encoder_trunk_layout, lambda n: n - 5)}


# A trunk op's outputs by name: xs = x_0 .. x_L (x_0 its sensor rows where x0bits is non-empty), xns =
# xn_0 .. xn_L (gnn_trunk_norm), the mask words, h = the heads' input; then the ops' own.  None: no such output.
# z: the diffused node init z_K (gnn_trunk / gnn_trunk_norm with hops > 0).
TrunkOut = namedtuple("TrunkOut", "xs xns ymask x0bits h stats h_seq gates z", defaults=(None, None, None, None))


def _positions(op: str, n_out: int, diffuse: bool = False) -> Dict[str, object]:  # (no cache: torch.compile traces through here)
    layout, layers = _LAYOUTS[op]
    return layout(layers(n_out, True), diffuse=True)[1] if diffuse else layout(layers(n_out))[1]


def trunk_fields(op: str, out, diffuse: bool = False) -> TrunkOut:
    """The flat output list of leakgnn::<op> (gnn_trunk, gnn_trunk_norm, encoder_trunk) by name.
    diffuse: the op ran with hops > 0 (the list ends in z)."""
    return TrunkOut(**{k: None if i is None else out[i] if isinstance(i, int) else [out[j] for j in i]
                       for k, i in _positions(op, len(out), diffuse).items()})


# ---------------------------------------------------------------------------- autograd glue
def _save_named(ctx, **named) -> None:
    """save_for_backward of a mapping name -> tensor, tensor list or None; names, list lengths and
    the None entries are recorded on ctx (a missing optional tensor saves nothing)."""
    runs = {k: [] if v is None else [v] if isinstance(v, Tensor) else list(v) for k, v in named.items()}
    ctx.saved_spec = tuple((k, None if v is None else -1 if isinstance(v, Tensor) else len(runs[k]))
                           for k, v in named.items())  # (name, None | -1: a tensor | list length)
    ctx.save_for_backward(*(t for run in runs.values() for t in run))


def _saved_named(ctx) -> Dict[str, object]:
    """The mapping _save_named was given, from ctx.saved_tensors."""
    spec = ctx.saved_spec
    runs = _split(ctx.saved_tensors, *(0 if n is None else 1 if n < 0 else n for _, n in spec))
    return {name: None if n is None else run[0] if n < 0 else run for (name, n), run in zip(spec, runs)}


@functools.lru_cache(maxsize=None)
def _positional(op) -> Tuple[Tuple[str, ...], tuple]:
    """(names, defaults) of a custom op's positional parameters (autograd sees no keyword-only one)."""
    ps = [q for q in inspect.signature(op._init_fn).parameters.values() if q.kind is not q.KEYWORD_ONLY]
    return tuple(q.name for q in ps), tuple(q.default for q in ps)


def _args_seen(op, inputs) -> int:
    """How many of `inputs` autograd saw: the dispatcher drops trailing arguments that equal
    their defaults before autograd sees them, and the backward returns one entry per argument
    it saw."""
    _, defaults = _positional(op)
    n = len(inputs)
    while n > 0 and defaults[n - 1] is not inspect.Parameter.empty and not isinstance(inputs[n - 1], Tensor) \
            and inputs[n - 1] == defaults[n - 1]:
        n -= 1
    return n


def _named_grads(op, n_seen: int, **grads) -> tuple:
    """A backward's return tuple: grads[name] at each of op's first n_seen parameters, None elsewhere."""
    names = _positional(op)[0]
    unknown = sorted(set(grads) - set(names))
    if unknown:
        raise KeyError(f"{op._qualname}: no parameter named {unknown}")
    return tuple(grads.get(name) for name in names[:n_seen])


def _trunk_ctx(ctx, op, inputs, output, hops: int = 0) -> Tuple[Dict[str, object], TrunkOut]:
    """The trunk ops' setup_context in common; returns (inputs by name, outputs by name).  Sets ctx.w_grad, ctx.n_in
    and ctx.h: the position of the heads' input, the one differentiable output (the rest serve the backward)."""
    a, name = dict(zip(_positional(op)[0], inputs)), op._qualname.split("::")[1]
    # learned edge weights (requires_grad, not needs_input_grad: that tuple is flat over the tensor lists here)
    ctx.w_grad = a["edge_w"] is not None and a["edge_w"].requires_grad
    ctx.n_in = _args_seen(op, inputs)
    if ctx.w_grad and hops > 0:
        raise NotImplementedError(f"{name}: the gradient of edge_w through the diffusion hops is not built "
                                  "(it would need every z_k saved): hops > 0 takes fixed edge weights only")
    ctx.h = _positions(name, len(output), hops > 0)["h"]
    ctx.mark_non_differentiable(*(o for i, o in enumerate(output) if i != ctx.h))
    ctx.set_materialize_grads(False)  # their gradients would be zero-filled (B, N, D) tensors
    return a, trunk_fields(name, output, hops > 0)


# ============================================================================ gnn_trunk
def _compress_x0(nodetab_s: Optional[Tensor], node_major: bool, L: int) -> bool:
    """Whether gnn_trunk keeps x_0 compressed (sensor rows + [x_0 > 0] bits).  Needs a layer
    after layer 0 (L >= 2): the last layer's backward reads its input mask through
    LG_F_MASK_IN, which the x0 backward has no form of (lg_gcn_bwd_nm_x0 returns
    LG_EUNSUPPORTED), so at L == 1 the dense node init runs.  A trunk-forward flag that selects
    another forward kernel (LG_F_NM3, LG_F_F32_MFMA: the A/B and exact-fp32 modes) has no x0
    variant either; it also gets the dense node init, so the flag applies to every layer."""
    other = GCN_FWD_NM_EXTRA_FLAGS & (nat.LG_F_NM3 | nat.LG_F_F32_MFMA)
    return nodetab_s is not None and node_major and L > 1 and not other


@torch.library.custom_op(f"{NS}::gnn_trunk", mutates_args=(), device_types="cuda")
def gnn_trunk(h_s: Tensor, proj_weight: Tensor, node_bias: Tensor, weights: List[Tensor], biases: List[Tensor],
              sensor_slot: Tensor, sensor_idx: Tensor, nonsensor_idx: Tensor, slot_live: Optional[Tensor],
              nodetab: Tensor, pairs: Tensor, rowptr: Tensor, col: Tensor, w: Tensor, nodetab_t: Tensor,
              pairs_t: Tensor, rowptr_t: Tensor, col_t: Tensor, w_t: Tensor, p: float, node_major: bool, seed: Tensor,
              nodetab_s: Optional[Tensor], pairs_s: Optional[Tensor], pos_slot_t: Optional[Tensor],
              edge_w: Optional[Tensor] = None, *, bf16: bool = False, skip: bool = False, hops: int = 0,
              alpha: float = 0.0) -> List[Tensor]:
    """[x_0, ..., x_L, ymask, x0bits]: sensor_to_node + node init (detector.py:160, 178-190),
    then L x dropout(relu(GCNConv)).

      x_0     = dropout(relu(slot >= 0 ? [h_s[b, slot], 1] W^T + b : b))   (lg_node_init_proj_fwd)
      x_{l+1} = dropout(relu(Ahat x_l W_l^T + b_l))                        (lg_gcn_fwd[_nm], fused)
    h_s: (B, S, Ds) sensor encodings; proj_weight: sensor_to_node.weight (D, Ds + 1);
    node_bias: its bias.  The projection is formed inside the node-init launch (no GEMM, no
    proj buffer).  node_major: features [N][B][D] (lg_gcn_fwd_nm), else [B][N][D].  p:
    dropout prob (0 = eval).  Every activation is returned: the backward reads its
    ReLU/dropout masks back as [x > 0] and needs x_l for dW.  ymask (node-major only, int16
    (mask_words(N, B),), else empty): [x_L > 0] as bits (lg_gcn_fwd_nm_bits), which the
    last layer's backward reads instead of gathering x_L.
    bf16: the node-major transform as one bf16 MFMA product (LG_F_BF16, the configs[2] tier).
    nodetab_s, pairs_s, pos_slot_t (ops.SensorMarks; node-major, L >= 1): x_0 stays
    compressed (lg_node_init_bits_fwd): the returned x_0 is its sensor rows (S, B, D), x0bits
    [x_0 > 0] of every row (int16, ymask's layout), and layer 0 reads them through the marked
    table (lg_gcn_fwd_nm_x0: the dense forward up to the order of its sums).  Otherwise x0bits is empty.
    edge_w: the graph's normalised coefficients `w` carrying an autograd edge (learned edge
    weights, leakgnn::gcn_edge_norm), or None.  An autograd anchor only: the kernels read the
    tables, which hold the same numbers; when it requires grad the backward returns dL/dw
    (_layer_dw: lg_sddmm_nm per layer).
    skip (keyword-only: the dispatcher drops positional defaults): identity skips,
      x_{l+1} = x_l + dropout(relu(Ahat x_l W_l^T + b_l))                  (lg_gcn_fwd_nm_skip)
    on the node-major fp32 tier with the dense node init.  [x_{l+1} > 0] is then no longer the
    branch's ReLU/dropout mask, so EVERY layer keeps its [f > 0] bits: ymask is (L * nmask,),
    layer l's words at [l * nmask, (l + 1) * nmask) (each 1/32 of an activation).
    hops, alpha (keyword-only, as skip): hops > 0 puts leakgnn::diffuse's stage between the node init
    and layer 0, z = z_hops of x_0 (lg_diffuse_fwd), on the node-major fp32 tier with the dense node
    init; the list gains z as its last entry, layer 0's input (the heads' at L == 0).  hops == 0:
    the layout, the saved state and the launches are the op's without the keywords."""
    lib = load_library()
    h_s, proj_weight, node_bias = _c(h_s), _c(proj_weight), _c(node_bias)
    weights, biases = [_c(t) for t in weights], [_c(t) for t in biases]
    _req(h_s, proj_weight, node_bias, *weights, *biases)
    B, S, Ds = h_s.shape
    D = proj_weight.shape[0]
    _check_d(D)
    if bf16 and not node_major:  # the window-major kernels have no bf16 form (ops.use_node_major)
        raise ValueError("gnn_trunk: the bf16 tier runs on the node-major layout only")
    if skip and (bf16 or not node_major):
        raise ValueError("gnn_trunk: skip=True runs on the node-major fp32 tier only")
    _check_trunk_diffuse("gnn_trunk", hops, alpha, node_major, bf16)
    if tuple(proj_weight.shape) != (D, Ds + 1):
        raise ValueError(f"proj_weight must be (D, Ds + 1) = ({D}, {Ds + 1}), got {tuple(proj_weight.shape)}")
    N, L = sensor_slot.shape[0], len(weights)
    x0c = _compress_x0(nodetab_s, node_major, L) and not skip and not hops
    t = _trunk(lib, h_s, B, N, S, D, L, p, seed, node_major=node_major, bf16=bf16, skip=skip, nnz=col.numel(),
               nodetab=nodetab, pairs=pairs, rowptr=rowptr, col=col, w=w, nodetab_s=nodetab_s, pairs_s=pairs_s,
               node_bias=node_bias, hops=hops, alpha=alpha)
    dflag, seed_v, sbit = t.drop
    out = _alloc(_gnn_trunk_layout(L, B, N, S, D, node_major, skip, x0c, hops > 0), h_s)
    f = trunk_fields("gnn_trunk", out, hops > 0)
    with _timed("node_init", t.dev):
        if x0c:
            check(lib.lg_node_init_bits_fwd(ptr(sensor_slot), ptr(sensor_idx), ptr(h_s), ptr(proj_weight),
                                            ptr(node_bias), ptr(f.xs[0]), ptr(f.x0bits), B, N, S, Ds, D, dflag, p,
                                            seed_v, 0 | sbit, t.st), "lg_node_init_bits_fwd")
        else:
            check(lib.lg_node_init_proj_fwd(ptr(sensor_slot), ptr(sensor_idx), ptr(h_s), ptr(proj_weight),
                                            ptr(node_bias), ptr(f.xs[0]), B, N, S, Ds, D,
                                            dflag | (nat.LG_F_NODE_MAJOR if node_major else 0), p, seed_v, 0 | sbit,
                                            t.st), "lg_node_init_proj_fwd")
    if hops:
        _trunk_diffuse_forward(t, f.xs[0], f.z)
    for l, (W, b) in enumerate(zip(weights, biases)):
        words = _layer_words(f.ymask, l, L) if skip else f.ymask if (node_major and l == L - 1) else None
        _layer_forward(t, l, f.z if (hops and l == 0) else f.xs[l], W, b, f.xs[l + 1], words,
                       x0bits=f.x0bits if (x0c and l == 0) else None, branch=skip)
    return out


@gnn_trunk.register_fake
def _(h_s, proj_weight, node_bias, weights, biases, sensor_slot, sensor_idx, nonsensor_idx, slot_live, nodetab, pairs,
      rowptr, col, w, nodetab_t, pairs_t, rowptr_t, col_t, w_t, p, node_major, seed, nodetab_s, pairs_s, pos_slot_t,
      edge_w=None, *, bf16=False, skip=False, hops=0, alpha=0.0):
    L = len(weights)
    x0c = _compress_x0(nodetab_s, node_major, L) and not skip and not hops
    return _alloc(_gnn_trunk_layout(L, h_s.shape[0], sensor_slot.shape[0], h_s.shape[1], proj_weight.shape[0],
                                    node_major, skip, x0c, hops > 0), h_s)


@torch.library.custom_op(f"{NS}::gnn_trunk_backward", mutates_args=(), device_types="cuda")
def gnn_trunk_backward(grad_out: Tensor, xs: List[Tensor], ymask: Tensor, h_s: Tensor, proj_weight: Tensor,
                       weights: List[Tensor],
                       sensor_slot: Tensor, sensor_idx: Tensor, nonsensor_idx: Tensor, slot_live: Optional[Tensor],
                       nodetab_t: Tensor, pairs_t: Tensor, rowptr_t: Tensor, col_t: Tensor, w_t: Tensor, p: float,
                       node_major: bool, x0bits: Optional[Tensor], x0_bias: Optional[Tensor],
                       pos_slot_t: Optional[Tensor], rowptr: Optional[Tensor] = None, col: Optional[Tensor] = None,
                       z: Optional[Tensor] = None, *, bf16: bool = False, skip: bool = False, hops: int = 0,
                       alpha: float = 0.0) -> Tuple[Tensor, Tensor, Tensor, List[Tensor], List[Tensor], Tensor]:
    """(dh_s, dproj_weight, dnode_bias, [dW_l], [db_l], dw): one fused lg_gcn_bwd[_nm] per layer,
    last first (ReLU/dropout masks of a layer's output and input applied inside the kernel
    from the saved activations; the non-sensor rows' node-bias gradient summed inside layer
    0's launch), then ONE lg_sensor_proj_bwd for the projection (gather of the sensor rows,
    dh_s, dW and the full bias gradient).  x0bits, x0_bias (the node init's bias), pos_slot_t: x_0 is
    compressed (gnn_trunk's x0marks path; xs[0] its sensor rows) and layer 0's backward reads
    it through lg_gcn_bwd_nm_x0.  rowptr, col (the FORWARD CSR): the edge coefficients learn, and
    dw is dL/dw over its slots (sum over the layers of _layer_dw); otherwise dw is empty.
    skip: gnn_trunk's identity skips (lg_gcn_bwd_nm_skip per layer, every layer's mask from its own
    words of ymask).  z, hops, alpha: gnn_trunk's diffusion stage (z = z_hops, layer 0's input): layer 0
    returns dL/dz unmasked, then ONE lg_diffuse_bwd runs the adjoint hops and applies the node init's
    mask from xs[0]; the non-sensor rows' bias sum is the torch expression of L == 0."""
    lib = load_library()
    L = len(weights)
    N, B, D = xs[-1].shape if node_major else xs[0].transpose(0, 1).shape
    t = _trunk(lib, grad_out, B, N, h_s.shape[1], D, L, p, node_major=node_major, bf16=bf16, skip=skip,
               nodetab_t=nodetab_t, pairs_t=pairs_t, rowptr_t=rowptr_t, col_t=col_t, w_t=w_t, pos_slot_t=pos_slot_t,
               sensor_slot=sensor_slot, node_bias=x0_bias, hops=hops, alpha=alpha)
    wgrad = _WGrad(rowptr, col)
    with _reduce_batch(lib, t.st):
        dy, dWs, dbs, dbias_ns, wss = _trunk_layer_launches(t, grad_out.contiguous(), xs, ymask, weights, x0bits, wgrad,
                                                            z if hops else None)
        if hops:
            dy, dbias_ns = _trunk_diffuse_backward(t, dy, xs[0], nonsensor_idx)
        elif L == 0:  # no layer-0 launch applied the node init's relu/dropout mask
            dy = dy * (xs[0] > 0) * t.scale
            dbias_ns = dy.index_select(0 if node_major else 1, nonsensor_idx).sum(dim=(0, 1))
        dh_s, dWp, dbp = _sensor_proj_backward(t, dy, h_s, proj_weight, sensor_idx, slot_live, dbias_ns, wss)
    return dh_s, dWp, dbp, dWs, dbs, wgrad.total(t.dev)


@gnn_trunk_backward.register_fake
def _(grad_out, xs, ymask, h_s, proj_weight, weights, sensor_slot, sensor_idx, nonsensor_idx, slot_live, nodetab_t,
      pairs_t, rowptr_t, col_t, w_t, p, node_major, x0bits, x0_bias, pos_slot_t, rowptr=None, col=None, z=None, *,
      bf16=False, skip=False, hops=0, alpha=0.0):
    D = proj_weight.shape[0]
    return (torch.empty_like(h_s), torch.empty_like(proj_weight), grad_out.new_empty(D),
            [torch.empty_like(t) for t in weights], [grad_out.new_empty(D) for _ in weights],
            grad_out.new_empty(col.shape[0] if col is not None else 0))


def _trunk_setup(ctx, inputs, keyword_only_inputs, output):
    hops, alpha = int(keyword_only_inputs.get("hops", 0)), float(keyword_only_inputs.get("alpha", 0.0))
    a, f = _trunk_ctx(ctx, gnn_trunk, inputs, output, hops)
    bf16, skip = bool(keyword_only_inputs.get("bf16", False)), bool(keyword_only_inputs.get("skip", False))
    if ctx.w_grad and bf16:
        raise NotImplementedError("gnn_trunk: the gradient of edge_w exists on the fp32 tier only")
    x0c = f.x0bits.numel() > 0  # x_0 compressed
    ctx.kw = dict(p=a["p"], node_major=a["node_major"], bf16=bf16, skip=skip,
                  **(dict(hops=hops, alpha=alpha) if hops else {}))
    # x_0 .. x_L and ymask as returned; the arguments of gnn_trunk_backward by name
    _save_named(ctx, xs=f.xs, ymask=f.ymask, **(dict(z=f.z) if hops else {}),
                rowptr=a["rowptr"] if ctx.w_grad else None,
                col=a["col"] if ctx.w_grad else None, x0bits=f.x0bits if x0c else None,
                x0_bias=a["node_bias"] if x0c else None, pos_slot_t=a["pos_slot_t"] if x0c else None,
                **{k: a[k] for k in ("h_s", "proj_weight", "weights", "sensor_slot", "sensor_idx", "nonsensor_idx",
                                     "slot_live", "nodetab_t", "pairs_t", "rowptr_t", "col_t", "w_t")})


def _trunk_bwd(ctx, grads):
    g = grads[ctx.h]
    if g is None:
        return _named_grads(gnn_trunk, ctx.n_in)
    dh_s, dWp, dbp, dWs, dbs, dw = torch.ops.leakgnn.gnn_trunk_backward(g, **_saved_named(ctx), **ctx.kw)
    return _named_grads(gnn_trunk, ctx.n_in, h_s=dh_s, proj_weight=dWp, node_bias=dbp, weights=dWs, biases=dbs,
                        edge_w=dw if ctx.w_grad else None)


gnn_trunk.register_autograd(_trunk_bwd, setup_context=_trunk_setup)


# ============================================================================ gnn_trunk_norm
# The pre-norm residual trunk (LeakDetector(skip="residual", norm="layer")): a LayerNorm in front
# of every branch and one in front of the heads,
#   xn_l = LN_l(x_l),  f_l = dropout(relu(Ahat xn_l W_l^T + b_l)),  x_{l+1} = x_l + f_l,  out = xn_L.
# Node-major, fp32 tier, dense node init.  The branch is the plain layer's kernel on a signed input
# (lg_gcn_fwd_nm_bits, every layer's [f > 0] bits kept); the skip's add and the next norm are one
# launch (lg_add_layernorm_fwd).  An op pair of its own: gnn_trunk's return layout stays as it is.
LN_EPS = 1e-5  # nn.LayerNorm's default


def _ln_fwd(lib, x, f, gamma, beta, xsum, xn, stats, eps, st):
    check(lib.lg_add_layernorm_fwd(ptr(x), ptr(f), ptr(gamma), ptr(beta), ptr(xsum), ptr(xn), ptr(stats),
                                   x.numel() // x.shape[-1], x.shape[-1], eps, st), "lg_add_layernorm_fwd")


@torch.library.custom_op(f"{NS}::gnn_trunk_norm", mutates_args=(), device_types="cuda")
def gnn_trunk_norm(h_s: Tensor, proj_weight: Tensor, node_bias: Tensor, weights: List[Tensor], biases: List[Tensor],
                   gammas: List[Tensor], betas: List[Tensor], sensor_slot: Tensor, sensor_idx: Tensor,
                   nonsensor_idx: Tensor, slot_live: Optional[Tensor], nodetab: Tensor, pairs: Tensor, rowptr: Tensor,
                   col: Tensor, nodetab_t: Tensor, pairs_t: Tensor, p: float, eps: float, seed: Tensor,
                   edge_w: Optional[Tensor] = None, *, hops: int = 0, alpha: float = 0.0) -> List[Tensor]:
    """[xn_L, x_0 .. x_L, xn_0 .. xn_{L-1}, stats, ymask], all node-major (N, B, D).
    xn_L (the heads' input) is the one differentiable output.  x_l: the residual stream; xn_l: the
    branches' inputs; stats (L + 1, N * B, 2): every norm's (mean, rstd); ymask (L * nmask,) int16:
    layer l's [f_l > 0] words at [l * nmask, (l + 1) * nmask) (gnn_trunk's layout under skip).
    gammas, betas: the L + 1 norms' weight and bias.  The backward keeps x_l AND xn_l per layer,
    two activations where the skip keeps one.  edge_w: gnn_trunk's autograd anchor.
    hops, alpha (keyword-only): gnn_trunk's diffusion stage; the list gains z = z_hops of x_0 as its
    last entry, the residual stream's start (xn_0 = LN_0(z), x_1 = z + f_0; x_0 stays the node init)."""
    lib = load_library()
    h_s, proj_weight, node_bias = _c(h_s), _c(proj_weight), _c(node_bias)
    weights, biases = [_c(t) for t in weights], [_c(t) for t in biases]
    gammas, betas = [_c(t) for t in gammas], [_c(t) for t in betas]
    _req(h_s, proj_weight, node_bias, *weights, *biases, *gammas, *betas)
    B, S, Ds = h_s.shape
    D = proj_weight.shape[0]
    _check_d(D)
    L = len(weights)
    if len(biases) != L or len(gammas) != L + 1 or len(betas) != L + 1:
        raise ValueError(f"gnn_trunk_norm: {L} layers need {L} biases and {L + 1} norms, got {len(biases)}, "
                         f"{len(gammas)} and {len(betas)}")
    if any(tuple(t.shape) != (D,) for t in gammas + betas):
        raise ValueError(f"gnn_trunk_norm: every norm's weight and bias must be ({D},)")
    if tuple(proj_weight.shape) != (D, Ds + 1):
        raise ValueError(f"proj_weight must be (D, Ds + 1) = ({D}, {Ds + 1}), got {tuple(proj_weight.shape)}")
    _check_trunk_diffuse("gnn_trunk_norm", hops, alpha)
    N = sensor_slot.shape[0]
    t = _trunk(lib, h_s, B, N, S, D, L, p, seed, nnz=col.numel(), nodetab=nodetab, pairs=pairs, hops=hops, alpha=alpha)
    dev, st, (dflag, seed_v, sbit) = t.dev, t.st, t.drop
    out = _alloc(_gnn_trunk_norm_layout(L, B, N, D, hops > 0), h_s)
    f = trunk_fields("gnn_trunk_norm", out, hops > 0)
    xs, xns, stats = f.xs, f.xns, f.stats
    with _timed("node_init", dev):
        check(lib.lg_node_init_proj_fwd(ptr(sensor_slot), ptr(sensor_idx), ptr(h_s), ptr(proj_weight), ptr(node_bias),
                                        ptr(xs[0]), B, N, S, Ds, D, dflag | nat.LG_F_NODE_MAJOR, p, seed_v, 0 | sbit, st),
              "lg_node_init_proj_fwd")
    if hops:
        _trunk_diffuse_forward(t, xs[0], f.z)
    stream = [f.z if hops else xs[0]] + xs[1:]  # the residual stream: it starts at z_K under hops
    with _timed("layernorm_fwd", dev):
        _ln_fwd(lib, stream[0], None, gammas[0], betas[0], None, xns[0], stats[0], eps, st)
    for l, (W, b) in enumerate(zip(weights, biases)):
        fl = torch.empty((N, B, D), device=dev, dtype=torch.float32)  # the branch's output, a temporary
        _layer_forward(t, l, xns[l], W, b, fl, _layer_words(f.ymask, l, L), branch=True)
        with _timed("layernorm_fwd", dev):
            _ln_fwd(lib, stream[l], fl, gammas[l + 1], betas[l + 1], xs[l + 1], xns[l + 1], stats[l + 1], eps, st)
    return out


@gnn_trunk_norm.register_fake
def _(h_s, proj_weight, node_bias, weights, biases, gammas, betas, sensor_slot, sensor_idx, nonsensor_idx, slot_live,
      nodetab, pairs, rowptr, col, nodetab_t, pairs_t, p, eps, seed, edge_w=None, *, hops=0, alpha=0.0):
    return _alloc(_gnn_trunk_norm_layout(len(weights), h_s.shape[0], sensor_slot.shape[0], proj_weight.shape[0],
                                         hops > 0), h_s)


@torch.library.custom_op(f"{NS}::gnn_trunk_norm_backward", mutates_args=(), device_types="cuda")
def gnn_trunk_norm_backward(grad_out: Tensor, xs: List[Tensor], xns: List[Tensor], stats: Tensor, ymask: Tensor,
                            h_s: Tensor, proj_weight: Tensor, weights: List[Tensor], gammas: List[Tensor],
                            sensor_slot: Tensor, sensor_idx: Tensor, nonsensor_idx: Tensor,
                            slot_live: Optional[Tensor], nodetab_t: Tensor, pairs_t: Tensor, p: float,
                            rowptr: Optional[Tensor] = None, col: Optional[Tensor] = None, z: Optional[Tensor] = None,
                            *, hops: int = 0, alpha: float = 0.0
                            ) -> Tuple[Tensor, Tensor, Tensor, List[Tensor], List[Tensor], List[Tensor], List[Tensor],
                                       Tensor]:
    """(dh_s, dproj_weight, dnode_bias, [dW_l], [db_l], [dgamma_l], [dbeta_l], dw).  With s = 1/(1-p)
    and a_l = dL/dx_l (which is also dL/df_{l-1}):
      a_L   = LNbwd_L(grad_out)
      dxn_l = (Ahat^T (a_{l+1} * s * [f_l > 0])) W_l, dW_l, db_l   lg_gcn_bwd_nm_bits, LG_F_MASK_IN on
                                                                  the layer's words, input xn_l
      a_l   = LNbwd_l(dxn_l) + a_{l+1}                             lg_layernorm_bwd with the carry
    and the entry norm's call applies the node init's mask (LG_F_MASK_OUT: a_0 * s * [x_0 > 0]).
    xs: x_0 .. x_L, xns: xn_0 .. xn_{L-1}.  rowptr, col (the forward CSR): the edge coefficients
    learn; layer l's share is lg_sddmm_nm on (a_{l+1}, xn_l, the layer's words).
    z, hops, alpha: the diffusion stage (the entry norm read z = z_hops): its lg_layernorm_bwd runs
    without the mask and returns dL/dz, then ONE lg_diffuse_bwd runs the adjoint hops and applies the
    node init's mask from xs[0]."""
    lib = load_library()
    L = len(weights)
    N, B, D = xs[0].shape
    t = _trunk(lib, grad_out, B, N, h_s.shape[1], D, L, p, nodetab_t=nodetab_t, pairs_t=pairs_t, hops=hops,
               alpha=alpha)
    x0 = xs[0]
    if hops:
        xs = [z] + list(xs[1:])  # the norms' inputs: the stream starts at z
    dev, st, scale, rows = t.dev, t.st, t.scale, N * B
    wgrad = _WGrad(rowptr, col)
    lnb, gcb = int(lib.lg_layernorm_bwd_workspace_bytes(D)), int(lib.lg_gcn_bwd_nm_workspace_bytes(D))
    wss: List[Tensor] = []  # every workspace lives until the reduce batch is flushed

    def ws(nbytes):
        wss.append(torch.empty(nbytes, device=dev, dtype=torch.uint8))
        return wss[-1]

    def ln_bwd(l, dxn, carry):
        dx = torch.empty((N, B, D), device=dev, dtype=torch.float32)
        dg, dbt = torch.empty(D, device=dev, dtype=torch.float32), torch.empty(D, device=dev, dtype=torch.float32)
        w = ws(lnb)
        with _timed("layernorm_bwd", dev):
            check(lib.lg_layernorm_bwd(ptr(dxn), ptr(xs[l]), ptr(stats[l]), ptr(gammas[l]), ptr(carry), ptr(dx), ptr(dg),
                                       ptr(dbt), rows, D, nat.LG_F_MASK_OUT if (l == 0 and not hops) else 0, scale,
                                       ptr(w), w.numel(),
                                       st), "lg_layernorm_bwd")
        dgs[l], dbts[l] = dg, dbt
        return dx

    dWs, dbs, dgs, dbts = ([grad_out] * n for n in (L, L, L + 1, L + 1))
    with _reduce_batch(lib, st):
        a = ln_bwd(L, grad_out.contiguous(), None)
        for l in range(L - 1, -1, -1):
            # the branch's input xn_l is a norm's output, not a ReLU's: no mask_out, no rescale of dxn
            dxn, dWs[l], dbs[l] = _layer_backward(t, l, a, xns[l], None, weights[l], _layer_words(ymask, l, L), ws(gcb),
                                                  mask_in=True, mask_out=False, scale_out=1.0, wgrad=wgrad)
            a = ln_bwd(l, dxn, a)
        # a: the node init's pre-activation gradient; its non-sensor rows' sum is the bias's share
        if hops:
            a, dbias_ns = _trunk_diffuse_backward(t, a, x0, nonsensor_idx)
        else:
            dbias_ns = a.index_select(0, nonsensor_idx).sum(dim=(0, 1))
        dh_s, dWp, dbp = _sensor_proj_backward(t, a, h_s, proj_weight, sensor_idx, slot_live, dbias_ns, wss)
    return dh_s, dWp, dbp, dWs, dbs, dgs, dbts, wgrad.total(dev)


@gnn_trunk_norm_backward.register_fake
def _(grad_out, xs, xns, stats, ymask, h_s, proj_weight, weights, gammas, sensor_slot, sensor_idx, nonsensor_idx,
      slot_live, nodetab_t, pairs_t, p, rowptr=None, col=None, z=None, *, hops=0, alpha=0.0):
    D = proj_weight.shape[0]
    return (torch.empty_like(h_s), torch.empty_like(proj_weight), grad_out.new_empty(D),
            [torch.empty_like(t) for t in weights], [grad_out.new_empty(D) for _ in weights],
            [torch.empty_like(t) for t in gammas], [torch.empty_like(t) for t in gammas],
            grad_out.new_empty(col.shape[0] if col is not None else 0))


def _trunk_norm_setup(ctx, inputs, keyword_only_inputs, output):
    hops, alpha = int(keyword_only_inputs.get("hops", 0)), float(keyword_only_inputs.get("alpha", 0.0))
    a, f = _trunk_ctx(ctx, gnn_trunk_norm, inputs, output, hops)
    ctx.kw = dict(p=a["p"], **(dict(hops=hops, alpha=alpha) if hops else {}))
    # the arguments of gnn_trunk_norm_backward by name (xns: xn_0 .. xn_{L-1}, the branches' inputs)
    _save_named(ctx, xs=f.xs, xns=f.xns[:-1], stats=f.stats, ymask=f.ymask, **(dict(z=f.z) if hops else {}),
                rowptr=a["rowptr"] if ctx.w_grad else None, col=a["col"] if ctx.w_grad else None,
                **{k: a[k] for k in ("h_s", "proj_weight", "weights", "gammas", "sensor_slot", "sensor_idx",
                                     "nonsensor_idx", "slot_live", "nodetab_t", "pairs_t")})


def _trunk_norm_bwd(ctx, grads):
    g = grads[ctx.h]
    if g is None:
        return _named_grads(gnn_trunk_norm, ctx.n_in)
    dh_s, dWp, dbp, dWs, dbs, dgs, dbts, dw = torch.ops.leakgnn.gnn_trunk_norm_backward(
        g, **_saved_named(ctx), **ctx.kw)
    return _named_grads(gnn_trunk_norm, ctx.n_in, h_s=dh_s, proj_weight=dWp, node_bias=dbp, weights=dWs, biases=dbs,
                        gammas=dgs, betas=dbts, edge_w=dw if ctx.w_grad else None)


gnn_trunk_norm.register_autograd(_trunk_norm_bwd, setup_context=_trunk_norm_setup)


# ============================================================================ encoder_trunk
# The sensor encoder, the node init and the GCN layers as ONE registered op (the node-major
# trunk with the compressed node init): the GRU's training forward forms the node init's
# sensor rows and [x0 > 0] words in its epilogue (lg_gru_node_init_fwd), and the backward runs
# the layers, then the GRU with the sensor projection's backward in its prologue / epilogue
# (lg_gru_node_init_bwd), all weight-gradient reductions in one launch.  Against gru_encoder +
# gnn_trunk: the node-init launch and the projection-backward launch leave the step, and the
# trunk's and the GRU's reductions share one launch.  Same arithmetic, bit for bit
# (tests/test_gpu_x0.py::test_encoder_trunk_equals_separate_ops).
def encoder_trunk_supported(B: int, N: int, H: int, D: int, L: int, node_major: bool, compress: bool) -> bool:
    """The fused op's case: node-major layout, the compressed node init (L >= 2, no alternate
    forward-kernel flag), node_hidden == sensor_hidden in {32, 64}."""
    return (node_major and compress and H == D and D in (32, 64)
            and _compress_x0(torch.empty(0), node_major, L))


def _gru_ni_rows(nseq: int) -> int:
    """Rows per step of lg_gru_node_init_fwd's h_seq / gates: the sequences rounded up to whole
    16-sequence blocks (include/leakgnn.h)."""
    return 16 * ((nseq + 15) // 16)


@torch.library.custom_op(f"{NS}::encoder_trunk", mutates_args=(), device_types="cuda")
def encoder_trunk(residual: Tensor, tfeat: Optional[Tensor], w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor,
                  proj_weight: Tensor, node_bias: Tensor, weights: List[Tensor], biases: List[Tensor],
                  sensor_slot: Tensor, sensor_idx: Tensor, slot_live: Optional[Tensor], nodetab: Tensor, pairs: Tensor,
                  nodetab_t: Tensor, pairs_t: Tensor, nodetab_s: Tensor, pairs_s: Tensor, pos_slot_t: Tensor, p: float,
                  seed: Tensor, save: bool, edge_w: Optional[Tensor] = None, rowptr: Optional[Tensor] = None,
                  col: Optional[Tensor] = None, *, bf16: bool = False) -> List[Tensor]:
    """[x_1, ..., x_L, ymask, xs0, x0bits, h_seq, gates]: SharedSensorGRUEncoder (detector.py:60-73),
    the node init (:179-190: h0, the mask column, sensor_to_node, ReLU, dropout) and L x
    dropout(relu(GCNConv)) (:198-201) on the node-major layout [N][B][D].  x_0 stays
    compressed: xs0 (S, B, D) its sensor rows, x0bits [x_0 > 0] of the other rows.  ymask: x_L's
    [x > 0] bits.  h_seq / gates: the GRU's saved steps (empty unless save).  residual and tfeat
    are data (no gradient).  edge_w: gnn_trunk's autograd anchor of learned edge coefficients,
    with the forward CSR rowptr / col its backward walks (all three None otherwise)."""
    lib = load_library()
    residual, tfeat = _c(residual), _c(tfeat)
    w_ih, w_hh, b_ih, b_hh, proj_weight, node_bias = (_c(t) for t in (w_ih, w_hh, b_ih, b_hh, proj_weight, node_bias))
    weights, biases = [_c(t) for t in weights], [_c(t) for t in biases]
    _req(residual, tfeat, w_ih, w_hh, b_ih, b_hh, proj_weight, node_bias, *weights, *biases)
    B, Lw, S = residual.shape
    I, H, D, N, L = w_ih.shape[1], w_hh.shape[1], proj_weight.shape[0], sensor_slot.shape[0], len(weights)
    if not encoder_trunk_supported(B, N, H, D, L, True, True):
        raise NotImplementedError("encoder_trunk: node-major trunk with the compressed node init, "
                                  "node_hidden == sensor_hidden in {32, 64}, at least two layers")
    if tuple(proj_weight.shape) != (D, H + 1):
        raise ValueError(f"proj_weight must be ({D}, {H + 1}), got {tuple(proj_weight.shape)}")
    t = _trunk(lib, residual, B, N, S, D, L, p, seed, bf16=bf16, nnz=pairs.shape[0], nodetab=nodetab, pairs=pairs,
               nodetab_s=nodetab_s, pairs_s=pairs_s, node_bias=node_bias)
    dev, (dflag, seed_v, sbit) = t.dev, t.drop
    out = _alloc(_encoder_trunk_layout(L, B, N, S, D, Lw, H, save), residual)
    f = trunk_fields("encoder_trunk", out)
    h_last = torch.empty(B, S, H, device=dev)
    with _timed("gru_fwd", dev):
        check(lib.lg_gru_node_init_fwd(ptr(residual), ptr(tfeat), ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh),
                                       ptr(f.h_seq) if save else None, ptr(f.gates) if save else None, ptr(h_last),
                                       ptr(sensor_slot), ptr(sensor_idx), ptr(proj_weight), ptr(node_bias), ptr(f.xs[0]),
                                       ptr(f.x0bits), B, Lw, S, I, H, N, dflag, p, seed_v, 0 | sbit, t.st),
              "lg_gru_node_init_fwd")
    for l, (W, b) in enumerate(zip(weights, biases)):
        _layer_forward(t, l, f.xs[l], W, b, f.xs[l + 1], f.ymask if l == L - 1 else None,
                       x0bits=f.x0bits if l == 0 else None)
    return out


@encoder_trunk.register_fake
def _(residual, tfeat, w_ih, w_hh, b_ih, b_hh, proj_weight, node_bias, weights, biases, sensor_slot, sensor_idx,
      slot_live, nodetab, pairs, nodetab_t, pairs_t, nodetab_s, pairs_s, pos_slot_t, p, seed, save, edge_w=None,
      rowptr=None, col=None, *, bf16=False):
    B, Lw, S = residual.shape
    return _alloc(_encoder_trunk_layout(len(weights), B, sensor_slot.shape[0], S, proj_weight.shape[0], Lw,
                                        w_hh.shape[1], save), residual)


@torch.library.custom_op(f"{NS}::encoder_trunk_backward", mutates_args=(), device_types="cuda")
def encoder_trunk_backward(grad_out: Tensor, xs: List[Tensor], ymask: Tensor, x0bits: Tensor, residual: Tensor,
                           tfeat: Optional[Tensor], w_ih: Tensor, w_hh: Tensor, h_seq: Tensor, gates: Tensor,
                           proj_weight: Tensor, node_bias: Tensor, weights: List[Tensor], sensor_slot: Tensor,
                           sensor_idx: Tensor, slot_live: Optional[Tensor], nodetab_t: Tensor, pairs_t: Tensor,
                           pos_slot_t: Tensor, p: float, rowptr: Optional[Tensor] = None,
                           col: Optional[Tensor] = None, *, bf16: bool = False) -> List[Tensor]:
    """[dw_ih, dw_hh, db_ih, db_hh, dproj_weight, dnode_bias, dW_0 .. dW_{L-1}, db_0 .. db_{L-1}, dw]: the
    layers' backward (last first; layer 0 on the compressed x_0, its dx for the sensor rows
    only), then lg_gru_node_init_bwd; one reduce batch for all of them.  rowptr, col (the
    forward CSR): dw = dL/dw of the edge coefficients as in gnn_trunk_backward, else empty."""
    lib = load_library()
    if h_seq.numel() == 0 or gates.numel() == 0:
        raise RuntimeError("encoder_trunk was run with save=False; no backward")
    L = len(weights)
    N, B, D = xs[-1].shape
    S, Lw = residual.shape[2], residual.shape[1]
    I, H = w_ih.shape[1], w_hh.shape[1]
    t = _trunk(lib, grad_out, B, N, S, D, L, p, bf16=bf16, nodetab_t=nodetab_t, pairs_t=pairs_t, pos_slot_t=pos_slot_t,
               sensor_slot=sensor_slot, node_bias=node_bias)
    dev = t.dev
    dw_ih, dw_hh = torch.empty_like(w_ih), torch.empty_like(w_hh)
    db_ih, db_hh = torch.empty(3 * H, device=dev), torch.empty(3 * H, device=dev)
    dWp, dbp = torch.empty_like(proj_weight), torch.empty(D, device=dev)
    wsg = torch.empty(int(lib.lg_gru_node_init_bwd_workspace_bytes(B, S, I, H)), device=dev, dtype=torch.uint8)
    wgrad = _WGrad(rowptr, col)
    with _reduce_batch(lib, t.st):
        dx0, dWs, dbs, dbias_ns, wss = _trunk_layer_launches(t, grad_out.contiguous(), xs, ymask, weights, x0bits, wgrad)
        with _timed("gru_bwd", dev):
            check(lib.lg_gru_node_init_bwd(ptr(residual), ptr(tfeat), ptr(w_ih), ptr(w_hh), ptr(h_seq), ptr(gates),
                                           ptr(dx0), ptr(sensor_idx), ptr(slot_live), ptr(proj_weight), ptr(dbias_ns),
                                           ptr(dw_ih), ptr(dw_hh), ptr(db_ih), ptr(db_hh), ptr(dWp), ptr(dbp), B, Lw, S,
                                           I, H, N, ptr(wsg), wsg.numel(), t.st), "lg_gru_node_init_bwd")
    return [dw_ih, dw_hh, db_ih, db_hh, dWp, dbp] + dWs + dbs + [wgrad.total(dev)]


@encoder_trunk_backward.register_fake
def _(grad_out, xs, ymask, x0bits, residual, tfeat, w_ih, w_hh, h_seq, gates, proj_weight, node_bias, weights,
      sensor_slot, sensor_idx, slot_live, nodetab_t, pairs_t, pos_slot_t, p, rowptr=None, col=None, *, bf16=False):
    H = w_hh.shape[1]
    D = proj_weight.shape[0]
    return ([torch.empty_like(w_ih), torch.empty_like(w_hh), w_ih.new_empty(3 * H), w_ih.new_empty(3 * H),
             torch.empty_like(proj_weight), proj_weight.new_empty(D)] + [torch.empty_like(t) for t in weights]
            + [proj_weight.new_empty(D) for _ in weights]
            + [proj_weight.new_empty(col.shape[0] if col is not None else 0)])


def _et_setup(ctx, inputs, keyword_only_inputs, output):
    a, f = _trunk_ctx(ctx, encoder_trunk, inputs, output)
    bf16 = bool(keyword_only_inputs.get("bf16", False))
    if ctx.w_grad and (bf16 or a["rowptr"] is None or a["col"] is None):
        raise NotImplementedError("encoder_trunk: the gradient of edge_w needs rowptr / col and the fp32 tier")
    ctx.kw = dict(p=a["p"], bf16=bf16)
    # the arguments of encoder_trunk_backward by name (xs: xs0, then x_1 .. x_L)
    _save_named(ctx, xs=f.xs, ymask=f.ymask, x0bits=f.x0bits, h_seq=f.h_seq, gates=f.gates,
                rowptr=a["rowptr"] if ctx.w_grad else None, col=a["col"] if ctx.w_grad else None,
                **{k: a[k] for k in ("residual", "tfeat", "w_ih", "w_hh", "proj_weight", "node_bias", "weights",
                                     "sensor_slot", "sensor_idx", "slot_live", "nodetab_t", "pairs_t", "pos_slot_t")})


def _et_bwd(ctx, grads):
    g = grads[ctx.h]
    if g is None:
        return _named_grads(encoder_trunk, ctx.n_in)
    out = torch.ops.leakgnn.encoder_trunk_backward(g, **_saved_named(ctx), **ctx.kw)
    L = (len(out) - 7) // 2
    (dw_ih, dw_hh, db_ih, db_hh, dWp, dbp), dWs, dbs, (dw,) = _split(out, 6, L, L, 1)
    return _named_grads(encoder_trunk, ctx.n_in, w_ih=dw_ih, w_hh=dw_hh, b_ih=db_ih, b_hh=db_hh, proj_weight=dWp,
                        node_bias=dbp, weights=dWs, biases=dbs, edge_w=dw if ctx.w_grad else None)


encoder_trunk.register_autograd(_et_bwd, setup_context=_et_setup)


# ============================================================================ detector_heads
@torch.library.custom_op(f"{NS}::detector_heads", mutates_args=(), device_types="cuda")
def detector_heads(h: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, nw1: Tensor, nb1: Tensor, nw2: Tensor,
                   nb2: Tensor, ends: Tensor, inc_rowptr: Tensor, inc_item: Tensor, p_edge: float, p_noleak: float,
                   node_major: bool, keep_hidden: bool, seed: Tensor, sched: Optional[Tensor] = None,
                   sched_hdr: Optional[List[int]] = None, *, bf16: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(logits (B, P+1), EdgeHead hidden, pooled, NoLeakHead hidden).  Columns [0, P) by
    lg_edge_head_fwd (endpoint gather -> MFMA MLP -> dot, the (B, P, 3D) features never
    stored), column P by lg_pool_head_fwd (mean pool + NoLeakHead): the torch.cat of
    detector.py:218 is never a separate copy.  keep_hidden: keep the EdgeHead hidden layer
    for a recompute-free backward (else it is empty).  bf16: the EdgeHead MLP as one bf16
    MFMA product (LG_F_BF16, the configs[2] tier); the NoLeakHead stays fp32.  sched /
    sched_hdr: the pipe schedule of inc_rowptr / inc_item (ops.Incidence.schedule(D)), for the
    backward's streamed node sums; None / [] for the per-window scatter."""
    lib = load_library()
    h, w1, b1, w2, b2, nw1, nb1, nw2, nb2 = (_c(t) for t in (h, w1, b1, w2, b2, nw1, nb1, nw2, nb2))
    _req(h, w1, b1, w2, b2, nw1, nb1, nw2, nb2)
    N, B, D = h.shape if node_major else (h.shape[1], h.shape[0], h.shape[2])
    _check_d(D)
    lay = nat.LG_F_NODE_MAJOR if node_major else 0
    hidden, nhidden = w1.shape[0], nw1.shape[0]
    P = ends.shape[0]
    seed_v, sbit = _seed_args(seed) if (p_edge > 0.0 or p_noleak > 0.0) else (0, 0)
    fe = (nat.LG_F_DROPOUT if p_edge > 0.0 else 0) | (nat.LG_F_BF16 if bf16 else 0)
    fn = nat.LG_F_DROPOUT if p_noleak > 0.0 else 0
    st = stream_of(h)
    dev = h.device
    logits = torch.empty(B, P + 1, device=dev, dtype=torch.float32)
    pooled = torch.empty(B, D, device=dev, dtype=torch.float32)
    hid = torch.empty(B, nhidden, device=dev, dtype=torch.float32)
    ehid = torch.empty(B * P, hidden, device=dev, dtype=torch.float32) if keep_hidden else torch.empty(0, device=dev)
    with _timed("edge_fwd", dev):
        check(lib.lg_edge_head_fwd(ptr(ends), ptr(h), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(logits), P + 1,
                                   ptr(ehid) if keep_hidden else None, B, N, P, D, hidden, fe | lay, p_edge, seed_v,
                                   EDGE_HEAD_SALT | sbit, st), "lg_edge_head_fwd")
    with _timed("pool_head", dev):
        check(lib.lg_pool_head_fwd(ptr(h), ptr(nw1), ptr(nb1), ptr(nw2), ptr(nb2), ptr(pooled), ptr(hid), ptr(logits),
                                   P + 1, P, B, N, D, nhidden, fn | lay, p_noleak, seed_v, NOLEAK_HEAD_SALT | sbit,
                                   st), "lg_pool_head_fwd")
    return logits, ehid, pooled, hid


@detector_heads.register_fake
def _(h, w1, b1, w2, b2, nw1, nb1, nw2, nb2, ends, inc_rowptr, inc_item, p_edge, p_noleak, node_major, keep_hidden,
      seed, sched=None, sched_hdr=None, *, bf16=False):
    B = h.shape[1] if node_major else h.shape[0]
    D = h.shape[2]
    P = ends.shape[0]
    ehid = h.new_empty(B * P, w1.shape[0]) if keep_hidden else h.new_empty(0)
    return h.new_empty(B, P + 1), ehid, h.new_empty(B, D), h.new_empty(B, nw1.shape[0])


@torch.library.custom_op(f"{NS}::detector_heads_backward", mutates_args=(), device_types="cuda")
def detector_heads_backward(dlogits: Tensor, h: Tensor, w1: Tensor, w2: Tensor, ehid: Tensor, pooled: Tensor,
                            hid: Tensor, nw1: Tensor, nw2: Tensor, ends: Tensor, inc_rowptr: Tensor, inc_item: Tensor,
                            sched: Optional[Tensor], sched_hdr: List[int], p_edge: float, p_noleak: float,
                            node_major: bool, *, bf16: bool = False
                            ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(dh, dW1, db1, dW2, db2, dnW1, dnb1, dnW2, dnb2): lg_pool_head_bwd -> dpooled and the
    NoLeakHead grads; lg_edge_head_bwd_scatter -> the per-pipe endpoint grads and, fused, their
    deterministic incidence reduce plus dpooled / N into every node row."""
    lib = load_library()
    if ehid.numel() == 0:
        raise RuntimeError("detector_heads was run with keep_hidden=False; no backward")
    dl, h = _c(dlogits), _c(h)
    N, B, D = h.shape if node_major else (h.shape[1], h.shape[0], h.shape[2])
    lay = nat.LG_F_NODE_MAJOR if node_major else 0
    P, hidden, nhidden = ends.shape[0], w1.shape[0], nw1.shape[0]
    fe = (nat.LG_F_DROPOUT if p_edge > 0.0 else 0) | (nat.LG_F_BF16 if bf16 else 0)
    fn = nat.LG_F_DROPOUT if p_noleak > 0.0 else 0
    dev = h.device
    st = stream_of(h)
    dpipe = torch.empty(B, P, 2, D, device=dev)
    dw1, db1 = torch.empty_like(w1), torch.empty(hidden, device=dev)
    dw2, db2 = torch.empty_like(w2), torch.empty(1, device=dev)
    ndw1, ndb1 = torch.empty_like(nw1), torch.empty(nhidden, device=dev)
    ndw2, ndb2 = torch.empty_like(nw2), torch.empty(1, device=dev)
    ws = torch.empty(int(lib.lg_edge_head_bwd_workspace_bytes(B, P, D, hidden)), device=dev, dtype=torch.uint8)
    wsn = torch.empty(int(lib.lg_pool_head_bwd_workspace_bytes(B, D, nhidden)), device=dev, dtype=torch.uint8)
    dh = torch.empty_like(h)
    # one launch for the EdgeHead's and the NoLeakHead's weight-grad reductions
    with _reduce_batch(lib, st):
        _heads_backward_launches(lib, dl, h, w1, w2, ehid, pooled, hid, nw1, nw2, ends, inc_rowptr, inc_item, sched,
                                 sched_hdr, P, B, N, D, hidden, nhidden, fe | lay, fn, p_edge, p_noleak, dpipe, dh, dw1,
                                 db1, dw2, db2, ndw1, ndb1, ndw2, ndb2, ws, wsn, st)
    return dh, dw1, db1, dw2, db2, ndw1, ndb1, ndw2, ndb2


# True: the pipe scatter fused into the EdgeHead backward (lg_edge_head_bwd_scatter): with the
# pipe schedule (ABI 22, the default at B >= the CU count) the node sums are STREAMED tile by
# tile from the dfeat rows in LDS, so no per-pipe row reaches HBM; without one, per window
# after its last tile (ABI 19).  False: two launches (lg_edge_head_bwd + lg_pipe_scatter_bwd).
# Same node gradient bit for bit (one incidence order for all;
# tests/test_gpu_library.py::test_fused_pipe_scatter_matches_two_launches).  Measured at
# B = 256 (DESIGN §3 "Round 4"): streamed 125-132 us in the step (profiles/r04/r04z3), against
# 152.6 us for the per-window form and 114.6 + 35.3 us for the two launches (round 3); since
# round 5 the streamed launch also runs the NoLeakHead backward (_FUSED_HEADS below):
# 135-139 us in the step for both heads (profiles/r05/r05p), against 125-132 + 10-11 us.
_FUSED_SCATTER = True
# True: with the streamed scatter, the NoLeakHead backward runs in the EdgeHead backward's
# prologue (lg_heads_bwd_scatter: one launch for both heads); False: lg_pool_head_bwd first
_FUSED_HEADS = True


def _heads_backward_launches(lib, dl, h, w1, w2, ehid, pooled, hid, nw1, nw2, ends, inc_rowptr, inc_item, sched,
                             sched_hdr, P, B, N, D, hidden, nhidden, fe, fn, p_edge, p_noleak, dpipe, dh, dw1, db1, dw2,
                             db2, ndw1, ndb1, ndw2, ndb2, ws, wsn, st):
    """NoLeakHead backward first (its dpooled feeds the node rows), then the EdgeHead backward
    with the incidence scatter fused in (lg_edge_head_bwd_scatter): dh complete."""
    dev = h.device
    dpooled = torch.empty(B, D, device=dev)
    lay = fe & nat.LG_F_NODE_MAJOR
    if _FUSED_SCATTER and _FUSED_HEADS:
        # both heads in one launch where the streamed form applies (else the two calls inside)
        with _timed("edge_bwd", dev):
            hdr = (ctypes.c_int32 * 16)(*sched_hdr) if (sched is not None and sched_hdr) else None
            check(lib.lg_heads_bwd_scatter(ptr(pooled), ptr(hid), ptr(nw1), ptr(nw2), ptr(ndw1), ptr(ndb1), ptr(ndw2),
                                           ptr(ndb2), fn, p_noleak, ptr(wsn), wsn.numel(), ptr(ends), ptr(h), ptr(w1),
                                           ptr(w2), ptr(ehid), ptr(dl), P + 1, ptr(dpipe), ptr(dw1), ptr(db1), ptr(dw2),
                                           ptr(db2), ptr(inc_rowptr), ptr(inc_item), ptr(sched) if hdr else None, hdr,
                                           ptr(dpooled), ptr(dh), B, N, P, D, hidden, fe, p_edge, ptr(ws), ws.numel(),
                                           st), "lg_heads_bwd_scatter")
        return
    with _timed("pool_head_bwd", dev):
        check(lib.lg_pool_head_bwd(ptr(pooled), ptr(hid), ptr(nw1), ptr(nw2), ptr(dl), P + 1, P, ptr(dpooled),
                                   ptr(ndw1), ptr(ndb1), ptr(ndw2), ptr(ndb2), B, D, nhidden, fn, p_noleak, ptr(wsn), wsn.numel(),
                                   st), "lg_pool_head_bwd")
    if _FUSED_SCATTER:
        with _timed("edge_bwd", dev):
            hdr = (ctypes.c_int32 * 16)(*sched_hdr) if (sched is not None and sched_hdr) else None
            check(lib.lg_edge_head_bwd_scatter(ptr(ends), ptr(h), ptr(w1), ptr(w2), ptr(ehid), ptr(dl), P + 1,
                                               ptr(dpipe), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(inc_rowptr),
                                               ptr(inc_item), ptr(sched) if hdr else None, hdr, ptr(dpooled), ptr(dh),
                                               B, N, P, D, hidden, fe, p_edge, ptr(ws), ws.numel(), st),
                  "lg_edge_head_bwd_scatter")
        return
    with _timed("edge_bwd", dev):
        check(lib.lg_edge_head_bwd(ptr(ends), ptr(h), ptr(w1), ptr(w2), ptr(ehid), ptr(dl), P + 1, ptr(dpipe),
                                   ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), B, N, P, D, hidden, fe, p_edge,
                                   ptr(ws), ws.numel(), st), "lg_edge_head_bwd")
    with _timed("pipe_scatter", dev):
        check(lib.lg_pipe_scatter_bwd(ptr(inc_rowptr), ptr(inc_item), ptr(dpipe), ptr(dpooled), ptr(dh), B, N, P, D,
                                      lay, st), "lg_pipe_scatter_bwd")


@detector_heads_backward.register_fake
def _(dlogits, h, w1, w2, ehid, pooled, hid, nw1, nw2, ends, inc_rowptr, inc_item, sched, sched_hdr, p_edge, p_noleak,
      node_major, *, bf16=False):
    H, NH = w1.shape[0], nw1.shape[0]
    return (torch.empty_like(h), torch.empty_like(w1), w1.new_empty(H), torch.empty_like(w2), w2.new_empty(1),
            torch.empty_like(nw1), nw1.new_empty(NH), torch.empty_like(nw2), nw2.new_empty(1))


def _heads_setup(ctx, inputs, keyword_only_inputs, output):
    (h, w1, b1, w2, b2, nw1, nb1, nw2, nb2, ends, inc_rowptr, inc_item, p_edge, p_noleak, node_major, _, _) = inputs[:17]
    sched = inputs[17] if len(inputs) > 17 else None
    sched_hdr = inputs[18] if len(inputs) > 18 else None
    bf16 = bool(keyword_only_inputs.get("bf16", False))
    _, ehid, pooled, hid = output
    ctx.mark_non_differentiable(ehid, pooled, hid)
    ctx.set_materialize_grads(False)  # else autograd zero-fills a (B*P, 128) gradient for ehid
    ctx.cfg = (p_edge, p_noleak, node_major, bf16, list(sched_hdr or []) if sched is not None else [])
    ctx.nin = len(inputs)
    ctx.save_for_backward(h, w1, w2, ehid, pooled, hid, nw1, nw2, ends, inc_rowptr, inc_item, sched)


def _heads_bwd(ctx, dlogits, _dehid, _dpooled, _dhid):
    if dlogits is None:
        return (None,) * ctx.nin
    h, w1, w2, ehid, pooled, hid, nw1, nw2, ends, inc_rowptr, inc_item, sched = ctx.saved_tensors
    p_edge, p_noleak, node_major, bf16, hdr = ctx.cfg
    g = torch.ops.leakgnn.detector_heads_backward(dlogits, h, w1, w2, ehid, pooled, hid, nw1, nw2, ends, inc_rowptr,
                                                  inc_item, sched, hdr, p_edge, p_noleak, node_major, bf16=bf16)
    return tuple(g) + (None,) * (ctx.nin - 9)


detector_heads.register_autograd(_heads_bwd, setup_context=_heads_setup)


# ============================================================================ evaluator tails
def _rows(op: str, logits: Tensor) -> Tuple[int, int, int]:
    """(rows, C, row stride) of a (rows, C) fp32 CUDA matrix with unit column stride; no copy is made."""
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"{op}: logits must be a (rows, C) float32 matrix, got {tuple(logits.shape)} {logits.dtype}")
    _req(logits)
    n, C = logits.shape
    if C > 1 and logits.stride(1) != 1:
        raise ValueError(f"{op}: logits need unit column stride (strides {logits.stride()})")
    ldx = logits.stride(0) if n > 1 else C
    if ldx < C:
        raise ValueError(f"{op}: logits rows overlap (row stride {ldx} < C = {C})")
    return n, C, ldx


def _vec(op: str, name: str, t: Optional[Tensor], dtype: torch.dtype, shape: Tuple[int, ...]) -> None:
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be a contiguous {dtype} CUDA tensor of shape {shape}, got "
                         f"{tuple(t.shape)} {t.dtype} on {t.device}")


@torch.library.custom_op(f"{NS}::window_metrics", mutates_args=("counters",), device_types="cuda")
def window_metrics(logits: Tensor, label: Tensor, nlc: int, topk: int, bucket: Optional[Tensor],
                   dist: Optional[Tensor], inv_rank: Optional[Tensor], radii: List[float], acc_is: List[int],
                   counters: Tensor) -> Tuple[Tensor, Tensor]:
    """(rank_out, atd_out) of lg_window_metrics; `counters` (int64, ops.WINDOW_COUNTERS order) is
    accumulated in place.  atd_out is empty without `dist`.  Allocates the two outputs, nothing
    else, and never synchronises."""
    op = "window_metrics"
    lib = load_library()
    B, C, ldx = _rows(op, logits)
    _vec(op, "label", label, torch.int64, (B,))
    _vec(op, "bucket", bucket, torch.int32, (B,))
    _vec(op, "dist", dist, torch.float64, (nlc, nlc))
    _vec(op, "inv_rank", inv_rank, torch.int32, (nlc, nlc))
    _vec(op, "counters", counters, torch.int64, (len(WINDOW_COUNTERS),))
    if len(radii) > WINDOW_MAX_LIST or len(acc_is) > WINDOW_MAX_LIST:
        raise ValueError(f"{op}: at most {WINDOW_MAX_LIST} radii and accuracy_is per call, got {len(radii)} / {len(acc_is)}")
    rank = torch.empty(B, dtype=torch.int32, device=logits.device)
    atd = torch.empty(B if dist is not None else 0, dtype=torch.float64, device=logits.device)
    if B == 0:
        return rank, atd
    rr = (ctypes.c_double * max(1, len(radii)))(*radii)
    ii = (ctypes.c_int64 * max(1, len(acc_is)))(*acc_is)
    check(lib.lg_window_metrics(ptr(logits), ptr(label), B, C, ldx, nlc, topk, ptr(bucket), ptr(dist), ptr(inv_rank),
                                ctypes.cast(rr, ctypes.c_void_p), len(radii), ctypes.cast(ii, ctypes.c_void_p),
                                len(acc_is), ptr(counters), counters.numel(), ptr(rank),
                                ptr(atd) if dist is not None else None, stream_of(logits)), "lg_window_metrics")
    return rank, atd


@window_metrics.register_fake
def _(logits, label, nlc, topk, bucket, dist, inv_rank, radii, acc_is, counters):
    B = logits.shape[0]
    return (logits.new_empty(B, dtype=torch.int32), logits.new_empty(B if dist is not None else 0, dtype=torch.float64))


@torch.library.custom_op(f"{NS}::event_decide", mutates_args=(), device_types="cuda")
def event_decide(logits: Tensor, end_ns: Tensor, agg_ns: int, noleak: int, want_sum: bool) -> Tuple[Tensor, Tensor]:
    """(int64 [trig, stop, pred], summed fp32 (C,), empty unless want_sum) of lg_event_decide."""
    op = "event_decide"
    lib = load_library()
    W, C, ldx = _rows(op, logits)
    _vec(op, "end_ns", end_ns, torch.int64, (W,))
    dev = logits.device
    out = torch.empty(3, dtype=torch.int64, device=dev)
    summed = torch.empty(C if want_sum else 0, dtype=torch.float32, device=dev)
    nws = int(lib.lg_event_decide_workspace_bytes(W))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    check(lib.lg_event_decide(ptr(logits) if W else None, ptr(end_ns) if W else None, W, C, ldx, agg_ns, noleak,
                              ptr(out), ptr(summed) if want_sum else None, ptr(ws), nws, stream_of(logits)),
          "lg_event_decide")
    return out, summed


@event_decide.register_fake
def _(logits, end_ns, agg_ns, noleak, want_sum):
    return (logits.new_empty(3, dtype=torch.int64), logits.new_empty(logits.shape[1] if want_sum else 0))


# ============================================================================ module-facing helpers
def seed_tensor(device: torch.device) -> Tensor:
    """The dropout seed of one call site as a tensor (see ops._new_seed): a CPU int64 value
    drawn from torch's CPU generator in eager mode; under HIP-graph capture a device word
    re-drawn on every replay (a SeedSlots slot, or torch's graph-safe CUDA generator)."""
    from . import ops
    if ops._SEED_SLOTS is not None:
        return ops._SEED_SLOTS.take_tensor()
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return torch.randint(0, 2 ** 62, (1,), dtype=torch.long, device=device)
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.long)


def detector_ops_available() -> bool:
    return hasattr(torch.ops, NS) and hasattr(torch.ops.leakgnn, "gnn_trunk")
