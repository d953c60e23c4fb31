"""ctypes binding of libleakgnn.so (the C ABI declared in include/leakgnn.h).

The product path has no CPU fallback: if the library is missing, or a tensor is
not on a ROCm device, the ops raise.  The library is built in-tree by
``make -C leak-det-gnn_amd`` (``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch

_PKG_ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = Path(os.environ.get("LEAKGNN_LIB", _PKG_ROOT / "lib" / "libleakgnn.so"))

ABI_VERSION = 26  # lg_abi_version() of the libleakgnn.so these signatures describe

LG_F_BIAS = 0x01
LG_F_RELU = 0x02
LG_F_DROPOUT = 0x04
LG_F_MASK_IN = 0x08
LG_F_MASK_OUT = 0x10
LG_F_NODE_MAJOR = 0x20
LG_F_DX_SENSOR_ROWS = 0x10000000  # lg_gcn_bwd_nm[_bits] with node_slot: non-sensor dx rows may stay unwritten
LG_SALT_SEED_PTR = 0x80000000  # salt bit 31: `seed` is the address of a device-resident uint64
LG_F_F32_MFMA = 0x00400000  # lg_gcn_fwd_nm: the per-wave pipeline on exact f32 MFMA (bit-identical to lg_gcn_fwd)
LG_F_BF16 = 0x40  # lg_gcn_fwd_nm / lg_gcn_bwd_nm / lg_edge_head_*: the bf16 node-MLP tier
LG_F_PC = 0x00004000  # with LG_F_BF16: the producer / consumer forward (default: nm3)
LG_F_BF16X3 = 0x00008000  # lg_gcn_fwd_nm fp32 tier: pc with the 3-way bf16 split (default: 2-way fp16 split)
LG_F_DIFFUSE_HOPWISE = 0x100  # lg_diffuse_fwd / _bwd: one launch per hop (default: LDS-resident when the graph fits)
LG_F_NM3 = 0x00020000  # lg_gcn_fwd_nm: the per-wave nm3 pipeline, 3-way bf16 split

_i32, _i64, _u32, _u64, _f32, _p = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64,
                                    ctypes.c_float, ctypes.c_void_p)

# name -> (restype, argtypes); mirrors include/leakgnn.h exactly.
SIGNATURES = {
    "lg_abi_version": (_i32, []),
    "lg_strerror": (ctypes.c_char_p, [_i32]),
    "lg_reduce_batch_begin": (_i32, []),
    "lg_reduce_batch_flush": (_i32, [_p]),
    "lg_stream_copy": (_i32, [_p, _p, _i64, _p]),
    "lg_seed_slots_advance": (_i32, [_p, _i64, _p, _p]),
    "lg_graph_replay": (_i32, [_p, _i64, _p]),
    "lg_cross_entropy_fwd": (_i32, [_p, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p]),
    "lg_cross_entropy_bwd": (_i32, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _i64, _p]),
    "lg_clip_adamw_workspace_bytes": (_i64, [_p, _i32]),
    "lg_clip_adamw": (_i32, [_p, _p, _i32, _p, _f32, _f32, _f32, _f32, _f32, _f32, _p, _p, _i64, _p]),
    "lg_clip_adamw_seeds": (_i32, [_p, _p, _i32, _p, _f32, _f32, _f32, _f32, _f32, _f32, _p, _p, _i64, _p, _i64, _p,
                                   _p]),
    "lg_spin_errors": (_i32, [_p, _i32]),
    "lg_timing_arm": (_i32, [_i32]),
    "lg_timing_disarm": (_i32, []),
    "lg_timing_elapsed": (_i32, [_i32, _p]),
    "lg_graph_workspace_bytes": (_i64, [_i64, _i64]),
    "lg_graph_build": (_i32, [_p, _i64, _i64, _i32, _i32, _f32, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    # edge weights (added to ABI 26 without a bump: additions only)
    "lg_graph_build_w_workspace_bytes": (_i64, [_i64, _i64]),
    "lg_graph_build_w": (_i32, [_p, _p, _i64, _i64, _i32, _i32, _f32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "lg_graph_reweight": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _p, _p, _p, _p]),
    "lg_gcn_norm_bwd_workspace_bytes": (_i64, [_i64, _i64]),
    "lg_gcn_norm_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _p, _p, _i64, _p]),
    "lg_sddmm_cols": (_i32, [_p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _p]),
    # dL/dw of a node-major trunk layer (added to ABI 26 without a bump: additions only)
    "lg_sddmm_nm_workspace_bytes": (_i64, [_i64, _i64]),
    "lg_sddmm_nm": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _p, _i64, _p]),
    "lg_nm_table_build": (_i32, [_p, _p, _i64, _p, _p, _p]),
    "lg_rcm_order": (_i32, [_p, _i64, _i64, _p]),
    "lg_incidence_workspace_bytes": (_i64, [_i64, _i64]),
    "lg_incidence_build": (_i32, [_p, _i64, _i64, _p, _p, _p, _i64, _p]),
    "lg_batchify_edge_index": (_i32, [_p, _i64, _i64, _i64, _p, _p]),
    "lg_linear_dw_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "lg_linear_dw": (_i32, [_p, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _p]),
    "lg_node_init_fwd": (_i32, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_node_init_proj_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32,
                                     _p]),
    "lg_sensor_proj_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "lg_sensor_proj_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32, _p, _i64, _p]),
    "lg_gcn_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_spmm": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p]),
    "lg_spmm_cols": (_i32, [_p, _p, _p, _p, _i64, _p, _p, _i64, _i64, _i64, _p]),
    "lg_gcn_bwd_workspace_bytes": (_i64, [_i64]),
    "lg_gcn_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _p, _i64, _p]),
    "lg_pipe_gather_fwd": (_i32, [_p, _p, _p, _i64, _i64, _i64, _i64, _p]),
    "lg_pipe_scatter_bwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _p]),
    "lg_gcn_fwd_nm": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_gcn_fwd_nm_bits": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p, _p]),
    "lg_nm_table_sensor_mark": (_i32, [_p, _p, _i64, _i64, _p, _p, _p, _p, _p]),
    "lg_node_init_bits_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32,
                                     _p]),
    "lg_node_init_expand": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _p]),
    "lg_gcn_fwd_nm_x0": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_gcn_bwd_nm_x0": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32,
                                _f32, _f32, _p, _i64, _p]),
    "lg_gcn_fwd_rows": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _p]),
    "lg_gcn_bwd_rows": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _p, _i64, _p]),
    "lg_gcn_bwd_nm_bits": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _f32, _p, _i64, _p, _p]),
    # residual trunk layers (added to ABI 26 without a bump: additions only)
    "lg_gcn_fwd_nm_skip": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p, _p]),
    "lg_gcn_bwd_nm_skip": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _f32, _p, _i64, _p, _p]),
    # LayerNorm of the pre-norm residual trunk (csrc/norm.hip; added to ABI 26 without a bump)
    "lg_add_layernorm_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _f32, _p]),
    "lg_layernorm_bwd_workspace_bytes": (_i64, [_i64]),
    "lg_layernorm_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _f32, _p, _i64, _p]),
    # K-hop diffusion of the node init (csrc/diffuse.hip; added to ABI 26 without a bump)
    "lg_diffuse_slice": (_i32, [_i64, _i64]),
    "lg_diffuse_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64, _i32, _i32]),
    "lg_diffuse_fwd": (_i32, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _f32, _i32, _p, _i64, _p]),
    "lg_diffuse_bwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _f32, _i32, _f32, _p, _i64, _p]),
    "lg_gcn_bwd_nm_workspace_bytes": (_i64, [_i64]),
    "lg_gcn_bwd_nm": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _f32, _p, _i64, _p]),
    "lg_edge_head_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i32, _f32,
                                _u64, _u32, _p]),
    "lg_edge_head_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "lg_edge_head_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i32, _f32, _p, _i64, _p]),
    "lg_edge_head_bwd_scatter": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64,
                                        _i64, _i64, _i64, _i32, _f32, _p, _i64, _p]),
    "lg_pipe_schedule_words": (_i64, [_i64, _i64, _i64]),
    "lg_pipe_schedule_build": (_i32, [_p, _i64, _i64, _i64, _p, _i64, _p, _p]),
    "lg_mean_pool_fwd": (_i32, [_p, _p, _i64, _i64, _i64, _p]),
    "lg_pool_head_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _f32, _u64,
                                _u32, _p]),
    "lg_pool_head_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "lg_pool_head_bwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i32, _f32, _p, _i64, _p]),
    "lg_heads_bwd_scatter": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _f32, _p, _i64,
                                    _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                    _i64, _i64, _i64, _i64, _i64, _i32, _f32, _p, _i64, _p]),
    "lg_gru_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "lg_gru_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "lg_gru_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p]),
    # stacked GRU layers (added to ABI 26 without a bump: additions only)
    "lg_gru_seq_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_gru_seq_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "lg_gru_seq_tiled": (_i32, [_i64, _i64, _i32]),
    "lg_gru_seq_infer": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_gru_win_fwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "lg_gru_seq_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64,
                              _i64, _i32, _f32, _u64, _u32, _p, _i64, _p]),
    "lg_gru_node_init_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                    _i64, _i64, _i64, _i64, _i64, _i64, _i32, _f32, _u64, _u32, _p]),
    "lg_gru_node_init_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "lg_gru_node_init_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                    _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p]),
    "lg_tcn_packed_weight_floats": (_i64, [_i64]),
    "lg_tcn_pack_weight": (_i32, [_p, _p, _i64, _p]),
    "lg_tcn_conv_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _f32, _p, _i64, _i64, _i64, _i64, _i64, _p]),
    "lg_tcn_pack_weight_t": (_i32, [_p, _p, _i64, _p]),
    "lg_tcn_conv_train_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _f32, _f32, _u64, _u32, _p, _p, _p, _p, _i64, _i64,
                                     _i64, _i64, _i64, _p]),
    "lg_tcn_conv_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "lg_tcn_conv_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f32, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64,
                               _i64, _i64, _p, _i64, _p]),
    # predictor head + MSE loss (added to ABI 26 without a bump: additions only)
    "lg_head_mse_fwd": (_i32, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p]),
    "lg_head_mse_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "lg_head_mse_bwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _p]),
    # cross entropy with weights, label smoothing (uniform or a table) and the three reductions
    # (added to ABI 26 without a bump: additions only)
    "lg_cross_entropy_opt_fwd": (_i32, [_p, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _f32, _i32, _p, _p, _p, _p, _p,
                                        _p, _p]),
    "lg_cross_entropy_opt_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _f32, _i32, _p,
                                        _i64, _p]),
    # evaluator tails: window metrics and the event decision (added to ABI 26 without a bump: additions only)
    "lg_window_metrics": (_i32, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _i32, _p, _i32, _p, _i64, _p,
                                 _p, _p]),
    "lg_event_decide_workspace_bytes": (_i64, [_i64]),
    "lg_event_decide": (_i32, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _i64, _p]),
    # device sampler: numpy-exact draws and the window gather (added to ABI 26 without a bump: additions only)
    "lg_draw_detector": (_i32, [_u64, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p, _p]),
    "lg_draw_detector_host": (_i32, [_u64, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p]),
    "lg_draw_predictor": (_i32, [_u64, _i64, _i64, _p, _i64, _p, _i64, _i64, _i64, _p, _p, _p]),
    "lg_draw_predictor_host": (_i32, [_u64, _i64, _i64, _p, _i64, _p, _i64, _i64, _i64, _p, _p]),
    "lg_np_stream_host": (_i32, [_u64, _p, _p, _p, _i64, _p, _p]),
    "lg_gather_windows": (_i32, [_p, _i64, _i64, _i64,
                                 _p, _i64, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _i64, _i64, _p,
                                 _p, _p, _p, _p, _p]),
}

_lib = None


def load_library() -> ctypes.CDLL:
    """Load libleakgnn.so once; raise ImportError (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        if not LIB_PATH.is_file():
            raise ImportError(
                f"libleakgnn.so not found at {LIB_PATH}; build it with `make -C {_PKG_ROOT}` "
                "(or __graft_entry__.build()). The GNN hot path has no CPU fallback.")
        lib = ctypes.CDLL(str(LIB_PATH))
        lib.lg_abi_version.restype = ctypes.c_int
        if lib.lg_abi_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} has ABI {lib.lg_abi_version()}, the bindings expect {ABI_VERSION}; "
                              f"rebuild with `make -C {_PKG_ROOT}`")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class LeakGNNError(RuntimeError):
    pass


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().lg_strerror(rc).decode()
        raise LeakGNNError(f"{what} failed: {msg} (code {rc})")


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def stream_of(t: torch.Tensor) -> int:
    """hipStream_t of torch's current stream on t's device (kernels are enqueued there)."""
    return torch.cuda.current_stream(t.device).cuda_stream


def require_device(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "leakgnn ops run only on a ROCm GPU (tensor on %s); there is no CPU path" % t.device)
        if not t.is_contiguous():
            raise RuntimeError("leakgnn ops need contiguous tensors")
