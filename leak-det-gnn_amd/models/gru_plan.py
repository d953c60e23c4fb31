"""Shared-window residual pass of the frozen NormalPredictorGRU (the GRU counterpart of
models/tcn_plan.py).

build_residual_sequence_from_segment (reference models/utils.py:169-216) evaluates the
predictor on the l_det shifted windows of every segment.  The first GRU layer's input product
W_ih [noisy[b, tau], time[b, tau]] + b_ih depends on the segment position tau = k + t alone,
not on the window k, so it is formed once per (b, tau) - l_pred + l_det rows per segment instead
of l_det * l_pred - and the recurrence reads it in place (lg_gru_win_fwd); the unfolded
(l_det * B, l_pred, S + 9) windows are never built.  The upper layers run lg_gru_seq_infer on the
h_seq below, the top one producing h_L alone.
"""
from __future__ import annotations

H_FAST = 128  # the width of the H = 128 kernels (csrc/gru128.hip), NormalPredictorGRU's default


def fast_path_eligible(predictor) -> bool:
    """True for a NormalPredictorGRU in eval mode with hidden_size 128, unidirectional, with bias
    (any num_layers >= 1).  Anything else goes through the module."""
    gru = getattr(predictor, "gru", None)
    if gru is None or getattr(predictor, "head", None) is None or predictor.training:
        return False
    import torch.nn as nn
    if not isinstance(gru, nn.GRU):
        return False
    return (gru.hidden_size == H_FAST and not gru.bidirectional and bool(gru.bias) and gru.proj_size == 0
            and gru.num_layers >= 1 and gru.batch_first)


def gru_residual(predictor, noisy_seg, time_seg, l_pred: int, l_det: int):
    """residual (B, l_det, S) = noisy_seg[:, l_pred:] - predictor(window k) for every window k,
    on the GPU: the layer-0 input gates as one GEMM over the (B * T, S + 9) segment rows,
    lg_gru_win_fwd, lg_gru_seq_infer for the upper layers, the head as a GEMM.  Matches the
    per-window evaluation within fp32 rounding."""
    import torch
    from . import _native as nat
    from .ops import _timed
    if not fast_path_eligible(predictor):
        raise ValueError("gru_residual needs a NormalPredictorGRU (hidden 128, unidirectional, biased) in eval mode")
    B, T, S = noisy_seg.shape
    if T != l_pred + l_det:
        raise ValueError(f"segment length {T} != l_pred + l_det = {l_pred + l_det}")
    dev = noisy_seg.device
    nat.require_device(noisy_seg.contiguous())
    lib = nat.load_library()
    g = predictor.gru
    H, nl, nseq = H_FAST, g.num_layers, l_det * B
    with torch.no_grad():
        x = torch.cat([noisy_seg, time_seg], dim=-1).reshape(B * T, -1).float()
        gi = torch.addmm(g.bias_ih_l0.float(), x, g.weight_ih_l0.float().t()).contiguous()  # (B*T, 3H)
        st = nat.stream_of(gi)
        h_last = torch.empty(nseq, H, dtype=torch.float32, device=dev)
        hs = torch.empty(l_pred, nseq, H, dtype=torch.float32, device=dev) if nl > 1 else None
        w_hh, b_hh = g.weight_hh_l0.float().contiguous(), g.bias_hh_l0.float().contiguous()
        with _timed("gru_win_fwd", dev):
            nat.check(lib.lg_gru_win_fwd(nat.ptr(gi), nat.ptr(w_hh), nat.ptr(b_hh), nat.ptr(hs),
                                         nat.ptr(h_last) if nl == 1 else None, B, T, l_pred, l_det, H, st),
                      "lg_gru_win_fwd")
        for l in range(1, nl):
            top = l == nl - 1
            ws = [getattr(g, f"{n}_l{l}").float().contiguous() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            out = None if top else torch.empty(l_pred, nseq, H, dtype=torch.float32, device=dev)
            with _timed("gru_seq_infer", dev):
                nat.check(lib.lg_gru_seq_infer(nat.ptr(hs), *(nat.ptr(w) for w in ws), nat.ptr(out),
                                               nat.ptr(h_last) if top else None, nseq, l_pred, H, H, 0, 0.0, 0, 0, st),
                          "lg_gru_seq_infer")
            hs = out
        head = predictor.head
        y_hat = torch.addmm(head.bias.float(), h_last, head.weight.float().t())  # rows k * B + b
        return noisy_seg[:, l_pred:, :] - y_hat.view(l_det, B, S).transpose(0, 1)
