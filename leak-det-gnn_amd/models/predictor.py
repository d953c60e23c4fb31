"""Frozen normal-state predictors that feed the detector (caller side of the hot path).

Same constructors, forward signatures and state-dict keys as reference
models/predictor.py (CausalConv1d :17-28, TCNBlock :31-52, NormalPredictorTCN
:55-81, NormalPredictorGRU :84-111).  They contain no message passing.  On a ROCm GPU the TCN of
the eligible shape (128 channels, kernel 3, dilations 2 ** i, L <= 2048) runs its conv stack on the
library whenever it is in training mode or under autograd (leakgnn::tcn_predictor: lg_tcn_conv_train_fwd /
lg_tcn_conv_bwd, exact fp32 MFMA kernels with the LayerNorm, ReLU, dropout and residual fused; the input
projection and the head stay torch GEMMs); an eval-mode no_grad call, every other shape and CPU tensors
run the stock module, and its frozen residual pass is models/tcn_plan.py.  On a ROCm
GPU NormalPredictorGRU's nn.GRU runs on the library (leakgnn::gru_predictor: lg_gru_seq_fwd /
lg_gru_seq_bwd, MFMA kernels at the default hidden_size 128, the generic kernels at other
widths), forward and backward; its frozen residual pass is models/gru_plan.py.  On CPU tensors it
is the stock module.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


# NormalPredictorTCN on a ROCm GPU, in training mode or under autograd: True = the conv stack runs on
# the library (leakgnn::tcn_predictor), False = the stock module (MIOpen conv).  DESIGN §12.
TCN_TRAIN_HIP = True


class CausalConv1d(nn.Module):
    """Conv1d padded on both sides by (k-1)*dilation, right pad cropped: y[t] sees x[<= t]."""

    def __init__(self, in_ch: int, out_ch: int, kernel_size: int, dilation: int = 1) -> None:
        super().__init__()
        self.pad = (kernel_size - 1) * dilation
        self.conv = nn.Conv1d(in_ch, out_ch, kernel_size, dilation=dilation, padding=self.pad)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.conv(x)
        return y[..., :-self.pad] if self.pad > 0 else y


class TCNBlock(nn.Module):
    """x + [conv -> LayerNorm(C) -> ReLU -> Dropout] x 2, on (B, C, L)."""

    def __init__(self, channels: int, kernel_size: int, dilation: int, dropout: float) -> None:
        super().__init__()
        self.conv1 = CausalConv1d(channels, channels, kernel_size, dilation=dilation)
        self.conv2 = CausalConv1d(channels, channels, kernel_size, dilation=dilation)
        self.dropout = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(channels)
        self.norm2 = nn.LayerNorm(channels)

    def _stage(self, conv: CausalConv1d, norm: nn.LayerNorm, h: torch.Tensor) -> torch.Tensor:
        h = norm(conv(h).transpose(1, 2))
        return self.dropout(F.relu(h)).transpose(1, 2)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x + self._stage(self.conv2, self.norm2, self._stage(self.conv1, self.norm1, x))


class NormalPredictorTCN(nn.Module):
    def __init__(self, num_sensors: int, time_dim: int = 9, hidden_channels: int = 128, kernel_size: int = 3,
                 num_blocks: int = 4, dropout: float = 0.1) -> None:
        super().__init__()
        self.num_sensors = int(num_sensors)
        self.time_dim = int(time_dim)
        self.input_proj = nn.Conv1d(self.num_sensors + self.time_dim, hidden_channels, kernel_size=1)
        self.tcn = nn.Sequential(*[TCNBlock(hidden_channels, kernel_size, 2 ** i, dropout) for i in range(num_blocks)])
        self.head = nn.Linear(hidden_channels, self.num_sensors)

    def _hip_train_shape(self, B: int, L: int) -> bool:
        """The shape leakgnn::tcn_predictor takes: 128 channels, kernel 3, dilations 2 ** i, biases,
        one eps and one dropout p for all stages, 1 <= L <= 2048, activations below 2 GiB."""
        proj = self.input_proj
        if (proj.out_channels != 128 or proj.kernel_size != (1,) or proj.bias is None or len(self.tcn) < 1
                or not 1 <= L <= 2048 or B < 1 or B * L * 512 >= 2 ** 31):
            return False
        n0 = self.tcn[0].norm1
        for i, blk in enumerate(self.tcn):
            for conv in (blk.conv1.conv, blk.conv2.conv):
                if (conv.kernel_size != (3,) or conv.dilation != (2 ** i,) or conv.in_channels != 128
                        or conv.out_channels != 128 or conv.padding != (2 * 2 ** i,) or conv.bias is None
                        or conv.groups != 1 or conv.stride != (1,)):
                    return False
            for norm in (blk.norm1, blk.norm2):
                if (tuple(norm.normalized_shape) != (128,) or norm.weight is None or norm.bias is None
                        or norm.eps != n0.eps):
                    return False
            if blk.dropout.p != self.tcn[0].dropout.p or not 0.0 <= blk.dropout.p < 1.0:
                return False
        return True

    def features(self, x: torch.Tensor, x_time: torch.Tensor) -> torch.Tensor:
        """(B, hidden): the last time step of the conv stack's output, everything before `head`."""
        xin = torch.cat([x, x_time], dim=-1)
        if TCN_TRAIN_HIP and xin.is_cuda and xin.dim() == 3 and xin.dtype == torch.float32:
            grad = torch.is_grad_enabled() and (xin.requires_grad or any(p.requires_grad for p in self.parameters()))
            B, L, _ = xin.shape
            if (self.training or grad) and self._hip_train_shape(B, L):
                from . import library
                proj = self.input_proj
                h = torch.addmm(proj.bias, xin.reshape(B * L, -1), proj.weight[:, :, 0].t()).view(B, L, 128)
                stages = [(c.conv, n) for blk in self.tcn for c, n in ((blk.conv1, blk.norm1), (blk.conv2, blk.norm2))]
                p = float(self.tcn[0].dropout.p) if self.training else 0.0
                seed = library.seed_tensor(xin.device) if p > 0.0 else torch.zeros(1, dtype=torch.int64)
                out = torch.ops.leakgnn.tcn_predictor(h, [c.weight for c, _ in stages], [c.bias for c, _ in stages],
                                                      [n.weight for _, n in stages], [n.bias for _, n in stages],
                                                      float(self.tcn[0].norm1.eps), p, seed, grad)
                return out[0]
        h = self.input_proj(xin.transpose(1, 2))                              # (B, hidden, L)
        return self.tcn(h)[:, :, -1]

    def forward(self, x: torch.Tensor, x_time: torch.Tensor) -> torch.Tensor:
        return self.head(self.features(x, x_time))                            # (B, S)


class NormalPredictorGRU(nn.Module):
    def __init__(self, num_sensors: int, time_dim: int = 9, hidden_size: int = 128, num_layers: int = 2,
                 dropout: float = 0.1) -> None:
        super().__init__()
        self.num_sensors = int(num_sensors)
        self.time_dim = int(time_dim)
        self.gru = nn.GRU(input_size=self.num_sensors + self.time_dim, hidden_size=hidden_size,
                          num_layers=num_layers, batch_first=True, dropout=dropout if num_layers > 1 else 0.0)
        self.head = nn.Linear(hidden_size, self.num_sensors)

    def features(self, x: torch.Tensor, x_time: torch.Tensor) -> torch.Tensor:
        """(B, hidden): the top layer's last hidden state, everything before `head`."""
        xin = torch.cat([x, x_time], dim=-1)
        g = self.gru
        if xin.is_cuda and xin.dim() == 3 and g.batch_first and not g.bidirectional and g.bias and g.proj_size == 0:
            from . import library
            nl = g.num_layers
            ws = [[getattr(g, f"{n}_l{l}") for l in range(nl)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            p = float(g.dropout) if (self.training and nl > 1) else 0.0
            save = torch.is_grad_enabled() and (xin.requires_grad or any(w.requires_grad for wl in ws for w in wl))
            seed = library.seed_tensor(xin.device) if p > 0.0 else torch.zeros(1, dtype=torch.int64)
            return torch.ops.leakgnn.gru_predictor(xin.float(), *ws, p, seed, save)[0]
        out, _ = g(xin)
        return out[:, -1, :]

    def forward(self, x: torch.Tensor, x_time: torch.Tensor) -> torch.Tensor:
        return self.head(self.features(x, x_time))
