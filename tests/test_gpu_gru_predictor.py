"""NormalPredictorGRU on the HIP kernels (csrc/gru128.hip): the H = 128 dense layers, dropout on
read, the inference and shared-window forms, the module and the residual builder, against
torch.nn.GRU on the CPU in fp64 (forwards at helpers.assert_close's 1e-5, gradients at
helpers.assert_grads_match_truth against a CPU fp32 run)."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import assert_close, assert_grads_match_truth

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 128
SEED, P_DROP = 0x1234_5678_9ABC, 0.25
NAMES = ("w_ih", "w_hh", "b_ih", "b_hh")


def _lib():
    from models import _native
    return _native.load_library()


def _weights(I, gen, Hh=H):
    k = 1.0 / Hh ** 0.5
    shapes = ((3 * Hh, I), (3 * Hh, Hh), (3 * Hh,), (3 * Hh,))
    return [(torch.rand(*s, generator=gen) * 2 - 1) * k for s in shapes]


def _layer_ref(ws, x, dhs, dhl, dt, mask=None):
    """One GRU layer over time-major x (L, N, I) in dtype dt on the CPU: (h_seq, gates, grads)."""
    L, N, I = x.shape
    Hh = ws[1].shape[1]
    g = nn.GRU(I, Hh, 1).to(dt)
    with torch.no_grad():
        for n, w in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), ws):
            getattr(g, n).copy_(w.to(dt))
    xx = x.to(dt).clone().requires_grad_(True)
    xe = xx if mask is None else xx * mask.to(dt) / (1.0 - P_DROP)
    out, _ = g(xe)
    loss = out.new_zeros(())
    if dhs is not None:
        loss = loss + (out * dhs.to(dt)).sum()
    if dhl is not None:
        loss = loss + (out[-1] * dhl.to(dt)).sum()
    loss.backward()
    with torch.no_grad():  # the saved gate values from the layer's own h
        hp = torch.cat([out.new_zeros(1, N, Hh), out[:-1]], 0)
        gi = xe @ g.weight_ih_l0.t() + g.bias_ih_l0
        gh = hp @ g.weight_hh_l0.t() + g.bias_hh_l0
        r = torch.sigmoid(gi[..., :Hh] + gh[..., :Hh])
        z = torch.sigmoid(gi[..., Hh:2 * Hh] + gh[..., Hh:2 * Hh])
        n_ = torch.tanh(gi[..., 2 * Hh:] + r * gh[..., 2 * Hh:])
        gates = torch.stack([r, z, n_, gh[..., 2 * Hh:]], 2)
    grads = {"x": xx.grad, "w_ih": g.weight_ih_l0.grad, "w_hh": g.weight_hh_l0.grad, "b_ih": g.bias_ih_l0.grad,
             "b_hh": g.bias_hh_l0.grad}
    return out.detach(), gates, {k: v.detach() for k, v in grads.items()}


def _fwd(ws_d, x_d, save=True, flags=0, p=0.0, salt=0):
    from models import ops
    lib = _lib()
    L, N, I = x_d.shape
    hs = torch.full((L, N, H), float("nan"), device=DEV)
    gates = torch.full((L, N, 4, H), float("nan"), device=DEV) if save else None
    ops.check(lib.lg_gru_seq_fwd(ops.ptr(x_d), *(ops.ptr(w) for w in ws_d), ops.ptr(hs), ops.ptr(gates), N, L, I, H,
                                 flags, p, SEED, salt, ops.stream_of(x_d)), "lg_gru_seq_fwd")
    return hs, gates


def _bwd(ws_d, x_d, hs, gates, dhs, dhl, want_dx=True, flags=0, p=0.0, salt=0, extra_ws=0):
    from models import ops
    lib = _lib()
    L, N, I = x_d.shape
    out = {"x": torch.full((L, N, I), float("nan"), device=DEV) if want_dx else None}
    for n, w in zip(NAMES, ws_d):
        out[n] = torch.full_like(w, float("nan"))
    ws = torch.empty(int(lib.lg_gru_seq_bwd_workspace_bytes(N, I, H)) + extra_ws, device=DEV, dtype=torch.uint8)
    ops.check(lib.lg_gru_seq_bwd(ops.ptr(x_d), None, None, ops.ptr(ws_d[0]), ops.ptr(ws_d[1]), ops.ptr(hs),
                                 ops.ptr(gates), ops.ptr(dhs), ops.ptr(dhl), ops.ptr(out["x"]), ops.ptr(out["w_ih"]),
                                 ops.ptr(out["w_hh"]), ops.ptr(out["b_ih"]), ops.ptr(out["b_hh"]), 0, 0, N, L, I, H,
                                 flags, p, SEED, salt, ops.ptr(ws), ws.numel(), ops.stream_of(x_d)), "lg_gru_seq_bwd")
    torch.cuda.synchronize()
    return {k: v for k, v in out.items() if v is not None}


def test_dispatch_predicate():
    lib = _lib()
    for I in (1, 38, 128, 1024):
        for d in (0, 1):
            assert lib.lg_gru_seq_tiled(I, 128, d) == 1
    assert lib.lg_gru_seq_tiled(38, 64, 0) == 0 and lib.lg_gru_seq_tiled(38, 64, 1) == 0


@pytest.mark.parametrize("shape", [(1, 1), (16, 2), (17, 7), (40, 36)])
@pytest.mark.parametrize("I", [1, 38, 42, 128, 130])
def test_dense_layer_h128(I, shape):
    N, L = shape
    gen = torch.Generator().manual_seed(1000 * I + 10 * N + L)
    ws = _weights(I, gen)
    x = torch.randn(L, N, I, generator=gen)
    dhs, dhl = torch.randn(L, N, H, generator=gen), torch.randn(N, H, generator=gen)
    ws_d, x_d = [w.to(DEV) for w in ws], x.to(DEV)
    hs, gates = _fwd(ws_d, x_d)
    h64, g64, _ = _layer_ref(ws, x, dhs, None, torch.float64)
    assert_close(hs, h64, what="h_seq")
    assert_close(gates, g64, what="gates")
    hs2, gates2 = _fwd(ws_d, x_d)
    assert torch.equal(hs, hs2) and torch.equal(gates, gates2)
    hs_only, _ = _fwd(ws_d, x_d, save=False)
    assert torch.equal(hs, hs_only)
    for use_s, use_l in ((True, False), (False, True), (True, True)):
        a, b = (dhs if use_s else None), (dhl if use_l else None)
        ad, bd = (a.to(DEV) if use_s else None), (b.to(DEV) if use_l else None)
        got = _bwd(ws_d, x_d, hs, gates, ad, bd)
        _, _, t64 = _layer_ref(ws, x, a, b, torch.float64)
        _, _, t32 = _layer_ref(ws, x, a, b, torch.float32)
        assert_grads_match_truth(got, t32, t64)
        if use_s and use_l:
            again = _bwd(ws_d, x_d, hs, gates, ad, bd)
            assert all(torch.equal(got[k], again[k]) for k in got), "backward not deterministic"
            nodx = _bwd(ws_d, x_d, hs, gates, ad, bd, want_dx=False)
            assert all(torch.equal(got[k], nodx[k]) for k in nodx), "dx == NULL changes the weight gradients"
            if L > 1:  # a workspace with room for every step: one pass instead of the planned ones
                one = _bwd(ws_d, x_d, hs, gates, ad, bd, extra_ws=L * N * 4 * H * 4)
                assert_grads_match_truth(one, t32, t64)


def test_backward_multi_pass():
    """A workspace with room for two steps of dG: the passes' partials add up to the one-pass result."""
    from models import ops
    lib = _lib()
    N, L, I = 17, 7, 38
    gen = torch.Generator().manual_seed(7)
    ws = _weights(I, gen)
    x = torch.randn(L, N, I, generator=gen)
    dhs, dhl = torch.randn(L, N, H, generator=gen), torch.randn(N, H, generator=gen)
    ws_d, x_d = [w.to(DEV) for w in ws], x.to(DEV)
    hs, gates = _fwd(ws_d, x_d)
    step = N * 4 * H * 4
    planned = int(lib.lg_gru_seq_bwd_workspace_bytes(N, I, H))
    fixed = planned - min(1024, (64 << 20) // step) * step
    out = {"x": torch.empty(L, N, I, device=DEV)}
    for n, w in zip(NAMES, ws_d):
        out[n] = torch.empty_like(w)
    wsb = torch.empty(fixed + 2 * step, device=DEV, dtype=torch.uint8)
    dhs_d, dhl_d = dhs.to(DEV), dhl.to(DEV)
    ops.check(lib.lg_gru_seq_bwd(ops.ptr(x_d), None, None, ops.ptr(ws_d[0]), ops.ptr(ws_d[1]), ops.ptr(hs),
                                 ops.ptr(gates), ops.ptr(dhs_d), ops.ptr(dhl_d), ops.ptr(out["x"]),
                                 ops.ptr(out["w_ih"]), ops.ptr(out["w_hh"]), ops.ptr(out["b_ih"]), ops.ptr(out["b_hh"]),
                                 0, 0, N, L, I, H, 0, 0.0, 0, 0, ops.ptr(wsb), wsb.numel(), ops.stream_of(x_d)),
              "lg_gru_seq_bwd")
    _, _, t64 = _layer_ref(ws, x, dhs, dhl, torch.float64)
    _, _, t32 = _layer_ref(ws, x, dhs, dhl, torch.float32)
    assert_grads_match_truth(out, t32, t64)


def test_dropout_on_read():
    from models import _native as nat
    from models.ops import GRU_PRED_SALT
    from oracle.dropout_ref import keep_mask
    N, L, I = 17, 7, 128
    gen = torch.Generator().manual_seed(3)
    ws = _weights(I, gen)
    x = torch.randn(L, N, I, generator=gen)
    dhs, dhl = torch.randn(L, N, H, generator=gen), torch.randn(N, H, generator=gen)
    mask = torch.from_numpy(keep_mask(SEED, GRU_PRED_SALT, np.arange(L * N * I, dtype=np.uint64), P_DROP)
                            .reshape(L, N, I))
    assert 0.6 < mask.float().mean().item() < 0.9
    ws_d, x_d = [w.to(DEV) for w in ws], x.to(DEV)
    kw = dict(flags=nat.LG_F_DROPOUT, p=P_DROP, salt=GRU_PRED_SALT)
    hs, gates = _fwd(ws_d, x_d, **kw)
    h64, g64, t64 = _layer_ref(ws, x, dhs, dhl, torch.float64, mask)
    _, _, t32 = _layer_ref(ws, x, dhs, dhl, torch.float32, mask)
    assert_close(hs, h64, what="h_seq")
    assert_close(gates, g64, what="gates")
    got = _bwd(ws_d, x_d, hs, gates, dhs.to(DEV), dhl.to(DEV), **kw)
    assert_grads_match_truth(got, t32, t64)
    assert bool((got["x"].cpu()[~mask] == 0).all()), "dx is not masked"


def test_seq_infer():
    from models import ops
    lib = _lib()
    N, L, I = 17, 7, 38
    gen = torch.Generator().manual_seed(5)
    ws_d = [w.to(DEV) for w in _weights(I, gen)]
    x_d = torch.randn(L, N, I, generator=gen).to(DEV)
    hs, _ = _fwd(ws_d, x_d, save=False)
    guard = torch.full((L, N, H), float("nan"), device=DEV)  # never passed: must stay untouched
    hl = torch.empty(N, H, device=DEV)
    ops.check(lib.lg_gru_seq_infer(ops.ptr(x_d), *(ops.ptr(w) for w in ws_d), None, ops.ptr(hl), N, L, I, H, 0, 0.0, 0,
                                   0, ops.stream_of(x_d)), "lg_gru_seq_infer")
    assert torch.equal(hl, hs[-1]) and bool(torch.isnan(guard).all())
    hs2, hl2 = torch.empty(L, N, H, device=DEV), torch.empty(N, H, device=DEV)
    ops.check(lib.lg_gru_seq_infer(ops.ptr(x_d), *(ops.ptr(w) for w in ws_d), ops.ptr(hs2), ops.ptr(hl2), N, L, I, H, 0,
                                   0.0, 0, 0, ops.stream_of(x_d)), "lg_gru_seq_infer")
    assert torch.equal(hs2, hs) and torch.equal(hl2, hs[-1])
    w64 = [w.to(DEV) for w in _weights(I, gen, 64)]
    h64 = torch.empty(L, N, 64, device=DEV)
    assert lib.lg_gru_seq_infer(ops.ptr(x_d), *(ops.ptr(w) for w in w64), ops.ptr(h64), None, N, L, I, 64, 0, 0.0, 0, 0,
                                ops.stream_of(x_d)) == -2


@pytest.mark.parametrize("lw", [(1, 1), (5, 4), (36, 36)])
@pytest.mark.parametrize("B", [1, 3])
def test_window_form(B, lw):
    from models import ops
    lib = _lib()
    l_pred, n_win = lw
    T, I = l_pred + n_win, 38
    gen = torch.Generator().manual_seed(100 * B + l_pred)
    ws = _weights(I, gen)
    seg = torch.randn(B, T, I, generator=gen)
    ws_d = [w.to(DEV) for w in ws]
    gi = torch.addmm(ws_d[2], seg.to(DEV).reshape(B * T, I), ws_d[0].t()).contiguous()
    N = n_win * B
    hs, hl = torch.empty(l_pred, N, H, device=DEV), torch.empty(N, H, device=DEV)
    ops.check(lib.lg_gru_win_fwd(ops.ptr(gi), ops.ptr(ws_d[1]), ops.ptr(ws_d[3]), ops.ptr(hs), ops.ptr(hl), B, T, l_pred,
                                 n_win, H, ops.stream_of(gi)), "lg_gru_win_fwd")
    # the explicitly unfolded windows, row k * B + b, time-major
    xw = seg.unfold(1, l_pred, 1)[:, :n_win].permute(3, 1, 0, 2).reshape(l_pred, N, I).contiguous()
    for k in range(n_win):
        for b in range(B):
            assert torch.equal(xw[:, k * B + b], seg[b, k:k + l_pred])
    h64, _, _ = _layer_ref(ws, xw, torch.zeros(l_pred, N, H), None, torch.float64)
    assert_close(hs, h64, what="window h_seq")
    assert_close(hl, h64[-1], what="window h_last")
    dense, _ = _fwd(ws_d, xw.to(DEV), save=False)
    assert_close(dense, h64, what="dense h_seq on the unfolded windows")
    hl_only = torch.empty(N, H, device=DEV)
    ops.check(lib.lg_gru_win_fwd(ops.ptr(gi), ops.ptr(ws_d[1]), ops.ptr(ws_d[3]), None, ops.ptr(hl_only), B, T, l_pred,
                                 n_win, H, ops.stream_of(gi)), "lg_gru_win_fwd")
    assert torch.equal(hl_only, hl)


def _module_truth(m, x, tf, up, dt):
    import copy
    ref = copy.deepcopy(m).cpu().to(dt).eval()
    xx, tt = x.detach().clone().to(dt).requires_grad_(True), tf.detach().clone().to(dt).requires_grad_(True)
    out = ref(xx, tt)
    out.backward(up.to(dt))
    grads = {n: p.grad.detach() for n, p in ref.named_parameters()}
    grads["x"], grads["x_time"] = xx.grad, tt.grad
    return out.detach(), grads


@pytest.mark.parametrize("cfg", [dict(S=29), dict(S=33), dict(S=29, num_layers=1), dict(S=29, hidden_size=48)])
@pytest.mark.parametrize("BL", [(1, 2), (5, 36), (5, 2), (1, 36)])
def test_module(cfg, BL):
    from models.predictor import NormalPredictorGRU
    cfg = dict(cfg)
    S = cfg.pop("S")
    B, L = BL
    torch.manual_seed(B * 100 + L + S)
    m = NormalPredictorGRU(S, 9, **cfg).eval()
    x, tf, up = torch.randn(B, L, S), torch.randn(B, L, 9), torch.randn(B, S)
    o64, g64 = _module_truth(m, x, tf, up, torch.float64)
    _, g32 = _module_truth(m, x, tf, up, torch.float32)
    md = m.to(DEV)
    xd, td = x.detach().to(DEV).requires_grad_(True), tf.detach().to(DEV).requires_grad_(True)
    out = md(xd, td)
    assert_close(out, o64, what="module output")
    out.backward(up.to(DEV))
    got = {n: p.grad for n, p in md.named_parameters()}
    got["x"], got["x_time"] = xd.grad, td.grad
    assert_grads_match_truth(got, g32, g64)
    with torch.no_grad():
        assert_close(md(xd, td), o64, what="module output (no_grad)")


def test_op_rejects_bad_layers():
    z = torch.zeros
    with pytest.raises(ValueError):
        torch.ops.leakgnn.gru_predictor(z(2, 3, 38, device=DEV), [z(384, 38, device=DEV), z(384, 38, device=DEV)],
                                        [z(384, 128, device=DEV)] * 2, [z(384, device=DEV)] * 2,
                                        [z(384, device=DEV)] * 2, 0.0, z(1, dtype=torch.int64), False)


@pytest.mark.parametrize("shape", [(3, 36, 36), (2, 5, 4)])
def test_residual_builder(shape, monkeypatch):
    from models import ops, utils
    from models.predictor import NormalPredictorGRU
    B, l_pred, l_det = shape
    S = 29
    torch.manual_seed(11 * B)
    m = NormalPredictorGRU(S, 9).eval()
    seg, tseg = torch.randn(B, l_pred + l_det, S), torch.randn(B, l_pred + l_det, 9)
    import copy
    with torch.no_grad():
        truth = utils.build_residual_sequence_from_segment(copy.deepcopy(m).double(), seg.double(), tseg.double(),
                                                            l_pred, l_det)
    md = m.to(DEV)
    timer = ops.KernelTimer(["gru_win_fwd", "gru_seq_infer"])
    timer.enabled = True
    ops.set_kernel_timer(timer)
    try:
        with torch.no_grad():
            fast = utils.build_residual_sequence_from_segment(md, seg.to(DEV), tseg.to(DEV), l_pred, l_det)
    finally:
        ops.set_kernel_timer(None)
    assert timer.count("gru_win_fwd") == 1 and timer.count("gru_seq_infer") == 1
    assert tuple(fast.shape) == (B, l_det, S)
    assert_close(fast, truth, what="fast residual")
    monkeypatch.setattr(utils, "RESIDUAL_FAST_PATH", False)
    with torch.no_grad():
        stock = utils.build_residual_sequence_from_segment(md, seg.to(DEV), tseg.to(DEV), l_pred, l_det)
    assert_close(stock, truth, what="per-window residual")
    monkeypatch.setattr(utils, "RESIDUAL_FAST_PATH", True)
    with torch.no_grad():
        sq = utils.build_residual_sequence_from_segment(md, seg[0].to(DEV), tseg[0].to(DEV), l_pred, l_det)
    assert tuple(sq.shape) == (l_det, S)
    assert_close(sq, truth[0], what="squeezed residual")
