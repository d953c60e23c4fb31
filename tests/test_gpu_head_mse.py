"""leakgnn::head_mse (csrc/head_mse.hip) against the same formula on the CPU: fp64 is the truth,
fp32 the yardstick.

    y_hat = h W^T + b,  loss = mean((y_hat - y)^2),  d = 2 g / (B S) (y_hat - y),
    dh = d W,  dW = d^T h,  db = sum_b d

loss and y_hat are held to helpers.assert_close's defaults (1e-5 of the tensor's scale), the
gradients to helpers.assert_grads_match_truth (within 4 x the CPU fp32 error or 1e-5 of scale),
under a non-unit upstream gradient g = 0.37."""
from __future__ import annotations

import functools

import pytest
import torch

from helpers import assert_close, assert_grads_match_truth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = 0.37

# (B, H, S); "loop": more rows than 4 x the CU count, so the forward's workgroups (one per CU at
# most, a row per wave) take a second round of rows
SHAPES = {
    "1x1x1": (1, 1, 1),
    "3x128x29": (3, 128, 29),
    "65x128x29": (65, 128, 29),       # rows past one wave and one workgroup
    "256x128x29": (256, 128, 29),     # the CLI's
    "5x100x70": (5, 100, 70),         # H no multiple of 64, S > 64
    "2x1024x1024": (2, 1024, 1024),   # the bounds; W (4 MB) not in LDS
    "loop": None,
}


def _shape(name):
    if SHAPES[name] is not None:
        return SHAPES[name]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (4 * cus + 5, 40, 3)


def _inputs(B, H, S, offset=0.0, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * H + S)
    h = torch.randn(B, H, generator=g) + offset
    w = torch.randn(S, H, generator=g) / H ** 0.5
    b = 0.1 * torch.randn(S, generator=g)
    y = torch.randn(B, S, generator=g) + offset
    return h, w, b, y


def _cpu(h, w, b, y, dt):
    h, w, b = (t.detach().to(dt).clone().requires_grad_(True) for t in (h, w, b))  # never the cached inputs
    yh = h @ w.t() + b
    loss = ((yh - y.to(dt)) ** 2).mean()
    loss.backward(torch.tensor(G, dtype=dt))
    return {"loss": loss.detach().reshape(1), "y_hat": yh.detach(), "dh": h.grad, "dW": w.grad, "db": b.grad}


def _gpu(h, w, b, y):
    from models import loss as _  # noqa: F401  registers leakgnn::head_mse
    h, w, b = (t.detach().to(DEV).requires_grad_(True) for t in (h, w, b))
    loss, yh = torch.ops.leakgnn.head_mse(h, w, b, y.to(DEV))
    loss.backward(torch.tensor(G, device=DEV))
    torch.cuda.synchronize()
    return {"loss": loss.detach().reshape(1), "y_hat": yh.detach(), "dh": h.grad, "dW": w.grad, "db": b.grad}


@functools.lru_cache(maxsize=None)
def _case(name, offset=0.0):
    """(inputs, fp64 truth, fp32 yardstick) of a shape: computed once, shared by the tests, never written."""
    x = _inputs(*_shape(name), offset=offset)
    return x, _cpu(*x, torch.float64), _cpu(*x, torch.float32)


@pytest.mark.parametrize("name", list(SHAPES))
def test_head_mse_matches_fp64(name):
    x, t64, t32 = _case(name)
    got = _gpu(*x)
    assert got["y_hat"].requires_grad is False
    assert_close(got["loss"], t64["loss"], what="loss")
    assert_close(got["y_hat"], t64["y_hat"], what="y_hat")
    grads = ("dh", "dW", "db")
    assert_grads_match_truth({k: got[k] for k in grads}, {k: t32[k] for k in grads}, {k: t64[k] for k in grads})


def test_head_mse_offset_targets():
    """h and the targets near 1e3: y_hat and the loss are differences of large numbers.  Every output
    is judged against the fp32 CPU yardstick (4 x its error vs fp64, or 1e-5 of scale)."""
    x, t64, t32 = _case("65x128x29", 1e3)
    got = _gpu(*x)
    assert_grads_match_truth(got, t32, t64)


def test_head_mse_target_gets_no_gradient_and_public_function_routes():
    from models.loss import head_mse_loss, head_mse_supported
    h, w, b, y = (t.detach().to(DEV) for t in _case("3x128x29")[0])
    h.requires_grad_(True)
    y.requires_grad_(True)
    loss = head_mse_loss(h, w, b, y)
    loss.backward()
    assert y.grad is None and h.grad is not None
    assert_close(loss, _case("3x128x29")[1]["loss"][0], what="public loss")
    assert head_mse_supported(h, w, b, y)
    # outside the op's range or dtype: torch's route, same value
    wide = torch.randn(2, 1025, device=DEV)
    ww, yy = torch.randn(3, 1025, device=DEV), torch.randn(2, 3, device=DEV)
    assert not head_mse_supported(wide, ww, b[:3], yy)
    ref = torch.nn.functional.mse_loss(torch.nn.functional.linear(wide, ww, b[:3]), yy)
    assert torch.equal(head_mse_loss(wide, ww, b[:3], yy), ref)
    assert not head_mse_supported(h.double(), w.double(), b.double(), y.double())


@pytest.mark.parametrize("name", ["256x128x29", "5x100x70", "loop"])
def test_head_mse_is_deterministic(name):
    x = _case(name)[0]
    a, b = _gpu(*x), _gpu(*x)
    for k in ("loss", "dh", "dW", "db"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["1x1x1", "256x128x29", "5x100x70", "2x1024x1024"])
def test_head_mse_overwrites_every_output(name):
    """The C entry points on outputs (and scratch) pre-filled with NaN: everything comes back
    finite and equal to the op's results, so nothing is accumulated into or left unwritten."""
    from models import _native as nat
    from models.loss import _counter
    lib = nat.load_library()
    B, H, S = _shape(name)
    h, w, b, y = (t.to(DEV) for t in _case(name)[0])
    nan = float("nan")
    loss, yh, rowsq = (torch.full(s, nan, device=DEV) for s in ((), (B, S), (B,)))
    st = nat.stream_of(h)
    nat.check(lib.lg_head_mse_fwd(nat.ptr(h), nat.ptr(w), nat.ptr(b), nat.ptr(y), B, H, S, nat.ptr(yh),
                                  nat.ptr(rowsq), nat.ptr(loss), nat.ptr(_counter(DEV, st)), st), "fwd")
    dh, dw, db = (torch.full(s, nan, device=DEV) for s in ((B, H), (S, H), (S,)))
    ws = torch.full((int(lib.lg_head_mse_bwd_workspace_bytes(B, H, S)) // 4,), nan, device=DEV)
    g = torch.tensor(G, device=DEV)
    nat.check(lib.lg_head_mse_bwd(nat.ptr(h), nat.ptr(w), nat.ptr(y), nat.ptr(yh), nat.ptr(g), B, H, S, nat.ptr(dh),
                                  nat.ptr(dw), nat.ptr(db), nat.ptr(ws), ws.numel() * 4, st), "bwd")
    torch.cuda.synchronize()
    ref = _gpu(*_case(name)[0])
    for k, t in (("loss", loss.reshape(1)), ("y_hat", yh), ("dh", dh), ("dW", dw), ("db", db)):
        assert torch.isfinite(t).all(), k
        assert torch.equal(t, ref[k]), k
    assert _counter(DEV, st).item() == 0  # the launch left its ticket counter at rest
