"""Host side of the predictor's fused tail (CPU): lg_head_mse_fwd / _bwd argument validation
(LG_EINVAL before any HIP call), loss.head_mse_loss's torch route, and train_predictor's
--capture switch on the CPU."""
from __future__ import annotations

import json

import pytest
import torch
import torch.nn.functional as F

from helpers import GOLD

SENSORS = json.loads((GOLD / "harness.json").read_text())["sensors"]
P = 0x1000  # any non-null address: a call that fails its argument checks never reads it


def test_head_mse_c_abi_validation():
    from models import _native
    lib = _native.load_library()
    fwd_ok = [P, P, P, P, 4, 128, 29, P, P, P, P, None]          # stream NULL is the default stream
    bwd_ok = [P, P, P, P, P, 4, 128, 29, P, P, P, P, 1 << 40, None]
    for i in (0, 1, 2, 3, 7, 8, 9, 10):                            # each pointer in turn
        a = list(fwd_ok)
        a[i] = None
        assert lib.lg_head_mse_fwd(*a) == -1, f"fwd: null argument {i}"
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        a = list(bwd_ok)
        a[i] = None
        assert lib.lg_head_mse_bwd(*a) == -1, f"bwd: null argument {i}"
    bad_dims = [(0, 128, 29), (4, 0, 29), (4, 128, 0), (4, 1025, 29), (4, 128, 1025), (-1, 128, 29),
                (2 ** 31 // (4 * 128), 128, 29),      # B * H * 4 == 2 GiB
                (2 ** 31 // (4 * 1024), 8, 1024)]     # B * S * 4 == 2 GiB
    for B, H, S in bad_dims:
        a = list(fwd_ok)
        a[4:7] = [B, H, S]
        assert lib.lg_head_mse_fwd(*a) == -1, (B, H, S)
        a = list(bwd_ok)
        a[5:8] = [B, H, S]
        assert lib.lg_head_mse_bwd(*a) == -1, (B, H, S)
        assert lib.lg_head_mse_bwd_workspace_bytes(B, H, S) == -1, (B, H, S)
    # the workspace: one [dW | db] partial per chunk of rows, at most 256 chunks and 64 MB
    assert lib.lg_head_mse_bwd_workspace_bytes(1, 1, 1) == 2 * 4
    assert lib.lg_head_mse_bwd_workspace_bytes(256, 128, 29) == 64 * (29 * 128 + 29) * 4
    assert lib.lg_head_mse_bwd_workspace_bytes(2 ** 31 // (4 * 128) - 1, 128, 29) == 256 * (29 * 128 + 29) * 4
    assert lib.lg_head_mse_bwd_workspace_bytes(4096, 1024, 1024) <= 64 << 20
    a = list(bwd_ok)
    a[5] = 256
    a[12] = 64 * (29 * 128 + 29) * 4 - 1   # a workspace one byte below its size is refused
    assert lib.lg_head_mse_bwd(*a) == -1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_head_mse_loss_cpu_fallback_is_torch(dtype):
    from models.loss import head_mse_loss
    g = torch.Generator().manual_seed(0)
    h = torch.randn(5, 20, generator=g, dtype=dtype, requires_grad=True)
    w = torch.randn(3, 20, generator=g, dtype=dtype, requires_grad=True)
    b = torch.randn(3, generator=g, dtype=dtype, requires_grad=True)
    y = torch.randn(5, 3, generator=g, dtype=dtype)
    got = head_mse_loss(h, w, b, y)
    ref = F.mse_loss(F.linear(h, w, b), y)
    assert torch.equal(got, ref)
    gg = torch.autograd.grad(got, (h, w, b))
    gr = torch.autograd.grad(ref, (h, w, b))
    for a, r in zip(gg, gr):
        assert torch.equal(a, r)


def test_features_then_head_is_forward():
    """forward == head(features) for both predictors (CPU: the stock modules)."""
    from models.predictor import NormalPredictorGRU, NormalPredictorTCN
    g = torch.Generator().manual_seed(1)
    x, xt = torch.randn(3, 12, 5, generator=g), torch.randn(3, 12, 9, generator=g)
    for m in (NormalPredictorTCN(5, 9, num_blocks=2).eval(), NormalPredictorGRU(5, 9, hidden_size=20).eval()):
        with torch.no_grad():
            f = m.features(x, xt)
            assert f.shape == (3, m.head.in_features)
            assert torch.equal(m(x, xt), m.head(f))


@pytest.fixture(scope="module")
def normal_set(tmp_path_factory):
    from models.synth import write_synthetic_normal_set
    d = tmp_path_factory.mktemp("synth_head_mse") / "normal"
    write_synthetic_normal_set(d, SENSORS, n_windows=12, T=577, seed=0)
    return d


def _cli(normal_set, out, *extra):
    return ["--normal_root", str(normal_set), "--out_dir", str(out), "--epochs", "1", "--steps_per_epoch", "3",
            "--val_steps", "2", "--test_steps", "2", "--batch_size", "2", "--log_every", "100", *extra]


def test_train_predictor_refuses_capture_on_cpu(normal_set, tmp_path):
    from models import train_predictor
    with pytest.raises(ValueError, match="--capture on needs the GPU path"):
        train_predictor.main(_cli(normal_set, tmp_path / "out", "--device", "cpu", "--capture", "on"))


@pytest.mark.parametrize("arch", ["tcn", "gru"])
def test_train_predictor_cpu_route_with_default_capture(normal_set, tmp_path, arch):
    """--device cpu, --capture auto (the default): torch's AdamW and nn.MSELoss train one tiny epoch."""
    from models import train_predictor
    out = tmp_path / "out"
    train_predictor.main(_cli(normal_set, out, "--device", "cpu", "--arch", arch))
    ck = torch.load(out / "predictor_last.ckpt", map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "arch", "model_state", "standardizer_mean", "standardizer_std", "sensor_ids", "args"}
    assert ck["arch"] == arch and ck["args"]["capture"] == "auto"
    assert all(torch.isfinite(v).all() for v in ck["model_state"].values())
