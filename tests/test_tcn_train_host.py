"""NormalPredictorTCN training on the library: the parts that need no GPU (module tree, CPU forward,
the new entry points' bindings and argument checks, the training tables, op registration)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

EINVAL, EUNSUP = -1, -2
F = 64  # a non-null address that is never read: every call below is rejected before a launch


def _lib():
    from models import _native
    return _native.load_library()


def test_entry_points_and_ops_exposed():
    from models import _native, library, ops  # noqa: F401
    lib = _lib()
    for name in ("lg_tcn_conv_train_fwd", "lg_tcn_conv_bwd", "lg_tcn_conv_bwd_workspace_bytes", "lg_tcn_pack_weight_t"):
        assert name in _native.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.lg_abi_version() == _native.ABI_VERSION == 26
    assert ops.TCN_SALT == 400
    for op in ("tcn_predictor", "tcn_predictor_backward"):
        assert hasattr(torch.ops.leakgnn, op)
        assert getattr(torch.ops.leakgnn, op).default is not None
    # a fake for each op, an autograd formula on the forward op
    assert library.tcn_predictor._abstract_fn is not None and library.tcn_predictor_backward._abstract_fn is not None
    assert library.tcn_predictor._backward_fn is library._tcn_predictor_bwd
    assert library.tcn_predictor._setup_context_fn is library._tcn_predictor_setup


def _train_fwd(lib, *, C=128, nseg=4, rows_in=36, rows_blk=0, rows_out=36, p=0.25, inp=F, blk=None, s=F, out=None,
               xhat=F, rstd=F, salt=400):
    return lib.lg_tcn_conv_train_fwd(inp, blk, F, F, F, F, F, 1e-5, p, 7, salt, s, out, xhat, rstd, nseg, rows_in,
                                     rows_blk, rows_out, C, None)


def test_train_fwd_rejections():
    lib = _lib()
    assert _train_fwd(lib, C=64) == EUNSUP
    assert _train_fwd(lib, rows_out=2049, rows_in=2049) == EUNSUP
    assert _train_fwd(lib, nseg=2 ** 22, rows_in=1, rows_out=1) == EUNSUP       # a 2 GiB tensor
    assert _train_fwd(lib, nseg=2 ** 22 - 1, rows_in=2, rows_out=1) == EUNSUP   # ... the input alone
    assert _train_fwd(lib, inp=None) == EINVAL
    assert _train_fwd(lib, s=None) == EINVAL
    assert _train_fwd(lib, blk=F, rows_blk=36, out=None) == EINVAL              # a residual needs out
    assert _train_fwd(lib, blk=F, rows_blk=0, out=F) == EINVAL
    assert _train_fwd(lib, xhat=None) == EINVAL                                  # xhat and rstd: both or neither
    assert _train_fwd(lib, p=1.0) == EINVAL and _train_fwd(lib, p=-0.1) == EINVAL
    assert _train_fwd(lib, rows_in=0) == EINVAL and _train_fwd(lib, nseg=-1) == EINVAL
    assert _train_fwd(lib, p=0.0, xhat=None, rstd=None, s=None, out=None) == EINVAL  # nowhere to write
    assert _train_fwd(lib, nseg=0) == 0
    assert _train_fwd(lib, nseg=0, p=0.0, xhat=None, rstd=None) == 0


def _bwd(lib, *, C=128, nseg=4, rows_in=36, rows_res=0, rows_out=36, p=0.25, dy=F, dres=None, plan_t=F, pkt=F, dx=F,
         dw=F, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.lg_tcn_conv_bwd_workspace_bytes(nseg, rows_out, 128)
    return lib.lg_tcn_conv_bwd(dy, F, F, F, F, dres, F, plan_t, pkt, F, p, F, dx, dw, F, F, F, nseg, rows_in, rows_res,
                               rows_out, C, ws, ws_bytes, None)


def test_bwd_rejections_and_workspace():
    lib = _lib()
    # per 32 rows one [dgamma | dbeta | db] partial, per 64 rows one 128 x 384 dW partial
    for nseg, rows in ((1, 1), (40, 36), (256, 36)):
        total = nseg * rows
        need = lib.lg_tcn_conv_bwd_workspace_bytes(nseg, rows, 128)
        assert need >= 4 * (-(-total // 32) * 384 + -(-total // 64) * 128 * 384)
        assert _bwd(lib, nseg=nseg, rows_in=rows, rows_out=rows, ws_bytes=need - 1) == EINVAL
    assert -(-9216 // 64) * 3 > 256  # more than 256 dW workgroups at the training shape (256 x 36 rows)
    assert lib.lg_tcn_conv_bwd_workspace_bytes(4, 36, 64) == 0
    assert _bwd(lib, ws=None) == EINVAL
    assert _bwd(lib, C=64) == EUNSUP
    assert _bwd(lib, rows_out=2049) == EUNSUP
    assert _bwd(lib, rows_in=2049) == EUNSUP and _bwd(lib, rows_in=2049, dx=None, plan_t=None, pkt=None, ws_bytes=0) == EINVAL
    assert _bwd(lib, nseg=2 ** 22, rows_in=1, rows_out=1, ws_bytes=2 ** 40) == EUNSUP
    assert _bwd(lib, dy=None) == EINVAL and _bwd(lib, dw=None) == EINVAL
    assert _bwd(lib, plan_t=None) == EINVAL and _bwd(lib, pkt=None) == EINVAL   # dx needs the transposed forms
    assert _bwd(lib, dres=F, rows_res=0) == EINVAL
    assert _bwd(lib, dx=None, dres=F, rows_res=36) == EINVAL
    assert _bwd(lib, p=1.0) == EINVAL
    assert _bwd(lib, nseg=0, ws_bytes=0) == 0
    assert lib.lg_tcn_pack_weight_t(F, F, 64, None) == EUNSUP and lib.lg_tcn_pack_weight_t(None, F, 128, None) == EINVAL


@pytest.mark.parametrize("L", [1, 5, 36])
def test_train_tables_brute_force(L):
    from models.tcn_plan import train_tables
    dil = (1, 2, 4, 8)
    fwd, tr = train_tables(L, dil)
    assert len(fwd) == len(tr) == 8
    for i in range(8):
        d, conv2 = dil[i // 2], i % 2 == 1
        assert fwd[i].shape == tr[i].shape == (L, 4) and fwd[i].dtype == tr[i].dtype == np.int32
        want_f = np.full((L, 4), -1, dtype=np.int32)
        want_t = np.full((L, 4), -1, dtype=np.int32)
        for t in range(L):
            for j in range(3):
                if t - j * d >= 0:
                    want_f[t, j] = t - j * d
            want_f[t, 3] = t if conv2 else -1
        for u in range(L):                      # transposed: the output row that reads u through tap j
            for j in range(3):
                readers = [t for t in range(L) if want_f[t, j] == u]
                assert len(readers) <= 1
                if readers:
                    want_t[u, j] = readers[0]
            want_t[u, 3] = -1 if conv2 else u
        assert np.array_equal(fwd[i], want_f), i
        assert np.array_equal(tr[i], want_t), i
    again = train_tables(L, dil)
    assert again[0][0] is fwd[0]  # cached


def test_state_dict_and_cpu_forward():
    import torch.nn.functional as Fn
    from models.predictor import NormalPredictorTCN
    torch.manual_seed(0)
    m = NormalPredictorTCN(29, 9)
    keys = ["input_proj.weight", "input_proj.bias"]
    for b in range(4):
        for n in ("conv1.conv.weight", "conv1.conv.bias", "conv2.conv.weight", "conv2.conv.bias", "norm1.weight",
                  "norm1.bias", "norm2.weight", "norm2.bias"):
            keys.append(f"tcn.{b}.{n}")
    assert list(m.state_dict()) == keys + ["head.weight", "head.bias"]
    assert [n for n, _ in m.named_children()] == ["input_proj", "tcn", "head"]
    x, tf = torch.randn(3, 7, 29), torch.randn(3, 7, 9)

    def stock(mod):
        h = mod.input_proj(torch.cat([x, tf], -1).transpose(1, 2))
        for blk in mod.tcn:
            r = h
            for conv, norm in ((blk.conv1, blk.norm1), (blk.conv2, blk.norm2)):
                y = conv.conv(h)[..., :-conv.pad]
                h = blk.dropout(Fn.relu(norm(y.transpose(1, 2)))).transpose(1, 2)
            h = r + h
        return mod.head(h[:, :, -1])

    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x, tf), stock(m))
    out = m(x, tf)                      # grad enabled, CPU: still the stock module
    assert torch.equal(out, stock(m)) and out.requires_grad
    m.train()
    torch.manual_seed(3)
    a = m(x, tf)
    torch.manual_seed(3)
    assert torch.equal(a, stock(m))


def test_hip_train_shape_predicate():
    from models.predictor import NormalPredictorTCN
    assert NormalPredictorTCN(29, 9)._hip_train_shape(256, 36)
    assert NormalPredictorTCN(29, 9, num_blocks=1)._hip_train_shape(2, 1)
    assert NormalPredictorTCN(29, 9, num_blocks=6)._hip_train_shape(2, 2048)
    assert not NormalPredictorTCN(29, 9)._hip_train_shape(2, 2049)
    assert not NormalPredictorTCN(29, 9, hidden_channels=64)._hip_train_shape(2, 36)
    assert not NormalPredictorTCN(29, 9, kernel_size=5)._hip_train_shape(2, 36)
    assert not NormalPredictorTCN(29, 9)._hip_train_shape(2 ** 16, 64)   # 2 GiB of activations: stock


def test_op_shape_checks():
    from models import library
    C = 128
    x = torch.zeros(2, 5, C)
    good = dict(conv_w=[torch.zeros(C, C, 3)] * 2, conv_b=[torch.zeros(C)] * 2, ln_w=[torch.zeros(C)] * 2,
                ln_b=[torch.zeros(C)] * 2)
    assert library._tcn_dims(x, **good) == (2, 5, 2)
    for key, bad in (("conv_w", [torch.zeros(C, C, 3)]), ("conv_w", [torch.zeros(C, C, 5)] * 2),
                     ("ln_b", [torch.zeros(C), torch.zeros(64)]), ("conv_b", [torch.zeros(C)] * 3)):
        with pytest.raises(ValueError):
            library._tcn_dims(x, **{**good, key: bad})
    with pytest.raises(ValueError):
        library._tcn_dims(torch.zeros(2, 5, 64), **good)
    with pytest.raises(ValueError):
        library._tcn_dims(torch.zeros(1, 2049, C), **good)
