"""Host side of the stacked-GRU entry points (no GPU): argument validation of lg_gru_seq_fwd /
lg_gru_seq_bwd (LG_EINVAL / LG_EUNSUPPORTED before any HIP call, with stand-in device
pointers), the workspace query's byte budget, and the detector's constructor arguments."""
from __future__ import annotations

import pytest
import torch

from conftest import LTA_INP
from helpers import lta_ids

EINVAL, EUNSUPPORTED = -1, -2
F = 16  # a non-NULL stand-in device pointer (never dereferenced on these paths)
LG_F_DROPOUT, LG_F_RELU = 0x04, 0x02


def _lib():
    from models import _native
    return _native.load_library()


def test_seq_fwd_validation():
    lib = _lib()
    ok = [F, F, F, F, F, F, F, 33, 36, 64, 64, 0, 0.0, 0, 0, None]
    for i in range(6):  # x, the four parameters, h_seq (gates may be NULL)
        a = list(ok)
        a[i] = None
        assert lib.lg_gru_seq_fwd(*a) == EINVAL, i
    for i, v, rc in [(7, -1, EINVAL), (8, 0, EINVAL), (9, 0, EINVAL), (10, 0, EINVAL), (10, 1025, EUNSUPPORTED),
                     (9, 1025, EUNSUPPORTED), (11, LG_F_RELU, EUNSUPPORTED)]:
        a = list(ok)
        a[i] = v
        assert lib.lg_gru_seq_fwd(*a) == rc, (i, v)
    a = list(ok)
    a[11], a[12] = LG_F_DROPOUT, 1.0
    assert lib.lg_gru_seq_fwd(*a) == EINVAL
    a = list(ok)
    a[7] = 0  # no sequences: nothing to launch
    assert lib.lg_gru_seq_fwd(*a) == 0


def test_seq_bwd_validation():
    lib = _lib()
    ws = lib.lg_gru_seq_bwd_workspace_bytes(33, 64, 64)

    def dense(**kw):
        a = dict(x=F, residual=None, tfeat=None, w_ih=F, w_hh=F, h_seq=F, gates=F, dh_seq=F, dh_last=F, dx=F, dw_ih=F,
                 dw_hh=F, db_ih=F, db_hh=F, B=0, S=0, Nseq=33, L=36, I=64, H=64, flags=0, p=0.0, seed=0, salt=0,
                 ws=F, ws_bytes=ws, stream=None)
        a.update(kw)
        return lib.lg_gru_seq_bwd(*a.values())

    for k in ("w_ih", "w_hh", "h_seq", "gates", "dw_ih", "dw_hh", "db_ih", "db_hh", "ws"):
        assert dense(**{k: None}) == EINVAL, k
    assert dense(x=None) == EINVAL                      # neither input form
    assert dense(dh_seq=None, dh_last=None) == EINVAL   # no upstream gradient at all
    assert dense(L=0) == EINVAL and dense(H=0) == EINVAL and dense(I=0) == EINVAL and dense(Nseq=-1) == EINVAL
    assert dense(H=1025) == EUNSUPPORTED and dense(I=1025) == EUNSUPPORTED
    assert dense(ws_bytes=ws - 1) == EINVAL
    assert dense(flags=LG_F_DROPOUT, p=-0.5) == EINVAL
    assert dense(flags=LG_F_RELU) == EUNSUPPORTED
    # the encoder input form: B * S == Nseq, I in {1, 10}, tfeat with I = 10, no dropout
    enc = dict(x=None, residual=F, tfeat=F, B=3, S=11, I=10, ws_bytes=lib.lg_gru_seq_bwd_workspace_bytes(33, 10, 64))
    assert dense(**{**enc, "S": 10}) == EINVAL
    assert dense(**{**enc, "tfeat": None}) == EINVAL
    assert dense(**{**enc, "I": 5}) == EUNSUPPORTED
    assert dense(**{**enc, "flags": LG_F_DROPOUT, "p": 0.1}) == EUNSUPPORTED
    assert dense(**{**enc, "ws_bytes": 4 * (3 * 64 * (64 + 10) + 6 * 64)}) == EINVAL  # one slab row of the 3 needed


def test_seq_bwd_workspace_query():
    lib = _lib()
    q = lib.lg_gru_seq_bwd_workspace_bytes
    assert q(-1, 64, 64) == EINVAL and q(5, 0, 64) == EINVAL and q(5, 64, 0) == EINVAL and q(5, 64, 1025) == EINVAL
    budget = 256 << 20
    for I, H in [(64, 64), (10, 64), (48, 48), (10, 17), (1024, 1024), (1, 1024)]:
        prev = 0
        for n in (0, 1, 15, 16, 17, 33, 500, 512, 513, 7424, 1 << 20):
            b = q(n, I, H)
            assert b > 0 and b >= prev, (I, H, n)
            prev = b
        row = 4 * (3 * H * (H + I) + 6 * H)
        assert q(1, I, H) == row
        if I == H and H in (32, 64):  # the dense tiled kernel: one row per 16 sequences
            assert q(33, I, H) == 3 * row
        if H not in (32, 64):  # the generic kernel: at most 512 rows, within the budget (or one row)
            assert prev <= max(row, min(budget, 512 * row)), (I, H)
    assert q(1 << 20, 1024, 1024) <= budget
    assert q(1 << 20, 1024, 1024) == q(1 << 21, 1024, 1024)  # capped


def test_detector_constructor_sensor_layers():
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    base = LeakDetector(LTA_INP, sensors, pipes)
    m = LeakDetector(LTA_INP, sensors, pipes, sensor_layers=2, sensor_dropout=0.2)
    extra = set(m.state_dict()) - set(base.state_dict())
    assert extra == {f"sensor_encoder.gru.{n}_l1" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    assert m.sensor_encoder.gru.num_layers == 2 and m.sensor_encoder.gru.dropout == 0.2
    m2 = LeakDetector(LTA_INP, sensors, pipes, sensor_layers=2)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(m2.sensor_encoder.gru.weight_ih_l1, m.sensor_encoder.gru.weight_ih_l1)
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 36, 29), torch.zeros(2, 36, 9))
