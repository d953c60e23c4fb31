"""Host side of the device sampler (CPU, no GPU): the library's restatement of numpy's
default_rng stream (csrc/np_rng.h) against the installed numpy, and the draw code's CPU twins
(lg_draw_detector_host / lg_draw_predictor_host, the same functions the kernels run) against the
datasets' own draw(), record by record.  tests/test_gpu_sampler.py holds the kernels to the twins."""
from __future__ import annotations

import json

import numpy as np
import pytest

from helpers import GOLD

INFO = json.loads((GOLD / "harness.json").read_text())
SEEDS = list(range(2000)) + [2**31 + 5, 2**32 - 1, 2**32, 2**32 + 7, 2**40 + 3, 2**63 + 11]
COUNTS = [1, 2, 3, 7, 72, 329, 1528, 2**32, 3 * 2**30 + 1]
DS_SEEDS = (5, 2**32 + 3)
N_IDX = 2000


def bank_index(ds) -> dict:
    """Scene id -> bank row, in the order DeviceBatchLoader packs its _DeviceBank."""
    ids = ds.scene_ids if hasattr(ds, "scene_ids") else list(ds.leak_scene_ids) + list(ds.noleak_scene_ids)
    return {sid: i for i, sid in enumerate(dict.fromkeys(ids))}


def empty_some_buckets(ds, every: int = 2) -> None:
    """Replace the late and pre time lists of every `every`-th leak scene by empty arrays (the
    attribute both ds.draw and the table builder read), so that attempts are repeated."""
    empty = np.array([], dtype=np.int64)
    for sid in ds.leak_scene_ids[::every]:
        ds._bucket_times[sid] = dict(ds._bucket_times[sid], late=empty, pre=empty)


def expected_detector_records(ds, index: dict, idxs) -> np.ndarray:
    """ds.draw(i) as records; attempts (word 5) is not observable from draw() and is left 0."""
    from models.sampler import BUCKETS
    out = np.zeros((len(idxs), 8), dtype=np.int32)
    for k, i in enumerate(idxs):
        d = ds.draw(i)
        out[k, :5] = (index[d["scenario_id"]], d["t"], d["label"], d["pipe_index"], BUCKETS.index(d["bucket"]))
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from models.synth import write_synthetic_leak_set, write_synthetic_normal_set
    d = tmp_path_factory.mktemp("synthds_sampler")
    write_synthetic_normal_set(d / "normal", INFO["sensors"][:4], n_windows=7, T=120, seed=0)
    write_synthetic_leak_set(d / "leak", INFO["sensors"][:4], INFO["pipes"], scenes_per_pipe=2, n_noleak=6, T=400, seed=0)
    return d


def test_np_stream_matches_numpy():
    """random() and integers(low, low + count) alternating, bit-equal with numpy for every seed; the
    count 3 * 2^30 + 1 rejects about a quarter of its draws, so Lemire's redraw loop runs."""
    from models import sampler
    n = 4 * len(COUNTS)
    ops = [sampler.NP_RANDOM if k % 2 == 0 else sampler.NP_BOUNDED for k in range(n)]
    counts = [COUNTS[(k // 2) % len(COUNTS)] for k in range(n)]
    lows = [0 if k % 4 == 1 else 35 - 1000 * (k % 3) for k in range(n)]
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        ref_f, ref_i = np.zeros(n), np.zeros(n, dtype=np.int64)
        for k in range(n):
            if ops[k] == sampler.NP_RANDOM:
                ref_f[k] = rng.random()
            else:
                ref_i[k] = rng.integers(lows[k], lows[k] + counts[k])
        rc, f, i = sampler.np_stream_host(seed, ops, lows, counts)
        assert rc == 0
        assert np.array_equal(f.view(np.uint64), ref_f.view(np.uint64)), seed
        assert np.array_equal(i, ref_i), seed


def test_np_stream_choice_is_bounded():
    """Scalar choice over a list of n items is integers(0, n) on the same stream."""
    from models import sampler
    items = [f"s{k}" for k in range(1528)]
    for seed in (0, 7, 2**32 + 7):
        rng = np.random.default_rng(seed)
        ref = [items.index(str(rng.choice(items))), int(rng.choice(np.arange(5, 77)))]
        rc, _, i = sampler.np_stream_host(seed, [sampler.NP_BOUNDED] * 2, [0, 5], [1528, 72])
        assert rc == 0 and i.tolist() == ref


def test_np_stream_refuses_wide_ranges():
    from models import sampler
    for count in (2**32 + 1, 2**40, 0):
        rc, _, _ = sampler.np_stream_host(3, [sampler.NP_RANDOM, sampler.NP_BOUNDED], [0, 0], [1, count])
        assert rc == -1, count
    assert sampler.np_stream_host(3, [2], [0], [1])[0] == -1  # an unknown op


@pytest.mark.parametrize("seed", DS_SEEDS)
@pytest.mark.parametrize("emptied", [False, True])
def test_detector_twin_equals_dataset_draw(data, seed, emptied):
    from models import sampler
    from models.datasets import AbruptLeakDetectorDataset
    ds = AbruptLeakDetectorDataset(data / "leak", steps_per_epoch=N_IDX, seed=seed, sensor_ids=INFO["sensors"][:4])
    if emptied:
        empty_some_buckets(ds)
    index = bank_index(ds)
    rec, failed = sampler.draw_detector_host(sampler.detector_tables(ds, index), 0, N_IDX)
    want = expected_detector_records(ds, index, range(N_IDX))
    assert failed == 0
    assert np.array_equal(rec[:, :5], want[:, :5])
    assert (rec[:, 6:] == 0).all() and (rec[:, 5] >= 1).all() and (rec[:, 5] <= 10).all()
    if emptied:
        assert (rec[:, 5] >= 2).any(), "no index repeated an attempt: the emptied buckets were never drawn"
    # a later index range is the same function of (seed, idx)
    rec2, _ = sampler.draw_detector_host(sampler.detector_tables(ds, index), 700, 50)
    assert np.array_equal(rec2, rec[700:750])


def test_detector_twin_follows_replaced_scene_lists(data):
    """train_detector replaces the two scene lists after construction: the tables follow the lists
    as they are when they are built (positions in the list, bank rows as values)."""
    from models import sampler
    from models.datasets import AbruptLeakDetectorDataset
    ds = AbruptLeakDetectorDataset(data / "leak", steps_per_epoch=300, seed=11, sensor_ids=INFO["sensors"][:4])
    index = bank_index(ds)  # the bank of the full lists
    ds.leak_scene_ids = ds.leak_scene_ids[1::3][::-1]
    ds.noleak_scene_ids = ds.noleak_scene_ids[:2]
    rec, failed = sampler.draw_detector_host(sampler.detector_tables(ds, index), 0, 300)
    assert failed == 0 and np.array_equal(rec[:, :5], expected_detector_records(ds, index, range(300))[:, :5])


def test_detector_twin_counts_exhausted_samples(data):
    """Every leak bucket empty: a sample whose ten attempts all pick a leak scene fails; its record
    is all -1 and the error word counts it, at the indices where ds.draw raises."""
    from models import sampler
    from models.datasets import AbruptLeakDetectorDataset
    ds = AbruptLeakDetectorDataset(data / "leak", steps_per_epoch=64, seed=5, sensor_ids=INFO["sensors"][:4])
    empty_all_leak_buckets(ds)
    raised = []
    for i in range(64):
        try:
            ds.draw(i)
        except RuntimeError:
            raised.append(i)
    assert raised, "no index of the 64 exhausts its attempts"
    rec, failed = sampler.draw_detector_host(sampler.detector_tables(ds, bank_index(ds)), 0, 64)
    assert failed == len(raised)
    assert np.flatnonzero(rec[:, 2] < 0).tolist() == raised
    assert (rec[raised, :5] == -1).all() and (rec[raised, 5] == 10).all()


def empty_all_leak_buckets(ds) -> None:
    empty = np.array([], dtype=np.int64)
    for sid in ds.leak_scene_ids:
        ds._bucket_times[sid] = {"early": empty, "late": empty, "pre": empty}


@pytest.mark.parametrize("seed", DS_SEEDS)
def test_predictor_twin_equals_dataset_draw(data, seed):
    from models import sampler
    from models.datasets import NormalPredictorDataset
    ds = NormalPredictorDataset(data / "normal", steps_per_epoch=N_IDX, seed=seed)
    index = bank_index(ds)
    rec, failed = sampler.draw_predictor_host(sampler.predictor_tables(ds, index), 0, N_IDX)
    assert failed == 0
    want = [ds.draw(i) for i in range(N_IDX)]
    assert [(index[s], t) for s, t in want] == [tuple(r) for r in rec[:, :2].tolist()]
    assert (rec[:, 2] == 0).all() and (rec[:, 3:5] == -1).all() and (rec[:, 5] == 1).all()
    assert len({r[0] for r in rec.tolist()}) == len(ds.scene_ids) and len({r[1] for r in rec.tolist()}) > 40


def test_table_builders_refuse_what_the_device_cannot_draw(data):
    from models import sampler
    from models.datasets import AbruptLeakDetectorDataset, NormalPredictorDataset
    nds = NormalPredictorDataset(data / "normal", l_in_steps=119, horizon_steps=2, steps_per_epoch=4, seed=1)
    with pytest.raises(ValueError, match="Scene too short"):  # T = 120 < l_in + h: raised at construction
        sampler.predictor_tables(nds, bank_index(nds))
    ds = AbruptLeakDetectorDataset(data / "leak", steps_per_epoch=4, seed=1, sensor_ids=INFO["sensors"][:4])
    index = bank_index(ds)
    sid = ds.leak_scene_ids[0]
    keep = ds._bucket_times[sid]
    ds._bucket_times[sid] = dict(keep, late=np.array([300, 302, 303]))
    with pytest.raises(ValueError, match="contiguous"):
        sampler.detector_tables(ds, index)
    ds._bucket_times[sid] = dict(keep, late=np.arange(390, 401))
    with pytest.raises(ValueError, match="leave the scene"):
        sampler.detector_tables(ds, index)
    ds._bucket_times[sid] = keep
    ds.seed = -1
    with pytest.raises(ValueError, match="seed"):
        sampler.detector_tables(ds, index)
    ds.seed = 2**64 - 3
    with pytest.raises(ValueError, match="seed"):
        sampler.detector_tables(ds, index)


def test_draw_and_gather_c_abi_validation():
    """LG_EINVAL before any HIP call for null pointers and sizes out of range; n == 0 is LG_OK."""
    from models import _native
    lib = _native.load_library()
    P = 0x1000
    cum = np.array([0.3, 0.6, 0.8, 1.0])
    # seed, i0, n, leak_list, n_leak, noleak_list, n_noleak, times, pipe, n_scenes, cum_host, nlc, records, err, stream
    ok = [5, 0, 0, P, 3, P, 2, P, P, 5, cum.ctypes.data, 4, P, P, None]
    assert lib.lg_draw_detector(*ok) == 0
    for i, vals in {1: [-1], 2: [-1, (1 << 20) + 1], 3: [None], 4: [0, 2**31], 5: [None], 6: [0], 7: [None],
                    8: [None], 9: [0, 2**31], 10: [None], 11: [-1], 13: [None]}.items():
        for v in vals:
            a = list(ok)
            a[i] = v
            assert lib.lg_draw_detector(*a) == -1, f"argument {i} = {v}"
    bad = np.array([0.3, 0.2, 0.8, 1.0])
    a = list(ok)
    a[10] = bad.ctypes.data
    assert lib.lg_draw_detector(*a) == -1
    # seed, i0, n, scene_list, n_list, scene_len, n_scenes, l_in, h, records, err, stream
    okp = [5, 0, 0, P, 3, P, 3, 36, 1, P, P, None]
    assert lib.lg_draw_predictor(*okp) == 0
    for i, vals in {1: [-1], 2: [-1, (1 << 20) + 1], 3: [None], 4: [0], 5: [None], 6: [0], 7: [0], 8: [-1],
                    10: [None]}.items():
        for v in vals:
            a = list(okp)
            a[i] = v
            assert lib.lg_draw_predictor(*a) == -1, f"argument {i} = {v}"
    # records, n, n_scenes, T_max, 3 x (src, C, off, len, dst), label, pipe_index, bucket_code, err, stream
    okg = [P, 0, 5, 400, P, 29, -71, 72, P, P, 9, -71, 72, P, None, 0, 0, 0, None, P, P, P, P, None]
    assert lib.lg_gather_windows(*okg) == 0
    for i, vals in {1: [-1], 2: [0], 3: [0], 5: [0], 6: [-401], 7: [0, 401], 22: [None]}.items():
        for v in vals:
            a = list(okg)
            a[i] = v
            assert lib.lg_gather_windows(*a) == -1, f"argument {i} = {v}"


def test_abi_version_and_names():
    from models import _native
    lib = _native.load_library()
    assert lib.lg_abi_version() == 26 == _native.ABI_VERSION
    for name in ("lg_draw_detector", "lg_draw_predictor", "lg_gather_windows", "lg_np_stream_host",
                 "lg_draw_detector_host", "lg_draw_predictor_host"):
        assert name in _native.SIGNATURES and hasattr(lib, name)


def test_loader_draw_argument():
    """draw="host" stays the default; an unknown mode is refused; draw="device" has no CPU path."""
    import inspect

    import torch

    from models.datasets import DeviceBatchLoader
    sig = inspect.signature(DeviceBatchLoader.__init__)
    assert sig.parameters["draw"].default == "host"
    assert list(sig.parameters)[1:6] == ["ds", "batch_size", "device", "shard", "draw"]
    with pytest.raises(ValueError, match="draw must be"):
        DeviceBatchLoader(object(), 8, torch.device("cpu"), draw="gpu")
