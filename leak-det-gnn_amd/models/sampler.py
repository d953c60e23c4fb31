"""Device sampler behind ``DeviceBatchLoader(draw="device")`` (csrc/sampler.hip).

A dataset's sample idx is a pure function of ``np.random.default_rng(seed + idx)``.  The draw
kernels replay that numpy stream on the device (csrc/np_rng.h), so the per-sample decisions
(scene, time step, label, bucket) of a whole epoch are one launch per 2^20 samples and the
batches are bit-identical to the host path's.  This module holds what the kernels read:

  detector_tables / predictor_tables   the dataset's lists and time ranges as int32 arrays keyed
                                       to the scene order of the HBM bank, built once per loader;
  draw_detector_host / draw_predictor_host / np_stream_host
                                       the CPU twins of the draw code (tests, no device needed);
  DeviceSampler                        tables on the device + the draw and gather launches.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _native

BUCKETS = ("early", "late", "pre", "noleak")  # bucket codes of a record (window_evaluator._BUCKETS)
RECORD = 8                                    # int32 words per record (LG_DRAW_RECORD)
MAX_SAMPLES = 1 << 20                         # samples per draw launch (LG_DRAW_MAX_SAMPLES)
NP_RANDOM, NP_BOUNDED = 0, 1                  # lg_np_stream_host script ops
FAILED = "Failed to sample a valid (scenario, time) after multiple attempts. Check data lengths/buckets."


@dataclass
class DetectorTables:
    leak_list: np.ndarray    # int32 [n_leak]: bank index of each entry of ds.leak_scene_ids
    noleak_list: np.ndarray  # int32 [n_noleak]
    times: np.ndarray        # int32 [n_scenes, 4, 2]: (start, count) of the scene's time list per bucket
    pipe: np.ndarray         # int32 [n_scenes]: pipe index, -1 for a no-leak scene
    cum: np.ndarray          # float64 [4]
    no_leak_class: int
    seed: int


@dataclass
class PredictorTables:
    scene_list: np.ndarray   # int32 [n_list]: bank index of each entry of ds.scene_ids
    scene_len: np.ndarray    # int32 [n_scenes]
    l_in: int
    h: int
    seed: int


def _check_seed(seed: int, n: int) -> int:
    if seed < 0 or seed + n > 1 << 64:
        raise ValueError(f"device draw needs 0 <= seed and seed + len(ds) <= 2^64 (seed {seed}, {n} samples)")
    return int(seed)


def _span(times: np.ndarray, t_min: int, T: int, what: str) -> Tuple[int, int]:
    """(start, count) of a time list, which must be a contiguous arange inside [t_min, T)."""
    a = np.asarray(times)
    if a.size == 0:
        return 0, 0
    start = int(a[0])
    if a.ndim != 1 or not np.array_equal(a, np.arange(start, start + a.size)):
        raise ValueError(f"{what}: the time list is not a contiguous range; the device draw cannot represent it")
    if start < t_min or start + a.size > T:
        raise ValueError(f"{what}: times [{start}, {start + a.size}) leave the scene's windows [{t_min}, {T})")
    return start, int(a.size)


def detector_tables(ds, index: Dict[str, int]) -> DetectorTables:
    """Tables of an AbruptLeakDetectorDataset from its CURRENT leak_scene_ids / noleak_scene_ids,
    _bucket_times, _noleak_times, _pipe_idx and _cum; `index` maps a scene id to its bank row."""
    if not ds.leak_scene_ids or not ds.noleak_scene_ids:
        raise ValueError("device draw needs at least one leak scene and one no-leak scene")
    n_scenes = len(index)
    times = np.zeros((n_scenes, 4, 2), dtype=np.int32)
    pipe = np.full((n_scenes,), -1, dtype=np.int32)
    t_min = ds.seg_len - 1
    for sid in dict.fromkeys(ds.leak_scene_ids):
        if sid not in ds._bucket_times or sid not in ds._pipe_idx:
            raise ValueError(f"leak scene {sid} has no bucket times")
        s = index[sid]
        pipe[s] = int(ds._pipe_idx[sid])
        for b, name in enumerate(BUCKETS[:3]):
            times[s, b] = _span(ds._bucket_times[sid][name], t_min, ds._T[sid], f"{sid}/{name}")
    for sid in dict.fromkeys(ds.noleak_scene_ids):
        if sid not in ds._noleak_times:
            raise ValueError(f"no-leak scene {sid} has no times")
        times[index[sid], 3] = _span(ds._noleak_times[sid], t_min, ds._T[sid], f"{sid}/noleak")
    return DetectorTables(
        leak_list=np.array([index[s] for s in ds.leak_scene_ids], dtype=np.int32),
        noleak_list=np.array([index[s] for s in ds.noleak_scene_ids], dtype=np.int32),
        times=times, pipe=pipe, cum=np.ascontiguousarray(ds._cum, dtype=np.float64),
        no_leak_class=int(ds.no_leak_class), seed=_check_seed(ds.seed, len(ds)))


def predictor_tables(ds, index: Dict[str, int]) -> PredictorTables:
    """Tables of a NormalPredictorDataset.  A listed scene shorter than l_in + h raises here (the
    host path raises only when such a scene is drawn)."""
    if not ds.scene_ids:
        raise ValueError("device draw needs at least one scene")
    scene_len = np.zeros((len(index),), dtype=np.int32)
    for sid in dict.fromkeys(ds.scene_ids):
        T = int(ds._scene_len(sid))
        if T - ds.h - 1 < ds.l_in - 1:
            raise ValueError(f"Scene too short for l_in={ds.l_in}, h={ds.h}: {sid} (T={T})")
        scene_len[index[sid]] = T
    return PredictorTables(scene_list=np.array([index[s] for s in ds.scene_ids], dtype=np.int32),
                           scene_len=scene_len, l_in=int(ds.l_in), h=int(ds.h), seed=_check_seed(ds.seed, len(ds)))


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


# ---------------------------------------------------------------------------- CPU twins
def np_stream_host(seed: int, ops: Sequence[int], low: Sequence[int], count: Sequence[int]):
    """Replay a script on default_rng(seed) through the library's CPU twin: (rc, doubles, integers)."""
    lib = _native.load_library()
    o = np.ascontiguousarray(ops, dtype=np.int32)
    lo = np.ascontiguousarray(low, dtype=np.int64)
    c = np.ascontiguousarray(count, dtype=np.uint64)
    f = np.zeros(o.size, dtype=np.float64)
    i = np.zeros(o.size, dtype=np.int64)
    rc = lib.lg_np_stream_host(int(seed), _np_ptr(o), _np_ptr(lo), _np_ptr(c), o.size, _np_ptr(f), _np_ptr(i))
    return rc, f, i


def draw_detector_host(tb: DetectorTables, i0: int, n: int) -> Tuple[np.ndarray, int]:
    """(records int32 (n, 8), failed samples) of sample indices [i0, i0 + n), on the CPU."""
    lib = _native.load_library()
    rec = np.zeros((n, RECORD), dtype=np.int32)
    err = np.zeros(2, dtype=np.uint32)
    _native.check(lib.lg_draw_detector_host(tb.seed, i0, n, _np_ptr(tb.leak_list), tb.leak_list.size,
                                            _np_ptr(tb.noleak_list), tb.noleak_list.size, _np_ptr(tb.times),
                                            _np_ptr(tb.pipe), tb.pipe.size, _np_ptr(tb.cum), tb.no_leak_class,
                                            _np_ptr(rec), _np_ptr(err)), "lg_draw_detector_host")
    return rec, int(err[0])


def draw_predictor_host(tb: PredictorTables, i0: int, n: int) -> Tuple[np.ndarray, int]:
    lib = _native.load_library()
    rec = np.zeros((n, RECORD), dtype=np.int32)
    err = np.zeros(2, dtype=np.uint32)
    _native.check(lib.lg_draw_predictor_host(tb.seed, i0, n, _np_ptr(tb.scene_list), tb.scene_list.size,
                                             _np_ptr(tb.scene_len), tb.scene_len.size, tb.l_in, tb.h,
                                             _np_ptr(rec), _np_ptr(err)), "lg_draw_predictor_host")
    return rec, int(err[0])


# ---------------------------------------------------------------------------- device side
class DeviceSampler:
    """Tables of one dataset on the device and the launches over them.  `kind` is "detector" or
    "predictor"; `bank` the loader's _DeviceBank (scene order = the tables' scene index)."""

    def __init__(self, ds, bank, kind: str) -> None:
        if bank.device.type != "cuda":
            raise RuntimeError(f"draw='device' runs only on a ROCm GPU (loader device {bank.device}); there is no CPU path")
        self.ds, self.bank, self.kind = ds, bank, kind
        self.device = bank.device
        self.scene_ids: List[str] = list(bank.index)
        self.n_scenes, self.T_max = int(bank.noisy.shape[0]), int(bank.noisy.shape[1])
        self.S = int(bank.noisy.shape[2])
        up = lambda a: torch.from_numpy(a).to(self.device)  # noqa: E731
        if kind == "detector":
            self.tb = detector_tables(ds, bank.index)
            self._dev = [up(self.tb.leak_list), up(self.tb.noleak_list), up(self.tb.times), up(self.tb.pipe)]
        elif kind == "predictor":
            self.tb = predictor_tables(ds, bank.index)
            self._dev = [up(self.tb.scene_list), up(self.tb.scene_len)]
        else:
            raise ValueError(kind)
        self._const: Dict[Tuple[int, int], torch.Tensor] = {}
        self._lib = _native.load_library()

    def new_error_words(self) -> torch.Tensor:
        return torch.zeros(2, dtype=torch.int32, device=self.device)

    def draw_range(self, i0: int, n: int, err: torch.Tensor) -> torch.Tensor:
        """Records (n, 8) int32 of sample indices [i0, i0 + n): ceil(n / 2^20) launches, no read-back."""
        rec = torch.empty((n, RECORD), dtype=torch.int32, device=self.device)
        st = _native.stream_of(rec)
        tb = self.tb
        for c0 in range(0, n, MAX_SAMPLES):
            m = min(MAX_SAMPLES, n - c0)
            out = rec[c0:c0 + m]
            if self.kind == "detector":
                ll, nl, tm, pp = self._dev
                rc = self._lib.lg_draw_detector(tb.seed, i0 + c0, m, ll.data_ptr(), ll.numel(), nl.data_ptr(),
                                                nl.numel(), tm.data_ptr(), pp.data_ptr(), self.n_scenes,
                                                _np_ptr(tb.cum), tb.no_leak_class, out.data_ptr(), err.data_ptr(), st)
                _native.check(rc, "lg_draw_detector")
            else:
                sl, ln = self._dev
                rc = self._lib.lg_draw_predictor(tb.seed, i0 + c0, m, sl.data_ptr(), sl.numel(), ln.data_ptr(),
                                                 self.n_scenes, tb.l_in, tb.h, out.data_ptr(), err.data_ptr(), st)
                _native.check(rc, "lg_draw_predictor")
        return rec

    def _full(self, n: int, value: int) -> torch.Tensor:
        key = (n, value)
        if key not in self._const:
            self._const[key] = torch.full((n,), value, dtype=torch.long, device=self.device)
        return self._const[key]

    def gather(self, rec: torch.Tensor, lo: int, hi: int, err: torch.Tensor) -> Dict[str, Any]:
        """The batch of records [lo, hi) as device tensors: one launch."""
        ds, bank, dev = self.ds, self.bank, self.device
        n = max(hi - lo, 0)
        r = rec[lo:lo + n]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        if self.kind == "detector":
            L = ds.seg_len
            a, b = f32(n, L, self.S), f32(n, L, 9)
            label = torch.empty((n,), dtype=torch.long, device=dev)
            pipe = torch.empty((n,), dtype=torch.long, device=dev)
            code = torch.empty((n,), dtype=torch.int32, device=dev)
            segs = [(bank.noisy, self.S, -(L - 1), L, a), (bank.time_feat, 9, -(L - 1), L, b), None]
            outs = (label.data_ptr(), pipe.data_ptr(), code.data_ptr())
            batch = {"noisy_seg": a, "time_seg": b, "label": label, "pipe_index": pipe,
                     "num_classes": self._full(n, ds.num_pipes + 1), "l_pred": self._full(n, ds.l_pred),
                     "l_det": self._full(n, ds.l_det), "bucket_code": code}
        else:
            x, xt, y = f32(n, ds.l_in, self.S), f32(n, ds.l_in, 9), f32(n, ds.h, self.S)
            segs = [(bank.noisy, self.S, -(ds.l_in - 1), ds.l_in, x), (bank.time_feat, 9, -(ds.l_in - 1), ds.l_in, xt),
                    (bank.gt, self.S, 1, ds.h, y) if ds.h > 0 else None]
            outs = (None, None, None)
            batch = {"x": x, "x_time": xt, "y": y}
        batch["scene"], batch["t_index"] = r[:, 0], r[:, 1]
        if n > 0:
            args: list = []
            for s in segs:
                args += [None, 0, 0, 0, None] if s is None else [s[0].data_ptr(), s[1], s[2], s[3], s[4].data_ptr()]
            rc = self._lib.lg_gather_windows(r.data_ptr(), n, self.n_scenes, self.T_max, *args, *outs, err.data_ptr(),
                                             _native.stream_of(rec))
            _native.check(rc, "lg_gather_windows")
        return batch

    def materialize(self, batch: Dict[str, Any]) -> Dict[str, Any]:
        """Read a device-mode batch back into exactly the dict the host mode yields."""
        scene = batch["scene"].cpu().tolist()
        t = batch["t_index"].cpu().tolist()
        if any(s < 0 for s in scene):
            raise RuntimeError(FAILED)
        stamps = [str(self.bank.timestamps[s][ti]) for s, ti in zip(scene, t)]
        ids = [self.scene_ids[s] for s in scene]
        out = {k: v for k, v in batch.items() if k not in ("scene", "t_index", "bucket_code")}
        if self.kind == "predictor":
            out.update({"scene_id": ids, "t": stamps})
            return out
        pipes = batch["pipe_index"].cpu().tolist()
        names = [self.ds._idx_to_pipe.get(p) if p >= 0 else None for p in pipes]
        out.update({"scenario_id": ids, "bucket": [BUCKETS[c] for c in batch["bucket_code"].cpu().tolist()],
                    "t": stamps, "pipe_id": [str(p) if p is not None else "NOLEAK" for p in names]})
        return out

    def check_errors(self, err: torch.Tensor) -> None:
        """The one read-back of an iteration: raise what the host path raises at the failing draw."""
        failed, bad = err.cpu().tolist()
        if failed:
            raise RuntimeError(FAILED)
        if bad:
            raise RuntimeError(f"{bad} drawn samples point outside the scene bank (sampler tables out of date?)")
