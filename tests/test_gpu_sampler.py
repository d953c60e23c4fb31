"""Device sampler on the GPU (csrc/sampler.hip): the draw kernels against their CPU twins (which
tests/test_sampler_host.py holds to numpy and to the datasets' draw()), DeviceBatchLoader
draw="device" against draw="host" batch by batch, the exhausted-attempts error word, the evaluator
on device bucket codes, and train_detector --loader device_draw end to end.  Shapes are those of
tests/test_gpu_harness.py."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from helpers import GOLD, LTA_INP
from test_sampler_host import DS_SEEDS, bank_index, empty_all_leak_buckets, empty_some_buckets

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INFO = json.loads((GOLD / "harness.json").read_text())


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from models.synth import write_synthetic_leak_set, write_synthetic_normal_set
    d = tmp_path_factory.mktemp("synthds_gpu_sampler")
    write_synthetic_normal_set(d / "normal", INFO["sensors"], n_windows=12, T=577, seed=0)
    write_synthetic_leak_set(d / "leak", INFO["sensors"], INFO["pipes"], scenes_per_pipe=2, n_noleak=6, T=400, seed=0)
    return d


@pytest.fixture(scope="module")
def stdzr(data):
    from models.datasets import compute_sensor_stats_from_normal
    return compute_sensor_stats_from_normal(data / "normal")


def _detector_ds(data, stdzr, steps, seed):
    from models.datasets import AbruptLeakDetectorDataset
    return AbruptLeakDetectorDataset(data / "leak", steps_per_epoch=steps, seed=seed, standardizer=stdzr,
                                     sensor_ids=INFO["sensors"])


def _same_batch(a: dict, b: dict):
    assert set(a) == set(b)
    for k in b:
        if torch.is_tensor(b[k]):
            assert a[k].dtype == b[k].dtype and a[k].device == b[k].device, k
            assert torch.equal(a[k], b[k]), k
        else:
            assert list(a[k]) == list(b[k]), k


@pytest.mark.parametrize("seed", DS_SEEDS)
@pytest.mark.parametrize("emptied", [False, True])
def test_draw_kernels_equal_host_twins(data, stdzr, seed, emptied):
    """Records of indices 0 .. 299 from the kernels == the CPU twins' (same tables, same code)."""
    from models import sampler
    from models.datasets import DeviceBatchLoader, NormalPredictorDataset
    ds = _detector_ds(data, stdzr, 300, seed)
    if emptied:
        empty_some_buckets(ds)
    sm = DeviceBatchLoader(ds, 8, DEV, draw="device")._sampler
    assert sm.bank.index == bank_index(ds)
    err = sm.new_error_words()
    rec = sm.draw_range(0, 300, err).cpu().numpy()
    want, failed = sampler.draw_detector_host(sm.tb, 0, 300)
    assert failed == 0 and err.tolist() == [0, 0]
    assert np.array_equal(rec, want)
    if emptied:
        assert (rec[:, 5] >= 2).any()
    part = sm.draw_range(257, 43, err).cpu().numpy()  # another first index, a partial workgroup
    assert np.array_equal(part, want[257:])
    nds = NormalPredictorDataset(data / "normal", steps_per_epoch=300, seed=seed, standardizer=stdzr)
    pm = DeviceBatchLoader(nds, 8, DEV, draw="device")._sampler
    prec = pm.draw_range(0, 300, err).cpu().numpy()
    pwant, pfailed = sampler.draw_predictor_host(pm.tb, 0, 300)
    assert pfailed == 0 and err.tolist() == [0, 0] and np.array_equal(prec, pwant)


@pytest.mark.parametrize("shard", [(0, 1), (1, 3)])
def test_device_draw_batches_equal_host_draw_batches(data, stdzr, shard):
    """materialize() of every draw="device" batch == the draw="host" batch: batch 8 over 37 samples
    (ragged tail of 5), whole and as rank 1 of 3, both dataset types."""
    from models.datasets import DeviceBatchLoader, NormalPredictorDataset
    for ds in (_detector_ds(data, stdzr, 37, 5),
               NormalPredictorDataset(data / "normal", steps_per_epoch=37, seed=3, standardizer=stdzr)):
        host = list(DeviceBatchLoader(ds, 8, DEV, shard=shard))
        loader = DeviceBatchLoader(ds, 8, DEV, shard=shard, draw="device")
        got = list(loader)
        assert len(host) == len(got) == len(loader) == 5
        for a, b in zip(got, host):
            assert all(torch.is_tensor(v) and v.is_cuda for v in a.values())  # device tensors only
            extra = {"scene", "t_index"} | ({"bucket_code"} if "label" in b else set())
            assert set(a) == {k for k, v in b.items() if torch.is_tensor(v)} | extra
            _same_batch(loader.materialize(a), b)
        if shard == (0, 1):
            assert sum(len(b["scene"]) for b in got) == 37 and len(got[-1]["scene"]) == 5
        assert list(loader.materialize(b)["t"] for b in loader) == [b["t"] for b in host]  # a second pass


def test_exhausted_attempts_raise_at_the_end(data, stdzr):
    """Every leak bucket empty: ds.draw raises within the 64 indices; device mode yields every batch
    (failed samples as zeros with label -1) and raises the same RuntimeError once exhausted."""
    from models.datasets import DeviceBatchLoader
    ds = _detector_ds(data, stdzr, 64, 5)
    empty_all_leak_buckets(ds)
    raised = []
    for i in range(64):
        try:
            ds.draw(i)
        except RuntimeError as e:
            assert "Failed to sample a valid (scenario, time)" in str(e)
            raised.append(i)
    assert raised
    loader = DeviceBatchLoader(ds, 16, DEV, draw="device")
    seen = []
    with pytest.raises(RuntimeError, match=r"Failed to sample a valid \(scenario, time\)"):
        for batch in loader:
            seen.append(batch)
    assert len(seen) == 4
    label = torch.cat([b["label"] for b in seen]).cpu()
    assert torch.nonzero(label < 0).flatten().tolist() == raised
    seg = torch.cat([b["noisy_seg"] for b in seen]).cpu()
    assert not seg[raised].any() and seg[[i for i in range(64) if i not in raised]].abs().sum(dim=(1, 2)).min() > 0


@pytest.mark.parametrize("fused", [True, False])
def test_evaluator_on_device_draw_loader(data, stdzr, fused):
    """DetectorEvaluator.evaluate over a 16-window device-draw loader returns exactly the dict it
    returns over the host-mode loader, on both routes; the device batches carry no host bucket list."""
    from models.datasets import DeviceBatchLoader
    from models.window_evaluator import DetectorEvaluator
    from test_harness import _fixed_detector, _tcn
    det = _fixed_detector(np.load(GOLD / "harness.npz"))  # the stand-in of tests/test_harness.py: tie-free logits
    ev = DetectorEvaluator(_tcn().to(DEV), det, DEV, l_pred=36, l_det=36, topk=3,
                           metric_groups=("basic", "binary", "bucket", "atd", "success", "accuracy_i"),
                           inp_path=LTA_INP, pipe_ids_in_order=INFO["pipe_ids_in_order"], fused=fused)
    ds = _detector_ds(data, stdzr, 16, 9)
    ref = ev.evaluate(DeviceBatchLoader(ds, 8, DEV))
    loader = DeviceBatchLoader(ds, 8, DEV, draw="device")
    assert all("bucket" not in b and b["bucket_code"].dtype == torch.int32 for b in loader)
    got = ev.evaluate(loader)
    assert ref["n_total"] == 16.0 and sum(ref[f"{b}_n"] for b in ("early", "late", "pre", "noleak")) == 16.0
    assert got == ref


def test_train_detector_cli_device_draw(data, tmp_path, capsys):
    """train_detector --loader device_draw runs end to end (1 epoch of 16 optimizer steps at batch 8)
    and prints the loss= values of the same command with --loader device."""
    from models import train_detector, train_predictor
    from models.synth import write_synthetic_leak_set
    write_synthetic_leak_set(tmp_path / "leak", INFO["sensors"], INFO["pipes"], scenes_per_pipe=4, n_noleak=12,
                             T=300, seed=1)
    out = tmp_path / "pred"
    train_predictor.main(["--normal_root", str(data / "normal"), "--out_dir", str(out), "--epochs", "1",
                          "--steps_per_epoch", "16", "--val_steps", "8", "--test_steps", "8", "--batch_size", "8",
                          "--device", "cuda", "--loader", "device_draw"])
    capsys.readouterr()

    def run(kind):
        train_detector.main(["--leak_root", str(tmp_path / "leak"), "--inp_path", str(LTA_INP), "--predictor_ckpt",
                             str(out / "predictor_best.ckpt"), "--out_dir", str(tmp_path / kind), "--epochs", "1",
                             "--steps_per_epoch", "128", "--val_steps", "16", "--test_steps", "16", "--batch_size", "8",
                             "--device", "cuda", "--log_every", "1", "--loader", kind])
        log = capsys.readouterr().out
        assert "[detector] TEST:" in log
        return [l.split("loss=")[1].split()[0] for l in log.splitlines() if "loss=" in l]
    a, b = run("device_draw"), run("device")
    print("device_draw:", a)
    print("device:     ", b)
    assert len(a) == len(b) == 17 and all(np.isfinite(float(v)) for v in a)  # 16 steps + the epoch's train_loss
    assert a == b
