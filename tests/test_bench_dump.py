"""bench.py --dump-outputs: the arrays of the last timed step, finite, float32 / float64, within the size budget, identical
from run to run.  CPU part: dump_outputs on stand-in filter / renderer objects.  GPU part: bench.py itself, one rank and
two (the gloo rehearsal on one device)."""
import glob
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL = ("scan", "weight_stats", "weights")
SHARD = ("raw_weights", "raw_weights_known", "resample_idx", "states")


def stand_ins(n, seed=0, rendered=True):
    rng = np.random.default_rng(seed)
    raw = rng.random(n).astype(np.float32)
    raw[::7] = np.nan                     # "too much unknown"
    raw[3] = 0.0                          # a gated particle
    info = torch.zeros(4)
    info[:1].view(torch.int32)[0] = 5
    info[1:4] = torch.tensor([1.5, 0.25, 0.125])
    f = types.SimpleNamespace(info=info, n_local=n, st=torch.from_numpy(rng.random((7, n + 9)).astype(np.float32)),
                              raw_weights=lambda: raw.copy(), weights=lambda: np.full(n, 1.0 / n, np.float32),
                              resample_indices=lambda: np.arange(n, dtype=np.int32)[::-1].copy())
    img = torch.from_numpy(rng.random((3, 16, 8)).astype(np.float32))

    def last_images():
        if not rendered:   # a renderer that never rendered (ScanRenderer._last is None)
            raise TypeError("'NoneType' object is not subscriptable")
        return img
    return f, types.SimpleNamespace(last_images=last_images), raw


@pytest.fixture
def no_device_sync(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)


def files(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def size(d):
    return sum(os.path.getsize(p) for p in glob.glob(os.path.join(d, "*.npy")))


def test_one_rank_writes_finite_float_arrays(tmp_path, no_device_sync):
    f, r, raw = stand_ins(1000)
    bench.dump_outputs(str(tmp_path), f, r, 1, 0)
    got = files(str(tmp_path))
    assert sorted(got) == sorted(GLOBAL + SHARD)
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
    # NaN raw weights are recoverable from the mask, and a raw weight of 0 stays a scored 0
    back = np.where(got["raw_weights_known"] > 0, got["raw_weights"], np.nan)
    assert np.array_equal(back, raw, equal_nan=True) and got["raw_weights_known"][3] == 1
    assert got["weight_stats"].tolist() == [5.0, 1.5, 0.25, 0.125]
    assert np.array_equal(got["states"], f.st[:, :1000].numpy())
    assert np.array_equal(got["resample_idx"], np.arange(1000)[::-1])


def test_over_the_budget_a_seeded_sample_is_kept(tmp_path, no_device_sync, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40000)
    f, r, raw = stand_ins(2000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), f, r, 1, 0)
    assert size(str(tmp_path / "a")) <= 40000
    a, b = files(str(tmp_path / "a")), files(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)    # the same sample every time
    sel = a["raw_weights_sample"].astype(np.int64)
    assert 0 < len(sel) < 2000 and np.all(np.diff(sel) > 0)
    assert np.array_equal(np.where(a["raw_weights_known"] > 0, a["raw_weights"], np.nan), raw[sel], equal_nan=True)
    assert np.array_equal(a["states"], f.st[:, :2000].numpy()[:, a["states_sample"].astype(np.int64)])
    assert a["scan"].shape == (3, 16, 8)                                       # not per particle: never cut


def test_several_ranks_rank_zero_writes_the_global_arrays(tmp_path, no_device_sync):
    # only rank 0 renders: the other ranks' renderers hold no image and must not be asked for one
    for rank in range(3):
        f, r, _ = stand_ins(300, seed=rank, rendered=rank == 0)
        bench.dump_outputs(str(tmp_path), f, r, 3, rank)
    got = files(str(tmp_path))
    assert sorted(got) == sorted(list(GLOBAL) + [f"{n}_rank{k}" for n in SHARD for k in range(3)])
    assert all(np.isfinite(a).all() for a in got.values())


def run_bench(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


SMALL = ["--config", "c1", "--steps", "3", "--warmup", "1", "--no-cpu"]


@pytest.mark.gpu
def test_bench_dumps_are_identical_from_run_to_run(tmp_path):
    for d in ("a", "b"):
        run_bench(SMALL + ["--gpus", "1", "--dump-outputs", str(tmp_path / d)], 600)
    a, b = files(str(tmp_path / "a")), files(str(tmp_path / "b"))
    assert sorted(a) == sorted(GLOBAL + SHARD)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and np.isfinite(a[name]).all(), name
        assert open(tmp_path / "a" / f"{name}.npy", "rb").read() == open(tmp_path / "b" / f"{name}.npy", "rb").read(), name
    assert size(str(tmp_path / "a")) <= bench.DUMP_BUDGET


@pytest.mark.gpu
def test_bench_dumps_every_rank(tmp_path):
    run_bench(SMALL + ["--gpus", "2", "--same-device", "--backend", "gloo", "--particles-per-gpu", "500",
                       "--dump-outputs", str(tmp_path)], 900)
    got = files(str(tmp_path))
    assert sorted(got) == sorted(list(GLOBAL) + [f"{n}_rank{k}" for n in SHARD for k in range(2)])
    assert all(np.isfinite(a).all() for a in got.values())
    assert got["weights"].shape == (1000,) and got["states_rank1"].shape == (7, 500)
    assert size(str(tmp_path)) <= bench.DUMP_BUDGET
