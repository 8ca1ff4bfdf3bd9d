"""bench.py's host-side pieces that need no GPU: the options of a plain / full run and the
``--dump-outputs`` writer (float32 arrays, a fixed seeded batch sample under the size cap)."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2) and a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_writes_small_arrays_whole_as_float32(tmp_path):
    g = torch.Generator().manual_seed(0)
    state = torch.rand(5, 4, 3, 3, generator=g)
    bench.dump_outputs(str(tmp_path / "d"), {"state": state, "loss": torch.tensor(0.25, dtype=torch.float64),
                                             "count": torch.arange(6).reshape(2, 3)})
    assert sorted(os.listdir(tmp_path / "d")) == ["count.npy", "loss.npy", "state.npy"]
    got = np.load(tmp_path / "d" / "state.npy")
    assert got.dtype == np.float32 and np.array_equal(got, state.numpy())
    loss = np.load(tmp_path / "d" / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [0.25]
    cnt = np.load(tmp_path / "d" / "count.npy")
    assert cnt.dtype == np.float32 and np.array_equal(cnt, np.arange(6, dtype=np.float32).reshape(2, 3))


def test_dump_samples_a_large_batch_the_same_way_every_time(tmp_path, monkeypatch):
    assert bench.DUMP_MAX_BYTES <= 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 10 * 64)   # two arrays: 10 rows of 16 floats each
    x = torch.arange(37 * 16, dtype=torch.float32).reshape(37, 4, 4)
    small = torch.ones(3, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"state": x, "small": small})
    a, b = np.load(tmp_path / "a" / "state.npy"), np.load(tmp_path / "b" / "state.npy")
    assert a.shape == (10, 4, 4) and np.array_equal(a, b)
    rows = (a[:, 0, 0] / 16).astype(int)           # row r of x starts at 16 r
    assert list(rows) == sorted(set(rows)) and np.array_equal(a, x.numpy()[rows])
    assert np.array_equal(rows, np.sort(np.random.default_rng(0).choice(37, 10, replace=False)))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 2 * 10 * 64 + 2 * 128
