"""-m "not gpu": bench.py's options and its output dump (--dump-outputs), without running the benchmark."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.steps == 3 and a.warmup == 1 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_within_budget_is_written_whole(bench, tmp_path):
    frame = np.random.RandomState(0).rand(1920 * 1080, 4).astype(np.float32)
    rnds = np.arange(1920 * 1080, dtype=np.float64)
    bench.dump_outputs(str(tmp_path), {"frame": frame, "rnds": rnds})
    assert sorted(os.listdir(tmp_path)) == ["frame.npy", "rnds.npy"]
    assert np.array_equal(np.load(tmp_path / "frame.npy"), frame) and np.load(tmp_path / "frame.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "rnds.npy"), rnds)


def test_dump_past_budget_is_a_fixed_sample_of_pixels(bench, tmp_path):
    n = 3840 * 2160
    frame = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
    rnds = np.arange(n, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"frame": frame, "rnds": rnds})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["frame.npy", "pixel_index.npy", "rnds.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rnds.npy"), idx)            # the same pixels in every array
    assert np.array_equal(np.load(tmp_path / "a" / "frame.npy"), frame[idx.astype(np.int64)])
    for f in files:                                                              # and the same sample in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
