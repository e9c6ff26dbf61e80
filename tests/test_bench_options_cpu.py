"""bench.py's --dump-outputs writer and --steps check, on CPU tensors: a small output is written whole and
exactly (s32 as float64), a larger one as the same seeded sample on every run, inside the size budget."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_small_output_whole_and_exact(tmp_path):
    t = torch.tensor([[-(2 ** 31), 2 ** 31 - 1], [2 ** 24 + 1, -7]], dtype=torch.int32)
    d = bench.dump_output(str(tmp_path), "dst", t)
    a = np.load(tmp_path / "dst.npy")
    assert d == {"file": "dst.npy", "dtype": "float64", "shape": [2, 2]}
    assert a.dtype == np.float64 and np.array_equal(a, t.numpy().astype(np.float64))
    u = torch.arange(256, dtype=torch.uint8).reshape(4, 64)
    bench.dump_output(str(tmp_path), "u8", u)
    b = np.load(tmp_path / "u8.npy")
    assert b.dtype == np.float32 and np.array_equal(b, u.numpy().astype(np.float32))


def test_dump_large_output_is_a_fixed_sample_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    t = torch.from_numpy(np.random.default_rng(3).integers(-1000, 1000, (8, 5, 7, 33)).astype(np.int32))
    d1 = bench.dump_output(str(tmp_path / "a"), "dst", t)
    d2 = bench.dump_output(str(tmp_path / "b"), "dst", t)
    a, b = np.load(tmp_path / "a" / "dst.npy"), np.load(tmp_path / "b" / "dst.npy")
    assert d1 == d2 and "sample" in d1 and d1["shape"] == [8, 5, 7, 33]
    assert np.array_equal(a, b) and 0 < a.nbytes <= 4096
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, t.numel(), 4096 // 8))
    assert np.array_equal(a, t.numpy().reshape(-1)[idx].astype(np.float64))


def test_bench_rejects_zero_steps_before_touching_the_gpu():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr
