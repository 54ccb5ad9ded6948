"""CPU: bench.py --dump-outputs' writer (bench.dump_outputs): dtypes, the
64 MB bound and the fixed, seeded pixel sample of a larger accumulator."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_small_accumulator_is_dumped_whole(tmp_path):
    a = np.random.default_rng(1).uniform(0, 4, size=(5, 7, 4)).astype(np.float32)
    bench.dump_outputs(tmp_path / "d", a, 3, 140)
    x = np.load(tmp_path / "d" / "sample_buffer.npy")
    assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), a.view(np.uint32))
    c = np.load(tmp_path / "d" / "frame_counts.npy")
    assert c.dtype == np.float64 and c.tolist() == [3.0, 140.0]


def test_large_accumulator_is_dumped_as_a_fixed_sample(tmp_path):
    """Over DUMP_MAX_BYTES the dump is the same seeded pixel sample each time."""
    px = bench.DUMP_MAX_BYTES // 16 + 4097
    a = np.arange(px * 4, dtype=np.float32).reshape(1, px, 4)
    bench.dump_outputs(tmp_path / "a", a, 7, 9)
    bench.dump_outputs(tmp_path / "b", a, 7, 9)
    x, y = np.load(tmp_path / "a" / "sample_buffer.npy"), np.load(tmp_path / "b" / "sample_buffer.npy")
    assert x.dtype == np.float32 and x.shape == (bench.DUMP_MAX_BYTES // 16, 4) and x.nbytes <= bench.DUMP_MAX_BYTES
    assert np.array_equal(x, y)
    assert np.all(np.diff(x[:, 0]) > 0) and np.all(x[:, 0] % 4 == 0)     # distinct pixels, ascending
    assert np.load(tmp_path / "a" / "frame_counts.npy").tolist() == [7.0, 9.0]
