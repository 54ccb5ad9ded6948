"""GPU: bench.py's command line on a small frame (C1, 4 spp).

A plain run prints the headline line alone and, with --dump-outputs, writes
the last timed frame; --full adds the secondary measurements.  The dumped
accumulator is compared bit for bit with the same frames rendered in this
process (bench.py's renderer settings, warm-up + steps frames in a row).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_parity import scene_for

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CONFIG, SPP, STEPS, WARMUP = 1, 4, 2, 1
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "limiter", "steady_state", "traversal", "cpu_baseline")


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--config", str(CONFIG), "--spp", str(SPP),
           "--steps", str(STEPS), "--warmup", str(WARMUP), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_frame(pt, dev, tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path / "dump"))
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["steps"] == STEPS and len(d["frame"]["rounds_per_frame_rank0"]) == STEPS
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["frame"]["rays"] / (d["ms_per_step"] * 1e-3 * STEPS) / 1e6, rel=5e-3)

    acc = np.load(tmp_path / "dump" / "sample_buffer.npy")
    counts = np.load(tmp_path / "dump" / "frame_counts.npy")
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == ["frame_counts.npy", "sample_buffer.npy"]
    assert acc.dtype == np.float32 and counts.dtype == np.float64

    # The same frames in this process: bench.py's settings, WARMUP + STEPS frames.
    s = scene_for(pt, CONFIG)
    info = s.info
    W, H = info.width, info.height
    ds = pt.DeviceScene(dev)
    ds.update(s)
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = info.render_flags
    r.PathTerminationProbability = info.termination_probability
    target = SPP * W * H
    for _ in range(WARMUP + STEPS):
        rounds, samples = r.render_frame(target)
    ref = sb.read()
    for x in (r, sb, ds):
        x.close()
    assert acc.shape == (H, W, 4)
    assert counts.tolist() == [rounds, samples] and samples >= target
    assert [rounds, samples] == [d["frame"]["rounds_per_frame_rank0"][-1], d["frame"]["samples_per_frame_rank0"][-1]]
    assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32)), "dumped accumulator differs"


def test_full_run_adds_the_secondary_measurements():
    d = run_bench("--full", "--no-cpu-baseline")
    for k in HEADLINE + ("roofline", "limiter", "steady_state", "traversal"):
        assert k in d, k
    assert d["roofline"]["launch_avg_ms"] and d["steady_state"]["rounds"] > 0
    assert d["traversal"]["steps_per_ray"] > 0
