"""GPU: per-tile statistics.  The device pass against
the host implementation bit for bit on the CPU tests' cases and on a rendered
pair, determinism, untouched inputs, one launch per call in the statistics
kernel slot, and the argument errors, which launch and write nothing."""
from __future__ import annotations

import numpy as np
import pytest

import tile_stats_cases as tc

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_matches_host(pt, dev, size):
    W, H = size
    for name, (a, b) in tc.cases(W, H).items():
        sa = pt.SampleBuffer(dev, W, H)
        sb = pt.SampleBuffer(dev, W, H) if b is not None else None
        sa.write(a)
        if sb is not None:
            sb.write(b)
        for threshold in tc.THRESHOLDS:
            host = pt.tile_statistics_host(a, b, threshold)
            got = sa.tile_statistics(sb, threshold)
            assert got.shape == host.shape and got.dtype == host.dtype
            differing = [k for k in host.dtype.names if not np.array_equal(bits(got[k]), bits(host[k]))]
            assert got.tobytes() == host.tobytes(), (name, threshold, differing)
            assert sa.tile_statistics(sb, threshold).tobytes() == got.tobytes(), (name, threshold)   # no atomics
        assert np.array_equal(bits(sa.read()), bits(a))                # inputs untouched
        if sb is not None:
            assert np.array_equal(bits(sb.read()), bits(b))
            sb.close()
        sa.close()


def test_rendered_pair(pt, dev):
    """Config 1 at 80x48 (5 x 3 tiles) as two halves of 12 rounds: the device
    records equal the host's on the read-back accumulators, every tile has
    pair pixels, and their sum is the frame statistics' pair count."""
    W, H = 80, 48
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    ra, rb = pt.BasicRenderer(dev, ds, sa), pt.BasicRenderer(dev, ds, sb)
    rb.FrameIndex = ra.FrameIndex + (1 << 24)
    for r in (ra, rb):
        r.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
        r.reset()
        r.run(2)
        r.run_rounds(10)
    for threshold in (0.0, 0.1, 0.5):
        got = sa.tile_statistics(sb, threshold)
        a, b = sa.read(), sb.read()
        assert got.tobytes() == pt.tile_statistics_host(a, b, threshold).tobytes()
    assert got.shape == (3, 5) and (got["pair"] > 0).all() and (got["filled"] + got["empty"] == 256).all()
    frame = sa.statistics(sb)
    assert int(got["pair"].sum()) == frame.noise_pixels and int(got["filled"].sum()) == frame.filled
    single = sa.tile_statistics()
    assert single.tobytes() == pt.tile_statistics_host(a).tobytes() and not single["pair"].any()
    for x in (rb, ra, sb, sa, ds):
        x.close()
    scene.close()


def test_one_launch_per_call(pt, dev):
    W, H = 67, 45
    a, b = tc.pair(W, H, 1)
    sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    sa.write(a)
    sb.write(b)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    sa.tile_statistics()
    sa.tile_statistics(sb, 0.25)
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_STATS)
    others = sum(dev.kernel_stats(k)[0] for k in range(11) if k != pt.KERNEL_STATS)
    dev.set_profiling(False)
    assert n == 2 and ms > 0 and others == 0
    for x in (sb, sa):
        x.close()


def test_errors(pt, dev):
    N = pt._native
    L = N.hip_lib()
    W, H = 33, 31
    a, b = tc.pair(W, H, 2)
    sa, sb, small = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H - 1)
    sa.write(a)
    sb.write(b)
    small.write(b[:H - 1])
    out = np.full(6 * 32, 0x5A, np.uint8).view(pt.TILE_STATS_DTYPE)
    marker = out.tobytes()
    p = out.ctypes.data
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    assert L.ptComputeTileStatistics(None, sa.handle, None, 0.1, p) != 0
    assert L.ptComputeTileStatistics(dev.handle, None, None, 0.1, p) != 0
    assert L.ptComputeTileStatistics(dev.handle, sa.handle, None, 0.1, None) != 0
    assert L.ptComputeTileStatistics(dev.handle, sa.handle, sa.handle, 0.1, p) != 0          # b is a
    assert L.ptComputeTileStatistics(dev.handle, sa.handle, small.handle, 0.1, p) != 0       # b of another size
    assert L.ptComputeTileStatistics(dev.handle, sa.handle, sb.handle, float("nan"), p) != 0
    assert L.ptComputeTileStatistics(dev.handle, sa.handle, sb.handle, -0.5, p) != 0
    assert L.ptComputeTileStatistics(dev.handle, sa.handle, None, -1e-30, p) != 0
    assert len(L.ptGetLastError()) > 0
    for call in (lambda: sa.tile_statistics(sa), lambda: sa.tile_statistics(small),
                 lambda: sa.tile_statistics(sb, float("nan"))):
        with pytest.raises(pt.PathTracerError):
            call()
    dev.synchronize()
    assert sum(dev.kernel_stats(k)[0] for k in range(11)) == 0     # nothing was launched
    dev.set_profiling(False)
    assert out.tobytes() == marker                                 # ... or written
    assert np.array_equal(bits(sa.read()), bits(a)) and np.array_equal(bits(sb.read()), bits(b))
    # a valid call still works after the failures
    assert sa.tile_statistics(sb, 0.1).tobytes() == pt.tile_statistics_host(a, b, 0.1).tobytes()
    for x in (small, sb, sa):
        x.close()
