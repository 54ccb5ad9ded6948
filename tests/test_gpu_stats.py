"""GPU: frame statistics.  The device pass (both
histogram-update variants) against the host implementation bit for bit in
every field, determinism, untouched inputs, the sample-buffer add against
numpy, the argument errors, the kernel-stat slot, and the whole flow: two
half renders until the noise figure falls below a threshold, combined on the
device and resolved at the automatic Brightness."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import oracle_lib
import stats_cases as sc
import stats_restatement as sr

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SIZES = sc.SIZES + [sc.LARGE]
CASES = ["crafted", "constant", "empty", "pair", "pair-constant", "pair-equal", "pair-empty"]
VARIANTS = ["auto", "plain", "uniform"]


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module", params=ALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def cases(request, pt):
    """{name: (A, B or None, the host's statistics)}, computed once per size."""
    return {name: (a, b, pt.frame_statistics_host(a, b)) for name, (a, b) in sc.cases(*request.param).items()}


@pytest.mark.parametrize("name", CASES)
def test_device_matches_host(pt, dev, cases, name):
    a, b, host = cases[name]
    H, W = a.shape[:2]
    sa = pt.SampleBuffer(dev, W, H)
    sb = pt.SampleBuffer(dev, W, H) if b is not None else None
    sa.write(a)
    if sb is not None:
        sb.write(b)
    results = {}
    for v in VARIANTS:
        dev.set_statistics_variant({"auto": pt.STATS_VARIANT_AUTO, "plain": pt.STATS_VARIANT_PLAIN,
                                    "uniform": pt.STATS_VARIANT_UNIFORM}[v])
        results[v] = sa.statistics(sb)
        again = sa.statistics(sb)                                  # the device struct is cleared every time
        assert again.tobytes() == results[v].tobytes(), v
    dev.set_statistics_variant(pt.STATS_VARIANT_AUTO)
    for v, got in results.items():
        assert sr.differences(got, host) == [], v
        assert got.tobytes() == host.tobytes(), v
    assert np.array_equal(bits(sa.read()), bits(a))                # inputs untouched
    if sb is not None:
        assert np.array_equal(bits(sb.read()), bits(b))
        sb.close()
    sa.close()


def test_accumulate_is_numpy_add(pt, dev):
    for W, H in ALL_SIZES:
        a, b = sc.pair(W, H, seed=W + 1)
        sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
        sa.write(a)
        sb.write(b)
        sa.accumulate(sb)
        with np.errstate(all="ignore"):
            want = a + b
        assert np.isnan(want).any() and np.isinf(want).any()
        same = dc.same_bits(sa.read(), want)
        assert same.all(), np.argwhere(~same)[:5]
        assert np.array_equal(bits(sb.read()), bits(b))            # src unchanged
        # the pair statistics' luminance part describes exactly this sum
        host = pt.frame_statistics_host(a, b)
        summed = sa.statistics()
        lum = lambda s: {k: v for k, v in sr.fields(s).items() if not k.startswith("noise")}   # noqa: E731
        assert lum(summed) == lum(host)
        sa.accumulate(sb)                                          # a second add: (a + b) + b
        with np.errstate(all="ignore"):
            want2 = want + b
        assert dc.same_bits(sa.read(), want2).all()
        for x in (sb, sa):
            x.close()


def test_errors(pt, dev):
    N = pt._native
    L = N.hip_lib()
    W, H = 32, 16
    a = dc.accumulators(W, H, 2)
    marker = np.full((H, W, 4), 5.0, F)
    sa, sb, small = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H - 1)
    sa.write(a)
    sb.write(marker)
    small.write(marker[:H - 1])

    def fails(call):
        with pytest.raises(pt.PathTracerError) as e:
            call()
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    dev.reset_kernel_stats()
    dev.set_profiling(True)
    fails(lambda: sa.statistics(sa))                               # b is a
    fails(lambda: sa.statistics(small))                            # b of another size
    fails(lambda: sa.accumulate(sa))                               # dst is src
    fails(lambda: sa.accumulate(small))
    fails(lambda: small.accumulate(sa))
    fails(lambda: dev.set_statistics_variant(3))
    out = N.pt_frame_statistics()
    out.pixels = 77
    assert L.ptComputeFrameStatistics(None, sa.handle, None, C.byref(out)) != 0
    assert L.ptComputeFrameStatistics(dev.handle, None, None, C.byref(out)) != 0
    assert L.ptComputeFrameStatistics(dev.handle, sa.handle, None, None) != 0
    assert L.ptComputeFrameStatistics(dev.handle, sa.handle, sa.handle, C.byref(out)) != 0
    assert L.ptComputeFrameStatistics(dev.handle, sa.handle, small.handle, C.byref(out)) != 0
    assert out.pixels == 77 and out.filled == 0                    # untouched
    assert L.ptAccumulateSampleBuffer(None, sa.handle, sb.handle) != 0
    assert L.ptAccumulateSampleBuffer(dev.handle, None, sb.handle) != 0
    assert L.ptAccumulateSampleBuffer(dev.handle, sa.handle, None) != 0
    assert len(L.ptGetLastError()) > 0
    dev.synchronize()
    assert dev.kernel_stats(pt.KERNEL_STATS)[0] == 0               # nothing was launched
    dev.set_profiling(False)
    assert np.array_equal(bits(sa.read()), bits(a))                # ... or written
    assert np.array_equal(bits(sb.read()), bits(marker))
    assert np.array_equal(bits(small.read()), bits(marker[:H - 1]))
    # a valid call still works after the failures
    assert sa.statistics().tobytes() == pt.frame_statistics_host(a).tobytes()
    assert sa.statistics(sb).tobytes() == pt.frame_statistics_host(a, marker).tobytes()
    sb.accumulate(sa)
    assert dc.same_bits(sb.read(), marker + a).all()
    for x in (small, sb, sa):
        x.close()


def test_kernel_stat_slot(pt, dev):
    W, H = 40, 24
    sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    sa.write(dc.accumulators(W, H, 1))
    sb.write(dc.accumulators(W, H, 2))
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    sa.statistics()
    sa.statistics(sb)
    sa.accumulate(sb)
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_STATS)
    resolves = dev.kernel_stats(pt._native.KERNEL_RESOLVE)[0]
    dev.set_profiling(False)
    assert n == 3 and ms > 0 and resolves == 0
    assert pt.KERNEL_STATS == 9
    for x in (sb, sa):
        x.close()


def test_whole_flow(pt, dev):
    """Config 1 at 64x32, two renderers on one scene: render_until_noise with
    a loose threshold stops before max_rounds, half the threshold needs at
    least as many rounds, the pair statistics equal the host's on the
    read-back halves, and accumulate + automatic Brightness + ACES resolve
    give the oracle's resolve of the summed accumulator."""
    W, H = 64, 32
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)

    def until(threshold, max_rounds=256):
        sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
        ra, rb = pt.BasicRenderer(dev, ds, sa), pt.BasicRenderer(dev, ds, sb)
        for r in (ra, rb):
            r.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
        rounds, stats = pt.render_until_noise(ra, rb, threshold, max_rounds=max_rounds)
        assert rb.FrameIndex - ra.FrameIndex == 1 << 24
        return rounds, stats, sa, sb, ra, rb

    # p95 of r on this frame: 0.18 at 16 rounds per half, 0.09 at 64 (CPU oracle)
    rounds, stats, sa, sb, ra, rb = until(0.25)
    assert rounds < 256 and rounds % 8 == 0
    assert stats.noise() <= 0.25 and stats.noise_pixels >= 0.99 * stats.pixels
    a, b = sa.read(), sb.read()
    assert stats.tobytes() == pt.frame_statistics_host(a, b).tobytes()
    assert stats.tobytes() == sa.statistics(sb).tobytes()
    assert (a != b).any()                                          # independent halves

    sa.accumulate(sb)
    with np.errstate(all="ignore"):
        total = a + b
    assert np.array_equal(bits(sa.read()), bits(total))
    p = pt.ResolveParameters.auto(stats, ToneMappingMode=pt.TONE_MAPPING_ACES)
    assert p.Brightness == stats.auto_brightness() and 0.1 < p.Brightness < 10.0
    sa.render(p)
    img, img8 = sa.read_resolved(), sa.read_srgb8()
    brightness = float(F(p.Brightness))                            # what the C struct holds
    exp, exp8 = oracle_lib.resolve(total, brightness, pt.TONE_MAPPING_ACES, 1.0)
    same = dc.same_bits(img, exp)
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(img8, exp8)
    assert 20 < img8[..., :3].mean() < 235                         # neither black nor white
    for x in (rb, ra, sb, sa):
        x.close()

    rounds2, stats2, *objs = until(0.125)
    assert rounds2 >= rounds
    assert stats2.noise() <= 0.125 or rounds2 == 256
    for x in reversed(objs):
        x.close()
    capped, stats3, *objs = until(1e-6, max_rounds=12)             # never reached: ends at max_rounds
    assert capped == 12 and stats3.noise() > 1e-6
    for x in reversed(objs):
        x.close()
    ds.close()
    scene.close()
