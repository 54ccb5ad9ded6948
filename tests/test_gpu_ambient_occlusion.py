"""GPU: the ambient-occlusion / sky-visibility image (ptRenderAmbientOcclusion;
DESIGN.md §6 row 14) against its numpy restatement, bit for bit.

The expected image is formed on the restatement's rays
(tests/visibility_restatement.py) twice: by counting the misses of the
oracle's ray query and of ptTraceRays.  The device image must equal both, for
every sample count, radius and stack format; the restatement's rays are
computed once per frame (16 samples; fewer samples are a prefix of a pixel's
stream) and shared."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import visibility_restatement as vr

pytestmark = pytest.mark.gpu

INF = float("inf")
SIZES = [(33, 17), (48, 48)]


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def render(pt, dev, ds, W, H, sb=None, **kw):
    own = sb is None
    sb = sb if sb is not None else pt.SampleBuffer(dev, W, H)
    sb.render_ambient_occlusion(ds, **kw)
    out = sb.read()
    if own:
        sb.close()
    return out


@pytest.mark.parametrize("size", SIZES, ids=["33x17", "48x48"])
@pytest.mark.parametrize("config", [1, 2, 3])
def test_image_equals_the_restatement(pt, dev, config, size):
    """Samples 1, 4, 16 x Radius 0.5, inf x the three stack formats: the
    device image against the restatement's rays through the oracle and
    through ptTraceRays."""
    W, H = size
    ds = pt.DeviceScene(dev)
    sb = pt.SampleBuffer(dev, W, H)
    for fmt in (0, 1, 2):
        ds.set_stack_format(fmt)
        ds.update(vr.config_case(config, W, H, 1, 0.5, 0)[0])
        for samples in (1, 4, 16):
            for radius in (0.5, INF):
                scene, rays, want = vr.config_case(config, W, H, samples, radius, 0)
                got = render(pt, dev, ds, W, H, sb=sb, camera_index=0, samples=samples, radius=radius, seed=0)
                assert np.array_equal(bits(got), bits(want)), (config, size, fmt, samples, radius)
                if fmt == 0:
                    records = ds.trace_rays(rays["origins"], rays["packed"], rays["durations"])
                    assert np.array_equal(bits(vr.image(rays, records)), bits(want)), (config, size, samples, radius)
    sb.close()
    ds.close()


def test_partial_visibility_is_exercised(pt, dev):
    """C2 at 48 x 48, 16 samples, infinite radius: on the CPU restatement
    90.9 % of the hit pixels have 0 < u < S (and every pixel is a hit pixel),
    so the per-pixel count is checked where it is neither end of its range."""
    scene, rays, want = vr.config_case(2, 48, 48, 16, INF, 0)
    u = want.reshape(-1, 4)[rays["pixels"], 0]
    share = float(((u > 0) & (u < 16)).mean())
    print(f"hit pixels with 0 < u < S: {100 * share:.1f} %")
    assert share >= 0.10
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    got = render(pt, dev, ds, 48, 48, samples=16, radius=INF, seed=0)
    assert np.array_equal(bits(got), bits(want))
    ds.close()


def test_seeds_accumulation_and_the_passes_behind_it(pt, dev):
    scene, rays, want = vr.config_case(1, 33, 17, 4, INF, 0)
    W, H, S = 33, 17, 4
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    a, b = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    a.render_ambient_occlusion(ds, samples=S, seed=0)
    first = a.read()
    a.render_ambient_occlusion(ds, samples=S, seed=0)
    assert np.array_equal(bits(a.read()), bits(first)) and np.array_equal(bits(first), bits(want))
    b.render_ambient_occlusion(ds, params=pt.AmbientOcclusionParameters(Samples=S, Seed=1))
    other = b.read()
    assert not np.array_equal(other, first)
    assert np.array_equal(other[..., 0], other[..., 1]) and np.array_equal(other[..., 1], other[..., 2])
    assert np.all(other[..., 3] == S) and np.all(other[..., 0] <= S) and np.all(other[..., 0] >= 0)
    a.accumulate(b)
    both = a.read()
    assert np.all(both[..., 3] == 2 * S) and np.array_equal(both[..., 1], first[..., 1] + other[..., 1])
    # the image is an accumulator: resolve and the denoiser take it
    a.render(pt.ResolveParameters())
    shown = a.read_resolved()
    assert shown.shape == (H, W, 4) and np.all(np.isfinite(shown))
    g = pt.DenoiseGuides(dev, W, H)
    g.render(ds, 0)
    out = a.denoise(g)
    smooth = out.read()
    assert np.all(np.isfinite(smooth)) and np.all(smooth[..., 3] == 1.0)
    assert smooth[..., 1].min() >= 0.0 and smooth[..., 1].max() <= 1.0 + 1e-5   # a visible fraction still
    for x in (out, g, a, b, ds):
        x.close()


def test_argument_errors_launch_nothing(pt, dev):
    """Every refused call leaves dst's bits and the launch count alone."""
    N = pt._native
    L = N.hip_lib()
    scene, _, _ = vr.config_case(1, 33, 17, 4, INF, 0)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    blank = pt.DeviceScene(dev)                     # never updated: no packs
    sb = pt.SampleBuffer(dev, 33, 17)
    fill = np.random.default_rng(1).uniform(0.0, 9.0, (17, 33, 4)).astype(np.float32)
    sb.write(fill)
    ok = N.pt_ambient_occlusion_parameters(4, 1.0, 0)

    def params(samples, radius):
        return N.pt_ambient_occlusion_parameters(samples, radius, 0)

    dev.set_profiling(True)
    dev.reset_kernel_stats()
    d, s, b = dev.handle, ds.handle, sb.handle
    bad = [(None, s, 0, ok, b), (d, None, 0, ok, b), (d, s, 0, None, b), (d, s, 0, ok, None),
           (d, blank.handle, 0, ok, b), (d, s, len(ds.cameras), ok, b), (d, s, 0xFFFFFFFF, ok, b),
           (d, s, 0, params(0, 1.0), b), (d, s, 0, params(65, 1.0), b), (d, s, 0, params(4, 0.0), b),
           (d, s, 0, params(4, -1.0), b), (d, s, 0, params(4, float("nan")), b), (d, s, 0, params(4, -INF), b)]
    for args in bad:
        p = None if args[3] is None else C.byref(args[3])
        assert L.ptRenderAmbientOcclusion(args[0], args[1], args[2], p, args[4]) != 0, args
        assert len(L.ptGetLastError()) > 0
    with pytest.raises(pt.PathTracerError):
        sb.render_ambient_occlusion(ds, samples=0)
    with pytest.raises(pt.PathTracerError):
        sb.render_ambient_occlusion(ds, radius=0.0)
    dev.synchronize()
    assert dev.kernel_stats(pt.KERNEL_GUIDES)[0] == 0
    assert np.array_equal(bits(sb.read()), bits(fill))
    assert L.ptRenderAmbientOcclusion(d, s, 0, C.byref(params(64, INF)), b) == 0
    dev.synchronize()
    assert dev.kernel_stats(pt.KERNEL_GUIDES)[0] == 1
    dev.set_profiling(False)
    assert np.all(sb.read()[..., 3] == 64.0)
    for x in (sb, blank, ds):
        x.close()
