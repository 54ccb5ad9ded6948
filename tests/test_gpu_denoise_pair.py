"""GPU: the variance-guided denoiser over two half renders (DESIGN.md §6 row
7).  The device filter (both kernel variants behind the prepare launch)
against the host implementation bit for bit, the whole path two renderers ->
guides -> denoise_pair -> resolve, the argument errors and the launch count."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import denoise_pair_cases as dpc
import resolve_restatement

pytestmark = pytest.mark.gpu

# (5, 3): smaller than every window, the prefilter touches every border;
# 40x24: smaller than one lattice block's window from step 2; 67x45: partial
# tiles, residue classes of unequal size; 130x70: more than one block per
# residue class at step 4.
SIZES = [(5, 3), (40, 24), (67, 45), (130, 70)]
ITERATIONS = [0, 1, 3, 5, 6]
MARKER = 3.0


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(pt, iterations):
    return pt.DenoisePairParameters(iterations, dpc.PARAMS["sigma_luminance"], dpc.PARAMS["sigma_normal"],
                                    dpc.PARAMS["sigma_depth"], dpc.PARAMS["sigma_albedo"])


def variant_of(pt, name):
    return {"auto": pt.DENOISE_VARIANT_AUTO, "gather": pt.DENOISE_VARIANT_GATHER,
            "lattice": pt.DENOISE_VARIANT_LATTICE}[name]


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def crafted(request, pt):
    """(A, B, guides, host results per iteration count), computed once per size."""
    W, H = request.param
    (a, b), g = dpc.pair(W, H, seed=W), dc.crafted_guides(W, H)
    return a, b, g, {it: pt.denoise_pair_host(a, b, g, params(pt, it)) for it in ITERATIONS}


@pytest.mark.parametrize("variant", ["auto", "gather", "lattice"])
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_filter_matches_host(pt, dev, crafted, iterations, variant):
    a, b, g, host = crafted
    H, W = a.shape[:2]
    sa, sb, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    guides = pt.DenoiseGuides(dev, W, H)
    guides.set_variant(variant_of(pt, variant))
    sa.write(a)
    sb.write(b)
    guides.write(g)
    p = params(pt, iterations)
    first = sa.denoise_pair(sb, guides, p, out=dst).read()
    dst.write(np.full((H, W, 4), MARKER, np.float32))        # the second run must rewrite every pixel
    second = sa.denoise_pair(sb, guides, p, out=dst).read()
    assert np.array_equal(bits(first), bits(second))
    same = dc.same_bits(first, host[iterations])
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(bits(sa.read()), bits(a))          # a and b are never written
    assert np.array_equal(bits(sb.read()), bits(b))
    assert np.array_equal(guides.read(), g)
    for x in (guides, dst, sb, sa):
        x.close()


def test_end_to_end(pt, dev):
    """Config 1 at 64x32: two renderers with FrameIndex 0 and 1 << 24, each
    reset, run(2), run(2); guides; denoise_pair; ACES resolve.  The display
    image and the sRGB8 bytes equal the restated resolve of the host filter on
    the read-back accumulators and guides; neither renderer's state,
    FrameIndex or sample buffer moved; the filter changed a pixel."""
    W, H = 64, 32
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    halves = []
    for frame_index in (0, 1 << 24):
        sb = pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
        r.FrameIndex = frame_index
        r.reset()
        r.run(2)
        r.run(2)
        halves.append((sb, r, r.read_state(), sb.read(), r.FrameIndex))
    (sa, ra, state_a, accum_a, frame_a), (sb, rb, state_b, accum_b, frame_b) = halves
    assert frame_b - frame_a == 1 << 24
    assert not np.array_equal(bits(accum_a), bits(accum_b))             # independent halves
    guides = pt.DenoiseGuides(dev, W, H)
    guides.render(ds, 0)
    out = sa.denoise_pair(sb, guides)
    out.render(ToneMappingMode=pt.TONE_MAPPING_ACES)
    img, img8 = out.read_resolved(), out.read_srgb8()
    host = pt.denoise_pair_host(accum_a, accum_b, guides.read())
    assert np.array_equal(bits(out.read()), bits(host))
    exp, exp8 = resolve_restatement.resolve(host, 1.0, resolve_restatement.ACES, 1.0)
    same = dc.same_bits(img, exp)
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(img8, exp8)
    for s, r, state0, accum0, frame0 in halves:
        assert np.array_equal(bits(s.read()), bits(accum0))
        assert r.read_state().tobytes() == state0.tobytes() and r.FrameIndex == frame0
    total = accum_a + accum_b
    assert (host[..., :3] != (total[..., :3] / np.maximum(total[..., 3:4], 1))).any()   # the filter acted
    for x in (out, guides, rb, ra, sb, sa, ds):
        x.close()
    scene.close()


def test_errors(pt, dev):
    N = pt._native
    L = N.hip_lib()
    W, H = 32, 16
    sa, sb, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    small = pt.SampleBuffer(dev, W, H - 1)
    guides, small_guides = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W - 1, H)
    a, b = dpc.pair(W, H, 2)
    marker = np.full((H, W, 4), 5.0, np.float32)
    sa.write(a)
    sb.write(b)
    dst.write(marker)
    small.write(marker[:H - 1])
    g0 = dc.crafted_guides(W, H)
    guides.write(g0)

    def fails(call):
        with pytest.raises(pt.PathTracerError) as e:
            call()
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    P = pt.DenoisePairParameters
    fails(lambda: sa.denoise_pair(sa, guides, out=dst))                            # a is b
    fails(lambda: sa.denoise_pair(sb, guides, out=sa))                             # a is dst
    fails(lambda: sa.denoise_pair(sb, guides, out=sb))                             # b is dst
    fails(lambda: sa.denoise_pair(sb, guides, out=small))                          # dst of another size
    fails(lambda: sa.denoise_pair(small, guides, out=dst))                         # b of another size
    fails(lambda: small.denoise_pair(sb, guides, out=dst))                         # a of another size
    fails(lambda: sa.denoise_pair(sb, small_guides, out=dst))                      # guides of another size
    fails(lambda: sa.denoise_pair(sb, guides, P(Iterations=9), out=dst))
    fails(lambda: sa.denoise_pair(sb, guides, P(SigmaLuminance=0.0), out=dst))
    fails(lambda: sa.denoise_pair(sb, guides, P(SigmaNormal=-1.0), out=dst))
    fails(lambda: sa.denoise_pair(sb, guides, P(SigmaDepth=0.0), out=dst))
    fails(lambda: sa.denoise_pair(sb, guides, P(SigmaAlbedo=float("nan")), out=dst))
    ok = P().as_struct()
    handles = [dev.handle, sa.handle, sb.handle, guides.handle, C.byref(ok), dst.handle]
    for i in range(len(handles)):                                                  # each NULL argument
        args = list(handles)
        args[i] = None
        assert L.ptDenoiseSampleBufferPair(*args) != 0
        assert len(L.ptGetLastError()) > 0
    other = pt.Device(0)                                # a second pt_device: its objects belong to another device
    foreign, foreign_guides = pt.SampleBuffer(other, W, H), pt.DenoiseGuides(other, W, H)
    foreign.write(marker)
    fails(lambda: sa.denoise_pair(foreign, guides, out=dst))                       # b of another device
    fails(lambda: sa.denoise_pair(sb, guides, out=foreign))                        # dst of another device
    fails(lambda: sa.denoise_pair(sb, foreign_guides, out=dst))                    # guides of another device
    fails(lambda: foreign.denoise_pair(sb, guides, out=dst))                       # a's device against all the rest
    assert np.array_equal(bits(foreign.read()), bits(marker))
    for x in (foreign_guides, foreign, other):
        x.close()
    dev.synchronize()
    assert np.array_equal(bits(dst.read()), bits(marker))                          # nothing was written
    assert np.array_equal(bits(small.read()), bits(marker[:H - 1]))
    assert np.array_equal(bits(sa.read()), bits(a))
    assert np.array_equal(bits(sb.read()), bits(b))
    assert np.array_equal(guides.read(), g0)
    for x in (small_guides, guides, small, dst, sb, sa):
        x.close()


@pytest.mark.parametrize("iterations", [0, 3])
def test_kernel_stats_count_prepare_and_iterations(pt, dev, iterations):
    W, H = 40, 24
    sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    guides = pt.DenoiseGuides(dev, W, H)
    a, b = dpc.pair(W, H, 1)
    sa.write(a)
    sb.write(b)
    guides.write(dc.crafted_guides(W, H))
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    dst = sa.denoise_pair(sb, guides, params(pt, iterations))
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_DENOISE)
    dev.set_profiling(False)
    assert n == iterations + 1 and ms > 0
    for x in (dst, guides, sb, sa):
        x.close()
