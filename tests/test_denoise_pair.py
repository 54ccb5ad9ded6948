"""The variance-guided denoiser over two half renders on the CPU (DESIGN.md
§6 row 7): the host implementation (ptsDenoisePair / pt.denoise_pair_host)
against the numpy restatement (tests/denoise_pair_restatement.py) bit for
bit, the filter's defining properties, argument checks, and real frames of
configs 1 and 2 on which it must beat the single-buffer filter."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import denoise_pair_cases as dpc
import denoise_pair_restatement as dpr
import denoise_restatement as dr
import oracle_lib

F = np.float32
NONE = 0xFFFFFFFF
# (5, 3): every step >= 4 exceeds the image and the 3x3 prefilter touches
# every border; the other two are the single-buffer test's.
SIZES = [(5, 3), (40, 24), (67, 45)]
ITERATIONS = [0, 1, 3, 5]
DEFAULTS = (5, 4.0, 0.25, 0.3, 0.1)


def params(pt, iterations):
    return pt.DenoisePairParameters(iterations, dpc.PARAMS["sigma_luminance"], dpc.PARAMS["sigma_normal"],
                                    dpc.PARAMS["sigma_depth"], dpc.PARAMS["sigma_albedo"])


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def crafted(request):
    """(A, B, guides, restated results for Iterations 0..5), computed once per size."""
    W, H = request.param
    (a, b), g = dpc.pair(W, H, seed=W), dc.crafted_guides(W, H)
    return a, b, g, dpr.denoise_pair(a, b, g, max(ITERATIONS), return_all=True, **dpc.PARAMS)


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_host_matches_restatement(pt, crafted, iterations):
    a, b, g, ref = crafted
    a0, b0 = a.copy(), b.copy()
    out = pt.denoise_pair_host(a, b, g, params(pt, iterations))
    same = dc.same_bits(out, ref[iterations])
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(a.view(np.uint32), a0.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), b0.view(np.uint32))
    if iterations and a.shape[0] > 3:
        # the filter did something: most filled pixels moved away from the plain mean
        moved = (out[..., :3] != ref[0][..., :3]).any(axis=-1)
        assert moved.sum() > 0.5 * ((a + b)[..., 3] > 0).sum()


def test_crafted_pairs_have_every_feature():
    for W, H in SIZES + [(130, 70)]:
        a, b = dpc.pair(W, H, seed=W)
        f = dpc.features(a, b)
        assert all(f.values()), (W, H, f)


def test_zero_iterations_is_the_mean_of_the_sum(pt):
    W, H = 40, 24
    (a, b), g = dpc.pair(W, H, 3), dc.crafted_guides(W, H)
    out = pt.denoise_pair_host(a, b, g, params(pt, 0))
    s = a + b                                     # binary32, per component
    live = s[..., 3] > 0
    assert live.any() and (~live).any()
    with np.errstate(all="ignore"):
        exp = s[..., :3] / s[..., 3:4]
    assert np.array_equal(out[live][:, :3].view(np.uint32), exp[live].view(np.uint32))
    assert np.all(out[live][:, 3] == 1.0)
    assert np.all(out[~live].view(np.uint32) == 0)               # empty pixels are +0, 0, 0, 0


@pytest.mark.parametrize("iterations", [1, 5, 6])
def test_empty_pixels_stay_empty(pt, iterations):
    W, H = 40, 24
    (a, b), g = dpc.pair(W, H, 4), dc.crafted_guides(W, H)
    out = pt.denoise_pair_host(a, b, g, params(pt, iterations))
    live = (a + b)[..., 3] > 0
    assert np.all(out[~live].view(np.uint32) == 0)
    assert np.all(out[live][:, 3] == 1.0)


def flat_guides(W, H):
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    g["shape"] = 1
    g["normal"] = (0.0, 0.0, 1.0)
    g["time"] = 2.0
    g["albedo"] = 0.5
    return g


def test_one_half_pixel_takes_the_squared_luminance(pt):
    """A pixel filled in one half only has no variance estimate and takes
    v = l(c_0)^2: through the restatement on a 1x1 image, both ways round, and
    on an isolated pixel of a larger image, whose 3x3 prefilter sees itself
    alone (k v / k = v exactly, k = 1/4).  The host implementation returns the
    restatement's bits in both."""
    one = np.array([[[1.5, 2.5, 0.5, 2.0]]], F)
    none = np.zeros((1, 1, 4), F)
    g1 = flat_guides(1, 1)
    lum = F(2.5) / F(2.0)
    for a, b in ((one, none), (none, one)):
        _, var = dpr.denoise_pair(a, b, g1, 1, return_all=True, return_variance=True)
        assert var[0][0, 0] == lum * lum                          # prefiltered: the only tap
        c, raw, filled = dpr.start(a, b)
        assert filled[0, 0] and raw[0, 0] == lum * lum
        out = pt.denoise_pair_host(a, b, g1, pt.DenoisePairParameters(1))
        assert np.array_equal(out.view(np.uint32), np.array([[[0.75, 1.25, 0.25, 1.0]]], F).view(np.uint32))
    both = dpr.start(one, one * F(3.0))[1][0, 0]
    assert both == F(0.0)                                         # the same mean in both halves: no variance

    W, H = 12, 9
    rng = np.random.default_rng(11)
    a = rng.uniform(0.1, 4, size=(H, W, 4)).astype(F)
    b = rng.uniform(0.1, 4, size=(H, W, 4)).astype(F)
    a[..., 3], b[..., 3] = 3.0, 5.0
    g = flat_guides(W, H)
    g["shape"][4, 6] = 5                                          # isolated by its shape
    b[4, 6] = 0                                                   # and filled in A only
    res, var = dpr.denoise_pair(a, b, g, 3, return_all=True, return_variance=True)
    l46 = a[4, 6, 1] / a[4, 6, 3]
    assert var[0][4, 6] == l46 * l46
    two = dpr.start(a, b)[1]
    d = (a[4, 5, 1] / F(3.0) - b[4, 5, 1] / F(5.0)) * F(0.5)
    assert two[4, 5] == d * d                                     # its neighbour is filled in both
    out = pt.denoise_pair_host(a, b, g, pt.DenoisePairParameters(3))
    assert dc.same_bits(out, res[3]).all()
    assert np.array_equal(out[4, 6, :3].view(np.uint32), (a[4, 6, :3] / F(3.0)).view(np.uint32))


def test_noise_does_not_cross_a_shape_edge(pt):
    """Two shapes with constant colours 0 and 1, noise only inside the
    second (independent in A and B): no output pixel of the first moves from
    0, and inside the second the noise shrinks."""
    W, H = 48, 32
    rng = np.random.default_rng(6)
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    ys, xs = np.mgrid[0:H, 0:W]
    second = xs + ys // 2 > W // 2
    g["shape"] = np.where(second, 2, 1)
    g["normal"] = (0.0, 0.0, 1.0)
    g["time"] = 1.0
    g["albedo"] = 0.5
    halves = []
    for _ in range(2):
        a = np.zeros((H, W, 4), F)
        a[..., 3] = 4.0
        a[second, :3] = 4.0 * (1.0 + rng.normal(0, 0.5, size=(int(second.sum()), 3)))
        halves.append(a)
    out = pt.denoise_pair_host(halves[0], halves[1], g, pt.DenoisePairParameters(5, 16.0, 1.0, 1.0, 1.0))
    assert np.all(out[~second][:, :3] == 0.0)
    noisy = (halves[0] + halves[1])[second][:, :3] / 8.0
    assert out[second][:, :3].std() < 0.5 * noisy.std()


def test_argument_errors_leave_out_untouched(pt):
    N = pt._native
    L = N.scene_lib()
    W, H = 4, 3
    a, b = np.ones((H, W, 4), F), np.full((H, W, 4), 2.0, F)
    g = np.zeros((H, W), N.DENOISE_GUIDE_DTYPE)
    out = np.full((H, W, 4), 7.0, F)
    P = N.pt_denoise_pair_parameters
    ok = P(5, 1.0, 1.0, 1.0, 1.0)
    A, B, G, O = N.fptr(a), N.fptr(b), g.ctypes.data, N.fptr(out)
    calls = [
        (W, H, None, B, G, C.byref(ok), O),
        (W, H, A, None, G, C.byref(ok), O),
        (W, H, A, B, None, C.byref(ok), O),
        (W, H, A, B, G, None, O),
        (W, H, A, B, G, C.byref(ok), None),
        (0, H, A, B, G, C.byref(ok), O),
        (W, 0, A, B, G, C.byref(ok), O),
        (W, H, A, A, G, C.byref(ok), O),                                   # accum_a is accum_b
        (W, H, A, B, G, C.byref(P(9, 1.0, 1.0, 1.0, 1.0)), O),
        (W, H, A, B, G, C.byref(P(5, 0.0, 1.0, 1.0, 1.0)), O),
        (W, H, A, B, G, C.byref(P(5, 1.0, 0.0, 1.0, 1.0)), O),
        (W, H, A, B, G, C.byref(P(5, 1.0, 1.0, -1.0, 1.0)), O),
        (W, H, A, B, G, C.byref(P(5, 1.0, 1.0, 1.0, 0.0)), O),
        (W, H, A, B, G, C.byref(P(5, float("nan"), 1.0, 1.0, 1.0)), O),
    ]
    for args in calls:
        assert L.ptsDenoisePair(*args) != 0
        assert np.all(out == 7.0)
    assert L.ptsDenoisePair(W, H, A, B, G, C.byref(ok), O) == 0
    assert np.all(out[..., 3] == 1.0)
    with pytest.raises(pt.PathTracerError):
        pt.denoise_pair_host(a, a, g)                                      # the same array twice
    with pytest.raises(pt.PathTracerError):
        pt.denoise_pair_host(a, b, g, pt.DenoisePairParameters(Iterations=9))
    with pytest.raises(ValueError):
        pt.denoise_pair_host(a, b[:2], g)
    with pytest.raises(ValueError):
        pt.denoise_pair_host(a, b, g[:2])


def test_defaults_are_the_recorded_ones(pt):
    p = pt.DenoisePairParameters()
    assert (p.Iterations, p.SigmaLuminance, p.SigmaNormal, p.SigmaDepth, p.SigmaAlbedo) == DEFAULTS
    d = pt.DenoiseParameters()
    assert (p.SigmaNormal, p.SigmaDepth, p.SigmaAlbedo) == (d.SigmaNormal, d.SigmaDepth, d.SigmaAlbedo)
    assert C.sizeof(p.as_struct()) == 20


def oracle_halves(pt, config, W, H, rounds, reference_rounds):
    """(A, B, reference, guides): halves of `rounds` rounds with FrameIndex 0
    and 1 << 24 (Reset, Run(2), Run(1) ...) and an independent reference
    (FrameIndex 2 << 24) of `reference_rounds` rounds, on the CPU oracle."""
    scene = pt.Scene.config(config)
    frames = []
    for frame_index, n in ((0, rounds), (1 << 24, rounds), (2 << 24, reference_rounds)):
        o = oracle_lib.OracleRenderer(scene.packs(), W, H)
        o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
        o.FrameIndex = frame_index
        o.reset()
        o.run(2)
        for _ in range(n - 2):
            o.run(1)
        frames.append(o.accum())
        o.close()
    g = dr.guides(scene, 0, W, H)
    scene.close()
    assert (g["shape"] != NONE).any()
    return frames[0], frames[1], frames[2], g


def ratios(pt, a, b, reference, g):
    """(pair, single): relative L2 error against the reference mean of the
    pair filter on (A, B) and of the single-buffer filter on A + B, both with
    their defaults, over the undenoised A + B frame's."""
    def mean(acc):
        with np.errstate(all="ignore"):
            return np.where(acc[..., 3:4] > 0, acc[..., :3] / acc[..., 3:4], 0).astype(np.float64)

    ref = mean(reference)
    s = a + b
    before = np.linalg.norm(mean(s) - ref)
    pair = np.linalg.norm(pt.denoise_pair_host(a, b, g)[..., :3].astype(np.float64) - ref) / before
    single = np.linalg.norm(pt.denoise_host(s, g)[..., :3].astype(np.float64) - ref) / before
    print(f"relative L2 over the undenoised frame's: pair {pair:.4f}, single-buffer {single:.4f}")
    return pair, single


def test_converged_frame_is_not_damaged(pt):
    """Config 1 at 64x32 on the CPU oracle, halves of 128 rounds against an
    independent 2048-round mean: the pair filter's error ratio is below 1 (it
    still helps a frame this converged) and below the single-buffer default
    filter's on A + B, which raises the error.  Measured with the host
    implementation and the defaults: pair 0.7196, single-buffer 1.4518 (the
    float64 prototype gave 0.745 and 1.558); the tighter bound asserted after
    the conditions themselves is halfway between the measured ratio and 1:
    0.8598."""
    a, b, reference, g = oracle_halves(pt, 1, 64, 32, 128, 2048)
    pair, single = ratios(pt, a, b, reference, g)
    assert pair < 1.0
    assert pair < single
    assert pair < 0.8598


def test_bright_noisy_frame_gains_more(pt):
    """Config 2 at 64x64, halves of 4 rounds against an independent
    2048-round mean: the pair filter's ratio is below the single-buffer
    default filter's, whose fixed colour sigma is small against this frame's
    noise.  Measured: pair 0.2478, single-buffer 0.3953 (prototype 0.248 and
    0.398); the tighter bound is halfway between the measured ratio and 1:
    0.6239."""
    a, b, reference, g = oracle_halves(pt, 2, 64, 64, 4, 2048)
    pair, single = ratios(pt, a, b, reference, g)
    assert pair < single
    assert pair < 0.6239
