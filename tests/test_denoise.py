"""The denoiser on the CPU: the host implementation
(ptsDenoise / pt.denoise_host) against the numpy restatement
(tests/denoise_restatement.py) bit for bit, the filter's defining
properties, argument checks, and a real 8-round frame of config 1 that must
come out closer to the 512-round mean than it went in."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import denoise_restatement as dr
import oracle_lib

F = np.float32
NONE = 0xFFFFFFFF
ITERATIONS = [0, 1, 3, 5, 6]      # at 6 the step, 32, exceeds half of both image sizes


def params(pt, iterations):
    return pt.DenoiseParameters(iterations, dc.PARAMS["sigma_color"], dc.PARAMS["sigma_normal"],
                                dc.PARAMS["sigma_depth"], dc.PARAMS["sigma_albedo"])


@pytest.fixture(scope="module", params=dc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def crafted(request):
    """(accumulator, guides, restated results for Iterations 0..6), computed once per size."""
    W, H = request.param
    a, g = dc.accumulators(W, H, seed=W), dc.crafted_guides(W, H)
    return a, g, dr.denoise(a, g, max(ITERATIONS), return_all=True, **dc.PARAMS)


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_host_matches_restatement(pt, crafted, iterations):
    a, g, ref = crafted
    before = a.copy()
    out = pt.denoise_host(a, g, params(pt, iterations))
    same = dc.same_bits(out, ref[iterations])
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(a.view(np.uint32), before.view(np.uint32))
    if iterations:
        # the filter did something: most filled pixels moved away from the plain mean
        moved = (out[..., :3] != ref[0][..., :3]).any(axis=-1)
        assert moved.sum() > 0.5 * (a[..., 3] > 0).sum()


def test_crafted_guides_have_every_feature():
    for W, H in dc.SIZES:
        g = dc.crafted_guides(W, H)
        s = g["shape"]
        assert set(np.unique(s)) == {0, 1, 2, NONE}
        assert ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] != NONE) & (s[:, :-1] != NONE)).any()      # vertical edge
        assert ((s[1:, :] != s[:-1, :])).any()                                                   # horizontal edge
        diag = (s[1:, 1:] == s[:-1, :-1]) & (s[1:, :-1] != s[:-1, 1:])
        assert diag.any()                                                                        # diagonal edge
        inside0 = (s[:, 1:] == 0) & (s[:, :-1] == 0)
        assert (np.abs(g["normal"][:, 1:] - g["normal"][:, :-1]).max(axis=-1)[inside0] > 0.3).any()   # crease
        assert len(np.unique(g["time"][s != NONE])) > 10                                         # depth ramp
        assert len(np.unique(g["albedo"][s == 0][:, 0])) == 2                                    # checkerboard


def test_zero_iterations_is_the_mean(pt):
    W, H = 40, 24
    a, g = dc.accumulators(W, H, 3), dc.crafted_guides(W, H)
    out = pt.denoise_host(a, g, params(pt, 0))
    live = a[..., 3] > 0
    assert live.any() and (~live).any()
    with np.errstate(all="ignore"):
        exp = a[..., :3] / a[..., 3:4]
    assert np.array_equal(out[live][:, :3].view(np.uint32), exp[live].view(np.uint32))
    assert np.all(out[live][:, 3] == 1.0)
    assert np.all(out[~live].view(np.uint32) == 0)               # empty pixels are +0, 0, 0, 0


@pytest.mark.parametrize("iterations", [1, 5, 6])
def test_empty_pixels_stay_empty(pt, iterations):
    W, H = 40, 24
    a, g = dc.accumulators(W, H, 4), dc.crafted_guides(W, H)
    out = pt.denoise_host(a, g, params(pt, iterations))
    live = a[..., 3] > 0
    assert np.all(out[~live].view(np.uint32) == 0)
    assert np.all(out[live][:, 3] == 1.0)


def test_isolated_pixel_returns_its_own_mean(pt):
    """A pixel whose 5x5 neighbours at every step are empty or of another
    shape has one tap, its own, so it returns (w c) / w.  That is c exactly
    when the centre weight is 9/64 (times a power of two cannot round): the
    guides here have an exactly unit normal, so dn = 0 and exp(-0) = 1."""
    W, H = 40, 24
    rng = np.random.default_rng(5)
    a = rng.uniform(0.1, 4, size=(H, W, 4)).astype(F)
    a[..., 3] = rng.integers(1, 9, size=(H, W)).astype(F)
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    g["shape"] = 1
    g["normal"] = (0.0, 0.0, 1.0)
    g["time"] = 2.0
    g["albedo"] = 0.5
    g["shape"][7, 9] = 5                         # another shape than all of its neighbours
    a[10, 30:] = 0                               # a pixel among empty ones ...
    a[10, 33, :] = (1.25, 2.5, 0.75, 3.0)
    for i in range(5):                           # ... at every step: its lattice taps are emptied too
        s = 1 << i
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y, x = 10 + s * dy, 33 + s * dx
                if (dy or dx) and 0 <= y < H and 0 <= x < W:
                    a[y, x] = 0
    out = pt.denoise_host(a, g, params(pt, 5))
    for y, x in ((7, 9), (10, 33)):
        exp = a[y, x, :3] / a[y, x, 3]
        assert np.array_equal(out[y, x, :3].view(np.uint32), exp.view(np.uint32)), (y, x)
        assert out[y, x, 3] == 1.0


def test_noise_does_not_cross_a_shape_edge(pt):
    """Two shapes with constant colours 0 and 1, noise only inside the
    second: no output pixel of the first moves from 0."""
    W, H = 48, 32
    rng = np.random.default_rng(6)
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    ys, xs = np.mgrid[0:H, 0:W]
    second = xs + ys // 2 > W // 2
    g["shape"] = np.where(second, 2, 1)
    g["normal"] = (0.0, 0.0, 1.0)
    g["time"] = 1.0
    g["albedo"] = 0.5
    a = np.zeros((H, W, 4), F)
    a[..., 3] = 4.0
    a[second, :3] = 4.0 * (1.0 + rng.normal(0, 0.5, size=(int(second.sum()), 3)))
    out = pt.denoise_host(a, g, pt.DenoiseParameters(5, 10.0, 1.0, 1.0, 1.0))     # wide colour sigma: only the shape stops it
    assert np.all(out[~second][:, :3] == 0.0)
    noisy = a[second][:, :3] / 4.0
    assert out[second][:, :3].std() < 0.5 * noisy.std()          # and inside the second shape the noise shrank


def test_argument_errors_leave_out_untouched(pt):
    N = pt._native
    L = N.scene_lib()
    W, H = 4, 3
    a = np.ones((H, W, 4), F)
    g = np.zeros((H, W), N.DENOISE_GUIDE_DTYPE)
    out = np.full((H, W, 4), 7.0, F)
    ok = N.pt_denoise_parameters(5, 1.0, 1.0, 1.0, 1.0)
    calls = [
        (W, H, None, g.ctypes.data, C.byref(ok), N.fptr(out)),
        (W, H, N.fptr(a), None, C.byref(ok), N.fptr(out)),
        (W, H, N.fptr(a), g.ctypes.data, None, N.fptr(out)),
        (W, H, N.fptr(a), g.ctypes.data, C.byref(ok), None),
        (W, H, N.fptr(a), g.ctypes.data, C.byref(N.pt_denoise_parameters(9, 1.0, 1.0, 1.0, 1.0)), N.fptr(out)),
        (W, H, N.fptr(a), g.ctypes.data, C.byref(N.pt_denoise_parameters(5, 0.0, 1.0, 1.0, 1.0)), N.fptr(out)),
        (W, H, N.fptr(a), g.ctypes.data, C.byref(N.pt_denoise_parameters(5, 1.0, 1.0, -1.0, 1.0)), N.fptr(out)),
        (W, H, N.fptr(a), g.ctypes.data, C.byref(N.pt_denoise_parameters(5, 1.0, 1.0, 1.0, float("nan"))), N.fptr(out)),
    ]
    for args in calls:
        assert L.ptsDenoise(*args) != 0
        assert np.all(out == 7.0)
    assert L.ptsDenoise(W, H, N.fptr(a), g.ctypes.data, C.byref(ok), N.fptr(out)) == 0
    with pytest.raises(pt.PathTracerError):
        pt.denoise_host(a, g, pt.DenoiseParameters(Iterations=9))
    with pytest.raises(ValueError):
        pt.denoise_host(a, g[:2], pt.DenoiseParameters())


def test_defaults_are_the_recorded_ones(pt):
    p = pt.DenoiseParameters()
    assert (p.Iterations, p.SigmaColor, p.SigmaNormal, p.SigmaDepth, p.SigmaAlbedo) == DEFAULTS
    s = p.as_struct()
    assert C.sizeof(s) == 20 and pt.DENOISE_GUIDE_DTYPE.itemsize == 32


DEFAULTS = (5, 0.5, 0.25, 0.3, 0.1)


def test_real_frame_gets_closer_to_the_converged_mean(pt):
    """Config 1 at 64x32 on the CPU oracle: 8 rounds (Reset, Run(2), six
    Run(1)) against 512 rounds.  The denoised frame's relative L2 error
    against the 512-round mean must be lower than the undenoised frame's.
    Measured with the host implementation and the default parameters: 0.0758
    against 0.2210, a ratio of 0.3429; the tighter bound asserted after the
    condition itself is halfway between that ratio and 1: 0.6715."""
    W, H = 64, 32
    scene = pt.Scene.config(1)
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.reset()
    o.run(2)
    for _ in range(6):
        o.run(1)
    noisy = o.accum()
    for _ in range(512 - 8):
        o.run(1)
    converged = o.accum()
    o.close()
    g = dr.guides(scene, 0, W, H)
    scene.close()
    assert (g["shape"] != NONE).any()

    def mean(acc):
        with np.errstate(all="ignore"):
            return np.where(acc[..., 3:4] > 0, acc[..., :3] / acc[..., 3:4], 0).astype(np.float64)

    ref = mean(converged)
    den = pt.denoise_host(noisy, g)[..., :3].astype(np.float64)
    before = np.linalg.norm(mean(noisy) - ref) / np.linalg.norm(ref)
    after = np.linalg.norm(den - ref) / np.linalg.norm(ref)
    print(f"relative L2 vs 512 rounds: undenoised {before:.4f}, denoised {after:.4f}, ratio {after / before:.4f}")
    assert after < before
    assert after / before < 0.6715


@pytest.mark.parametrize("config,camera", [(1, 0), (5, 1)], ids=["c1-pinhole", "c5-360"])
def test_central_ray_is_the_unjittered_first_ray(pt, config, camera):
    """Without jitter and with a zero aperture (C1's pinhole; the 360 model
    has no lens) the integrator's first ray of a pixel is its central ray:
    the restated central ray equals the oracle's raygen, origin bits and
    packed velocity."""
    W, H = 24, 18
    scene = pt.Scene.config(config)
    cam = scene.arrays()["cameras"][camera]
    assert int(cam["Model"]) == 2 or float(cam["ApertureRadius"]) == 0.0
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.CameraIndex = camera
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE          # no SAMPLE_JITTER
    o.reset()
    st = o.state()
    o.close()
    for y in range(H):
        for x in range(W):
            org, pv = dr.central_ray(cam, x, y, W, H)
            assert np.array_equal(np.array(org, F).view(np.uint32), st[y, x]["origin"].view(np.uint32)), (x, y)
            assert pv == int(st[y, x]["packed_velocity"]), (x, y)
    scene.close()
