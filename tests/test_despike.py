"""CPU: the firefly clamp.  ptsDespike against the numpy
restatement bit for bit on every case of tests/despike_cases.py; the
properties that follow from the definition; the rejected arguments; the Python
surface; and, on frames rendered by the oracle, what the clamp is for: the
denoiser's error on config 2 drops, config 1 is left alone."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_restatement as dr
import despike_cases as xc
import despike_restatement as xd
import oracle_lib

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(pt, case, **kw):
    return pt.despike_host(case["src"], case["guides"], xc.params_object(pt, dict(case["params"], **kw)))


@pytest.mark.parametrize("name", xc.names())
def test_host_matches_restatement(pt, name):
    case, ref = xc.all_cases()[name]
    src, guides = case["src"].copy(), case["guides"].copy()
    got = host(pt, case)
    same = xc.same_bits(got, ref)
    assert same.all(), np.argwhere(~same)[:5]
    assert case["src"].tobytes() == src.tobytes() and case["guides"].tobytes() == guides.tobytes()


def test_names_are_the_cases():
    assert sorted(xc.names()) == sorted(xc.all_cases())


@pytest.mark.parametrize("name", xc.names())
def test_properties(pt, name):
    """.w keeps its bits; a pixel either keeps all its bits or is usable and
    has v(out) <= v(src), its colour scaled by one factor in [0, 1)."""
    case, _ = xc.all_cases()[name]
    src, out = case["src"], host(pt, case)
    assert np.array_equal(bits(out[..., 3]), bits(src[..., 3]))
    changed = ~xc.same_bits(out, src).all(axis=-1)
    assert xd.ok(src[changed]).all()
    with np.errstate(all="ignore"):
        assert (xd.value(out[changed]) <= xd.value(src[changed])).all()
        assert (np.abs(out[changed][:, :3]) <= np.abs(src[changed][:, :3])).all()


def test_zero_block_clamps_its_positive_pixel_to_plus_zero(pt):
    """The yardstick of the pixel inside the block of zeros is a zero of
    either sign; the limit is +0 whichever it is, and the clamped colour
    (positive sums times +0) is +0 in every component."""
    for name in ("16x16-r1", "33x18-r2", "67x45-r3"):
        case, _ = xc.all_cases()[name]
        H, W = case["guides"].shape
        _, inside, _ = xc.blocks(W, H)
        out = host(pt, case)
        assert (case["src"][inside][:, :3] > 0).all()
        assert not bits(out[inside][:, :3]).any(), name


def test_rejected_arguments_leave_out_untouched(pt):
    N = pt._native
    L = N.scene_lib()
    case, _ = xc.all_cases()["16x16-r1"]
    src, g = case["src"].copy(), np.ascontiguousarray(case["guides"])
    marker = np.full((16, 16, 4), 7.0, F)
    out = marker.copy()
    P = pt.DespikeParameters
    ok = P().as_struct()

    def call(w=16, h=16, a=src, gp=g.ctypes.data, p=ok, o=out):
        return L.ptsDespike(w, h, None if a is None else N.fptr(a), gp, None if p is None else C.byref(p),
                            None if o is None else N.fptr(o))

    assert call(a=None) != 0 and call(gp=None) != 0 and call(p=None) != 0 and call(o=None) != 0
    assert call(w=0) != 0 and call(h=0) != 0
    assert call(o=src) != 0                                                # out is the input
    nan, inf = float("nan"), float("inf")
    for bad in (P(Radius=0), P(Radius=4), P(Rank=0), P(Rank=5), P(Rank=3, MinNeighbours=2), P(MinNeighbours=0),
                P(Radius=3, MinNeighbours=49), P(Radius=2, MinNeighbours=25), P(Radius=1, MinNeighbours=9),
                P(Scale=-0.5), P(Scale=nan), P(Scale=inf), P(Floor=-0.5), P(Floor=nan), P(Floor=inf), P(Floor=-0.0),
                P(NormalCosine=-1.0), P(NormalCosine=1.01), P(NormalCosine=nan)):
        assert call(p=bad.as_struct()) != 0, vars(bad)
        with pytest.raises(pt.PathTracerError):
            pt.despike_host(src, g, bad)
    assert np.array_equal(bits(out), bits(marker))
    assert src.tobytes() == case["src"].tobytes()
    for good in (P(), P(Radius=1, Rank=1, MinNeighbours=1, Scale=0.0, Floor=0.0, NormalCosine=1.0),
                 P(Radius=3, Rank=4, MinNeighbours=48), P(Radius=2, MinNeighbours=24), P(Radius=1, MinNeighbours=8),
                 P(Floor=3.0, NormalCosine=-0.99)):
        assert call(p=good.as_struct()) == 0, vars(good)
    assert not np.array_equal(bits(out), bits(marker))
    with pytest.raises(ValueError):
        pt.despike_host(src[:15], g)
    with pytest.raises(ValueError):
        pt.despike_host(src, g[:, :15])


def test_parameters_defaults_and_struct_round_trip(pt):
    p = pt.DespikeParameters()
    names = ("Radius", "Rank", "MinNeighbours", "Scale", "Floor", "NormalCosine")
    assert tuple(getattr(p, n) for n in names) == tuple(
        xd.DEFAULTS[k] for k in ("radius", "rank", "min_neighbours", "scale", "floor", "normal_cosine"))
    s = pt.DespikeParameters(2, 4, 5, 1.5, 0.25, 0.5).as_struct()
    assert C.sizeof(s) == 24
    assert tuple(getattr(s, n) for n in names) == (2, 4, 5, 1.5, 0.25, 0.5)
    raw = np.frombuffer(bytes(s), np.uint32)
    assert raw[:3].tolist() == [2, 4, 5] and raw[3:].view(F).tolist() == [1.5, 0.25, 0.5]
    assert "DespikeParameters" in pt.__all__ and "despike_host" in pt.__all__
    assert hasattr(pt.SampleBuffer, "despike")


def render(pt, config, W, H, rounds, frame_index=0):
    scene = pt.Scene.config(config)
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.FrameIndex = frame_index
    o.reset()
    o.run(2)
    for _ in range(rounds - 2):
        o.run(1)
    accum = o.accum()
    o.close()
    return scene, accum


def mean(acc):
    w = acc[..., 3:4]
    return np.where(w > 0, acc[..., :3] / np.maximum(w, 1e-30), 0.0).astype(np.float64)


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.slow
def test_rendered_frames(pt):
    """Config 2 at 64x64, 8 rounds, against 1024 rounds of stream 1 << 24: the
    denoiser after the clamp has at most 0.75 of the denoiser's error alone
    (default parameters both), and the clamp touches 1 % to 20 % of the frame.
    Config 1 at 64x32 has no fireflies: the clamped frame's error is at most
    1.02 of the unclamped one's."""
    scene, noisy = render(pt, 2, 64, 64, 8)
    g = dr.guides(scene, 0, 64, 64)
    scene.close()
    scene, ref = render(pt, 2, 64, 64, 1024, 1 << 24)
    scene.close()
    ref = mean(ref)
    plain = rel_l2(pt.denoise_host(noisy, g)[..., :3].astype(np.float64), ref)
    clamped = rel_l2(pt.denoise_host(pt.despike_host(noisy, g), g)[..., :3].astype(np.float64), ref)
    _, d = xd.despike(noisy, g, detail=True, **xd.DEFAULTS)
    share = float(d["clamped"].mean())
    print(f"C2: denoised {plain:.4f}, clamped then denoised {clamped:.4f}, ratio {clamped / plain:.4f}, "
          f"clamped share {share:.4f}")
    assert clamped <= 0.75 * plain
    assert 0.01 <= share <= 0.20

    scene, noisy = render(pt, 1, 64, 32, 8)
    g = dr.guides(scene, 0, 64, 32)
    scene.close()
    scene, ref = render(pt, 1, 64, 32, 1024, 1 << 24)
    scene.close()
    ref = mean(ref)
    before, after = rel_l2(mean(noisy), ref), rel_l2(mean(pt.despike_host(noisy, g)), ref)
    print(f"C1: unclamped {before:.4f}, clamped {after:.4f}, ratio {after / before:.4f}")
    assert after <= 1.02 * before
