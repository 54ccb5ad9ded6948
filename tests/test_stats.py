"""Frame statistics on the CPU: the host implementation
(ptsFrameStatistics / pt.frame_statistics_host) against the numpy
restatement (tests/stats_restatement.py) in every field, the double helpers
against hand-built histograms, the struct layout, argument checks, and the
CPU oracle's config 1: automatic exposure lands on the key, and the noise
figure of two half renders falls as they converge."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib
import stats_cases as sc
import stats_restatement as sr

F = np.float32
ALL_SIZES = sc.SIZES + [sc.LARGE]
CASES = ["crafted", "constant", "empty", "pair", "pair-constant", "pair-equal", "pair-empty"]


@pytest.fixture(scope="module", params=ALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def cases(request):
    return sc.cases(*request.param)


@pytest.mark.parametrize("name", CASES)
def test_host_matches_restatement(pt, cases, name):
    a, b = cases[name]
    before = a.copy(), None if b is None else b.copy()
    got = pt.frame_statistics_host(a, b)
    want = sr.statistics(a, b)
    assert sr.differences(got, want) == []
    assert got.pixels == a.shape[0] * a.shape[1] == got.filled + got.empty + got.nonfinite
    assert int(got.luminance_histogram.sum()) == got.filled - got.dark
    assert int(got.noise_histogram.sum()) == got.noise_pixels
    assert np.array_equal(a.view(np.uint32), before[0].view(np.uint32))
    if b is None:
        assert got.noise_pixels == got.noise_skipped == 0 and not got.noise_histogram.any()
    else:
        assert np.array_equal(b.view(np.uint32), before[1].view(np.uint32))


def test_crafted_cases_exercise_every_rule(pt):
    W, H = sc.SIZES[0]
    s = sr.statistics(sc.crafted(W, H, seed=W))
    assert s["nonfinite"] >= 8 and s["empty"] > 10 and s["dark"] >= 3 + 8     # planted + the negative-sum run
    h = s["luminance_histogram"]
    assert h[0] >= 4 and h[255] >= 4                       # 2 denormals, 2^-32, just below; 1.75 2^31, 2^32, 2^40, +inf
    for k in (-31, -3, 0, 5, 31):                          # each planted edge opens its own bin
        for m in range(4):
            assert h[128 + 4 * k + m] >= 1, (k, m)
    assert math.isinf(float(s["max_luminance"])) and 0 < float(s["min_luminance"]) < 1e-44
    assert s["min_samples"] == F(1e-3) and s["max_samples"] == F(1e3)
    a, b = sc.pair(W, H, seed=W)
    p = sr.statistics(a, b)
    assert p["noise_skipped"] >= 3 and p["noise_histogram"][0] >= 7 and p["noise_histogram"][128] >= 1
    fa, fb = sr.classes(a.reshape(-1, 4))[2], sr.classes(b.reshape(-1, 4))[2]
    assert (fa & ~fb).sum() > 5 and (fb & ~fa).sum() > 5   # the filled-in-both rule matters
    assert p["noise_pixels"] + p["noise_skipped"] == (fa & fb).sum()
    assert p["nonfinite"] > sr.statistics(a)["nonfinite"]  # sums that are not finite although the halves are
    c = sr.statistics(sc.constant(W, H))
    assert c["luminance_histogram"][pt._native.scene_lib().ptsStatsBin(0.125)] == W * H
    e = sr.statistics(sc.empty(W, H))
    assert e["empty"] == W * H and all(float(e[k]) == 0 for k in sr.FLOATS)


def test_bin_function_and_edges(pt):
    L = pt._native.scene_lib()
    edges = pt.FrameStatistics.bin_edges()
    assert edges.shape == (257,) and edges[128] == 1.0 and edges[0] == 2.0 ** -32 and edges[256] == 2.0 ** 32
    assert edges[129] == 1.25 and edges[131] == 1.75 and edges[132] == 2.0
    assert [sr.edge(b) for b in range(257)] == list(edges)
    for b in range(256):
        lo, hi = F(edges[b]), F(edges[b + 1])
        assert L.ptsStatsBin(lo) == b and L.ptsStatsBin(np.nextafter(hi, F(0))) == b
    assert L.ptsStatsBin(F(0)) == 0 and L.ptsStatsBin(F(1e-45)) == 0 and L.ptsStatsBin(np.nextafter(F(2.0 ** -32), F(0))) == 0
    assert L.ptsStatsBin(F(2.0 ** 32)) == 255 and L.ptsStatsBin(F(np.inf)) == 255 and L.ptsStatsBin(F(3e38)) == 255
    v = np.random.default_rng(3).uniform(-40, 40, 4096)
    v = (2.0 ** v).astype(F)
    assert [L.ptsStatsBin(x) for x in v] == list(sr.bins(v))
    assert L.ptsStatsBinEdge(-1) == 0.0 and L.ptsStatsBinEdge(257) == 0.0


def stats_with(pt, lum=None, noise=None):
    s = pt._native.pt_frame_statistics()
    for field, h in (("luminance_histogram", lum), ("noise_histogram", noise)):
        if h is not None:
            getattr(s, field)[:] = [int(x) for x in h]
    return pt.FrameStatistics(s)


def test_helpers_on_hand_built_histograms(pt):
    h = np.zeros(256, np.uint32)
    empty = stats_with(pt)
    assert empty.percentile(0.5) == -1 and empty.percentile(0.5, "noise") == -1
    assert empty.log_average() == 0.0 and empty.auto_brightness() == 1.0 and math.isinf(empty.noise())
    h[[10, 100, 130, 200]] = (3, 4, 1, 8)                  # total 16: q = 1 / 16 is exact
    s = stats_with(pt, lum=h, noise=h)
    for which in ("luminance", "noise"):
        assert s.percentile(1.0, which) == 200
        assert s.percentile(1.0 / 16, which) == 10         # the first pixel
        assert s.percentile(3.0 / 16, which) == 10 and s.percentile(4.0 / 16, which) == 100
        assert s.percentile(0.5, which) == 130 and s.percentile(0.51, which) == 200
    for q in (1e-9, 0.01, 0.3, 0.5, 0.95, 0.99, 1.0):
        assert s.percentile(q) == sr.percentile_bin(h, q)
        assert s.noise(q) == pytest.approx(sr.noise({"noise_histogram": h}, q), rel=1e-9)
    assert s.noise(0.5) == sr.edge(131) == 1.75            # the upper edge: conservative
    one = np.zeros(256, np.uint32)
    one[141] = 7                                           # a single bin: its geometric centre
    s1 = stats_with(pt, lum=one)
    centre = math.sqrt(sr.edge(141) * sr.edge(142))
    assert s1.log_average() == pytest.approx(centre, rel=1e-12)
    assert s1.auto_brightness() == pytest.approx(0.18 / centre, rel=1e-12)
    assert s1.auto_brightness(key=0.5) == pytest.approx(0.5 / centre, rel=1e-12)
    rng = np.random.default_rng(8)
    for _ in range(20):
        h = rng.integers(0, 1000, 256).astype(np.uint32) * (rng.uniform(size=256) < 0.2)
        s = stats_with(pt, lum=h, noise=h)
        d = {"luminance_histogram": h, "noise_histogram": h}
        for q_lo, q_hi in ((0.01, 0.99), (0.25, 0.75), (0.5, 0.5), (0.9, 0.1)):
            assert s.log_average(q_lo, q_hi) == pytest.approx(sr.log_average(h, q_lo, q_hi), rel=1e-9)
            assert s.auto_brightness(0.18, q_lo, q_hi) == pytest.approx(sr.auto_brightness(d, 0.18, q_lo, q_hi), rel=1e-9)
        assert s.noise() == pytest.approx(sr.noise(d, 0.95), rel=1e-9)
    p = pt.ResolveParameters.auto(s1, ToneMappingMode=pt.TONE_MAPPING_ACES)
    assert p.Brightness == s1.auto_brightness() and p.ToneMappingMode == pt.TONE_MAPPING_ACES
    assert pt.ResolveParameters.auto(s1, key=0.36).Brightness == pytest.approx(2 * p.Brightness, rel=1e-12)


def test_struct_layout(pt):
    S = pt._native.pt_frame_statistics
    assert C.sizeof(S) == 2120 and pt.STATS_BINS == 256
    want = {"pixels": 0, "filled": 8, "empty": 16, "nonfinite": 24, "dark": 32, "luminance_histogram": 40,
            "min_luminance": 1064, "max_luminance": 1068, "min_samples": 1072, "max_samples": 1076,
            "noise_pixels": 1080, "noise_skipped": 1088, "noise_histogram": 1096}
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == want
    # the C side agrees: a host result read through the mirror has its fields where the restatement puts them
    a = sc.crafted(*sc.SIZES[0])
    assert sr.differences(pt.frame_statistics_host(a), sr.statistics(a)) == []
    assert len(pt.frame_statistics_host(a).tobytes()) == 2120


def test_argument_errors(pt):
    N = pt._native
    L = N.scene_lib()
    a, b = np.ones((3, 4, 4), F), np.ones((3, 4, 4), F)
    out = N.pt_frame_statistics()
    out.pixels = 77
    assert L.ptsFrameStatistics(4, 3, None, None, C.byref(out)) != 0
    assert L.ptsFrameStatistics(4, 3, N.fptr(a), None, None) != 0
    assert L.ptsFrameStatistics(0, 3, N.fptr(a), None, C.byref(out)) != 0
    assert L.ptsFrameStatistics(4, 0, N.fptr(a), None, C.byref(out)) != 0
    assert L.ptsFrameStatistics(4, 3, N.fptr(a), N.fptr(a), C.byref(out)) != 0      # b is a
    assert out.pixels == 77 and out.filled == 0                                       # untouched
    assert L.ptsFrameStatistics(4, 3, N.fptr(a), N.fptr(b), C.byref(out)) == 0 and out.pixels == 12
    with pytest.raises(pt.PathTracerError):
        pt.frame_statistics_host(a, a)
    with pytest.raises(ValueError):
        pt.frame_statistics_host(a, b[:2])
    with pytest.raises(ValueError):
        pt.frame_statistics_host(a[..., :3])
    assert L.ptsStatsPercentileBin(None, 0.5) == -1 and L.ptsStatsAutoBrightness(None, 0.18, 0.01, 0.99) == 1.0


@pytest.fixture(scope="module")
def halves(pt):
    """Config 1 at 64x32 on the CPU oracle, as two independent halves
    (FrameIndex 0 and 1 << 24): {rounds: (A, B)} at 16 and 64 rounds each
    (Reset, Run(2), then Run(1) rounds)."""
    W, H = 64, 32
    scene = pt.Scene.config(1)
    out = {16: [], 64: []}
    for frame in (0, 1 << 24):
        o = oracle_lib.OracleRenderer(scene.packs(), W, H)
        o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
        o.FrameIndex = frame
        o.reset()
        o.run(2)
        for rounds in range(3, 65):
            o.run(1)
            if rounds in out:
                out[rounds].append(o.accum())
        o.close()
    scene.close()
    return {k: tuple(v) for k, v in out.items()}


def test_auto_exposure_puts_the_log_average_at_the_key(pt, halves):
    """b = auto_brightness() at its defaults; the exact log-average of b Y,
    in float64 over the pixels whose bins lie between the two percentile
    bins, is within a factor 1.25 of 0.18: every such pixel is within its
    bin, and a bin is at most a factor 1.25 wide, so the mean of log2 Y and
    the mean of the bins' log2 centres differ by less than log2 1.25."""
    a = halves[16][0]
    s = pt.frame_statistics_host(a)
    b = s.auto_brightness()
    lo, hi = s.percentile(0.01), s.percentile(0.99)
    assert 0 <= lo <= hi
    flat = a.reshape(-1, 4)
    _, _, filled, Y = sr.classes(flat)
    lit = filled & (Y > 0)
    inside = lit.copy()
    inside[lit] = (sr.bins(Y[lit]) >= lo) & (sr.bins(Y[lit]) <= hi)
    assert inside.sum() >= 0.9 * lit.sum()
    exact = 2.0 ** np.mean(np.log2(Y[inside].astype(np.float64)))
    print(f"auto brightness {b:.4f}: exact log-average of b Y = {b * exact:.4f} (key 0.18), "
          f"bins {lo}..{hi}, {inside.sum()} of {lit.sum()} pixels")
    assert 0.18 / 1.25 <= b * exact <= 0.18 * 1.25


def test_noise_falls_as_the_halves_converge(pt, halves):
    """noise(0.5) of the pair at 64 rounds per half is below the one at 16
    (measured on the exact values: 0.015 against 0.029, about two bins
    apart), and at both at least 99 % of the pixels are filled in both."""
    s16 = pt.frame_statistics_host(*halves[16])
    s64 = pt.frame_statistics_host(*halves[64])
    for s in (s16, s64):
        print(f"pair fraction {s.noise_pixels / s.pixels:.4f}, noise(0.5) {s.noise(0.5):.4f}, noise(0.95) {s.noise():.4f}")
        assert s.noise_pixels / s.pixels >= 0.99
        assert s.filled + s.empty == s.pixels                  # a sane frame: nothing is NaN or inf
    assert s64.noise(0.5) < s16.noise(0.5)
    assert s64.noise(0.95) < s16.noise(0.95)
    both = halves[16][0] + halves[16][1]                       # the luminance part describes A + B
    assert sr.differences(pt.frame_statistics_host(both), dict(sr.statistics(both))) == []
    lum = {k: v for k, v in sr.fields(s16).items() if not k.startswith("noise")}
    assert lum == {k: v for k, v in sr.fields(pt.frame_statistics_host(both)).items() if not k.startswith("noise")}
