"""Inputs shared by the firefly-clamp tests (tests/test_despike.py on the CPU,
tests/test_gpu_despike.py on the device).

Synthetic cases, sizes 1x1, 5x3 (smaller than every window), 16x16, 17x16,
33x18 (windows cross tile borders in both directions) and 67x45, each with
Radius 1, 2 and 3 and Rank cycling over 1..4: rectify_cases' guide records (a
sky band, a flat shape and a round one whose normal turns from pixel to pixel)
and its noisy two-sample accumulator.  At most one perturbation per pixel,
chosen by (x + 5 y) mod 97, so that no two pixels of one kind share a window
(|dx + 5 dy| <= 18 there): a spike of 50x; two spikes side by side; Src empty,
NaN, with an infinite component, with a denormal .w (v = +inf); the shape
flipped; the normal tilted just inside and just outside NormalCosine; and,
placed last because the limit depends on everything else, a centre exactly on
its limit L (left half of the frame) or one ulp above it (right half).  Two
blocks lie in the lower half: one of exact zeros, its colours a mix of +0 and
-0, with one positive pixel inside, and one of constant colour.  Extreme
parameters on some of the sizes: MinNeighbours = every neighbour, Scale 0,
Floor > 0, and Rank = MinNeighbours = 1 on 1x1, where nothing can be tested.

Coherent cases: real guides of config 2 at 64x64 and config 5 at 64x32
(denoise_restatement.guides) under the same accumulator recipe.

all_cases() computes the restatement once per case and asserts the coverage
the tests rely on (listed there)."""
from __future__ import annotations

import functools
import sys

import numpy as np

import denoise_restatement as dr
import despike_restatement as xd
import rectify_cases as rc

F = np.float32
NONE = 0xFFFFFFFF
SIZES = ((1, 1), (5, 3), (16, 16), (17, 16), (33, 18), (67, 45))
MIN_NEIGHBOURS = {1: 4, 2: 8, 3: 12}
MODULUS = 97
SPIKE, PAIR, EMPTY, NAN, INF, DENORMAL, FLIP, TILT_IN, TILT_OUT, ON_LIMIT = 0, (40, 41), 9, 18, 27, 36, 45, 54, 63, 72
same_bits = rc.same_bits


def params(radius, rank, **kw):
    return dict(dict(radius=radius, rank=rank, min_neighbours=MIN_NEIGHBOURS[radius], scale=2.0, floor=0.0,
                     normal_cosine=0.9), **kw)


def params_object(pt, p):
    return pt.DespikeParameters(p["radius"], p["rank"], p["min_neighbours"], p["scale"], p["floor"], p["normal_cosine"])


def blocks(W, H):
    """(the block of zeros, its positive pixel, the block of constant colour)."""
    ys, xs = np.mgrid[0:H, 0:W]
    low = (ys >= H // 2) & (H >= 16)
    zeros = low & (xs < W // 3)
    constant = low & (xs >= W // 3) & (xs < 2 * (W // 3))
    inside = zeros & (ys == (H // 2 + H) // 2) & (xs == W // 6)
    return zeros, inside, constant


CONSTANT = F(0.5)


def perturb(case):
    p = case["params"]
    g, src = case["guides"].copy(), case["src"].copy()
    H, W = g.shape
    ys, xs = np.mgrid[0:H, 0:W]
    k = (xs + 5 * ys) % MODULUS
    hit = g["shape"] != NONE
    src[(k == SPIKE) | (k == PAIR[0]) | (k == PAIR[1]), :3] *= F(50.0)
    src[k == EMPTY] = 0
    src[k == NAN, 1] = np.nan
    src[k == INF, 0] = np.inf
    src[k == DENORMAL, 3] = 1e-42                                   # a denormal count: the colour overflows
    g["shape"][(k == FLIP) & hit] += 1                              # another shape
    g["shape"][(k == FLIP) & ~hit] = 0                              # the sky becomes a shape
    angle = float(np.arccos(p["normal_cosine"]))
    g["normal"][(k == TILT_IN) & hit] = rc._tilt(g["normal"][(k == TILT_IN) & hit], 0.98 * angle)
    g["normal"][(k == TILT_OUT) & hit] = rc._tilt(g["normal"][(k == TILT_OUT) & hit], 1.02 * angle)
    zeros, inside, constant = blocks(W, H)
    for block in (zeros, constant):
        g["shape"][block] = 0
        g["normal"][block] = (0.0, 0.0, 1.0)
        src[block, 3] = 2.0
    src[zeros, :3] = np.where((xs + ys)[zeros][:, None] % 2 == 0, F(0.0), F(-0.0))
    src[zeros & (xs % 3 == 0), 1] = F(0.0)                          # zeros of both signs within a pixel
    src[inside, :3] = (0.25, 0.5, 0.125)
    src[constant, :3] = CONSTANT * F(2.0)
    # A pixel is not in its own window, so its limit does not move with it,
    # and no other pixel placed here lies in that window.
    _, d = xd.despike(src, g, detail=True, **p)
    with np.errstate(all="ignore"):
        sel = (k == ON_LIMIT) & ~zeros & ~constant & np.isfinite(d["L"]) & (d["L"] > 0) & (d["m"] >= p["min_neighbours"])
        above = sel & (xs >= (W + 1) // 2 + 4)
        on = sel & (xs < (W + 1) // 2 - 4)
    for where, values in ((on, d["L"]), (above, np.nextafter(d["L"], F(np.inf)))):
        src[where, 0] = values[where]
        src[where, 1] = values[where] * F(0.5)
        src[where, 2] = values[where] * F(0.25)
        src[where, 3] = 1.0                                         # the colour is the stored value
    return dict(case, guides=g, src=src)


def _case(guides, radius, rank, seed, **kw):
    H, W = guides.shape
    return dict(guides=guides, src=rc.current(W, H, seed), params=params(radius, rank, **kw))


@functools.lru_cache(maxsize=None)
def _synthetic():
    out = {}
    for i, (W, H) in enumerate(SIZES):
        for R in (1, 2, 3):
            out[f"{W}x{H}-r{R}"] = perturb(_case(rc.synthetic_guides(W, H), R, (3 * i + R - 1) % 4 + 1, 10 * i + R))
    one = _case(rc.synthetic_guides(1, 1), 1, 1, 70, min_neighbours=1)
    one["guides"]["shape"][0, 0] = 0
    out["1x1-rank1-min1"] = one
    out["33x18-r2-min24"] = perturb(_case(rc.synthetic_guides(33, 18), 2, 3, 71, min_neighbours=24))
    out["17x16-r2-scale0"] = perturb(_case(rc.synthetic_guides(17, 16), 2, 2, 72, scale=0.0))
    out["16x16-r1-floor"] = perturb(_case(rc.synthetic_guides(16, 16), 1, 3, 73, scale=1.0, floor=0.3))
    return out


@functools.lru_cache(maxsize=None)
def _coherent():
    pt = sys.modules["path_tracer_amd"]       # loaded by tests/conftest.py
    out = {}
    for name, config, (W, H), radius, rank in (("config2", 2, (64, 64), 3, 3), ("config5", 5, (64, 32), 2, 2)):
        scene = pt.Scene.config(config)
        scene.pack()
        out[name] = perturb(_case(dr.guides(scene, 0, W, H), radius, rank, 80 + config))
        scene.close()
    return out


COVERAGE = ("clamped", "unclamped", "untested", "not_usable", "shape_cut", "normal_cut", "t_inf", "zero_clamp",
            "floor_deciding", "on_limit", "ulp_above")


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (case, the restatement's result)}.  Asserted over the set, from
    the restatement's detail: a clamped pixel and a tested one that is not; an
    untested one (m < MinNeighbours); a centre that is not usable; a tested
    window cut by a shape edge and one cut by a normal edge; t = +inf; t a
    zero with the centre clamped to 0; a pixel above Scale * t that Floor
    keeps; a tested centre exactly on L (kept) and one an ulp above (clamped).
    Every coherent case clamps between 1 % and 25 % of its pixels and leaves
    at least half untouched."""
    out, seen = {}, {c: 0 for c in COVERAGE}
    for kind, cases in (("synthetic", _synthetic()), ("coherent", _coherent())):
        for name, case in cases.items():
            ref, d = xd.despike(case["src"], case["guides"], detail=True, **case["params"])
            out[name] = (case, ref)
            with np.errstate(all="ignore"):
                d["on_limit"] = d["unclamped"] & (d["v"] == d["L"]) & (d["L"] > 0)
                d["ulp_above"] = d["clamped"] & (d["v"] == np.nextafter(d["L"], F(np.inf)))
            for c in COVERAGE:
                seen[c] += int(d[c].sum())
            if kind == "coherent":
                untouched = same_bits(ref, case["src"]).all(axis=-1)
                assert 0.01 <= d["clamped"].mean() <= 0.25 and untouched.mean() >= 0.5, (name, d["clamped"].mean())
    assert all(seen.values()), seen
    return out


def names():
    return ([f"{W}x{H}-r{R}" for W, H in SIZES for R in (1, 2, 3)] +
            ["1x1-rank1-min1", "33x18-r2-min24", "17x16-r2-scale0", "16x16-r1-floor", "config2", "config5"])
