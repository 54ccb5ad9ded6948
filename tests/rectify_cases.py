"""Inputs shared by the history-validation tests (tests/test_rectify.py on the
CPU, tests/test_gpu_rectify.py on the device).

Synthetic cases, sizes 1x1, 5x3 (smaller than every window), 16x16, 17x16,
33x18 (windows cross tile borders in both directions) and 67x45, each with
Radius 1, 2 and 3: guide records of a sky band, a flat shape and a round one
whose normal turns from pixel to pixel, a noisy two-sample accumulator Cur, and
a history Hist that is the smoothed Cur on the left of the frame and far too
bright or too dark on the right.  One perturbation per pixel, chosen by
(x + 5 y) mod 12: Cur empty, NaN, infinite or with a denormal .w; Hist empty or
NaN; the shape flipped; the normal tilted just inside and just outside
NormalCosine; Hist exactly on lo, exactly on hi, and one ulp outside each (with
n = 1, so that the mean is the stored value).  A block of exactly constant Cur
(sigma = 0) with a history on and off that value lies in the lower left.
Extreme parameters on some of the sizes: MinNeighbours 1 and 49, Sigma 0,
ClampedHistory inf.

Coherent cases: real guides of config 1 and config 5 at 64x32
(denoise_restatement.guides) under the same Cur and Hist recipe, unperturbed.

all_cases() computes the restatement once per case and asserts the coverage
the tests rely on (listed there)."""
from __future__ import annotations

import functools
import sys

import numpy as np

import denoise_restatement as dr
import rectify_restatement as xr

F = np.float32
NONE = 0xFFFFFFFF
SIZES = ((1, 1), (5, 3), (16, 16), (17, 16), (33, 18), (67, 45))
MIN_NEIGHBOURS = {1: 3, 2: 6, 3: 9}


def params(radius, **kw):
    return dict(dict(xr.DEFAULTS, radius=radius, min_neighbours=MIN_NEIGHBOURS[radius]), **kw)


def params_object(pt, p):
    return pt.RectifyParameters(p["radius"], p["min_neighbours"], p["sigma"], p["clamped_history"], p["normal_cosine"])


def synthetic_guides(W, H):
    g = np.zeros((H, W), dr.GUIDE_DTYPE)
    ys, xs = np.mgrid[0:H, 0:W]
    g["shape"] = 0
    g["normal"] = (0.0, 0.0, 1.0)
    g["time"] = 4.0
    g["albedo"] = 0.5
    # A round shape on the right: the normal turns by a few degrees per pixel.
    cx, cy, r = 0.7 * W, 0.55 * H, max(0.3 * min(W, H), 1.0)
    u, v = (xs - cx) / (2.5 * r), (ys - cy) / (2.5 * r)
    disc = u * u + v * v < 0.16
    n = np.stack([u, v, np.sqrt(np.maximum(1.0 - u * u - v * v, 0.0))], axis=-1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    g["shape"][disc] = 1
    g["normal"][disc] = n[disc].astype(F)
    sky = ys < H // 5
    g["shape"][sky] = NONE
    g["normal"][sky] = 0
    g["time"][sky] = 0
    return g


def current(W, H, seed):
    """Two samples a pixel of a smooth image plus noise."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    base = 0.6 + 0.3 * np.sin(0.3 * xs)[..., None] + 0.2 * np.cos(0.2 * ys)[..., None] + np.array([0.0, 0.1, 0.2])
    mean = (base * rng.uniform(0.6, 1.4, size=(H, W, 3))).astype(F)
    a = np.zeros((H, W, 4), F)
    a[..., :3] = mean * F(2.0)
    a[..., 3] = 2.0
    return a


def history(cur, seed):
    """The 3x3 box mean of Cur's colours with counts in 1..64 on the left 60 %
    of the frame; three times too bright, or five times too dark, on the rest."""
    rng = np.random.default_rng(seed)
    H, W = cur.shape[:2]
    c = (cur[..., :3] / cur[..., 3:4]).astype(np.float64)
    p = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    smooth = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    ys, xs = np.mgrid[0:H, 0:W]
    off = xs >= 0.6 * W
    smooth[off & (ys % 2 == 0)] *= 3.0
    smooth[off & (ys % 2 == 1)] *= 0.2
    n = rng.integers(1, 65, size=(H, W)).astype(F)
    a = np.zeros((H, W, 4), F)
    a[..., :3] = smooth.astype(F) * n[..., None]
    a[..., 3] = n
    return a


def _tilt(n, angle):
    """Unit normals n (.., 3) turned by `angle` about an axis at right angles."""
    n = n.astype(np.float64)
    a = np.where(np.abs(n[..., :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(n, a)
    t /= np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-30)
    return (np.cos(angle) * n + np.sin(angle) * t).astype(F)


CONSTANT = F(0.5)


def perturb(case):
    """One perturbation per pixel, chosen by (x + 5 y) mod 12; then the block
    of constant Cur; then the histories placed on the box's bounds, which
    depend on everything before."""
    p = case["params"]
    g, cur, hist = case["guides"].copy(), case["cur"].copy(), case["hist"].copy()
    H, W = g.shape
    ys, xs = np.mgrid[0:H, 0:W]
    k = (xs + 5 * ys) % 12
    hit = g["shape"] != NONE
    cur[k == 0] = 0                                                   # Cur empty
    cur[k == 1, 1] = np.nan
    cur[(k == 2) & (xs % 2 == 0), 0] = np.inf
    cur[(k == 2) & (xs % 2 == 1), 3] = 1e-42                          # a denormal count: the colour overflows
    hist[k == 3] = 0                                                  # Hist empty
    hist[k == 4, 2] = np.nan
    g["shape"][(k == 5) & hit] += 1                                   # another shape
    g["shape"][(k == 5) & ~hit] = 0                                   # the sky becomes a shape
    angle = float(np.arccos(p["normal_cosine"]))
    g["normal"][(k == 6) & hit] = _tilt(g["normal"][(k == 6) & hit], 0.98 * angle)   # just inside NormalCosine
    g["normal"][(k == 7) & hit] = _tilt(g["normal"][(k == 7) & hit], 1.02 * angle)   # just outside
    block = (ys >= H // 2) & (xs < W // 3) & (H >= 16)
    cur[block, :3] = CONSTANT * F(2.0)
    cur[block, 3] = 2.0
    g["shape"][block] = 0
    g["normal"][block] = (0.0, 0.0, 1.0)
    hist[block, :3] = CONSTANT * F(64.0)                              # on the value: h' == h
    hist[block, 3] = 64.0
    hist[block & (xs % 3 == 1), :3] = F(0.75) * F(64.0)              # off it: clipped to the value, n cut to 8
    _, d = xr.rectify(hist, cur, g, detail=True, **p)
    finite = np.isfinite(d["lo"]).all(axis=-1) & np.isfinite(d["hi"]).all(axis=-1) & ~block
    for code, values in ((8, d["lo"]), (9, d["hi"]),
                         (10, np.nextafter(d["lo"], F(-np.inf))), (11, np.nextafter(d["hi"], F(np.inf)))):
        sel = (k == code) & finite
        hist[sel, :3] = values[sel] if code < 10 else d["mu"][sel]
        if code >= 10:
            hist[sel, 0] = values[sel][:, 0]                          # one ulp outside in one channel
        hist[sel, 3] = 1.0
    return dict(case, guides=g, cur=cur, hist=hist)


def _case(guides, radius, seed, **kw):
    H, W = guides.shape
    cur = current(W, H, seed)
    return dict(guides=guides, cur=cur, hist=history(cur, seed + 1000), params=params(radius, **kw))


@functools.lru_cache(maxsize=None)
def _synthetic():
    out = {}
    for i, (W, H) in enumerate(SIZES):
        for R in (1, 2, 3):
            out[f"{W}x{H}-r{R}"] = perturb(_case(synthetic_guides(W, H), R, 10 * i + R))
    one = _case(synthetic_guides(1, 1), 1, 70, min_neighbours=1)
    one["guides"]["shape"][0, 0] = 0
    out["1x1-min1"] = one
    out["17x16-r2-sigma0"] = perturb(_case(synthetic_guides(17, 16), 2, 71, sigma=0.0))
    out["33x18-r3-min49-clamp-inf"] = perturb(_case(synthetic_guides(33, 18), 3, 72, min_neighbours=49,
                                                    clamped_history=float("inf")))
    out["16x16-r1-min1"] = perturb(_case(synthetic_guides(16, 16), 1, 73, min_neighbours=1))
    return out


@functools.lru_cache(maxsize=None)
def _coherent():
    pt = sys.modules["path_tracer_amd"]       # loaded by tests/conftest.py
    out = {}
    for name, config, radius in (("config1", 1, 3), ("config5", 5, 2)):
        scene = pt.Scene.config(config)
        scene.pack()
        out[name] = _case(dr.guides(scene, 0, 64, 32), radius, 80 + config)
        scene.close()
    return out


COVERAGE = ("untested", "low", "high", "unclipped", "no_history", "centre_through_neighbours", "shape_cut",
            "normal_cut", "count_cut", "count_kept", "unstable")


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (case, the restatement's result)}.  Asserted over the set: some
    pixel with m < MinNeighbours; one clipped low, one clipped high, one
    unclipped; one without a usable history; a centre whose own Cur is
    unusable and which is tested through its neighbours; a tested window cut
    by a shape edge and one cut by a normal edge; a clipped pixel whose count
    ClampedHistory cuts and one whose count is already below it; a non-finite
    moment.  Every coherent case both clips and keeps at least 10 % of its
    pixels."""
    out, seen = {}, {c: 0 for c in COVERAGE}
    for kind, cases in (("synthetic", _synthetic()), ("coherent", _coherent())):
        for name, case in cases.items():
            ref, d = xr.rectify(case["hist"], case["cur"], case["guides"], detail=True, **case["params"])
            out[name] = (case, ref)
            for c in COVERAGE:
                seen[c] += int(d[c].sum())
            if kind == "coherent":
                assert d["clipped"].mean() >= 0.1 and d["unclipped"].mean() >= 0.1, (name, d["clipped"].mean())
    assert all(seen.values()), seen
    return out


def names():
    return ([f"{W}x{H}-r{R}" for W, H in SIZES for R in (1, 2, 3)] +
            ["1x1-min1", "17x16-r2-sigma0", "33x18-r3-min49-clamp-inf", "16x16-r1-min1", "config1", "config5"])


def same_bits(a, b):
    """Elementwise: equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
