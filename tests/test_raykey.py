"""The ray key of the traversal-length table (include/pt_raykey.h) through the
host library's ptsRayKey: an 8^3 cell of the origin over the world bounds
times an 8 x 8 octahedral bin of the direction.  Checked against a restatement
in numpy binary32, at the places where such a key goes wrong: origins on and
outside the bounds, signed zeros, every bin edge, a flat scene, non-finite
input."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

f32 = np.float32
LO, HI = (-2.0, 0.5, -1.0), (6.0, 4.5, 1.0)   # extents 8, 4, 2: binary32-exact scales 1, 2, 4


def key(pt, o, v, lo=LO, hi=HI):
    N = pt._native
    a = [np.asarray(x, dtype=np.float32).copy() for x in (o, v, lo, hi)]
    return int(N.scene_lib().ptsRayKey(*(N.fptr(x) for x in a)))


def to_bin(x, n=8):
    x = x if x >= 0 else f32(0)          # NaN compares false
    x = x if x <= f32(n - 1) else f32(n - 1)
    return int(x)


def key_ref(o, v, lo=LO, hi=HI):
    """pt_ray_key restated: the same binary32 operations in the same order."""
    with np.errstate(all="ignore"):
        o, v, lo, hi = (np.asarray(x, dtype=f32) for x in (o, v, lo, hi))
        c = []
        for k in range(3):
            e = hi[k] - lo[k]
            ok = e > 0 and e < f32(1e30) and lo[k] > f32(-1e30)
            scale = f32(8) / e if ok else f32(0)
            base = lo[k] if f32(-1e30) < lo[k] < f32(1e30) else f32(0)
            c.append(to_bin((o[k] - base) * scale))
        inv = f32(1) / (abs(v[0]) + abs(v[1]) + abs(v[2]))
        u, w = v[0] * inv, v[1] * inv
        if v[2] < 0:
            u, w = ((f32(1) - abs(w)) * (f32(-1) if v[0] < 0 else f32(1)),
                    (f32(1) - abs(u)) * (f32(-1) if v[1] < 0 else f32(1)))
        bu, bv = to_bin(u * f32(4) + f32(4)), to_bin(w * f32(4) + f32(4))
    return (((c[2] * 8 + c[1]) * 8 + c[0]) * 8 + bv) * 8 + bu


def split(k):
    return {"cx": (k >> 6) & 7, "cy": (k >> 9) & 7, "cz": (k >> 12) & 7, "bu": k & 7, "bv": (k >> 3) & 7}


def test_cells_on_and_outside_the_bounds(pt):
    v = (0.3, -0.2, 0.9)
    # lower bound: cell 0; upper bound: 8 clamped to 7; every interior cell edge belongs to the upper cell
    for k, name in enumerate(("cx", "cy", "cz")):
        e = HI[k] - LO[k]
        for i in range(9):
            o = [0.5 * (LO[j] + HI[j]) for j in range(3)]
            o[k] = LO[k] + e * i / 8          # exact in binary32 for these bounds
            got = split(key(pt, o, v))
            assert got[name] == min(i, 7), (name, i)
            assert key(pt, o, v) == key_ref(o, v)
        for far, cell in ((-1e3, 0), (1e3, 7), (-3e38, 0), (3e38, 7), (-np.inf, 0), (np.inf, 7), (np.nan, 0)):
            o = [0.5 * (LO[j] + HI[j]) for j in range(3)]
            o[k] = far
            assert split(key(pt, o, v))[name] == cell, (name, far)
    assert split(key(pt, (2.0, 2.5, 0.0), v)) | {"bu": 0, "bv": 0} == {"cx": 4, "cy": 4, "cz": 4, "bu": 0, "bv": 0}


def test_signed_zero_direction_components(pt):
    o = (1.0, 1.0, 0.0)
    for x, y, z in itertools.product((0.0, 0.6, -0.6), repeat=3):
        if x == y == z == 0.0:
            continue
        base = key(pt, o, (x, y, z))
        for sx, sy, sz in itertools.product((1.0, -1.0), repeat=3):
            flipped = tuple(np.copysign(c, s) if c == 0.0 else c for c, s in ((x, sx), (y, sy), (z, sz)))
            assert key(pt, o, flipped) == base, (x, y, z, flipped)
        assert base == key_ref(o, (x, y, z))
    # the six axes land in six different bins
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    assert len({key(pt, o, a) & 63 for a in axes}) == 6
    # the zero vector and non-finite directions still give a key in range
    for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 1, 0), (1, -np.inf, np.nan)):
        assert 0 <= key(pt, o, bad) < 32768


def test_every_octahedral_bin_edge(pt):
    """Directions exactly on the bin edges u, v = k/4 - 1 of both hemispheres
    (|x| + |y| + |z| = 1 exactly, so the normalisation is exact): an edge
    belongs to the upper bin, the last edge to bin 7."""
    o = (1.0, 1.0, 0.0)
    for i, j in itertools.product(range(9), repeat=2):
        u, v = i / 4 - 1, j / 4 - 1
        if abs(u) + abs(v) <= 1:
            d = (u, v, 1 - abs(u) - abs(v))
            got = split(key(pt, o, d))
            if d[2] > 0:   # on the fold line z = 0 the upper formula applies
                assert (got["bu"], got["bv"]) == (min(i, 7), min(j, 7)), (i, j)
            assert key(pt, o, d) == key_ref(o, d)
        else:
            # lower hemisphere: the direction whose folded coordinates are (u, v)
            sx, sy = (1 if u >= 0 else -1), (1 if v >= 0 else -1)
            x, y = (1 - abs(v)) * sx, (1 - abs(u)) * sy
            d = (x, y, -(1 - abs(x) - abs(y)))
            got = split(key(pt, o, d))
            if abs(u) < 1 and abs(v) < 1:   # on the map's border x or y is a zero, whose sign the fold does not read
                assert (got["bu"], got["bv"]) == (min(i, 7), min(j, 7)), (i, j)
            assert key(pt, o, d) == key_ref(o, d)


def test_flat_and_unbounded_scenes(pt):
    v = (0.1, 0.2, -0.97)
    flat_lo, flat_hi = (-1.0, -1.0, 0.25), (1.0, 1.0, 0.25)     # a scene in the plane z = 0.25
    for z in (-5.0, 0.25, 7.0, np.inf, np.nan):
        got = split(key(pt, (0.5, -0.5, z), v, flat_lo, flat_hi))
        assert (got["cx"], got["cy"], got["cz"]) == (6, 2, 0), z
    # a point scene, inverted bounds, and an infinite plane's bounds: one cell on those axes
    for lo, hi in (((1, 1, 1), (1, 1, 1)), ((2, 2, 2), (1, 1, 1)), ((-1e30, -1e30, 0), (1e30, 1e30, 0)),
                   ((-np.inf, 0, 0), (np.inf, 1, 1)), ((np.nan, 0, 0), (np.nan, 1, 1))):
        k = key(pt, (0.3, 0.6, 0.9), v, lo, hi)
        assert split(k)["cx"] == 0 and 0 <= k < 32768, (lo, hi)
        assert k == key_ref((0.3, 0.6, 0.9), v, lo, hi)


def test_random_rays_match_the_restatement(pt):
    rng = np.random.default_rng(11)
    n = 4000
    o = rng.uniform(-4.0, 8.0, size=(n, 3)).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32)
    d[::7, rng.integers(0, 3)] = 0.0
    seen = set()
    for i in range(n):
        k = key(pt, o[i], d[i])
        assert k == key_ref(o[i], d[i]), i
        seen.add(k)
    assert max(seen) < 32768 and len(seen) > n // 4
    assert key(pt, o[0], d[0]) == key(pt, o[0], d[0] * f32(3.0))   # the length of the direction does not matter


def test_null_arguments(pt):
    N = pt._native
    a = np.zeros(3, dtype=np.float32)
    assert N.scene_lib().ptsRayKey(None, N.fptr(a), N.fptr(a), N.fptr(a)) == 0xFFFFFFFF
