"""Case sets and the host reference of the traversal's slab test
(test_slab_cases.py on the host, test_gpu_slab_domain.py against ptEvalSlabTest).

The device evaluates a box test's six quotients (Min - O) / V with an
FMA-corrected reciprocal that has no guard of its own (pt_device.hpp FastQuot)
whenever the ray and the scene lie inside the domain DESIGN.md §2 writes down:

    every box coordinate and ray-origin component is 0 or has magnitude in
    [2^-50, 2^40], every ray-velocity component has magnitude in [2^-59, 2^27]

and divides otherwise.  A case is one ray (origin, velocity, reach) and one
box; the classes below put the operands where that argument is tightest and
where the gates must refuse.  Everything is numpy and seeded; nothing here
reads the device code.
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
F64 = np.float64
INF = F32(1e30)                    # PT_INFINITY: a miss
HIT_TIME_LIMIT = F32(1048576.0)    # PT_HIT_TIME_LIMIT
COORD_E = (-50, 40)                # coordinates: 0 or 2^-50 <= |c| <= 2^40
VEL_E = (-59, 27)                  # velocities:       2^-59 <= |v| <= 2^27

SIZES = {"bulk": 1 << 19, "edges": 1 << 19, "near": 1 << 18, "outside": 1 << 18, "reach": 1 << 18}
CLASSES = tuple(SIZES)
IN_DOMAIN = ("bulk", "edges", "near")       # classes built to hit (the share of finite entry times is asserted)
BOTH_FLAGS = ("edges", "near", "outside")   # classes that hold rays on both sides of the ray gate

# Operand pairs outside the domain whose unguarded quotient is not the IEEE
# one: (a, b, bits of RN(a / b)).  a * RN(1/b) or RN(1/b) itself overflows, so
# the correction adds infinities of opposite sign and gives NaN.  Each is a
# case with Min.x = a, O = 0, V.x = b (the first cases of "outside").
KNOWN_ANSWERS = (
    (float.fromhex("-0x1.000002p+58"), float.fromhex("0x1.954b1cp-88"), 0xFF800000),   # -inf
    (float.fromhex("0x1p+40"), float.fromhex("-0x1.2p-90"), 0xFF800000),               # -inf
    (float.fromhex("0x1.234568p-30"), float.fromhex("0x1p-128"), 0x7091A2B4),          # 0x1.234568p+98
    (float.fromhex("-0x1.fffffep+39"), float.fromhex("0x1.000002p-89"), 0xFF800000),   # -inf
    (float.fromhex("0x1.4p+10"), float.fromhex("0x1.8p-129"), 0x7F800000),             # +inf
)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(F32)


# --- the reference ---------------------------------------------------------------

def _fmin(a, b):
    """fminf with -0 ordered below +0 (the order v_min_f32 and the host's pt_min keep)."""
    pick_a = (a < b) | ((a == b) & np.signbit(a))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(pick_a, a, b)))


def _fmax(a, b):
    pick_a = (a > b) | ((a == b) & ~np.signbit(a))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(pick_a, a, b)))


def reference(o, v, reach, lo, hi, division="ieee"):
    """IntersectBoundingBox (common.glsl.inc:153-185) over n cases in float32:
    IEEE division (or, for "rcp", the product with the rounded reciprocal) and
    GLSL min / max, which drop a NaN operand.  The vector form of ieee_slab in
    test_slab_convention.py.  Returns the entry times, INF for a miss."""
    o, v, lo, hi = (np.asarray(x, dtype=F32) for x in (o, v, lo, hi))
    reach = np.asarray(reach, dtype=F32)
    with np.errstate(all="ignore"):
        if division == "ieee":
            a, b = (lo - o) / v, (hi - o) / v
        else:
            y = F32(1.0) / v
            a, b = (lo - o) * y, (hi - o) * y
        assert a.dtype == F32 and b.dtype == F32
        early, late = _fmin(a, b), _fmax(a, b)
        e = _fmax(_fmax(early[:, 0], early[:, 1]), early[:, 2])
        x = _fmin(_fmin(late[:, 0], late[:, 1]), late[:, 2])
        miss = (x < e) | (x <= 0) | (e >= reach)
    return np.where(miss, INF, e).astype(F32)


def _in_range(x, e):
    m = np.abs(np.asarray(x, dtype=F64))
    return (m >= 2.0 ** e[0]) & (m <= 2.0 ** e[1])


def expected_flag(o, v):
    """The ray's side of the domain, from DESIGN.md §2's statement of it."""
    o, v = np.asarray(o, dtype=F32), np.asarray(v, dtype=F32)
    return ((o == 0) | _in_range(o, COORD_E)).all(axis=1) & _in_range(v, VEL_E).all(axis=1)


def boxes_in_range(lo, hi):
    """The scene's side: what an upload of these boxes would set the gate to."""
    c = np.concatenate([np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)], axis=1)
    return ((c == 0) | _in_range(c, COORD_E)).all(axis=1)


# --- values --------------------------------------------------------------------------

def _values(rng, shape, e, zeros=0.0):
    """+-m 2^k: m a random 24-bit significand in [1, 2), k uniform over [e[0], e[1])."""
    m = 1.0 + rng.integers(0, 1 << 23, shape) / float(1 << 23)
    x = np.ldexp(m, rng.integers(e[0], e[1], shape)) * rng.choice([-1.0, 1.0], shape)
    if zeros:
        x[rng.random(shape) < zeros] = 0.0
    return x.astype(F32)


def _edge_values(rng, shape, e, which=None):
    """Around the bounds 2^e[0] and 2^e[1] (which: 0 or 1 for one of them): exponent fields within two of the
    bound with significand 1.0, all ones or random; a quarter are the bound
    itself and the floats one ulp inside and outside it."""
    bound = np.where(rng.random(shape) < 0.5, e[0], e[1]) if which is None else np.full(shape, e[which])
    kind = rng.integers(0, 3, shape)
    frac = np.where(kind == 0, 0, np.where(kind == 1, (1 << 23) - 1, rng.integers(0, 1 << 23, shape)))
    x = np.ldexp(1.0 + frac / float(1 << 23), bound + rng.integers(-2, 3, shape)).astype(F32)
    at = (bits(np.ldexp(1.0, bound)).astype(np.int64) + rng.integers(-1, 2, shape)).astype(np.uint32)
    x = np.where(rng.random(shape) < 0.25, from_bits(at).reshape(x.shape), x)
    return (x * rng.choice([-1.0, 1.0], shape)).astype(F32)


def _mixed(rng, shape, e, zeros=0.0, edge_share=0.5):
    return np.where(rng.random(shape) < edge_share, _edge_values(rng, shape, e), _values(rng, shape, e, zeros))


def _step(x, k):
    """x moved by k ulps (k in -2..2, towards +inf for k > 0)."""
    x = np.asarray(x, dtype=F32).copy()
    for j in range(2):
        up, down = k > j, k < -j
        x = np.where(up, np.nextafter(x, F32(np.inf)), np.where(down, np.nextafter(x, F32(-np.inf)), x))
    return x.astype(F32)


def _coordinate(x):
    """A derived coordinate brought into {0} U [2^-50, 2^40] (NaN stays)."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(x, dtype=F64)
        m = np.abs(x)
        x = np.where((m > 0) & (m < 2.0 ** COORD_E[0]), 0.0, x)
        x = np.where(m > 2.0 ** COORD_E[1], np.copysign(2.0 ** COORD_E[1], x), x)
    return x.astype(F32)


def _width(rng, scale):
    """scale * 2^-u, u in 1..20 (at least four ulps of scale); 2^-50..2^-10 where scale is 0 or not finite."""
    scale = np.abs(np.asarray(scale, dtype=F64))
    w = scale * np.ldexp(1.0, -rng.integers(1, 21, scale.shape))
    free = np.ldexp(1.0 + rng.random(scale.shape), rng.integers(-50, -10, scale.shape))
    return np.where(np.isfinite(scale) & (scale > 0), w, free)


# --- assembling a case -------------------------------------------------------------------

def _assemble(rng, o_pick, lo_pick, v, from_box):
    """A box around the point O + t V of each ray, t > 0, so that hits are
    common.  Per component either the origin is the picked value and the box
    is laid around the ray's point (from_box False), or the box minimum is the
    picked value and the origin is laid so that the ray passes the box at t
    (from_box True).  Derived values are brought into the coordinate range.
    Returns o, lo, hi (float32 (n, 3)) and t (float64 (n,))."""
    n = len(v)
    with np.errstate(all="ignore"):
        vmax = np.abs(v.astype(F64)).max(axis=1)
        emax = np.where(np.isfinite(vmax) & (vmax > 0), np.frexp(vmax)[1], 0)
        t = np.ldexp(1.0 + rng.random(n), 37 - emax - rng.integers(0, 40, n))    # t |V| < 2^39
        tv = t[:, None] * v.astype(F64)
        tv = np.where(np.isfinite(tv), tv, 0.0)
        # the origin picked
        at = (o_pick.astype(F64) + tv).astype(F32)
        lo_a = _coordinate(at.astype(F64) - _width(rng, at))
        hi_a = _coordinate(at.astype(F64) + _width(rng, at))
        # the box minimum picked
        w = _width(rng, np.abs(lo_pick.astype(F64)) + np.abs(tv))
        hi_b = _coordinate(lo_pick.astype(F64) + w)
        o_b = _coordinate(lo_pick.astype(F64) + 0.5 * w - tv)
    o = np.where(from_box, o_b, o_pick).astype(F32)
    lo = np.where(from_box, lo_pick, lo_a).astype(F32)
    hi = np.where(from_box, hi_b, hi_a).astype(F32)
    return o, lo, hi, t


def _reaches(rng, t):
    """PT_INFINITY, PT_HIT_TIME_LIMIT or four times the ray's time at the box."""
    sel = rng.integers(0, 4, len(t))
    with np.errstate(over="ignore"):
        r = np.where(sel == 1, F64(HIT_TIME_LIMIT), np.where(sel == 2, 4.0 * t, F64(INF)))
    return np.minimum(r, F64(INF)).astype(F32)


def _pack(o, v, reach, lo, hi):
    out = {"o": o, "v": v, "reach": reach, "lo": lo, "hi": hi}
    n = len(reach)
    for k, a in out.items():
        assert a.dtype == F32 and a.shape == ((n,) if k == "reach" else (n, 3)), k
        a.setflags(write=False)
    return out


def _bulk(rng, n, edge_share=0.0, with_time=False):
    o_pick = _mixed(rng, (n, 3), COORD_E, 1 / 16, edge_share)
    lo_pick = _mixed(rng, (n, 3), COORD_E, 1 / 16, edge_share)
    v = _mixed(rng, (n, 3), VEL_E, 0.0, edge_share)
    o, lo, hi, t = _assemble(rng, o_pick, lo_pick, v, rng.random((n, 3)) < 0.3)
    return (o, v, _reaches(rng, t), lo, hi) + ((t,) if with_time else ())


def _near(rng, n):
    """The origin within +-2 ulps of a box plane on one axis (on it for 0): the
    smallest nonzero numerators, down to 2^-73 beside a plane at 2^-50.  In
    half of the cases the box holds the origin on the other two axes, so the
    near plane's quotient is the entry time itself."""
    o, v, reach, lo, hi, t = _bulk(rng, n, with_time=True)
    i = np.arange(n)
    c = rng.integers(0, 3, n)
    upper = rng.random(n) < 0.5                 # the near plane is the box maximum
    k = rng.integers(-2, 3, n)
    inside = rng.random(n) < 0.5
    other = inside[:, None] & (np.arange(3)[None, :] != c[:, None])
    lo[other] = _coordinate(o.astype(F64) - _width(rng, o))[other]
    hi[other] = _coordinate(o.astype(F64) + _width(rng, o))[other]
    plane = _mixed(rng, n, COORD_E, 1 / 16, 0.25)
    oc = _step(plane, k)
    enter = np.where(upper, -1.0, 1.0) * np.where(rng.random(n) < 0.125, -1.0, 1.0)
    vc = (np.abs(_mixed(rng, n, VEL_E, 0.0, 0.25)) * enter).astype(F32)      # 2^-73 / 2^27 = 2^-100 among them
    with np.errstate(all="ignore"):
        w = np.where(inside, _width(rng, plane), 2.0 * t * np.abs(vc.astype(F64)))
    far = _coordinate(plane.astype(F64) + np.where(upper, -w, w))
    o[i, c], v[i, c] = oc, vc
    lo[i, c] = np.where(upper, far, plane)
    hi[i, c] = np.where(upper, plane, far)
    return o, v, reach, lo, hi


def _extremes(rng, n):
    """The largest quotients of the domain, about 2^41 / 2^-59 = 2^100 on
    either side of PT_INFINITY.  On every axis the origin sits at one end of
    the coordinate range and moves towards the other at a velocity near 2^-59;
    the box spans the range on two axes (exit times near 2^100) and begins
    near the far end on the third, whose near plane gives the entry time."""
    top = F32(2.0 ** COORD_E[1])
    s = rng.choice([-1.0, 1.0], (n, 3)).astype(F32)
    ev = np.abs(_edge_values(rng, (n, 3), VEL_E, 0))
    e1, e2 = np.abs(_edge_values(rng, (n, 3), COORD_E, 1)), np.abs(_edge_values(rng, n, COORD_E, 1))
    keep = rng.random(n) < 0.75                             # three quarters stay inside the domain
    ev = np.where(keep[:, None], np.maximum(ev, F32(2.0 ** VEL_E[0])), ev)
    e1, e2 = np.where(keep[:, None], np.minimum(e1, top), e1), np.where(keep, np.minimum(e2, top), e2)
    o, v = (-s * e1).astype(F32), (s * ev).astype(F32)
    lo, hi = np.full((n, 3), -top, F32), np.full((n, 3), top, F32)
    i, c = np.arange(n), rng.integers(0, 3, n)
    far = np.maximum(e2, top)
    lo[i, c] = np.where(s[i, c] > 0, e2, -far)
    hi[i, c] = np.where(s[i, c] > 0, far, -e2)
    return o, v, np.full(n, INF, F32), lo, hi


def _edges(rng, n):
    a, b = _bulk(rng, n - n // 8, 0.5), _extremes(rng, n // 8)
    return tuple(np.concatenate([x, y]).astype(F32) for x, y in zip(a, b))


_DENORMALS = [0x00000001, 0x007FFFFF, 0x00012345, 0x00400000]
SPECIALS = from_bits(np.array(
    [s | u for u in _DENORMALS + [0x00800000, 0x0D800000, 0x71800000, 0x7F800000, 0x00000000] for s in (0, 0x80000000)]
    + [0x7FC00000], dtype=np.uint32))           # denormals, 2^-126, 2^-100, 2^100, inf, 0 (both signs), NaN


def _outside(rng, n):
    parts = []
    # the known-answer pairs
    m = len(KNOWN_ANSWERS)
    o = np.zeros((m, 3), F32)
    v = np.ones((m, 3), F32)
    lo, hi = np.full((m, 3), -1, F32), np.full((m, 3), 1, F32)
    for j, (a, b, _) in enumerate(KNOWN_ANSWERS):
        v[j, 0], lo[j, 0] = b, a
        hi[j, 0] = 2.0 ** 40 if a > 0 else 1.0
    parts.append((o, v, np.full(m, INF, F32), lo, hi))
    # zero velocity components: the planes at +-inf, or 0 / 0 with the origin on a plane
    nz = n // 4
    o, v, reach, lo, hi = (x.copy() for x in _bulk(rng, nz))
    zero = rng.random((nz, 3)) < 0.4
    zero[np.arange(nz), rng.integers(0, 3, nz)] = True
    v[zero] = np.where(rng.random((nz, 3)) < 0.5, F32(0.0), F32(-0.0))[zero]
    on = zero & (rng.random((nz, 3)) < 0.25)
    lo[on] = o[on]
    off = zero & ~on & (rng.random((nz, 3)) < 0.25)
    hi[off] = lo[off]
    parts.append((o, v, reach, lo, hi))
    # a special value in every operand position, a second one in a quarter of the cases
    ns = n // 2
    p = np.arange(ns) % 13
    s = SPECIALS[(np.arange(ns) // 13) % len(SPECIALS)]
    o_pick, lo_pick = _values(rng, (ns, 3), COORD_E, 1 / 16), _values(rng, (ns, 3), COORD_E, 1 / 16)
    v = _values(rng, (ns, 3), VEL_E)
    from_box = rng.random((ns, 3)) < 0.3
    col = np.arange(3)[None, :]
    at_o, at_v, at_lo = (p[:, None] == col), (p[:, None] == col + 3), (p[:, None] == col + 6)
    o_pick = np.where(at_o, s[:, None], o_pick)
    v = np.where(at_v, s[:, None], v)
    lo_pick = np.where(at_lo, s[:, None], lo_pick)
    from_box = (from_box | at_lo) & ~at_o
    o, lo, hi, t = _assemble(rng, o_pick, lo_pick, v, from_box)
    reach = _reaches(rng, t)
    hi = np.where(p[:, None] == col + 9, s[:, None], hi)
    reach = np.where(p == 12, s, reach)
    second = rng.random(ns) < 0.25
    q = rng.integers(0, 12, ns)
    s2 = SPECIALS[rng.integers(0, len(SPECIALS), ns)]
    for base, arr in ((0, o), (3, v), (6, lo), (9, hi)):
        sel = second[:, None] & (q[:, None] == col + base)
        arr[sel] = np.broadcast_to(s2[:, None], arr.shape)[sel]
    parts.append((o.astype(F32), v.astype(F32), reach.astype(F32), lo.astype(F32), hi.astype(F32)))
    # denormal and vanishing quotients as the entry time: the box holds the
    # origin on two axes; on the third a tiny numerator (a box plane below
    # 2^-100 seen from 0, or an origin a step from an in-range plane) over a
    # velocity of 1 .. 2^27 or beyond 2^27
    nt = n - m - nz - ns
    o, v, reach, lo, hi = (x.copy() for x in _bulk(rng, nt))
    lo, hi = _coordinate(o.astype(F64) - _width(rng, o)), _coordinate(o.astype(F64) + _width(rng, o))
    i, c = np.arange(nt), rng.integers(0, 3, nt)
    tiny_box = rng.random(nt) < 0.5
    tiny = np.where(rng.random(nt) < 0.5, np.abs(SPECIALS[rng.integers(0, 12, nt)]),
                    np.abs(_values(rng, nt, (-140, -100)).astype(F32)))
    plane = np.abs(_values(rng, nt, (-50, -36)))
    vc = np.where(tiny_box, np.abs(_values(rng, nt, (0, 27))), np.abs(_values(rng, nt, (28, 127))))
    v[i, c] = vc
    o[i, c] = np.where(tiny_box, F32(0.0), _step(plane, -rng.integers(1, 3, nt)))
    lo[i, c] = np.where(tiny_box, tiny, plane)
    hi[i, c] = np.where(tiny_box, F32(1.0), plane * F32(2.0))
    parts.append((o, v, np.full(nt, INF, F32), lo.astype(F32), hi.astype(F32)))
    return tuple(np.concatenate([x[j] for x in parts]).astype(F32) for j in range(5))


def _reach(rng, n):
    """In-domain rays whose reach decides: PT_HIT_TIME_LIMIT, PT_INFINITY, 0,
    negative and small values, and the reference's own entry time (the tie of
    EntryT >= Reach) with its two neighbours."""
    a, b = _bulk(rng, n // 2), _near(rng, n - n // 2)
    o, v, _, lo, hi = (np.concatenate([x, y]) for x, y in zip(a, b))
    e = reference(o, v, np.full(n, INF, F32), lo, hi)
    k = np.arange(n) % 8
    small = np.abs(_values(rng, n, (-80, 1)))
    reach = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6],
                      [np.full(n, HIT_TIME_LIMIT), np.full(n, INF), np.zeros(n, F32), -small, small, e,
                       np.nextafter(e, F32(np.inf))], np.nextafter(e, F32(-np.inf))).astype(F32)
    return o, v, reach, lo, hi


_BUILDERS = {"bulk": _bulk, "edges": _edges, "near": _near, "outside": _outside,
             "reach": _reach}


@functools.lru_cache(maxsize=None)
def cases(name):
    """The class's cases: {"o", "v", "lo", "hi": (n, 3), "reach": (n,)}, float32, read-only, the same at every call."""
    rng = np.random.default_rng([0x51AB, CLASSES.index(name)])
    return _pack(*(np.ascontiguousarray(x, dtype=F32) for x in _BUILDERS[name](rng, SIZES[name])))


@functools.lru_cache(maxsize=None)
def expected(name):
    """(entry times of the IEEE reference, the ray gate, the box gate) of the class, computed once."""
    c = cases(name)
    out = (reference(c["o"], c["v"], c["reach"], c["lo"], c["hi"]), expected_flag(c["o"], c["v"]),
           boxes_in_range(c["lo"], c["hi"]))
    for a in out:
        a.setflags(write=False)
    return out


def same_entry(got_bits, ref):
    """Bit equality of entry times, with two zeros of either sign equal (a zero
    numerator may give the other zero, and every consumer compares) and two
    NaNs equal.  Returns the per-case verdict."""
    got = from_bits(got_bits)
    return (bits(got) == bits(ref)) | ((got == 0) & (ref == 0)) | (np.isnan(got) & np.isnan(ref))
