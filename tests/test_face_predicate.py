"""The lean face test's two predicates (include/pt_facetest.h) through the host
library's ptsFaceTest, against the reference form of FaceTest restated here in
numpy binary32:

    InvDet = 1 / Det;  U = InvDet * a;  W = InvDet * b;  T = InvDet * c
    miss = |Det| < eps | U < 0 | U > 1 | W < 0 | U + W > 1 | T < 0 | T > Time

The folded flag must equal the seven-term one on every operand set, and U, W,
T must carry the reference's bits whenever the reference says hit (a hit's
values go into the hit record).  A hit with a NaN determinant is one the
reference accepts too (every compare with a NaN is false); there the values
are NaN on both sides and a NaN's payload is not compared: IEEE arithmetic does
not define it.

Operands: a few million seeded random sets (raw bit patterns, and sets around
the unit triangle), and the cross product of the values at which such a
predicate goes wrong: NaN, infinities, zeros of both signs, denormals, 0 and 1
and their neighbours for U and W, pairs whose sum is 1 or the next float, T at
0, -0, Time and its neighbours, |Det| at eps, 2^-126 and 2^126 and their
neighbours.

The gate of the fast reciprocal (pt_face_needs_division) is returned per
determinant and held to "not |d| < 2^126" on every one of those sets; where it
lets a determinant below 2^-126 through, the reference must miss."""
from __future__ import annotations

import numpy as np

f32 = np.float32
EPS = f32(1e-9)
INF, NAN = f32(np.inf), f32(np.nan)


def lean(pt, det, a, b, c, time):
    N = pt._native
    n = len(det)
    arrs = [np.ascontiguousarray(x, dtype=np.float32) for x in (det, a, b, c, time)]
    miss = np.zeros(n, np.uint32)
    divides = np.full(n, 7, np.uint32)
    u, w, t = (np.zeros(n, np.float32) for _ in range(3))
    rc = N.scene_lib().ptsFaceTest(n, *(N.fptr(x) for x in arrs), N.u32ptr(miss), N.fptr(u), N.fptr(w), N.fptr(t),
                                   N.u32ptr(divides))
    assert rc == 0
    assert np.all(divides <= 1)
    return miss != 0, u, w, t, divides != 0


def reference(det, a, b, c, time):
    with np.errstate(all="ignore"):
        inv = f32(1.0) / det
        u, w, t = inv * a, inv * b, inv * c
        miss = ((np.abs(det) < EPS) | (u < 0) | (u > 1) | (w < 0) | (u + w > 1) | (t < 0) | (t > time))
    return miss, u, w, t


RCP_MIN, RCP_MAX = f32(2.0 ** -126), f32(2.0 ** 126)   # FastRcp is the IEEE quotient for RCP_MIN <= |d| < RCP_MAX


def check_gate(det, divides, reference_miss):
    """The gate's flag, as the host library returns it per determinant: the
    division is asked for exactly where |d| < 2^126 does not hold (the huge,
    the infinite and the NaN), and wherever it is not asked for below the
    reciprocal's range, the reference misses the face, so the quotient is
    never read."""
    with np.errstate(all="ignore"):
        want = ~(np.abs(det) < RCP_MAX)
        bad = np.flatnonzero(divides != want)
        assert bad.size == 0, f"gate differs on {bad.size} determinants; first: det={det[bad[0]]!r} gate={divides[bad[0]]}"
        unproven = ~divides & ~(np.abs(det) >= RCP_MIN)
    bad = np.flatnonzero(unproven & ~reference_miss)
    assert bad.size == 0, f"{bad.size} hits take the fast reciprocal outside its range; first: det={det[bad[0]]!r}"
    return want


def check(pt, det, a, b, c, time):
    det, a, b, c, time = (np.ascontiguousarray(x, dtype=np.float32) for x in (det, a, b, c, time))
    got = lean(pt, det, a, b, c, time)
    want = reference(det, a, b, c, time)
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, (f"{bad.size} flags differ; first: det={det[bad[0]]!r} a={a[bad[0]]!r} b={b[bad[0]]!r} "
                           f"c={c[bad[0]]!r} time={time[bad[0]]!r} lean={got[0][bad[0]]} reference={want[0][bad[0]]}")
    check_gate(det, got[4], want[0])
    hit = ~want[0]
    for name, g, r in zip("UWT", got[1:4], want[1:]):
        same = (g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))
        bad = np.flatnonzero(hit & ~same)
        assert bad.size == 0, (f"{name} differs on {bad.size} hits; first: det={det[bad[0]]!r} "
                               f"lean={g[bad[0]]!r} reference={r[bad[0]]!r}")
    return int(hit.sum())


def nxt(x, to):
    return np.nextafter(f32(x), f32(to), dtype=np.float32)


def test_random_bit_patterns(pt):
    """Every operand a random binary32 pattern: all classes of value in every slot."""
    rng = np.random.default_rng(20240611)
    n = 1 << 21
    ops = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(5)]
    check(pt, *ops)


def test_random_around_the_triangle(pt):
    """Determinants over every exponent, coordinates and times around their
    bounds: a good part of the sets are hits, so the stored values are compared."""
    rng = np.random.default_rng(7)
    n = 1 << 21
    det = (np.exp2(rng.uniform(-140, 128, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    det[: n // 2] = rng.uniform(-4, 4, n // 2).astype(np.float32)
    u = rng.uniform(-0.25, 1.25, n).astype(np.float32)
    w = rng.uniform(-0.25, 1.25, n).astype(np.float32)
    t = rng.uniform(-1, 8, n).astype(np.float32)
    time = rng.choice(np.array([1048576.0, 4.0, 1.0], np.float32), n)
    with np.errstate(all="ignore"):
        hits = check(pt, det, u * det, w * det, t * det, time)
    assert hits > n // 16


DETS = [NAN, INF, -INF, 0.0, -0.0, 1e-45, -1e-45, 1e-40, EPS, -EPS, nxt(EPS, 0), nxt(EPS, 1), -nxt(EPS, 0), -nxt(EPS, 1),
        2.0 ** -126, nxt(2.0 ** -126, 0), nxt(2.0 ** -126, 1), -(2.0 ** -126), 2.0 ** -127, 2.0 ** 126, nxt(2.0 ** 126, 0),
        nxt(2.0 ** 126, INF), -(2.0 ** 126), -nxt(2.0 ** 126, 0), 2.0 ** 127, 3.4028234663852886e38, 1.0, -1.0, 2.0, 0.5,
        3.0, -0.75]
UW = [NAN, INF, -INF, 0.0, -0.0, 1e-45, -1e-45, 1.0, nxt(1, 2), nxt(1, 0), nxt(0, -1), 0.5, nxt(0.5, 1), nxt(0.5, 0),
      0.25, 0.75, nxt(0.75, 1)]
TS = [NAN, INF, -INF, 0.0, -0.0, 1e-45, -1e-45, 1.0, nxt(1, 2), nxt(1, 0), 1048576.0, nxt(1048576.0, INF),
      nxt(1048576.0, 0), 3.0]
TIMES = [1048576.0, 1.0, 0.0, INF, NAN]


def test_adversarial_cross_product(pt):
    """Every combination of the special values above.  The numerators are the
    wanted U, W, T times the determinant, so with Det = 1, -1, 2, 0.5 the
    coordinates land exactly on the listed values (U + W exactly 1, the next
    float, T exactly Time), and with the other determinants whatever the
    arithmetic makes of them, NaN and infinities included."""
    g = np.meshgrid(*(np.array(x, np.float32) for x in (DETS, UW, UW, TS, TIMES)), indexing="ij")
    det, u, w, t, time = (x.ravel() for x in g)
    with np.errstate(all="ignore"):
        hits = check(pt, det, u * det, w * det, t * det, time)
        hits += check(pt, det, u, w, t, time)   # the values as numerators
    assert hits > 0


def test_gate_of_the_fast_reciprocal(pt):
    """pt_face_needs_division at its bound, flag by flag (check_gate also runs
    on every operand set of the tests above, the random bit patterns and the
    adversarial determinants included).  The values cannot show the gate on
    the host: its model of the fast reciprocal starts from the correctly
    rounded quotient, and a Newton step on that returns it at 2^126 and beyond
    too.  So the flag itself is returned and compared."""
    big = [2.0 ** 126, nxt(2.0 ** 126, INF), 1.5 * 2.0 ** 126, 2.0 ** 127, 3.4028234663852886e38, INF, NAN]
    small = [nxt(2.0 ** 126, 0), 2.0 ** 125, 1.0, EPS, 2.0 ** -126, nxt(2.0 ** -126, 0), 2.0 ** -127, 1e-45, 0.0]
    det = np.array(big + [-x for x in big] + small + [-x for x in small], np.float32)
    with np.errstate(all="ignore"):
        ops = (det, det * f32(0.25), det * f32(0.0), det, np.full(len(det), 4.0, np.float32))   # U about 1/4, W 0, T about 1
    miss, u, w, t, divides = lean(pt, *ops)
    assert divides.tolist() == [True] * (2 * len(big)) + [False] * (2 * len(small))
    ref = reference(*ops)
    check_gate(det, divides, ref[0])
    assert np.array_equal(miss, ref[0])
    finite_big = np.isfinite(det) & divides
    assert finite_big.sum() == 10 and not miss[finite_big].any()      # faces that are hit through the division
    assert np.array_equal(u[finite_big].view(np.uint32), ref[1][finite_big].view(np.uint32))
    tiny = np.abs(det) < RCP_MIN
    assert tiny.sum() == 8 and miss[tiny].all()                       # below the range: missed, the quotient unread


def test_null_arguments(pt):
    N = pt._native
    a = np.zeros(1, np.float32)
    m = np.zeros(1, np.uint32)
    assert N.scene_lib().ptsFaceTest(1, None, N.fptr(a), N.fptr(a), N.fptr(a), N.fptr(a), N.u32ptr(m), N.fptr(a),
                                     N.fptr(a), N.fptr(a), N.u32ptr(m)) == -1
    assert N.scene_lib().ptsFaceTest(1, N.fptr(a), N.fptr(a), N.fptr(a), N.fptr(a), N.fptr(a), N.u32ptr(m), N.fptr(a),
                                     N.fptr(a), N.fptr(a), None) == -1
