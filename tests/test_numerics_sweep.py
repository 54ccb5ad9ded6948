"""The host side of the numerics convention (include/pt_fp.h, evaluated in
batches through oracle_fp_eval) against numpy float64 over the in-domain input
sets of tests/numerics_cases.py: every exponent, the cut points of every
reduction and branch, denormals, specials in every operand position.

Bounds are the project's own (tests/test_numerics.py): exp, log, sin, cos
within 2 ulp, asin and atan2 within 3 ulp, sin / cos also within 4e-7 absolute
near their zeros (the argument reduction's error).  The error is measured
against the float64 value in units of the float32 spacing at that value; a
result whose exact value lies below 2^-126 is held to one 2^-149 step.
Exactly specified operations must give numpy's float32 bits (two NaNs count
as equal, the rule of test_resolve_bit_exact).  Each test prints its worst
figure before it asserts.

Conventions the references follow: the transcendental kernels know no signed
zero (GLSL), so atan2's reference takes -0 as 0, and pt_atan2(0, 0) = 0;
atan2 of two infinities is NaN here (inf / inf), which the reference pins;
rint / round are compared by value (either zero); min / max order -0 below
+0; pt_pow
is defined as pt_exp(y * pt_log(x)) and is checked as that composition.
"""
from __future__ import annotations

import numpy as np
import pytest

import kat
import numerics_cases as nc
import oracle_lib

F32 = np.float32


def host(op):
    c = nc.cases(op)["in_domain"]
    return c, oracle_lib.fp_eval(op, *c)


def assert_bits(op, got, want, operands):
    """Bit equality; positions where both are NaN count as equal."""
    got = np.asarray(got, dtype=np.uint32).reshape(len(operands[0]), -1)
    want = np.asarray(want, dtype=np.uint32).reshape(len(operands[0]), -1)

    def nan(u):
        return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    bad = np.any((got != want) & ~(nan(got) & nan(want)), axis=1)
    idx = np.flatnonzero(bad)[:5]
    rows = [" ".join(f"{int(x[i]):08x}" for x in operands) + " -> " + " ".join(f"{int(v):08x}" for v in got[i]) +
            " want " + " ".join(f"{int(v):08x}" for v in want[i]) for i in idx]
    print(f"{op}: {int(bad.sum())} of {len(bad)} differ")
    assert not bad.any(), f"{op}: {int(bad.sum())} of {len(bad)} differ; first: " + "; ".join(rows)


def assert_values(op, got_bits, want, operands):
    """Equality as floats (-0 == +0), NaN exactly where the reference has one."""
    got = nc.u2f(got_bits)
    want = np.asarray(want, dtype=F32)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    idx = np.flatnonzero(bad)[:5]
    rows = [" ".join(f"{int(x[i]):08x}" for x in operands) + f" -> {got[i]!r} want {want[i]!r}" for i in idx]
    print(f"{op}: {int(bad.sum())} of {len(bad)} differ")
    assert not bad.any(), f"{op}: {int(bad.sum())} of {len(bad)} differ; first: " + "; ".join(rows)


def ulp_error(got: np.ndarray, exact: np.ndarray) -> np.ndarray:
    """|got - exact| in float32 spacings at `exact` (2^-149 below 2^-126; an
    infinite result counts as 2^128, the value it rounds from)."""
    g = got.astype(np.float64)
    g = np.where(np.isinf(g), np.sign(g) * 2.0 ** 128, g)
    x = np.sign(exact) * np.minimum(np.abs(exact), 2.0 ** 128)     # beyond the format: what inf rounds from
    _, e = np.frexp(np.abs(x))
    ulp = np.ldexp(1.0, np.clip(e - 24, -149, 104))
    return np.abs(g - x) / ulp


def check_accuracy(op, operands, got_bits, exact, max_ulp, floor=0.0):
    """got within max_ulp of `exact` (float64) or within `floor` absolutely;
    one 2^-149 step where the exact value is below 2^-126; NaN where exact is."""
    got = nc.u2f(got_bits)
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(exact)
        err = ulp_error(got, np.where(nan, 0.0, exact))
        bound = np.where(np.abs(exact) < 2.0 ** -126, 1.0, float(max_ulp))
        ok = (err <= bound) | (np.abs(got.astype(np.float64) - exact) <= floor)
        ok = np.where(nan, np.isnan(got), ok & ~np.isnan(got))
    fin = np.where(nan | np.isnan(got), 0.0, err)
    w = int(np.argmax(fin))
    with np.errstate(invalid="ignore"):
        over = np.where((fin > bound) & np.isfinite(exact), np.abs(got.astype(np.float64) - exact), 0.0)
    print(f"{op}: worst {fin[w]:.3f} ulp at " + " ".join(f"{int(x[w]):08x}" for x in operands) +
          f" over {len(got)} inputs; largest absolute error beyond the ulp bound {over.max():.3g}; "
          f"outside bound and floor: {int((~ok).sum())}")
    idx = np.flatnonzero(~ok)
    worst = idx[np.argsort(-fin[idx])][:5]
    rows = [" ".join(f"{int(x[i]):08x}" for x in operands) + f" -> {int(got_bits[i]):08x} ({fin[i]:.2f} ulp)" for i in worst]
    assert ok.all(), f"{op}: {int((~ok).sum())} of {len(ok)} beyond {max_ulp} ulp; worst: " + "; ".join(rows)


# --- exactly specified operations -------------------------------------------------

def fma_reference(a, b, c):
    """Correctly rounded a * b + c: the product is exact in float64; the sum is
    rounded to odd at 53 bits (TwoSum's error tells inexactness and its side),
    after which the rounding to 24 bits is the correct one (Boldo-Melquiond)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        z = c.astype(np.float64)
        s = p + z
        bb = s - p
        err = (p - (s - bb)) + (z - bb)
        even = (s.view(np.uint64) & np.uint64(1)) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F32)


@pytest.mark.parametrize("op", ["add", "mul", "div", "sqrt", "fma"])
def test_arithmetic_equals_ieee(op):
    c, got = host(op)
    f = [nc.u2f(x) for x in c]
    with np.errstate(all="ignore"):
        want = {"add": lambda: f[0] + f[1], "mul": lambda: f[0] * f[1], "div": lambda: f[0] / f[1],
                "sqrt": lambda: np.sqrt(f[0]), "fma": lambda: fma_reference(*f)}[op]()
    assert want.dtype == F32
    assert_bits(op, got, nc.f2u(want), c)


def minnum(a, b):
    """minNum with -0 ordered below +0 (include/pt_fp.h pt_min), as bit patterns' floats."""
    return np.where(a == b, nc.u2f(nc.f2u(a) | nc.f2u(b)), np.fmin(a, b)).astype(F32)


def maxnum(a, b):
    return np.where(a == b, nc.u2f(nc.f2u(a) & nc.f2u(b)), np.fmax(a, b)).astype(F32)


def test_min_max_clamp_follow_minnum():
    """IEEE minNum / maxNum: a quiet NaN operand loses, and -0 lies below +0
    (what v_min_f32 / v_max_f32 do; C leaves the zeros to the library)."""
    for op in ("min", "max", "clamp"):
        c, got = host(op)
        f = [nc.u2f(x) for x in c]
        want = {"min": lambda: minnum(f[0], f[1]), "max": lambda: maxnum(f[0], f[1]),
                "clamp": lambda: minnum(maxnum(f[0], f[1]), f[2])}[op]()
        assert_bits(op, got, nc.f2u(want), c)
    assert nc.f2u(minnum(F32([0.0, -0.0]), F32([-0.0, 0.0]))).tolist() == [0x80000000] * 2
    assert nc.f2u(maxnum(F32([0.0, -0.0]), F32([-0.0, 0.0]))).tolist() == [0] * 2


def test_floor_fract_mix():
    c, got = host("floor")
    assert_bits("floor", got, nc.f2u(np.floor(nc.u2f(c[0]))), c)
    c, got = host("fract")
    x = nc.u2f(c[0])
    with np.errstate(invalid="ignore"):
        want = x - np.floor(x)
    assert_bits("fract", got, nc.f2u(want), c)
    assert np.any(want == F32(1.0)), "the set must reach fract(x) == 1.0f"
    c, got = host("mix")
    x, y, a = (nc.u2f(v) for v in c)
    with np.errstate(all="ignore"):
        want = x * (F32(1.0) - a) + y * a
    assert_bits("mix", got, nc.f2u(want), c)


def test_rint_and_round_half_away():
    c, got = host("rint")
    x = nc.u2f(c[0])
    assert np.all(np.abs(x) < 2.0 ** 22)
    assert_values("rint", got, np.rint(x), c)        # ties to even
    c, got = host("round_half_away")
    x = nc.u2f(c[0]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        want = np.where(np.abs(x - t) >= 0.5, t + np.where(x < 0, -1.0, 1.0), t)
    assert_values("round_half_away", got, want.astype(F32), c)


def test_conversions():
    c, got = host("u32_to_float")
    assert_bits("u32_to_float", got, nc.f2u(c[0].astype(F32)), c)
    c, got = host("floor_to_int")
    x = nc.u2f(c[0])
    assert_bits("floor_to_int", got, (np.floor(x.astype(np.float64)).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32), c)
    c, got = host("random")
    state, value = nc.pcg(c[0])
    assert_bits("random", got, np.stack([state, value], axis=1), c)
    c, got = host("random01")
    want = value.astype(F32) * F32(2.0 ** -32)
    assert_bits("random01", got, nc.f2u(want), c)
    assert np.any(want == F32(1.0)) and np.count_nonzero(value >= 2 ** 32 - 128) >= 128


def pack_snorm16_reference(v):
    """round-half-away(clamp(v, -1, 1) * 32767); a NaN clamps to -1 (minNum / maxNum)."""
    v = np.asarray(v, dtype=F32)
    s = np.fmin(np.fmax(v, F32(-1)), F32(1)) * F32(32767.0)
    q = (np.sign(s) * np.floor(np.abs(s.astype(np.float64)) + 0.5)).astype(np.int64)
    return (q & 0xFFFF).astype(np.uint32)


def test_packing():
    c, got = host("pack_snorm16")
    assert_bits("pack_snorm16", got, pack_snorm16_reference(nc.u2f(c[0])), c)
    c, got = host("unpack_snorm16")
    x = c[0].astype(np.uint16).view(np.int16).astype(F32)
    assert_bits("unpack_snorm16", got, nc.f2u(np.clip(x / F32(32767.0), F32(-1), F32(1))), c)
    c, got = host("half_to_float")
    assert_bits("half_to_float", got, nc.f2u(c[0].astype(np.uint16).view(np.float16).astype(F32)), c)


def test_unit_vectors():
    """PackUnitVector / UnpackUnitVector against float32 numpy restatements
    (kat.unpack_unit_vector; the pack restated here with minNum clamping, so
    that the zero vector's NaNs are defined)."""
    c, got = host("pack_unit_vector")
    v = np.stack([nc.u2f(x) for x in c], axis=1)
    with np.errstate(all="ignore"):
        l1 = (np.abs(v[:, 0]) + np.abs(v[:, 1])) + np.abs(v[:, 2])
        inv = F32(1.0) / l1
        p = v[:, :2] * inv[:, None]
        fold = (F32(1.0) - np.abs(p[:, ::-1])) * np.where(p >= 0, F32(1), F32(-1))
        p = np.where((v[:, 2] <= 0)[:, None], fold, p).astype(F32)
    want = pack_snorm16_reference(p[:, 0]) | (pack_snorm16_reference(p[:, 1]) << 16)
    assert_bits("pack_unit_vector", got, want, c)
    c, got = host("unpack_unit_vector")
    with np.errstate(all="ignore"):
        want = kat.unpack_unit_vector(c[0])
    assert_bits("unpack_unit_vector", got, nc.f2u(want), c)


# --- transcendentals against float64 ----------------------------------------------

@pytest.mark.parametrize("op,max_ulp,floor", [("exp", 2, 0.0), ("log", 2, 0.0), ("sin", 2, 4e-7), ("cos", 2, 4e-7),
                                              ("asin", 3, 0.0)])
def test_transcendental_accuracy(op, max_ulp, floor):
    c, got = host(op)
    x = nc.u2f(c[0]).astype(np.float64)
    with np.errstate(all="ignore"):
        exact = {"exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "asin": np.arcsin}[op](x)
    if op in ("sin", "cos"):
        assert np.all(np.abs(x) < 8192.0)
    check_accuracy(op, c, got, exact, max_ulp, floor)


def test_atan2_accuracy():
    c, got = host("atan2")
    y, x = (nc.u2f(v).astype(np.float64) + 0.0 for v in c)      # + 0.0: -0 -> +0
    with np.errstate(all="ignore"):
        exact = np.arctan2(y, x)
    exact = np.where((x == 0) & (y == 0), 0.0, exact)
    exact = np.where(np.isinf(x) & np.isinf(y), np.nan, exact)
    check_accuracy("atan2", c, got, exact, 3)


def test_pow_is_exp_of_y_log_x():
    c, got = host("pow")
    x, y = (nc.u2f(v) for v in c)
    assert not np.any(x < 0)
    with np.errstate(all="ignore"):
        arg = y * nc.u2f(oracle_lib.fp_eval("log", c[0]))
    assert_bits("pow", got, oracle_lib.fp_eval("exp", nc.f2u(arg)), c)


def test_sets_are_disjoint_and_sized():
    """Every op has its sets; signalling NaNs and out-of-domain arguments are
    kept out of the asserted set; no set outgrows what a test can run."""
    from path_tracer_amd import _native as N
    for op in N.NUMERICS_OPS:
        c = nc.cases(op)
        assert set(c) == {"in_domain", "out_of_domain", "snan"}
        k = N.NUMERICS_OPERANDS.get(op, 1)
        assert all(len(v) == k and len({len(x) for x in v}) == 1 for v in c.values())
        assert 60000 <= len(c["in_domain"][0]) <= 10_000_000
        if op not in nc.INTEGER_OPERAND:
            assert len(c["snan"][0]) > 0
            assert not any(nc.is_snan(x).any() for x in c["in_domain"] + c["out_of_domain"])
    assert len(nc.cases("sin")["out_of_domain"][0]) > 0 and len(nc.cases("pow")["out_of_domain"][0]) > 0
