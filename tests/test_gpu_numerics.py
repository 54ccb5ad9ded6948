"""GPU: the numerics convention on the device against the host, bit for bit.

include/pt_fp.h promises the same bits on gfx950 as on the host; the CPU
oracle is a reference for the kernels only because of that.  ptEvalNumerics
evaluates each operation of include/pt_numerics.h in a kernel that calls the
functions as the product kernels do (probe.hip, the product's compile flags);
oracle_fp_eval does the same on the host.  Over every in-domain input of
tests/numerics_cases.py the two must agree in every bit (two NaNs count as
equal, the rule of test_resolve_bit_exact); nothing is skipped.  The
device-only forms FastRcp (inside FastRcpRange) and XDiv are held against
numpy's float32 division, which test_numerics_sweep.py also holds the host's
`/` against: device and host division are compared through it.

Out-of-domain arguments and signalling NaNs are evaluated and compared too,
but only recorded (printed, and in the report's properties): the two sides
are known to differ there, (int) of an out-of-range float saturating on the
device (v_cvt_i32_f32) and giving 0x80000000 on x86, and a signalling NaN
losing in the device's min / max where fminf / fmaxf return a quiet NaN.
DESIGN.md §2 lists the call sites and why their arguments stay in domain;
profiles/numerics_probe/README.md keeps the counts of the first runs, and what
the in-domain sets found and had fixed (the zeros' order in min / max, XDiv's
tiny numerators).
"""
from __future__ import annotations

import numpy as np
import pytest

import numerics_cases as nc
import oracle_lib
from path_tracer_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def is_nan(u):
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


def differing(op, got, want):
    """Rows whose words differ, two NaNs counting as equal (float results only)."""
    got = got.reshape(len(got), -1)
    want = want.reshape(len(want), -1)
    diff = got != want
    if op not in ("floor_to_int", "random", "pack_snorm16", "pack_unit_vector"):     # integer results
        diff &= ~(is_nan(got) & is_nan(want))
    return np.any(diff, axis=1)


def describe(op, operands, got, want, bad):
    got = got.reshape(len(got), -1)
    want = want.reshape(len(want), -1)
    rows = []
    for i in np.flatnonzero(bad)[:5]:
        rows.append("(" + " ".join(f"{int(x[i]):08x}" for x in operands) + ") device " +
                    " ".join(f"{int(v):08x}" for v in got[i]) + " host " + " ".join(f"{int(v):08x}" for v in want[i]))
    return f"{op}: {int(bad.sum())} of {len(bad)} inputs differ; first: " + "; ".join(rows)


def reference(op, operands):
    """The host's words: oracle_fp_eval, or numpy's float32 quotient for the
    device-only division forms."""
    if op == "fast_rcp":
        with np.errstate(all="ignore"):
            return nc.f2u(np.float32(1.0) / nc.u2f(operands[0]))
    if op == "xdiv":
        with np.errstate(all="ignore"):
            return nc.f2u(nc.u2f(operands[0]) / nc.u2f(operands[1]))
    return oracle_lib.fp_eval(op, *operands)


def split_fast_rcp(operands):
    """FastRcpRange (pt_device.hpp): 2^-126 <= |d| < 2^126; callers keep IEEE division outside."""
    m = np.abs(nc.u2f(operands[0]))
    with np.errstate(invalid="ignore"):
        inside = (m >= np.float32(2.0 ** -126)) & (m < np.float32(2.0 ** 126))
    return (operands[0][inside],), (operands[0][~inside],)


@pytest.mark.parametrize("op", N.NUMERICS_OPS)
def test_device_equals_host_bit_for_bit(dev, op, record_property):
    sets = dict(nc.cases(op))
    if op == "fast_rcp":
        inside, outside = split_fast_rcp(sets["in_domain"])
        sets["in_domain"] = inside
        sets["out_of_domain"] = tuple(np.concatenate([a, b]) for a, b in zip(sets["out_of_domain"], outside))
    # recorded sets first, so that their counts are reported whatever the assertion does
    for name in ("out_of_domain", "snan"):
        operands = sets[name]
        n = len(operands[0])
        count = 0
        if n:
            got, want = dev.eval_numerics(op, *operands), reference(op, operands)
            bad = differing(op, got, want)
            count = int(bad.sum())
            if count:
                print(f"[recorded] {name} " + describe(op, operands, got, want, bad))
        print(f"[recorded] {op} {name}: {count} of {n} differ")
        record_property(f"{name}_differ", f"{count}/{n}")
    operands = sets["in_domain"]
    assert len(operands[0]) > 0
    got, want = dev.eval_numerics(op, *operands), reference(op, operands)
    bad = differing(op, got, want)
    print(f"{op} in_domain: {int(bad.sum())} of {len(bad)} differ")
    assert not bad.any(), describe(op, operands, got, want, bad)


def test_argument_errors_write_nothing(pt, dev):
    L = N.hip_lib()
    a = np.arange(4, dtype=np.uint32)
    out = np.full(4, 0xDEADBEEF, dtype=np.uint32)
    assert L.ptEvalNumerics(dev.handle, len(N.NUMERICS_OPS), 4, N.u32ptr(a), None, None, N.u32ptr(out)) != 0
    assert b"unknown op" in L.ptGetLastError()
    assert L.ptEvalNumerics(dev.handle, N.NUMERICS_OPS.index("add"), 4, N.u32ptr(a), None, None, N.u32ptr(out)) != 0
    assert L.ptEvalNumerics(dev.handle, N.NUMERICS_OPS.index("fma"), 4, N.u32ptr(a), N.u32ptr(a), None, N.u32ptr(out)) != 0
    assert L.ptEvalNumerics(dev.handle, N.NUMERICS_OPS.index("exp"), 4, N.u32ptr(a), None, None, None) != 0
    assert L.ptEvalNumerics(None, 0, 4, N.u32ptr(a), N.u32ptr(a), None, N.u32ptr(out)) != 0
    assert np.all(out == 0xDEADBEEF)
    assert L.ptEvalNumerics(dev.handle, 0, 0, None, None, None, None) == 0
    with pytest.raises(pt.PathTracerError):
        dev.eval_numerics("add", a)
    # one element, and a count that is no multiple of the block
    assert dev.eval_numerics("add", a[:1], a[:1])[0] == 0
    x = nc.f2u(np.arange(257, dtype=np.float32))
    assert np.array_equal(dev.eval_numerics("add", x, x), nc.f2u(np.arange(257, dtype=np.float32) * 2))
