"""Input sets of the numerics sweep, shared by the host test
(test_numerics_sweep.py: include/pt_fp.h against float64) and the device test
(test_gpu_numerics.py: ptEvalNumerics against oracle_fp_eval, bit for bit).

Seeded and deterministic, built once per process.  cases(op) returns the
operand words (uint32: float bit patterns or integers) of one operation of
include/pt_numerics.h in three named sets:

    in_domain      everything the convention defines; both tests assert on it
    out_of_domain  arguments outside a function's documented domain (sin / cos
                   at |x| >= 2^13 or non-finite, rint at |x| >= 2^22, pow with
                   x < 0, (int)floor(x) beyond the int range or of a NaN)
    snan           elements with a signalling NaN operand (arithmetic never
                   produces one; pt_half_to_float can)

The last two are compared and recorded by the device test, not asserted.

What the sets hold (each op's in-domain set is about 2.2 M elements; rint's
holds every half-integer of its domain and has 9.6 M, unpack_unit_vector's
every x field against 64 y fields, 4.3 M):
  * every exponent: all 256 exponent fields x both signs x the mantissas
    0..63, 2^23-64..2^23-1 and 4096 seeded random ones; binary ops pair the set
    with a fixed permutation of itself (quotients, products and sums reach
    overflow, underflow and denormal results), fma with a second one;
  * 64 floats on each side of every constant the code branches or reduces on;
  * specials (+-0, +-inf, quiet NaNs of both signs and with a payload, two
    signalling NaNs, the extreme finite values) in every operand position;
  * exhaustive sets where the input is 16 bits wide.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

SEED = 20250

INTEGER_OPERAND = ("u32_to_float", "random", "random01", "unpack_snorm16", "half_to_float", "unpack_unit_vector")

SNANS = np.array([0x7F800001, 0xFFA00000], dtype=np.uint32)
SPECIALS = np.concatenate([np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,       # +-0, +-inf
    0x7FC00000, 0xFFC00000, 0x7FC12345,                   # quiet NaNs: both signs, a payload
    0x3F800000, 0xBF800000, 0x00000001, 0x80000001,       # +-1, +-smallest denormal
    0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,       # largest denormal, smallest normal, +-largest
    0x3F000000, 0x40490FDB,                               # 0.5, pi
], dtype=np.uint32), SNANS])


def f2u(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def u2f(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def is_snan(u) -> np.ndarray:
    u = np.asarray(u, dtype=np.uint32)
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0) & ((u & 0x00400000) == 0)


def around(values, k=64) -> np.ndarray:
    """The k floats below and above each value, and the value (bit patterns):
    neighbours in the ordering of the reals, across zero and up to +-inf."""
    u = f2u(np.atleast_1d(np.asarray(values, dtype=np.float32))).astype(np.int64)
    key = np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)            # monotonic integer of the float
    key = (key[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).reshape(-1)
    key = np.clip(key, -0x7F800000, 0x7F800000)
    out = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return np.concatenate([out, np.array([0x80000000], dtype=np.uint32)]) if np.any(key == 0) else out


@functools.lru_cache(maxsize=None)
def exponent_set() -> np.ndarray:
    rng = np.random.default_rng(SEED)
    fixed = np.concatenate([np.arange(64), np.arange(2**23 - 64, 2**23)]).astype(np.uint32)
    out = []
    for sign in (0, 1):
        for e in range(256):
            m = np.concatenate([fixed, rng.integers(0, 2**23, 4096, dtype=np.uint32)])
            out.append((np.uint32(sign << 31) | np.uint32(e << 23)) | m)
    out = np.concatenate(out).astype(np.uint32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def permutation(k: int) -> np.ndarray:
    return np.random.default_rng(SEED + k).permutation(len(exponent_set()))


def product(k: int):
    """SPECIALS in every position of a k-operand op."""
    grid = np.array(list(itertools.product(SPECIALS.tolist(), repeat=k)), dtype=np.uint32)
    return tuple(np.ascontiguousarray(grid[:, i]) for i in range(k))


def pcg(state: np.ndarray):
    """pt_random restated (common.glsl.inc:189-196): (new state, value)."""
    s = (state.astype(np.uint64) * 747796405 + 2891336453) & 0xFFFFFFFF
    w = ((((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * 277803737) & 0xFFFFFFFF)
    return s.astype(np.uint32), ((w >> np.uint64(22)) ^ w).astype(np.uint32)


def pcg_state_for(value: int) -> int:
    """The state whose pt_random value is `value` (every step is invertible)."""
    M = 1 << 32
    w = value ^ (value >> 22)
    x = (w * pow(277803737, -1, M)) % M
    sh = (x >> 28) + 4
    s = x
    for _ in range(8):
        s = x ^ (s >> sh)
    return ((s - 2891336453) * pow(747796405, -1, M)) % M


def _cuts(op: str) -> np.ndarray:
    ln2 = np.log(2.0)
    if op == "exp":
        c = [-103.972084, np.log(2.0 ** -126), 88.72284, 0.0] + [(j + 0.5) * ln2 for j in range(-150, 129)]
        return around(c)
    if op == "log":
        return around([2.0 ** -126, 1.0] + [np.sqrt(0.5) * 2.0 ** e for e in range(-148, 128)])
    if op in ("sin", "cos"):
        return around(np.concatenate([np.arange(-5215, 5216) * (np.pi / 2), [-8192.0, 8192.0]]))
    if op == "asin":
        return around([-1.0, -0.5, 0.5, 1.0])
    if op == "sqrt":
        n = np.arange(1, 4097, dtype=np.float64) ** 2
        sq = np.concatenate([n * 4.0 ** e for e in (-70, -63, -12, 0, 1, 20, 50)])
        return np.concatenate([around(sq, 1), np.arange(0, 8192, dtype=np.uint32),
                               around([2.0 ** -126, 2.0 ** -127, 2.0 ** -149 * 3], 8)])
    if op == "rint":       # every half-integer of the domain |x| < 2^22, and the border
        h = np.arange(0, 2 ** 22, dtype=np.float64) + 0.5
        return np.concatenate([f2u(h), f2u(-h), around([-(2.0 ** 22), 2.0 ** 22])])
    if op in ("round_half_away", "floor", "fract", "floor_to_int"):
        h = np.arange(0, 32768, dtype=np.float64) + 0.5
        ints = np.concatenate([np.arange(0, 4100), 2 ** np.arange(12, 32)]).astype(np.float64)
        c = np.concatenate([around(h[:512], 2), around(-h[:512], 2), f2u(h), f2u(-h), around(ints, 2),
                            around(-ints, 2), f2u([-(2.0 ** -30), 1e6, 2.0 ** 24 + 2])])
        return c
    if op == "pack_snorm16":
        k = np.arange(-32767, 32767, dtype=np.float64)
        return np.concatenate([around((k + 0.5) / 32767.0, 2), around([-1.0, 1.0]),
                               f2u([1.5, -1.5, 2.0, -2.0, 1e10, -1e10, 3.4e38, -3.4e38])])
    return np.zeros(0, dtype=np.uint32)


def _unit_vectors():
    rng = np.random.default_rng(SEED + 7)
    v = rng.normal(size=(1 << 20, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v.astype(np.float32)
    axes = []
    for s in (1.0, -1.0):
        for i in range(3):
            e = np.zeros(3, dtype=np.float32)
            e[i] = s
            axes.append(e)
    # octant borders: one or two components +-0, the rest random; diagonals
    b = rng.normal(size=(6000, 3)).astype(np.float32)
    b[:1000, 0] = 0.0; b[1000:2000, 1] = 0.0; b[2000:3000, 2] = 0.0
    b[3000:4000, 0] = -0.0; b[4000:5000, 1] = -0.0; b[5000:6000, 2] = -0.0
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    d = np.array(list(itertools.product((-1.0, 0.0, -0.0, 1.0), repeat=3)), dtype=np.float32)   # holds the zero vector
    tiny = np.array([[1e-30, 0, 0], [1e-40, 1e-40, 1e-40], [1e30, 1e30, -1e30], [3e38, 3e38, 3e38]], dtype=np.float32)
    allv = np.concatenate([v, np.array(axes), b, d, d * np.float32(0.57735026), tiny])
    u = f2u(allv)
    sp = product(3)
    return tuple(np.concatenate([np.ascontiguousarray(u[:, i]), sp[i]]) for i in range(3))


def _packed_unit_vectors():
    rng = np.random.default_rng(SEED + 8)
    ys = np.concatenate([np.array([0, 1, 2, 0x3FFF, 0x4000, 0x4001, 0x7FFE, 0x7FFF, 0x8000, 0x8001, 0x8002, 0xBFFF,
                                   0xC000, 0xC001, 0xFFFE, 0xFFFF], dtype=np.uint32),
                         rng.integers(0, 65536, 48, dtype=np.uint32)])
    x = np.arange(65536, dtype=np.uint32)
    grid = (x[None, :] | (ys[:, None] << 16)).reshape(-1)
    corner = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    corners = (corner[None, :] | (corner[:, None] << 16)).reshape(-1)
    swapped = (ys[None, :] | (x[:1024, None] << 16)).reshape(-1)
    return np.concatenate([grid, corners, swapped]).astype(np.uint32)


def _raw(op: str):
    """All operand tuples of an op before the split into named sets."""
    from path_tracer_amd import _native as N
    k = N.NUMERICS_OPERANDS.get(op, 1)
    E = exponent_set()
    if op in ("unpack_snorm16", "half_to_float"):
        return (np.arange(65536, dtype=np.uint32),)
    if op in ("random", "random01"):
        rng = np.random.default_rng(SEED + 9)
        top = np.array([pcg_state_for(v) for v in range(2 ** 32 - 192, 2 ** 32)], dtype=np.uint32)
        assert np.array_equal(pcg(top)[1], np.arange(2 ** 32 - 192, 2 ** 32, dtype=np.uint64).astype(np.uint32))
        rest = (1 << 20) - len(top) - 4096
        return (np.concatenate([np.arange(2048, dtype=np.uint32), np.arange(2 ** 32 - 2048, 2 ** 32, dtype=np.uint64)
                                .astype(np.uint32), top, rng.integers(0, 2 ** 32, rest, dtype=np.uint32)]),)
    if op == "unpack_unit_vector":
        return (_packed_unit_vectors(),)
    if op == "pack_unit_vector":
        return _unit_vectors()
    if op == "u32_to_float":
        ints = np.concatenate([(1 << np.arange(0, 32)).astype(np.int64) + d for d in range(-130, 131)])
        ints = ints[(ints >= 0) & (ints < 2 ** 32)]
        return (np.concatenate([E, ints.astype(np.uint32), np.arange(2 ** 32 - 4096, 2 ** 32, dtype=np.uint64)
                                .astype(np.uint32), np.arange(2 ** 24 - 2048, 2 ** 24 + 4096, dtype=np.uint32)]),)
    parts = [tuple(E if i == 0 else E[permutation(i)] for i in range(k)), product(k)]
    if k == 1:
        c = _cuts(op)
        if len(c):
            parts.append((c,))
        if op in ("sin", "cos"):       # beyond the domain: 2^13 .. 2^31, 3e9, 1e20
            big = np.concatenate([around(2.0 ** np.arange(13, 32), 8), f2u([3e9, -3e9, 1e20, -1e20])])
            parts.append((big,))
    if op == "atan2":
        r = np.concatenate([around(np.tan(np.pi / 8)), around(np.tan(3 * np.pi / 8)), around(1.0)])
        for x in (1.0, 3.0, 2.0 ** -60, 2.0 ** 60, 0.7):
            for sx, sy in itertools.product((1.0, -1.0), repeat=2):
                y = (u2f(r).astype(np.float64) * x).astype(np.float32)
                parts.append((f2u(sy * y), f2u(np.full(len(y), sx * x, dtype=np.float32))))
                parts.append((f2u(np.full(len(y), sy * x, dtype=np.float32)), f2u(sx * y)))   # the other branch
        fin = f2u([1.0, -1.0, 1e-40, -1e-40, 3e38, -3e38, 0.0, -0.0, np.inf, -np.inf])
        g = np.array(list(itertools.product(fin.tolist(), repeat=2)), dtype=np.uint32)
        parts.append((np.ascontiguousarray(g[:, 0]), np.ascontiguousarray(g[:, 1])))
    if op == "pow":                    # the uses in the kernels: moderate bases and exponents
        rng = np.random.default_rng(SEED + 10)
        x = rng.uniform(0.0, 4.0, 1 << 18).astype(np.float32)
        y = rng.uniform(-8.0, 8.0, 1 << 18).astype(np.float32)
        parts.append((f2u(x), f2u(y)))
        parts.append((f2u(-x[:4096]), f2u(y[:4096])))
    if op in ("div", "xdiv"):          # quotients that are exact, tie or sit next to a rounding boundary
        rng = np.random.default_rng(SEED + 11)
        b = rng.integers(1, 1 << 24, 1 << 18).astype(np.float32)
        q = rng.integers(1, 1 << 24, 1 << 18).astype(np.float32)
        parts.append((f2u(q * b), f2u(b)))
        parts.append((f2u(rng.integers(1, 1 << 24, 1 << 18).astype(np.float32)), f2u(b)))
    if op in ("min", "max", "clamp"):  # equal magnitudes and zeros of either sign
        z = f2u([0.0, -0.0, 1.0, -1.0])
        g = np.array(list(itertools.product(z.tolist(), repeat=k)), dtype=np.uint32)
        parts.append(tuple(np.ascontiguousarray(g[:, i]) for i in range(k)))
    if op == "mix":                    # the sampler's use: placements and a fract in [0, 1]
        rng = np.random.default_rng(SEED + 12)
        lo = rng.uniform(0, 1, 1 << 16).astype(np.float32)
        hi = rng.uniform(0, 1, 1 << 16).astype(np.float32)
        t = np.concatenate([rng.uniform(0, 1, (1 << 16) - 4).astype(np.float32), np.float32([0, 1, -0.0, 0.5])])
        parts.append((f2u(lo), f2u(hi), f2u(t)))
    return tuple(np.concatenate([p[i] for p in parts]).astype(np.uint32) for i in range(k))


def in_domain_mask(op: str, operands) -> np.ndarray:
    """Elements inside the op's documented domain (signalling NaNs apart)."""
    a = u2f(operands[0])
    with np.errstate(invalid="ignore"):
        if op in ("sin", "cos"):
            return np.abs(a) < np.float32(8192.0)
        if op == "rint":
            return np.abs(a) < np.float32(2.0 ** 22)
        if op == "pow":
            return ~(a < 0)
        if op == "floor_to_int":
            return (a >= np.float32(-2.0 ** 31)) & (a < np.float32(2.0 ** 31))
    return np.ones(len(a), dtype=bool)


@functools.lru_cache(maxsize=None)
def cases(op: str) -> dict:
    raw = _raw(op)
    n = len(raw[0])
    snan = np.zeros(n, dtype=bool)
    if op not in INTEGER_OPERAND:
        for x in raw:
            snan |= is_snan(x)
    dom = in_domain_mask(op, raw) if op not in INTEGER_OPERAND else np.ones(n, dtype=bool)
    out = {}
    for name, mask in (("in_domain", dom & ~snan), ("out_of_domain", ~dom & ~snan), ("snan", snan)):
        sel = tuple(np.ascontiguousarray(x[mask]) for x in raw)
        for x in sel:
            x.setflags(write=False)
        out[name] = sel
    return out


def ops():
    from path_tracer_amd import _native as N
    return N.NUMERICS_OPS
