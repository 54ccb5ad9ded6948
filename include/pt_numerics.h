/*
 * pt_numerics.h — the operations of the numerics probe.
 *
 * ptEvalNumerics (pt_api.h) evaluates one of these operations on the device
 * over caller-given operand bit patterns; oracle_fp_eval (oracle/pt_oracle.h)
 * does the same on the host.  Both call the functions of pt_fp.h as product
 * code does, through pt_numerics_eval below, so a test can hold the two
 * sides' result bits against each other at chosen inputs (tests/
 * numerics_cases.py, tests/test_gpu_numerics.py).  The unit-vector packing
 * and the device-only division helpers live outside pt_fp.h; each side adds
 * them from its own source (pt_device.hpp, pt_oracle.cpp).
 *
 * Operands and results are 32-bit words: a float's bit pattern, or the
 * integer itself.  An operation reads pt_numerics_operands(op) operand arrays
 * and writes pt_numerics_outputs(op) words per element, element i at
 * out[i * outputs + j].  tests/test_abi.py keeps the Python list
 * (path-tracer_amd/_native.py NUMERICS_OPS) equal to this enum.
 */
#ifndef PT_NUMERICS_H
#define PT_NUMERICS_H

#include "pt_fp.h"

enum {
    /* arithmetic as the compiler lowers it */
    PT_NUM_ADD = 0,               /* a + b */
    PT_NUM_MUL = 1,               /* a * b */
    PT_NUM_DIV = 2,               /* a / b */
    PT_NUM_SQRT = 3,              /* pt_sqrt(a) */
    PT_NUM_FMA = 4,               /* pt_fma(a, b, c) */
    PT_NUM_MIN = 5,               /* pt_min(a, b) */
    PT_NUM_MAX = 6,               /* pt_max(a, b) */
    PT_NUM_CLAMP = 7,             /* pt_clamp(a, b, c) */
    PT_NUM_FLOOR = 8,
    PT_NUM_FRACT = 9,
    PT_NUM_RINT = 10,
    PT_NUM_ROUND_HALF_AWAY = 11,
    PT_NUM_MIX = 12,              /* pt_mix(a, b, c) */
    /* transcendentals */
    PT_NUM_EXP = 13,
    PT_NUM_LOG = 14,
    PT_NUM_POW = 15,              /* pt_pow(a, b) */
    PT_NUM_SIN = 16,
    PT_NUM_COS = 17,
    PT_NUM_ATAN2 = 18,            /* pt_atan2(a, b): a = y, b = x */
    PT_NUM_ASIN = 19,
    /* conversions the kernels use */
    PT_NUM_U32_TO_FLOAT = 20,     /* (float)a for the integer a */
    PT_NUM_FLOOR_TO_INT = 21,     /* (int)pt_floor(a), as SampleTexture converts */
    PT_NUM_RANDOM = 22,           /* pt_random: state a -> {new state, value} */
    PT_NUM_RANDOM01 = 23,         /* pt_random01 of state a */
    /* packing */
    PT_NUM_PACK_SNORM16 = 24,
    PT_NUM_UNPACK_SNORM16 = 25,
    PT_NUM_HALF_TO_FLOAT = 26,
    PT_NUM_PACK_UNIT_VECTOR = 27,   /* PackUnitVector(a, b, c) */
    PT_NUM_UNPACK_UNIT_VECTOR = 28, /* UnpackUnitVector(a) -> {x, y, z} */
    /* device-only forms (pt_device.hpp); the host has no counterpart */
    PT_NUM_FAST_RCP = 29,         /* FastRcp(a) */
    PT_NUM_XDIV = 30,             /* XDiv(a, b, RecipForDiv(b)) */
    PT_NUM_OP_COUNT = 31,
};

/* Operand arrays an operation reads (0 for an unknown op). */
PT_HD uint32_t pt_numerics_operands(uint32_t op)
{
    switch (op) {
        case PT_NUM_FMA: case PT_NUM_CLAMP: case PT_NUM_MIX: case PT_NUM_PACK_UNIT_VECTOR:
            return 3;
        case PT_NUM_ADD: case PT_NUM_MUL: case PT_NUM_DIV: case PT_NUM_MIN: case PT_NUM_MAX: case PT_NUM_POW:
        case PT_NUM_ATAN2: case PT_NUM_XDIV:
            return 2;
        default:
            return op < PT_NUM_OP_COUNT ? 1u : 0u;
    }
}

/* Result words per element (0 for an unknown op). */
PT_HD uint32_t pt_numerics_outputs(uint32_t op)
{
    if (op == PT_NUM_RANDOM) return 2;
    if (op == PT_NUM_UNPACK_UNIT_VECTOR) return 3;
    return op < PT_NUM_OP_COUNT ? 1u : 0u;
}

/* The operations pt_fp.h defines.  Returns 0, writing nothing, for the
 * others (unit vectors, device-only forms, unknown ids). */
PT_HD int pt_numerics_eval(uint32_t op, uint32_t ua, uint32_t ub, uint32_t uc, uint32_t* out)
{
    const float a = pt_u2f(ua), b = pt_u2f(ub), c = pt_u2f(uc);
    switch (op) {
        case PT_NUM_ADD: out[0] = pt_f2u(a + b); return 1;
        case PT_NUM_MUL: out[0] = pt_f2u(a * b); return 1;
        case PT_NUM_DIV: out[0] = pt_f2u(a / b); return 1;
        case PT_NUM_SQRT: out[0] = pt_f2u(pt_sqrt(a)); return 1;
        case PT_NUM_FMA: out[0] = pt_f2u(pt_fma(a, b, c)); return 1;
        case PT_NUM_MIN: out[0] = pt_f2u(pt_min(a, b)); return 1;
        case PT_NUM_MAX: out[0] = pt_f2u(pt_max(a, b)); return 1;
        case PT_NUM_CLAMP: out[0] = pt_f2u(pt_clamp(a, b, c)); return 1;
        case PT_NUM_FLOOR: out[0] = pt_f2u(pt_floor(a)); return 1;
        case PT_NUM_FRACT: out[0] = pt_f2u(pt_fract(a)); return 1;
        case PT_NUM_RINT: out[0] = pt_f2u(pt_rint(a)); return 1;
        case PT_NUM_ROUND_HALF_AWAY: out[0] = pt_f2u(pt_round_half_away(a)); return 1;
        case PT_NUM_MIX: out[0] = pt_f2u(pt_mix(a, b, c)); return 1;
        case PT_NUM_EXP: out[0] = pt_f2u(pt_exp(a)); return 1;
        case PT_NUM_LOG: out[0] = pt_f2u(pt_log(a)); return 1;
        case PT_NUM_POW: out[0] = pt_f2u(pt_pow(a, b)); return 1;
        case PT_NUM_SIN: out[0] = pt_f2u(pt_sin(a)); return 1;
        case PT_NUM_COS: out[0] = pt_f2u(pt_cos(a)); return 1;
        case PT_NUM_ATAN2: out[0] = pt_f2u(pt_atan2(a, b)); return 1;
        case PT_NUM_ASIN: out[0] = pt_f2u(pt_asin(a)); return 1;
        case PT_NUM_U32_TO_FLOAT: out[0] = pt_f2u((float)ua); return 1;
        case PT_NUM_FLOOR_TO_INT: out[0] = (uint32_t)(int)pt_floor(a); return 1;
        case PT_NUM_RANDOM: { uint32_t s = ua; uint32_t v = pt_random(&s); out[0] = s; out[1] = v; return 1; }
        case PT_NUM_RANDOM01: { uint32_t s = ua; out[0] = pt_f2u(pt_random01(&s)); return 1; }
        case PT_NUM_PACK_SNORM16: out[0] = pt_pack_snorm16(a); return 1;
        case PT_NUM_UNPACK_SNORM16: out[0] = pt_f2u(pt_unpack_snorm16(ua)); return 1;
        case PT_NUM_HALF_TO_FLOAT: out[0] = pt_f2u(pt_half_to_float(ua)); return 1;
        default: return 0;
    }
}

#endif /* PT_NUMERICS_H */
