/*
 * pt_denoise.h — the edge-avoiding a-trous filter's per-tap arithmetic
 * (Dammertz et al. 2010; definition in DESIGN.md §6) and that of its
 * variance-guided form over two half renders (row 7), written once for the
 * device kernels (csrc/hip/denoise.hip) and the host implementation
 * (csrc/scene/denoise.cpp) under pt_fp.h's convention: IEEE binary32, no
 * contraction, sums left to right, pt_exp.  No filter logic beyond one tap
 * lives here: the tap loop, its order and the skip rules are the callers'.
 */
#ifndef PT_DENOISE_H
#define PT_DENOISE_H

#include "pt_fp.h"
#include "pt_packed.h"

typedef struct pt_dn3 { float x, y, z; } pt_dn3;

/* One pixel as the filter sees it: its colour in the current iteration and
 * its guide record. */
typedef struct pt_denoise_pixel {
    pt_dn3   c;
    pt_dn3   n;
    float    t;
    pt_dn3   a;
    uint32_t shape;
} pt_denoise_pixel;

/* The per-call constants of one iteration. */
typedef struct pt_denoise_sigmas {
    float color2;       /* (SigmaColor * 2^-i)^2 */
    float albedo2;      /* SigmaAlbedo^2 */
    float normal;
    float depth;
} pt_denoise_sigmas;

/* B3 spline taps {1/16, 1/4, 3/8, 1/4, 1/16}, i = d + 2. */
PT_HD float pt_denoise_k(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

/* Iteration i's constants; the colour sigma is scaled by 2^-i, an exact
 * power of two (i <= PT_DENOISE_MAX_ITERATIONS). */
PT_HD pt_denoise_sigmas pt_denoise_iteration_sigmas(const pt_denoise_parameters* p, uint32_t i)
{
    pt_denoise_sigmas s;
    float sc = p->SigmaColor * pt_pow2i(-(int)i);
    s.color2 = sc * sc;
    s.albedo2 = p->SigmaAlbedo * p->SigmaAlbedo;
    s.normal = p->SigmaNormal;
    s.depth = p->SigmaDepth;
    return s;
}

PT_HD float pt_dn_dist2(pt_dn3 a, pt_dn3 b)
{
    float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

/* The guide terms of tap q seen from pixel p (same shape): albedo, normal
 * and depth distances; dn = dz = 0 on misses. */
PT_HD void pt_denoise_guide_terms(const pt_denoise_pixel* p, const pt_denoise_pixel* q, float albedo2, float normal,
                                  float depth, float* da, float* dn, float* dz)
{
    *da = pt_dn_dist2(p->a, q->a) / albedo2;
    *dn = 0.0f;
    *dz = 0.0f;
    if (p->shape != PT_SHAPE_INDEX_NONE) {
        float d = (p->n.x * q->n.x + p->n.y * q->n.y) + p->n.z * q->n.z;
        *dn = pt_max(0.0f, 1.0f - d) / normal;
        *dz = pt_abs(p->t - q->t) / (depth * pt_max(p->t, 1e-6f));
    }
}

/* Weight of tap q seen from pixel p (same shape; the caller has skipped every
 * other tap): h * exp(-(((dc + da) + dn) + dz)). */
PT_HD float pt_denoise_weight(float h, const pt_denoise_pixel* p, const pt_denoise_pixel* q, const pt_denoise_sigmas* s)
{
    float dc = pt_dn_dist2(p->c, q->c) / s->color2;
    float da, dn, dz;
    pt_denoise_guide_terms(p, q, s->albedo2, s->normal, s->depth, &da, &dn, &dz);
    return h * pt_exp(-(((dc + da) + dn) + dz));
}

PT_HD int pt_denoise_parameters_ok(const pt_denoise_parameters* p)
{
    return p->Iterations <= PT_DENOISE_MAX_ITERATIONS && p->SigmaColor > 0.0f && p->SigmaNormal > 0.0f &&
           p->SigmaDepth > 0.0f && p->SigmaAlbedo > 0.0f;
}

/* --- the variance-guided filter over two half renders ---
 *
 * Per-pixel and per-tap arithmetic of ptDenoiseSampleBufferPair / ptsDenoisePair.
 * As above, the tap loops, their order and the skip rules are the callers'. */

/* A pixel of the combined frame S = A + B: filled iff S.w > 0; c = S.xyz / S.w;
 * v = the raw variance of the combined mean's luminance (c.y). */
typedef struct pt_denoise_pair_start {
    pt_dn3 c;
    float  v;
    int    filled;
} pt_denoise_pair_start;

PT_HD pt_denoise_pair_start pt_denoise_pair_begin(const float* a, const float* b)
{
    pt_denoise_pair_start s;
    float sx = a[0] + b[0], sy = a[1] + b[1], sz = a[2] + b[2], sw = a[3] + b[3];
    s.filled = sw > 0.0f;
    s.c.x = 0.0f; s.c.y = 0.0f; s.c.z = 0.0f;
    s.v = 0.0f;
    if (!s.filled) return s;
    s.c.x = sx / sw; s.c.y = sy / sw; s.c.z = sz / sw;
    if (a[3] > 0.0f && b[3] > 0.0f) {
        float d = (a[1] / a[3] - b[1] / b[3]) * 0.5f;
        s.v = d * d;
    } else {
        s.v = s.c.y * s.c.y;        /* one half only: no estimate, so the mean itself */
    }
    return s;
}

/* The 3x3 variance prefilter's taps {1/4, 1/2, 1/4}, i = d + 1. */
PT_HD float pt_denoise_k3(int i) { return i == 1 ? 0.5f : 0.25f; }

/* The per-call constants of the pair filter (the same in every iteration). */
typedef struct pt_denoise_pair_sigmas {
    float luminance;
    float albedo2;      /* SigmaAlbedo^2 */
    float normal;
    float depth;
} pt_denoise_pair_sigmas;

PT_HD pt_denoise_pair_sigmas pt_denoise_pair_make_sigmas(const pt_denoise_pair_parameters* p)
{
    pt_denoise_pair_sigmas s;
    s.luminance = p->SigmaLuminance;
    s.albedo2 = p->SigmaAlbedo * p->SigmaAlbedo;
    s.normal = p->SigmaNormal;
    s.depth = p->SigmaDepth;
    return s;
}

/* The luminance edge-stop's denominator at a centre of variance v. */
PT_HD float pt_denoise_pair_scale(const pt_denoise_pair_sigmas* s, float v)
{
    return s->luminance * pt_sqrt(pt_max(v, 0.0f)) + 1e-10f;
}

/* Weight of tap q seen from pixel p (same shape), D = pt_denoise_pair_scale
 * of p's variance: h * exp(-(((dl + da) + dn) + dz)). */
PT_HD float pt_denoise_pair_weight(float h, const pt_denoise_pixel* p, const pt_denoise_pixel* q, float D,
                                   const pt_denoise_pair_sigmas* s)
{
    float dl = pt_abs(p->c.y - q->c.y) / D;
    float da, dn, dz;
    pt_denoise_guide_terms(p, q, s->albedo2, s->normal, s->depth, &da, &dn, &dz);
    return h * pt_exp(-(((dl + da) + dn) + dz));
}

PT_HD int pt_denoise_pair_parameters_ok(const pt_denoise_pair_parameters* p)
{
    return p->Iterations <= PT_DENOISE_MAX_ITERATIONS && p->SigmaLuminance > 0.0f && p->SigmaNormal > 0.0f &&
           p->SigmaDepth > 0.0f && p->SigmaAlbedo > 0.0f;
}

#endif /* PT_DENOISE_H */
