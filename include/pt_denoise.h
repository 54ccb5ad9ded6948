/*
 * pt_denoise.h — the edge-avoiding a-trous filter's per-tap arithmetic
 * (Dammertz et al. 2010; definition in DESIGN.md §6), written once for the
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

/* Weight of tap q seen from pixel p (same shape; the caller has skipped every
 * other tap): h * exp(-(((dc + da) + dn) + dz)). */
PT_HD float pt_denoise_weight(float h, const pt_denoise_pixel* p, const pt_denoise_pixel* q, const pt_denoise_sigmas* s)
{
    float dc = pt_dn_dist2(p->c, q->c) / s->color2;
    float da = pt_dn_dist2(p->a, q->a) / s->albedo2;
    float dn = 0.0f, dz = 0.0f;
    if (p->shape != PT_SHAPE_INDEX_NONE) {
        float d = (p->n.x * q->n.x + p->n.y * q->n.y) + p->n.z * q->n.z;
        dn = pt_max(0.0f, 1.0f - d) / s->normal;
        dz = pt_abs(p->t - q->t) / (s->depth * pt_max(p->t, 1e-6f));
    }
    return h * pt_exp(-(((dc + da) + dn) + dz));
}

PT_HD int pt_denoise_parameters_ok(const pt_denoise_parameters* p)
{
    return p->Iterations <= PT_DENOISE_MAX_ITERATIONS && p->SigmaColor > 0.0f && p->SigmaNormal > 0.0f &&
           p->SigmaDepth > 0.0f && p->SigmaAlbedo > 0.0f;
}

#endif /* PT_DENOISE_H */
