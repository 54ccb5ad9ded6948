/*
 * pt_rectify.h — validation of a carried history against the new frame's
 * samples (variance clipping, Salvi 2016; definition in DESIGN.md §6 row 11),
 * written once for the device kernel (csrc/hip/rectify.hip) and the host
 * implementation (csrc/scene/rectify.cpp) under pt_fp.h's convention: IEEE
 * binary32, no contraction, IEEE / and sqrt, sums in window order.  Per-pixel
 * and per-tap arithmetic only: the loop over the image, the walk over the
 * window (rows y - R .. y + R, columns x - R .. x + R, row-major) and the
 * store of the result are the callers'.
 *
 * For a pixel: the members of its window (pixels of the new accumulator that
 * are filled and show the centre's surface), the mean and the standard
 * deviation of their colours, the box mean +- Sigma deviations, and the
 * history's mean colour pulled into that box with its sample count cut where
 * it had to be pulled.
 */
#ifndef PT_RECTIFY_H
#define PT_RECTIFY_H

#include "pt_fp.h"
#include "pt_packed.h"
#include "pt_reproject.h"

#define PT_RECTIFY_MAX_RADIUS 3

PT_HD int pt_rectify_parameters_ok(const pt_rectify_parameters* p)
{
    const uint32_t side = 2u * PT_RECTIFY_MAX_RADIUS + 1u;
    return p->Radius >= 1u && p->Radius <= PT_RECTIFY_MAX_RADIUS && p->MinNeighbours >= 1u &&
           p->MinNeighbours <= side * side && p->Sigma >= 0.0f && pt_reproject_finite(p->Sigma) &&
           p->ClampedHistory > 0.0f && p->NormalCosine > -1.0f && p->NormalCosine <= 1.0f;
}

/* What a tap needs of a window pixel q, 32 bytes in two 16-byte halves: its
 * colour Cur(q).xyz / Cur(q).w with the shape word its guide shows, and the
 * guide's normal with the same shape word again.  A pixel that belongs to no
 * window whatever the centre (outside the image, or not ok(Cur)) carries
 * PT_RECTIFY_NOT_A_MEMBER in the first half's shape word, so that a tap has
 * one test; a guide's shape is <= 0xFFFF or PT_SHAPE_INDEX_NONE, never that
 * value.  The second half keeps the guide's own shape word: a centre reads
 * its surface from there, and is tested through its neighbours even where its
 * own new sample is unusable. */
#define PT_RECTIFY_NOT_A_MEMBER 0xFFFFFFFEu

typedef struct pt_rectify_record {
    float    c[3];
    uint32_t member_shape;
    float    normal[3];
    uint32_t shape;
} pt_rectify_record;

/* inside: q lies in the image; cur, g are read only then. */
PT_HD void pt_rectify_stage(int inside, const float* cur, const pt_denoise_guide* g, pt_rectify_record* r)
{
    r->c[0] = 0.0f; r->c[1] = 0.0f; r->c[2] = 0.0f;
    r->member_shape = PT_RECTIFY_NOT_A_MEMBER;
    r->normal[0] = 0.0f; r->normal[1] = 0.0f; r->normal[2] = 0.0f;
    r->shape = PT_RECTIFY_NOT_A_MEMBER;
    if (!inside) return;
    r->normal[0] = g->normal[0]; r->normal[1] = g->normal[1]; r->normal[2] = g->normal[2];
    r->shape = g->shape;
    if (!pt_reproject_history_ok(cur)) return;
    r->c[0] = cur[0] / cur[3]; r->c[1] = cur[1] / cur[3]; r->c[2] = cur[2] / cur[3];
    r->member_shape = g->shape;
}

/* q belongs to the window of a centre that shows (shape, normal). */
PT_HD int pt_rectify_member(const pt_rectify_parameters* p, uint32_t shape, const float* normal,
                            uint32_t member_shape, const float* q_normal)
{
    if (member_shape != shape) return 0;
    if (shape == PT_SHAPE_INDEX_NONE) return 1;
    float d = (q_normal[0] * normal[0] + q_normal[1] * normal[1]) + q_normal[2] * normal[2];
    return d >= p->NormalCosine;
}

/* The two window passes.  S starts at -0: -0 + c has c's bits for every c, so
 * the sum starts from the first member as the definition has it.  D's terms
 * are squares (+0 or greater, or NaN), for which 0 + t = t. */
typedef struct pt_rectify_sums { float S[3]; float D[3]; uint32_t m; } pt_rectify_sums;

PT_HD void pt_rectify_begin(pt_rectify_sums* A)
{
    A->S[0] = -0.0f; A->S[1] = -0.0f; A->S[2] = -0.0f;
    A->D[0] = 0.0f; A->D[1] = 0.0f; A->D[2] = 0.0f;
    A->m = 0u;
}

PT_HD void pt_rectify_add_colour(pt_rectify_sums* A, const float* c)
{
    A->S[0] = A->S[0] + c[0];
    A->S[1] = A->S[1] + c[1];
    A->S[2] = A->S[2] + c[2];
    A->m = A->m + 1u;
}

/* After the first pass, m > 0. */
PT_HD void pt_rectify_mean(const pt_rectify_sums* A, float* mu)
{
    const float m = (float)A->m;
    mu[0] = A->S[0] / m; mu[1] = A->S[1] / m; mu[2] = A->S[2] / m;
}

PT_HD void pt_rectify_add_deviation(pt_rectify_sums* A, const float* mu, const float* c)
{
    const float d0 = c[0] - mu[0], d1 = c[1] - mu[1], d2 = c[2] - mu[2];
    A->D[0] = A->D[0] + d0 * d0;
    A->D[1] = A->D[1] + d1 * d1;
    A->D[2] = A->D[2] + d2 * d2;
}

/* Step 3's decision, which needs the first pass only: 0 with out written
 * (no usable history: zeros; too few members: the history's bits), 1 when
 * the second pass and pt_rectify_clip follow. */
PT_HD int pt_rectify_tested(const pt_rectify_parameters* p, const float* hist, uint32_t m, float* out)
{
    if (!pt_reproject_history_ok(hist)) {
        out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = 0.0f;
        return 0;
    }
    if (m < p->MinNeighbours) {
        out[0] = hist[0]; out[1] = hist[1]; out[2] = hist[2]; out[3] = hist[3];
        return 0;
    }
    return 1;
}

/* Steps 4 and 5 after both passes, for a pixel pt_rectify_tested returned 1
 * for.  hist may be out. */
PT_HD void pt_rectify_clip(const pt_rectify_parameters* p, const float* hist, const pt_rectify_sums* A,
                           const float* mu, float* out)
{
    const float H[4] = {hist[0], hist[1], hist[2], hist[3]};
    const float m = (float)A->m;
    float sd[3], hc[3];
    int finite = 1, moved = 0;
    for (int j = 0; j < 3; j++) {
        sd[j] = pt_sqrt(A->D[j] / m);
        finite = finite && pt_reproject_finite(mu[j]) && pt_reproject_finite(sd[j]);
    }
    out[0] = H[0]; out[1] = H[1]; out[2] = H[2]; out[3] = H[3];
    if (!finite) return;
    const float n = H[3];
    for (int j = 0; j < 3; j++) {
        const float h = H[j] / n;
        const float e = p->Sigma * sd[j];
        const float lo = mu[j] - e, hi = mu[j] + e;
        /* pt_min(pt_max(h, lo), hi) of operands that are never NaN, lo <= hi,
         * written as comparisons: where h and a bound are zeros of either
         * sign, minNum / maxNum may return either and this keeps h. */
        const float t = h < lo ? lo : h;
        hc[j] = t > hi ? hi : t;
        moved = moved || !(hc[j] == h);
    }
    if (!moved) return;
    const float nc = pt_min(n, p->ClampedHistory);
    out[0] = hc[0] * nc; out[1] = hc[1] * nc; out[2] = hc[2] * nc; out[3] = nc;
}

#endif /* PT_RECTIFY_H */
