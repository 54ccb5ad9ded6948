/*
 * pt_despike.h — the neighbourhood firefly clamp in front of the denoisers
 * (definition in DESIGN.md §6 row 12), written once for the device kernel
 * (csrc/hip/despike.hip) and the host implementation (csrc/scene/despike.cpp)
 * under pt_fp.h's convention: IEEE binary32, no contraction, IEEE /, the
 * window walked row-major.  Per-pixel and per-tap arithmetic only: the loop
 * over the image, the walk over the window (rows y - R .. y + R, columns
 * x - R .. x + R, the centre left out) and the store of the result are the
 * callers'.
 *
 * For a pixel p of an accumulator Src: its value v(p), the largest component
 * of its colour Src.xyz / Src.w; the members of its window (usable pixels
 * other than p that show p's surface by row 11's rule); t, the Rank-th
 * largest value among them; the limit L = Scale * t + Floor; and Src(p) with
 * its colour scaled by L / v(p) where v(p) > L, its bits otherwise.
 *
 * Open points, settled here:
 *
 * Signed zeros.  The order statistic compares values, and +0 and -0 are the
 * one pair of equal values with different bits: which of them ends up as t
 * depends on the order of insertion (and, in a restatement, on the sort).  t
 * enters the result through L alone, and Scale * t for t = +-0 is a zero, to
 * which + Floor gives Floor's bits when Floor > 0 and +0 when Floor is +0
 * (-0 + +0 = +0 in round-to-nearest).  Only Floor = -0 would let the zero's
 * sign through (-0 + -0 = -0, and then f = -0 and a clamped colour of -0
 * where the others give +0), so pt_despike_parameters_ok refuses a Floor
 * whose sign bit is set, -0 included.  Scale may be -0: it only ever reaches
 * the sum as the sign of a zero.
 *
 * Comparisons, not min/max.  The value v(q) and the insertion are written
 * with >, as the definition has them.  fminf / fmaxf would be admissible in
 * the insertion alone (all they could change is which zero is kept, which
 * the paragraph above shows not to reach the result); they are not used, so
 * that one text serves both sides.  v(q) must stay comparisons: its bits are
 * divided by and so reach the output (L / +0 and L / -0 differ).
 *
 * No NaN among members.  A member is usable: four finite components and
 * .w > 0.  A finite x over a finite w > 0 is finite, an infinity (overflow
 * under a denormal w) or a zero, never NaN: 0 / 0 and inf / inf need a zero
 * or infinite w.  So every comparison here is between ordered operands, the
 * sentinel -inf of a non-member included, and t is never NaN.  L may be: 0 *
 * inf when Scale is 0 and t infinite; L >= 0 is then false and the pixel
 * keeps its bits.
 */
#ifndef PT_DESPIKE_H
#define PT_DESPIKE_H

#include "pt_fp.h"
#include "pt_packed.h"
#include "pt_reproject.h"
#include "pt_rectify.h"

#define PT_DESPIKE_MAX_RADIUS 3
#define PT_DESPIKE_MAX_RANK   4

PT_HD int pt_despike_parameters_ok(const pt_despike_parameters* p)
{
    if (!(p->Radius >= 1u && p->Radius <= PT_DESPIKE_MAX_RADIUS)) return 0;
    const uint32_t side = 2u * p->Radius + 1u;
    return p->Rank >= 1u && p->Rank <= PT_DESPIKE_MAX_RANK && p->MinNeighbours >= p->Rank &&
           p->MinNeighbours <= side * side - 1u && p->Scale >= 0.0f && pt_reproject_finite(p->Scale) &&
           p->Floor >= 0.0f && pt_reproject_finite(p->Floor) && (pt_f2u(p->Floor) & 0x80000000u) == 0u &&
           p->NormalCosine > -1.0f && p->NormalCosine <= 1.0f;
}

/* -inf: below or equal to every value, so inserting it changes no register. */
#define PT_DESPIKE_NO_VALUE_BITS 0xFF800000u

/* What a tap needs of a window pixel q, five words: the guide's normal, the
 * shape word its guide shows, and its value.  A pixel that belongs to no
 * window whatever the centre (outside the image, or not usable) carries
 * PT_RECTIFY_NOT_A_MEMBER in the shape word, as in row 11's records (a
 * guide's shape is never that value), and -inf as its value.  A centre reads
 * its own record too: an unusable centre keeps its bits whatever its window
 * holds, so its surface is not needed. */
typedef struct pt_despike_record {
    float    normal[3];
    uint32_t member_shape;
    float    v;
} pt_despike_record;

/* Step 2 for a usable pixel: the largest component of src.xyz / src.w. */
PT_HD float pt_despike_value(const float* src)
{
    const float cx = src[0] / src[3], cy = src[1] / src[3], cz = src[2] / src[3];
    float v = cx;
    if (cy > v) v = cy;
    if (cz > v) v = cz;
    return v;
}

/* inside: q lies in the image; src, g are read only then. */
PT_HD void pt_despike_stage(int inside, const float* src, const pt_denoise_guide* g, pt_despike_record* r)
{
    r->normal[0] = 0.0f; r->normal[1] = 0.0f; r->normal[2] = 0.0f;
    r->member_shape = PT_RECTIFY_NOT_A_MEMBER;
    r->v = pt_u2f(PT_DESPIKE_NO_VALUE_BITS);
    if (!inside) return;
    if (!pt_reproject_history_ok(src)) return;
    r->normal[0] = g->normal[0]; r->normal[1] = g->normal[1]; r->normal[2] = g->normal[2];
    r->member_shape = g->shape;
    r->v = pt_despike_value(src);
}

/* q (not the centre) belongs to the window of a usable centre whose record
 * shows (shape, normal): row 11's rule with this call's NormalCosine. */
PT_HD int pt_despike_member(const pt_despike_parameters* p, uint32_t shape, const float* normal,
                            uint32_t member_shape, const float* q_normal)
{
    pt_rectify_parameters same_surface = {0u, 0u, 0.0f, 0.0f, p->NormalCosine};
    return pt_rectify_member(&same_surface, shape, normal, member_shape, q_normal);
}

/* The four largest values seen, a0 >= a1 >= a2 >= a3, and the number of
 * members.  Four named registers and no array: nothing here is indexed. */
typedef struct pt_despike_top { float a0, a1, a2, a3; uint32_t m; } pt_despike_top;

PT_HD void pt_despike_begin(pt_despike_top* T)
{
    T->a0 = T->a1 = T->a2 = T->a3 = pt_u2f(PT_DESPIKE_NO_VALUE_BITS);
    T->m = 0u;
}

/* *a keeps the larger of *a and *x, *x carries the smaller on; equal values
 * (zeros of either sign among them) stay where they are. */
PT_HD void pt_despike_sink(float* a, float* x)
{
    const int above = *x > *a;
    const float hi = above ? *x : *a;
    *x = above ? *a : *x;
    *a = hi;
}

/* One tap: a member's value sinks into the sorted registers; a non-member's
 * is replaced by -inf, which moves nothing, so that a tap is the same
 * instructions either way. */
PT_HD void pt_despike_insert(pt_despike_top* T, int member, float v)
{
    float x = member ? v : pt_u2f(PT_DESPIKE_NO_VALUE_BITS);
    T->m = T->m + (member ? 1u : 0u);
    pt_despike_sink(&T->a0, &x);
    pt_despike_sink(&T->a1, &x);
    pt_despike_sink(&T->a2, &x);
    pt_despike_sink(&T->a3, &x);
}

/* Steps 4 to 6 after the window pass.  src: the centre's four components; v:
 * its value (read only where src is usable).  out may be src. */
PT_HD void pt_despike_decide(const pt_despike_parameters* p, const float* src, float v, const pt_despike_top* T,
                             float* out)
{
    const float S[4] = {src[0], src[1], src[2], src[3]};
    out[0] = S[0]; out[1] = S[1]; out[2] = S[2]; out[3] = S[3];
    if (!pt_reproject_history_ok(S)) return;
    if (T->m < p->MinNeighbours) return;
    /* m >= MinNeighbours >= Rank: register Rank - 1 holds a member's value. */
    /* All four read first and one chosen by value: chosen by address, the
     * registers would have to live in memory. */
    const float a0 = T->a0, a1 = T->a1, a2 = T->a2, a3 = T->a3;
    const float t = p->Rank == 1u ? a0 : (p->Rank == 2u ? a1 : (p->Rank == 3u ? a2 : a3));
    const float L = p->Scale * t + p->Floor;
    if (!(L >= 0.0f)) return;
    if (!(v > L)) return;
    const float f = L / v;
    out[0] = S[0] * f; out[1] = S[1] * f; out[2] = S[2] * f;
}

#endif /* PT_DESPIKE_H */
