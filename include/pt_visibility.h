/*
 * pt_visibility.h — the rays of the ambient-occlusion / sky-visibility image
 * (definition in DESIGN.md §6 row 14), written once for the device kernel
 * (csrc/hip/occlusion.hip, ambient_occlusion_kernel) and for the host helper
 * the tests compare it with (csrc/scene/visibility.cpp,
 * ptsAmbientOcclusionRays; restated in numpy in
 * tests/visibility_restatement.py) under pt_fp.h's convention: IEEE binary32,
 * no contraction, sums left to right, pt_sqrt / pt_sin / pt_cos.  Per-pixel
 * arithmetic only: the primary trace, the hit's attributes, the any-hit
 * traces and the store of the pixel are the caller's.
 *
 * A pixel (x, y) of a w x h frame, parameters {Samples S, Radius, Seed}:
 *
 *   primary ray  (O, V) = pt_reproject_central_ray, duration PT_HIT_TIME_LIMIT,
 *                closest hit at time t; Nq = unpack(pack(N)) of the hit's
 *                normal: ptRenderDenoiseGuides' ray and normal.
 *   miss, or an unknown camera model: the pixel is (S, S, S, S).
 *   hit:  N  = dot(Nq, V) > 0 ? -Nq : Nq       (the side the ray came from;
 *                a NaN dot keeps Nq)
 *         X, Y = ComputeCoordinateFrame(N)     (common.glsl.inc:120-125, the
 *                frame basic_scatter builds around a direction)
 *         state = pt_seed(x, y, Seed)          (the integrator's stream seed
 *                of pixel (x, y) in frame Seed: basic_scatter.glsl:315-318)
 *         P  = O + t V
 *         for k = 0 .. S-1, in this order, two draws each:
 *           D  = RandomDirection(state)        (common.glsl.inc:212-218)
 *           L  = SafeNormalize(D + (0, 0, 1))  (basic_diffuse's cosine lobe)
 *           W  = (L.x X + L.y Y) + L.z N
 *           ray k: origin P + 1e-3 W, velocity unpack(pack(W))
 *                (pt_guide_restart, basic_scatter.glsl's restart), duration
 *                pt_visibility_duration(Radius)
 *         u = the number of the S rays with nothing within their duration
 *         the pixel is (u, u, u, S).
 *
 * pt_visibility_duration: a Radius at or beyond PT_HIT_TIME_LIMIT (+inf
 * included) is PT_HIT_TIME_LIMIT, every integrator ray's duration: visibility
 * of the sky.
 *
 * Nothing here traps or leaves the float domain on any input: a zero or NaN
 * normal gives a NaN frame and NaN rays, whose packed velocity is still a
 * defined word and whose traversal ends as any ray's does.
 */
#ifndef PT_VISIBILITY_H
#define PT_VISIBILITY_H

#include "pt_fp.h"
#include "pt_glsl.h"
#include "pt_packed.h"
#include "pt_reproject.h"
#include "pt_guides.h"

#define PT_AMBIENT_OCCLUSION_MAX_SAMPLES 64u

/* Samples in 1..64; Radius > 0 (a NaN is not). */
PT_HD int pt_visibility_parameters_ok(const pt_ambient_occlusion_parameters* p)
{
    return p->Samples >= 1u && p->Samples <= PT_AMBIENT_OCCLUSION_MAX_SAMPLES && p->Radius > 0.0f;
}

PT_HD float pt_visibility_duration(float Radius) { return Radius < PT_HIT_TIME_LIMIT ? Radius : PT_HIT_TIME_LIMIT; }

PT_HD uint32_t pt_visibility_seed(uint32_t x, uint32_t y, uint32_t Seed) { return pt_seed(x, y, Seed); }

/* SafeNormalize (common.glsl.inc:93-100). */
PT_HD pt3 pt_visibility_safe_normalize(pt3 V)
{
    const float LenSq = dot(V, V);
    if (LenSq < 1e-12f) return v3(0, 0, 1);
    return V / pt_sqrt(LenSq);
}

/* RandomDirection (common.glsl.inc:212-218): two draws. */
PT_HD pt3 pt_visibility_random_direction(uint32_t* state)
{
    const float Z = 2 * pt_random01(state) - 1;
    const float R = pt_sqrt(1 - Z * Z);
    const float Phi = PT_TAU * pt_random01(state);
    return v3(R * pt_cos(Phi), R * pt_sin(Phi), Z);
}

/* The shading frame of a hit: N facing the side the primary ray came from,
 * and ComputeCoordinateFrame's X, Y around it. */
typedef struct pt_visibility_frame {
    pt3 X, Y, N;
} pt_visibility_frame;

PT_HD pt_visibility_frame pt_visibility_make_frame(pt3 Nq, pt3 V)
{
    pt_visibility_frame F;
    F.N = dot(Nq, V) > 0.0f ? -Nq : Nq;
    const pt3 A = pt_abs(F.N.x) < 0.9f ? v3(1, 0, 0) : v3(0, 1, 0);
    F.X = normalize(cross(A, F.N));
    F.Y = cross(F.X, F.N);
    return F;
}

/* The next sample ray of a pixel whose primary ray (O, V) hit at time t: its
 * origin, and its velocity as the packed word (pt_guide_restart's ray; the
 * velocity traced is pt_reproject_unpack_unit of the word). */
PT_HD uint32_t pt_visibility_ray(const pt_visibility_frame* F, pt3 O, pt3 V, float t, uint32_t* state, pt3* RO)
{
    const pt3 D = pt_visibility_random_direction(state);
    const pt3 L = pt_visibility_safe_normalize(D + v3(0, 0, 1));
    const pt3 W = (L.x * F->X + L.y * F->Y) + L.z * F->N;
    const pt3 Pos = O + t * V;
    *RO = Pos + PT_GUIDE_RESTART_OFFSET * W;
    return pt_reproject_pack_unit(W);
}

/* --- visibility gathered at caller-given points ---------
 *
 * The device kernel is visibility_gather_kernel (csrc/hip/occlusion.hip), the
 * host twins ptsGatherVisibilityRays / ptsGatherVisibilityReduce
 * (csrc/scene/visibility.cpp), the numpy restatement
 * tests/gather_restatement.py.
 *
 * Point i of n, position P and normal N as given (neither normalised nor
 * quantised), parameters {Samples S, Radius, Seed, Offset, FirstIndex}:
 *
 *   j  = FirstIndex + i
 *   s0 = pt_seed(j & 0xFFFF, j >> 16, Seed)   (injective in (x < 65536, y): the
 *            points' streams do not collide)
 *   frame: F.N = N; X, Y as pt_visibility_make_frame derives them from F.N
 *   sample k = 0 .. S-1:
 *     state = s0 advanced by 2 k steps of pt_random's LCG (pt_visibility_skip)
 *     D = RandomDirection(state); L = SafeNormalize(D + (0, 0, 1))
 *     W = (L.x X + L.y Y) + L.z N
 *     ray k: origin P + Offset W (multiply, then add, per component), velocity
 *            unpack(pack(W)), duration pt_visibility_duration(Radius)
 *   occ_k = whether anything lies within ray k's duration
 *   record (pt_visibility_record): OccludedMask bit k = occ_k; Unoccluded =
 *     S - popcount; Samples = S; Reserved = 0; Bent = the component-wise
 *     pairwise sum of b_k = occ_k ? (0, 0, 0) : velocity_k, b'_m = b_2m +
 *     b_2m+1 for log2 S levels (float addition is commutative, so the tree
 *     has one result whichever operand a lane holds).
 *
 * A point's first S' rays are the rays of Samples = S' (nesting), and a call
 * on points [a, b) with FirstIndex = a equals that slice of the whole call
 * (partition independence). */

#define PT_VISIBILITY_GATHER_MAX_POINTS (1u << 26)
#define PT_VISIBILITY_GATHER_MAX_LANES (1u << 22)   /* (point, sample) pairs of one launch */

/* Samples a power of two in 1..64; Radius > 0 (a NaN is not); Offset finite and
 * >= 0; n <= 2^26 and FirstIndex + n <= 2^32. */
PT_HD int pt_visibility_gather_parameters_ok(const pt_visibility_gather_parameters* p, uint32_t n)
{
    const uint32_t S = p->Samples;
    if (S < 1u || S > PT_AMBIENT_OCCLUSION_MAX_SAMPLES || (S & (S - 1u)) != 0u) return 0;
    if (!(p->Radius > 0.0f)) return 0;
    if (!(p->Offset >= 0.0f && p->Offset <= 3.402823466e+38f)) return 0;
    if (n > PT_VISIBILITY_GATHER_MAX_POINTS) return 0;
    return (uint64_t)p->FirstIndex + (uint64_t)n <= 4294967296ull;
}

/* `state` after `steps` steps of pt_random's LCG (x -> 747796405 x +
 * 2891336453 mod 2^32), in log2(steps) rounds: the composition of affine maps
 * by repeated squaring, all in exact arithmetic mod 2^32, so it equals
 * sequential stepping bit for bit. */
PT_HD uint32_t pt_visibility_skip(uint32_t state, uint32_t steps)
{
    uint32_t a = 747796405u, c = 2891336453u;   /* the map of 2^r steps */
    uint32_t A = 1u, C = 0u;                    /* the map of the steps taken so far */
    while (steps != 0u) {
        if (steps & 1u) {
            A = A * a;
            C = C * a + c;
        }
        c = (a + 1u) * c;
        a = a * a;
        steps >>= 1u;
    }
    return A * state + C;
}

PT_HD uint32_t pt_visibility_gather_seed(uint32_t j, uint32_t Seed) { return pt_seed(j & 0xFFFFu, j >> 16u, Seed); }

/* The frame around a point's normal, used as given: pt_visibility_make_frame's
 * X and Y around F.N = N. */
PT_HD pt_visibility_frame pt_visibility_gather_frame(pt3 N)
{
    pt_visibility_frame F;
    F.N = N;
    const pt3 A = pt_abs(F.N.x) < 0.9f ? v3(1, 0, 0) : v3(0, 1, 0);
    F.X = normalize(cross(A, F.N));
    F.Y = cross(F.X, F.N);
    return F;
}

/* Sample k of the point at P whose stream starts at s0: its origin, and its
 * velocity as the packed word (the velocity traced is pt_reproject_unpack_unit
 * of the word). */
PT_HD uint32_t pt_visibility_gather_ray(const pt_visibility_frame* F, pt3 P, float Offset, uint32_t s0, uint32_t k,
                                        pt3* RO)
{
    uint32_t state = pt_visibility_skip(s0, 2u * k);
    const pt3 D = pt_visibility_random_direction(&state);
    const pt3 L = pt_visibility_safe_normalize(D + v3(0, 0, 1));
    const pt3 W = (L.x * F->X + L.y * F->Y) + L.z * F->N;
    *RO = P + Offset * W;
    return pt_reproject_pack_unit(W);
}

/* A point's record from its S packed velocities and its occluded bits: the
 * tree the device kernel's cross-lane rounds form. */
PT_HD pt_visibility_record pt_visibility_reduce(uint32_t S, const uint32_t* packed, uint64_t occluded)
{
    pt3 b[PT_AMBIENT_OCCLUSION_MAX_SAMPLES];
    uint32_t count = 0u;
    b[0] = v3(0, 0, 0);
    for (uint32_t k = 0; k < S; k++) {
        const int occ = (int)((occluded >> k) & 1u);
        count += (uint32_t)occ;
        b[k] = occ ? v3(0, 0, 0) : pt_reproject_unpack_unit(packed[k]);
    }
    for (uint32_t w = S; w > 1u; w >>= 1u)
        for (uint32_t m = 0; m < w / 2u; m++) b[m] = b[2u * m] + b[2u * m + 1u];
    pt_visibility_record R;
    R.Bent[0] = b[0].x;
    R.Bent[1] = b[0].y;
    R.Bent[2] = b[0].z;
    R.Unoccluded = (float)(S - count);
    R.OccludedMask = S < 64u ? occluded & ((1ull << S) - 1ull) : occluded;
    R.Samples = (float)S;
    R.Reserved = 0u;
    return R;
}

/* --- sky light gathered at caller-given points -----------
 *
 * The device kernel is sky_gather_kernel (csrc/hip/occlusion.hip), the host
 * twins ptsSkyGatherRays / ptsSkyGatherReduce (csrc/scene/visibility.cpp),
 * the numpy restatement tests/sky_gather_restatement.py.
 *
 * Point i of n, position P and (COSINE only) normal N as given, parameters
 * {Samples S, Radius, Seed, Offset, FirstIndex, Lobe}:
 *
 *   j  = FirstIndex + i;  s0 = pt_visibility_gather_seed(j, Seed)
 *   sample k = 0 .. S-1:
 *     state = pt_visibility_skip(s0, 2 k); D = RandomDirection(state)
 *     COSINE: W as row 15's (ray k is row 15's ray k, bit for bit)
 *     SPHERE: W = D, uniform over the sphere; N is not read
 *     word = pack(W), V = unpack(word); origin P + Offset W; duration
 *            pt_visibility_duration(Radius)
 *     lstate = pt_visibility_skip(s0, 128 + k)   (past the 128 direction draws
 *            of the largest S); L0 = Random0To1(lstate); Lambda = PathLambda(L0)
 *     occ_k = whether anything lies within ray k's duration
 *     C_k = occ_k ? (0, 0, 0) : EscapeContribution(scene, V, Lambda, (1, 1, 1, 1), 4)
 *            (csrc/hip/path.hpp: what a camera ray leaving the scene along V
 *            adds to its pixel, CIE XYZ)
 *     Y[0..8] = pt_sky_gather_basis(V);  t[i][c] = C_k[c] * Y[i]
 *   record (pt_sky_record): SH[i][c] = the pairwise tree sum of t[i][c] over k
 *     (b'_m = b_2m + b_2m+1 for log2 S levels, row 15's tree per float);
 *     OccludedMask, Unoccluded, Samples as row 15's; Reserved = 0.
 *
 * The sky evaluation itself is the device's (and the restatement's): this
 * header has the rays, L0, the basis and the tree.  Nesting and partition
 * independence hold as in row 15. */

/* pt_visibility_gather_parameters_ok's ranges, and a known Lobe. */
PT_HD int pt_sky_gather_parameters_ok(const pt_sky_gather_parameters* p, uint32_t n)
{
    pt_visibility_gather_parameters q;
    q.Samples = p->Samples;
    q.Radius = p->Radius;
    q.Seed = p->Seed;
    q.Offset = p->Offset;
    q.FirstIndex = p->FirstIndex;
    if (p->Lobe != PT_SKY_GATHER_COSINE && p->Lobe != PT_SKY_GATHER_SPHERE) return 0;
    return pt_visibility_gather_parameters_ok(&q, n);
}

/* Sample k of the point at P whose stream starts at s0: its origin, and its
 * velocity as the packed word.  COSINE: pt_visibility_gather_ray around N.
 * SPHERE: the drawn direction itself; N is not used. */
PT_HD uint32_t pt_sky_gather_ray(uint32_t Lobe, pt3 N, pt3 P, float Offset, uint32_t s0, uint32_t k, pt3* RO)
{
    if (Lobe == PT_SKY_GATHER_COSINE) {
        const pt_visibility_frame F = pt_visibility_gather_frame(N);
        return pt_visibility_gather_ray(&F, P, Offset, s0, k, RO);
    }
    uint32_t state = pt_visibility_skip(s0, 2u * k);
    const pt3 W = pt_visibility_random_direction(&state);
    *RO = P + Offset * W;
    return pt_reproject_pack_unit(W);
}

/* Sample k's normalised first wavelength: draw 128 + k of the point's stream. */
PT_HD float pt_sky_gather_lambda0(uint32_t s0, uint32_t k)
{
    uint32_t lstate = pt_visibility_skip(s0, 128u + k);
    return pt_random01(&lstate);
}

/* The real spherical harmonics of bands 0..2 at the unit vector V, z up. */
PT_HD void pt_sky_gather_basis(pt3 V, float Y[9])
{
    const float x = V.x, y = V.y, z = V.z;
    Y[0] = 0.28209479f;
    Y[1] = 0.48860251f * y;
    Y[2] = 0.48860251f * z;
    Y[3] = 0.48860251f * x;
    Y[4] = 1.09254843f * (x * y);
    Y[5] = 1.09254843f * (y * z);
    Y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.09254843f * (x * z);
    Y[8] = 0.54627422f * (x * x - y * y);
}

/* A point's record from its S packed velocities, its occluded bits and its
 * rays' contributions (3 floats per ray; an occluded ray's is taken as zero):
 * the basis, the 27 products per ray and the tree the device kernel's
 * cross-lane rounds form. */
PT_HD pt_sky_record pt_sky_gather_reduce(uint32_t S, const uint32_t* packed, uint64_t occluded, const float* contributions)
{
    float b[PT_AMBIENT_OCCLUSION_MAX_SAMPLES][27];
    uint32_t count = 0u;
    for (uint32_t k = 0; k < S; k++) {
        const int occ = (int)((occluded >> k) & 1u);
        count += (uint32_t)occ;
        float Y[9];
        pt_sky_gather_basis(pt_reproject_unpack_unit(packed[k]), Y);
        for (uint32_t i = 0; i < 9u; i++)
            for (uint32_t c = 0; c < 3u; c++) b[k][3u * i + c] = (occ ? 0.0f : contributions[3u * k + c]) * Y[i];
    }
    for (uint32_t w = S; w > 1u; w >>= 1u)
        for (uint32_t m = 0; m < w / 2u; m++)
            for (uint32_t e = 0; e < 27u; e++) b[m][e] = b[2u * m][e] + b[2u * m + 1u][e];
    pt_sky_record R;
    for (uint32_t i = 0; i < 9u; i++)
        for (uint32_t c = 0; c < 3u; c++) R.SH[i][c] = b[0][3u * i + c];
    R.Unoccluded = (float)(S - count);
    R.OccludedMask = S < 64u ? occluded & ((1ull << S) - 1ull) : occluded;
    R.Samples = (float)S;
    R.Reserved[0] = 0u;
    return R;
}

#endif /* PT_VISIBILITY_H */
