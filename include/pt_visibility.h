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

#endif /* PT_VISIBILITY_H */
