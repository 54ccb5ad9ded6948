/*
 * pt_reproject.h — temporal reprojection of an accumulator into a new view
 * (definition in DESIGN.md §6 row 8; row 9, which follows moved shapes, at the
 * end), written once for the device kernel
 * (csrc/hip/reproject.hip) and the host implementation
 * (csrc/scene/reproject.cpp) under pt_fp.h's convention: IEEE binary32, no
 * contraction, sums left to right, pt_sin / pt_cos / pt_atan2 / pt_asin /
 * pt_sqrt.  Per-pixel and per-tap arithmetic only: the loop over the image,
 * the loads of the four taps and the store of the result are the callers'.
 * What rows 8 and 9 have in common is written once: the central ray, the
 * position in the previous frame (pt_reproject_locate_tail) and the history
 * and depth tests of a tap; row 9 adds only what a motion record changes.
 *
 * For a pixel of the current view: its central camera ray, the world point
 * its guide record saw (or the ray's direction on a miss), that point's
 * continuous position in the previous view, and the bilinear blend of the
 * previous accumulator's taps that still show the same surface.
 */
#ifndef PT_REPROJECT_H
#define PT_REPROJECT_H

#include "pt_fp.h"
#include "pt_glsl.h"
#include "pt_packed.h"

PT_HD int pt_reproject_parameters_ok(const pt_reproject_parameters* p)
{
    return p->NormalCosine > -1.0f && p->NormalCosine <= 1.0f && p->DepthTolerance > 0.0f && p->MinWeight > 0.0f &&
           p->MinWeight <= 1.0f && p->MaxHistory > 0.0f;
}

PT_HD int pt_reproject_finite(float x) { return (pt_f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* PackUnitVector / UnpackUnitVector (src/core/common.glsl.inc:137-151): the
 * octahedral snorm16x2 form every ray's velocity takes between raygen and
 * extend. */
PT_HD uint32_t pt_reproject_pack_unit(pt3 V)
{
    float s = 1.0f / (pt_abs(V.x) + pt_abs(V.y) + pt_abs(V.z));
    float Px = V.x * s, Py = V.y * s;
    if (V.z <= 0.0f) {
        float Sx = Px >= 0.0f ? 1.0f : -1.0f, Sy = Py >= 0.0f ? 1.0f : -1.0f;
        float Nx = (1.0f - pt_abs(Py)) * Sx;
        float Ny = (1.0f - pt_abs(Px)) * Sy;
        Px = Nx; Py = Ny;
    }
    return pt_pack_snorm16(Px) | (pt_pack_snorm16(Py) << 16);
}

PT_HD pt3 pt_reproject_unpack_unit(uint32_t P)
{
    float Px = pt_unpack_snorm16(P & 0xFFFFu), Py = pt_unpack_snorm16(P >> 16);
    float Z = 1.0f - pt_abs(Px) - pt_abs(Py);
    if (Z < 0.0f) {
        float Sx = Px >= 0.0f ? 1.0f : -1.0f, Sy = Py >= 0.0f ? 1.0f : -1.0f;
        float Nx = (1.0f - pt_abs(Py)) * Sx;
        float Ny = (1.0f - pt_abs(Px)) * Sy;
        Px = Nx; Py = Ny;
    }
    return normalize(v3(Px, Py, Z));
}

/* A camera whose central rays this header can form and invert: a known
 * model, and for the thin lens a sensor behind the focal plane
 * (SensorDistance > FocalLength; otherwise the ray through the lens centre
 * leaves on the sensor's side, or nowhere). */
PT_HD int pt_reproject_camera_ok(const pt_packed_camera* Cam)
{
    if (Cam->Model == PT_CAMERA_MODEL_PINHOLE || Cam->Model == PT_CAMERA_MODEL_360) return 1;
    if (Cam->Model == PT_CAMERA_MODEL_THIN_LENS) return Cam->SensorDistance > Cam->FocalLength;
    return 0;
}

/* The central camera ray of pixel (x, y) of a w x h frame: GenerateCameraRay
 * (src/scene/scene.glsl.inc:613-655) at the pixel centre through the lens
 * centre, then the packed velocity's round trip.  The guide kernel
 * (csrc/hip/denoise.hip) takes its rays from here too, so the ray a guide
 * record was seen along is the ray reprojection inverts.  0: unknown model,
 * O = 0, V = (0, 0, 1). */
PT_HD int pt_reproject_central_ray(const pt_packed_camera* Cam, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                   pt3* RO, pt3* RV)
{
    float SPx = (float)x, SPy = (float)y;
    SPx = SPx + 0.5f; SPy = SPy + 0.5f;
    float Nx = SPx / (float)w, Ny = SPy / (float)h;
    uint32_t Model = Cam->Model;
    pt3 O = v3(0, 0, 0), V;
    if (Model == PT_CAMERA_MODEL_PINHOLE || Model == PT_CAMERA_MODEL_THIN_LENS) {
        pt3 SP = v3(-Cam->SensorSize[0] * (Nx - 0.5f), -Cam->SensorSize[1] * (0.5f - Ny), Cam->SensorDistance);
        if (Model == PT_CAMERA_MODEL_PINHOLE) {
            V = normalize(O - SP);
        } else {
            pt3 OP = -SP * Cam->FocalLength / (SP.z - Cam->FocalLength);
            V = normalize(OP - O);
        }
    } else if (Model == PT_CAMERA_MODEL_360) {
        float Phi = (Nx - 0.5f) * PT_TAU;
        float Theta = (0.5f - Ny) * PT_PI;
        V = v3(pt_cos(Theta) * pt_sin(Phi), pt_sin(Theta), -pt_cos(Theta) * pt_cos(Phi));
    } else {
        *RO = v3s(0); *RV = v3(0, 0, 1);
        return 0;
    }
    const float* To = Cam->Transform.To;
    *RO = mat4_mul_point(To, O);
    *RV = pt_reproject_unpack_unit(pt_reproject_pack_unit(mat4_mul_vector(To, V)));
    return 1;
}

/* The inverse of the mapping above for a point (or, on a miss, a direction)
 * L in the camera's own frame: its normalised sensor position.  The pinhole
 * and the thin lens (SensorDistance > FocalLength) look along -z and send
 * sensor position (Nx, Ny) to a positive multiple of
 * (SensorSize.x (Nx - 0.5), SensorSize.y (0.5 - Ny), -SensorDistance).
 * 0: behind the camera (or in its plane). */
PT_HD int pt_reproject_project(const pt_packed_camera* Cam, pt3 L, float* Nx, float* Ny)
{
    if (Cam->Model == PT_CAMERA_MODEL_360) {
        float Phi = pt_atan2(L.x, -L.z);
        float Theta = pt_asin(L.y / length(L));
        *Nx = Phi / PT_TAU + 0.5f;
        *Ny = 0.5f - Theta / PT_PI;
        return 1;
    }
    if (!(L.z < 0.0f)) return 0;
    float k = Cam->SensorDistance / -L.z;
    *Nx = (L.x * k) / Cam->SensorSize[0] + 0.5f;
    *Ny = 0.5f - (L.y * k) / Cam->SensorSize[1];
    return 1;
}

/* Where a current pixel's history lies in the previous frame. */
typedef struct pt_reproject_target {
    int64_t x0, y0;     /* the first tap; the others are +1 in x, +1 in y, +1 in both */
    float   fx, fy;     /* the continuous position's fractions */
    float   dist;       /* hits: the world point's distance from the previous camera */
} pt_reproject_target;

/* Step 3, shared by rows 8 and 9: L, the point (or direction) in the previous
 * camera's frame, to its continuous position in the wp x hp previous frame
 * and that position's first tap and fractions.  0: behind the previous
 * camera, or a position none of whose taps can lie inside the frame, a
 * non-finite one included. */
PT_HD int pt_reproject_locate_tail(const pt_packed_camera* Cp, pt3 L, uint32_t wp, uint32_t hp,
                                   pt_reproject_target* T)
{
    float Nx, Ny;
    if (!pt_reproject_project(Cp, L, &Nx, &Ny)) return 0;
    float u = Nx * (float)wp - 0.5f, v = Ny * (float)hp - 0.5f;
    if (!(u > -1.0f && u < (float)wp && v > -1.0f && v < (float)hp)) return 0;
    float fu = pt_floor(u), fv = pt_floor(v);
    T->x0 = (int64_t)fu;
    T->y0 = (int64_t)fv;
    T->fx = u - fu;
    T->fy = v - fv;
    return 1;
}

/* Steps 1-3.  shape, time: the current pixel's guide record.  0: no history
 * (a camera this header cannot invert, or pt_reproject_locate_tail's 0). */
PT_HD int pt_reproject_locate(const pt_packed_camera* Cc, const pt_packed_camera* Cp, uint32_t x, uint32_t y,
                              uint32_t w, uint32_t h, uint32_t wp, uint32_t hp, uint32_t shape, float time,
                              pt_reproject_target* T)
{
    if (!pt_reproject_camera_ok(Cc) || !pt_reproject_camera_ok(Cp)) return 0;
    pt3 O, V;
    pt_reproject_central_ray(Cc, x, y, w, h, &O, &V);
    pt3 L;
    T->dist = 0.0f;
    if (shape != PT_SHAPE_INDEX_NONE) {
        pt3 P = v3(O.x + V.x * time, O.y + V.y * time, O.z + V.z * time);
        L = mat4_mul_point(Cp->Transform.From, P);
        T->dist = length(P - mat4_mul_point(Cp->Transform.To, v3s(0)));
    } else {
        L = mat4_mul_vector(Cp->Transform.From, V);
    }
    return pt_reproject_locate_tail(Cp, L, wp, hp, T);
}

/* Bilinear weight of tap i = 0..3 ((0,0), (1,0), (0,1), (1,1)). */
PT_HD float pt_reproject_tap_weight(const pt_reproject_target* T, int i)
{
    float wx = (i & 1) ? T->fx : 1.0f - T->fx;
    float wy = (i & 2) ? T->fy : 1.0f - T->fy;
    return wx * wy;
}

/* Step 4's two tests that rows 8 and 9 share.  A tap's accumulator value hp
 * is a usable history: finite sums and a positive, finite sample count. */
PT_HD int pt_reproject_history_ok(const float* hp)
{
    return pt_reproject_finite(hp[0]) && pt_reproject_finite(hp[1]) && pt_reproject_finite(hp[2]) &&
           pt_reproject_finite(hp[3]) && hp[3] > 0.0f;
}

/* The tap's guide saw its surface at the distance the target expects. */
PT_HD int pt_reproject_depth_ok(const pt_reproject_parameters* p, const pt_reproject_target* T,
                                const pt_denoise_guide* gp)
{
    return pt_abs(gp->time - T->dist) <= p->DepthTolerance * T->dist;
}

/* Step 4 for a tap inside the previous image: hp its accumulator value, gp
 * its guide record, gc the current pixel's. */
PT_HD int pt_reproject_tap_valid(const pt_reproject_parameters* p, const pt_reproject_target* T,
                                 const pt_denoise_guide* gc, const float* hp, const pt_denoise_guide* gp)
{
    if (!pt_reproject_history_ok(hp)) return 0;
    if (gp->shape != gc->shape) return 0;
    if (gc->shape == PT_SHAPE_INDEX_NONE) return 1;
    float d = (gp->normal[0] * gc->normal[0] + gp->normal[1] * gc->normal[1]) + gp->normal[2] * gc->normal[2];
    if (!(d >= p->NormalCosine)) return 0;
    return pt_reproject_depth_ok(p, T, gp);
}

/* Step 5: the sums over the valid taps, in tap order. */
typedef struct pt_reproject_sums { float x, y, z, n, w; } pt_reproject_sums;

PT_HD void pt_reproject_add(pt_reproject_sums* S, float w, const float* hp)
{
    S->x = S->x + w * (hp[0] / hp[3]);
    S->y = S->y + w * (hp[1] / hp[3]);
    S->z = S->z + w * (hp[2] / hp[3]);
    S->n = S->n + w * hp[3];
    S->w = S->w + w;
}

/* The reprojected accumulator value: (mean * n, n), or zeros without a history. */
PT_HD void pt_reproject_finish(const pt_reproject_parameters* p, const pt_reproject_sums* S, float* out)
{
    if (!(S->w >= p->MinWeight)) {
        out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = 0.0f;
        return;
    }
    float n = pt_min(S->n / S->w, p->MaxHistory);
    out[0] = (S->x / S->w) * n;
    out[1] = (S->y / S->w) * n;
    out[2] = (S->z / S->w) * n;
    out[3] = n;
}

/* --- Row 9: reprojection that follows moved shapes ---------------------------
 *
 * Everything above holds, except for a hit pixel whose guide shape s has a
 * motion record (pt_shape_motion, pt_packed.h; ptsShapeMotion fills a table
 * of them from two packed scenes).  What a pixel does with its shape: */
enum {
    PT_REPROJECT_MOTION_STATIC = 0,   /* a miss, or Flags without either bit: row 8, same operations, same bits */
    PT_REPROJECT_MOTION_MOVED  = 1,   /* the record's Point and Normal are applied */
    PT_REPROJECT_MOTION_NONE   = 2,   /* s >= motion_count or PT_SHAPE_MOTION_NO_HISTORY: no history */
};

/* From the record's Flags alone (NO_HISTORY wins over MOVED; other bits are
 * ignored).  The caller has checked shape != PT_SHAPE_INDEX_NONE and
 * shape < motion_count. */
PT_HD int pt_reproject_motion_kind(uint32_t Flags)
{
    if (Flags & PT_SHAPE_MOTION_NO_HISTORY) return PT_REPROJECT_MOTION_NONE;
    return (Flags & PT_SHAPE_MOTION_MOVED) ? PT_REPROJECT_MOTION_MOVED : PT_REPROJECT_MOTION_STATIC;
}

/* Steps 1-3 for a hit pixel of a moved shape.  P as in row 8; Pp = Point (P, 1)
 * is where that surface point was in the previous world; the previous view
 * is asked for Pp, and dist is Pp's distance from the previous ray origin.
 * *Ne: the normal the previous guide should show, normalize(Normal n) with
 * the rows summed left to right.  0: no history (as pt_reproject_locate, or
 * a normal whose image has a squared length that is not > 0 or not finite). */
PT_HD int pt_reproject_locate_moved(const pt_packed_camera* Cc, const pt_packed_camera* Cp, uint32_t x, uint32_t y,
                                    uint32_t w, uint32_t h, uint32_t wp, uint32_t hp, const float* normal, float time,
                                    const float* Point, const float* Normal, pt_reproject_target* T, pt3* Ne)
{
    if (!pt_reproject_camera_ok(Cc) || !pt_reproject_camera_ok(Cp)) return 0;
    pt3 O, V;
    pt_reproject_central_ray(Cc, x, y, w, h, &O, &V);
    pt3 P = v3(O.x + V.x * time, O.y + V.y * time, O.z + V.z * time);
    pt3 Pp = v3(((Point[0] * P.x + Point[1] * P.y) + Point[2] * P.z) + Point[3],
                ((Point[4] * P.x + Point[5] * P.y) + Point[6] * P.z) + Point[7],
                ((Point[8] * P.x + Point[9] * P.y) + Point[10] * P.z) + Point[11]);
    pt3 L = mat4_mul_point(Cp->Transform.From, Pp);
    T->dist = length(Pp - mat4_mul_point(Cp->Transform.To, v3s(0)));
    pt3 N = v3((Normal[0] * normal[0] + Normal[1] * normal[1]) + Normal[2] * normal[2],
               (Normal[3] * normal[0] + Normal[4] * normal[1]) + Normal[5] * normal[2],
               (Normal[6] * normal[0] + Normal[7] * normal[1]) + Normal[8] * normal[2]);
    float q = dot(N, N);
    if (!(q > 0.0f) || !pt_reproject_finite(q)) return 0;
    *Ne = N * (1.0f / pt_sqrt(q));
    return pt_reproject_locate_tail(Cp, L, wp, hp, T);
}

/* Step 4 for a tap of a moved shape's pixel: pt_reproject_tap_valid with the
 * expected normal Ne in the current normal's place. */
PT_HD int pt_reproject_tap_valid_moved(const pt_reproject_parameters* p, const pt_reproject_target* T, uint32_t shape,
                                       pt3 Ne, const float* hp, const pt_denoise_guide* gp)
{
    if (!pt_reproject_history_ok(hp)) return 0;
    if (gp->shape != shape) return 0;
    float d = (gp->normal[0] * Ne.x + gp->normal[1] * Ne.y) + gp->normal[2] * Ne.z;
    if (!(d >= p->NormalCosine)) return 0;
    return pt_reproject_depth_ok(p, T, gp);
}

#endif /* PT_REPROJECT_H */
