// reproject.hip — temporal reprojection of an accumulator into a new view (no
// reference counterpart).  One thread per pixel of the
// current frame: its central camera ray, the world point its guide record
// saw, that point's position in the previous frame, and the bilinear blend of
// the previous accumulator's four taps that still show the same surface.  The
// per-pixel and per-tap arithmetic is include/pt_reproject.h's, shared with
// the host implementation (csrc/scene/reproject.cpp); taps run in the order
// (0,0), (1,0), (0,1), (1,1), sums left to right, no atomics, no LDS.
//
// One kernel template, reproject_kernel<MOVING>.  MOVING = false is row 8.
// MOVING = true is row 9: a motion table between the guide and the taps.  The
// tap loads, the per-tap decisions and the epilogue are written once; the
// table lookup is compiled into the MOVING instantiation only, so the row 8
// code neither reads the table nor waits on it.
//
// A gather-bound streaming kernel: per pixel 32 B of current guide, four taps
// of 16 B accumulator + 32 B guide that neighbouring pixels share (about 48 B
// of unique previous-frame traffic under smooth motion), and 16 B written.
// Guide records are read as the two float4 they are.  Pixels map in 16x16
// tiles per 256-thread block, like the guide kernel, so a block's taps fall in
// a compact 17x17 region of the previous image.  A pixel without a history by
// the projection alone (off frame, behind the previous camera) loads no tap.
// The four taps are loaded together from coordinates clamped into the
// previous image, before any of the per-tap decisions.  Measured against a
// row-major thread mapping, against no early exit, and against a first form
// that tested each tap before loading it (one dependent load after another,
// 1.2 x as long): DESIGN.md §6 row 8.
#include "pt_device.hpp"
#include "kernels.hpp"
#include "../../../include/pt_reproject.h"

namespace ptd {

struct reproject_args {
    pt_packed_camera camera, prev_camera;
    pt_reproject_parameters params;
    uint32_t w, h, wp, hp;
    uint32_t motion_count;      // MOVING only
};

PT_DEV pt_denoise_guide ReprojectGuide(float4 ga, float4 gb)
{
    pt_denoise_guide g;
    g.normal[0] = ga.x; g.normal[1] = ga.y; g.normal[2] = ga.z;
    g.time = ga.w;
    g.albedo[0] = gb.x; g.albedo[1] = gb.y; g.albedo[2] = gb.z;
    g.shape = __float_as_uint(gb.w);
    return g;
}

// A motion record is six float4 (Point's rows; Normal and Flags in the last
// three); a lane loads its shape's Flags first and the other 84 bytes only
// when the shape moved.  The cost over row 8 is that dependent load, guide ->
// motion record -> taps.  Measured against a form that read the record
// through scalar loads when a wave's active lanes share one shape (3-5 %
// faster where every wave does, one wave per SIMD fewer, a second code path):
// DESIGN.md §6 row 9.
PT_DEV void LoadMotion(const float4* __restrict__ rec, float* Point, float* Normal)
{
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
    const float n8 = reinterpret_cast<const float*>(rec)[20];
    Point[0] = r0.x; Point[1] = r0.y; Point[2] = r0.z; Point[3] = r0.w;
    Point[4] = r1.x; Point[5] = r1.y; Point[6] = r1.z; Point[7] = r1.w;
    Point[8] = r2.x; Point[9] = r2.y; Point[10] = r2.z; Point[11] = r2.w;
    Normal[0] = r3.x; Normal[1] = r3.y; Normal[2] = r3.z; Normal[3] = r3.w;
    Normal[4] = r4.x; Normal[5] = r4.y; Normal[6] = r4.z; Normal[7] = r4.w;
    Normal[8] = n8;
}

template <bool MOVING>
__global__ __launch_bounds__(256) void reproject_kernel(const float4* __restrict__ prev,
                                                        const float4* __restrict__ prev_guides,
                                                        const float4* __restrict__ guides,
                                                        const float4* __restrict__ motion, reproject_args P,
                                                        float4* __restrict__ out)
{
    const uint32_t x = blockIdx.x * 16 + (threadIdx.x & 15u), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= P.w || y >= P.h) return;
    const size_t ip = (size_t)y * P.w + x;
    const pt_denoise_guide gc = ReprojectGuide(guides[2 * ip], guides[2 * ip + 1]);
    pt_reproject_target T;
    pt_reproject_sums S{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    pt3 Ne = v3s(0);
    int kind = PT_REPROJECT_MOTION_STATIC, located = 0;
    if constexpr (MOVING) {
        if (gc.shape != PT_SHAPE_INDEX_NONE) {
            if (gc.shape >= P.motion_count) {
                kind = PT_REPROJECT_MOTION_NONE;
            } else {
                // gc.shape < motion_count: inside the table.
                const float4* rec = motion + 6 * (size_t)gc.shape;
                kind = pt_reproject_motion_kind(reinterpret_cast<const uint32_t*>(rec)[21]);
                if (kind == PT_REPROJECT_MOTION_MOVED) {
                    float Point[12], Normal[9];
                    LoadMotion(rec, Point, Normal);
                    located = pt_reproject_locate_moved(&P.camera, &P.prev_camera, x, y, P.w, P.h, P.wp, P.hp,
                                                        gc.normal, gc.time, Point, Normal, &T, &Ne);
                }
            }
        }
    }
    if (kind == PT_REPROJECT_MOTION_STATIC)
        located = pt_reproject_locate(&P.camera, &P.prev_camera, x, y, P.w, P.h, P.wp, P.hp, gc.shape, gc.time, &T);
    if (located) {
        // All four taps are loaded first, from coordinates clamped into the
        // previous image (wp, hp >= 1: always in bounds), so the twelve
        // loads are in flight together; the decisions follow.
        float4 c[4], ga[4], gb[4];
        bool inside[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int64_t qx = T.x0 + (i & 1), qy = T.y0 + (i >> 1);
            inside[i] = qx >= 0 && qy >= 0 && qx < (int64_t)P.wp && qy < (int64_t)P.hp;
            const int64_t cx = qx < 0 ? 0 : (qx >= (int64_t)P.wp ? (int64_t)P.wp - 1 : qx);
            const int64_t cy = qy < 0 ? 0 : (qy >= (int64_t)P.hp ? (int64_t)P.hp - 1 : qy);
            const size_t iq = (size_t)cy * P.wp + (size_t)cx;
            c[i] = prev[iq];
            ga[i] = prev_guides[2 * iq];
            gb[i] = prev_guides[2 * iq + 1];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!inside[i]) continue;
            const float hp[4] = {c[i].x, c[i].y, c[i].z, c[i].w};
            const pt_denoise_guide gp = ReprojectGuide(ga[i], gb[i]);
            // Without MOVING, kind is the constant STATIC.
            const int ok = kind == PT_REPROJECT_MOTION_MOVED
                               ? pt_reproject_tap_valid_moved(&P.params, &T, gc.shape, Ne, hp, &gp)
                               : pt_reproject_tap_valid(&P.params, &T, &gc, hp, &gp);
            if (!ok) continue;
            pt_reproject_add(&S, pt_reproject_tap_weight(&T, i), hp);
        }
    }
    float r[4];
    pt_reproject_finish(&P.params, &S, r);
    out[ip] = make_float4(r[0], r[1], r[2], r[3]);
}

}  // namespace ptd

hipError_t pt_launch_reproject(const float4* prev, const float4* prev_guides, uint32_t wp, uint32_t hp,
                               const pt_packed_camera* prev_camera, const float4* guides, uint32_t w, uint32_t h,
                               const pt_packed_camera* camera, const pt_shape_motion* motion, uint32_t motion_count,
                               const pt_reproject_parameters* p, float4* out, hipStream_t st)
{
    if (w == 0 || h == 0 || wp == 0 || hp == 0) return hipSuccess;
    ptd::reproject_args P;
    P.camera = *camera;
    P.prev_camera = *prev_camera;
    P.params = *p;
    P.w = w; P.h = h; P.wp = wp; P.hp = hp; P.motion_count = motion_count;
    hipLaunchKernelGGL(motion ? ptd::reproject_kernel<true> : ptd::reproject_kernel<false>,
                       dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, st, prev, prev_guides, guides,
                       reinterpret_cast<const float4*>(motion), P, out);
    return hipGetLastError();
}
