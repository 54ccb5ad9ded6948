// reproject.cpp — ptsReproject and ptsReprojectMoving (include/pt_scene.h):
// temporal reprojection of an accumulator into a new view (DESIGN.md §6 rows
// 8 and 9) on the host.  The CPU path for saved frames and the second
// implementation the device kernel (csrc/hip/reproject.hip) is compared with:
// the same definition, the same per-pixel and per-tap arithmetic
// (include/pt_reproject.h), the same tap order.  Single-threaded.  One image
// loop serves both rows: row 8 is the loop without a motion table.
// ptsShapeMotion fills row 9's table.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_reproject.h"

#include <cstring>
#include <new>
#include <vector>

// motion == nullptr: row 8, every pixel takes the static path.
static int Reproject(uint32_t prev_width, uint32_t prev_height, const float* prev_accum,
                     const pt_denoise_guide* prev_guides, const pt_packed_camera* prev_camera, uint32_t width,
                     uint32_t height, const pt_denoise_guide* guides, const pt_packed_camera* camera,
                     const pt_shape_motion* motion, uint32_t motion_count, const pt_reproject_parameters* params,
                     float* out_rgba)
{
    if (!motion && motion_count) return -1;
    if (!prev_accum || !prev_guides || !prev_camera || !guides || !camera || !params || !out_rgba) return -1;
    if (prev_width == 0 || prev_height == 0 || width == 0 || height == 0) return -1;
    if (prev_accum == out_rgba || prev_guides == guides) return -1;
    if (!pt_reproject_parameters_ok(params)) return -1;
    const size_t n = (size_t)width * height;
    try {
        std::vector<float> out(4 * n);
        for (uint32_t y = 0; y < height; y++) {
            for (uint32_t x = 0; x < width; x++) {
                const size_t ip = (size_t)y * width + x;
                const pt_denoise_guide& gc = guides[ip];
                pt_reproject_sums S{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                pt_reproject_target T;
                pt3 Ne = v3s(0);
                int kind = PT_REPROJECT_MOTION_STATIC, located = 0;
                const pt_shape_motion* m = nullptr;
                if (motion && gc.shape != PT_SHAPE_INDEX_NONE) {
                    if (gc.shape >= motion_count) {
                        kind = PT_REPROJECT_MOTION_NONE;
                    } else {
                        m = &motion[gc.shape];
                        kind = pt_reproject_motion_kind(m->Flags);
                    }
                }
                if (kind == PT_REPROJECT_MOTION_STATIC)
                    located = pt_reproject_locate(camera, prev_camera, x, y, width, height, prev_width, prev_height,
                                                  gc.shape, gc.time, &T);
                else if (kind == PT_REPROJECT_MOTION_MOVED)
                    located = pt_reproject_locate_moved(camera, prev_camera, x, y, width, height, prev_width,
                                                        prev_height, gc.normal, gc.time, m->Point, m->Normal, &T, &Ne);
                if (located) {
                    for (int i = 0; i < 4; i++) {
                        const int64_t qx = T.x0 + (i & 1), qy = T.y0 + (i >> 1);
                        if (qx < 0 || qy < 0 || qx >= (int64_t)prev_width || qy >= (int64_t)prev_height) continue;
                        const size_t iq = (size_t)qy * prev_width + (size_t)qx;
                        const float* hp = prev_accum + 4 * iq;
                        const int ok = kind == PT_REPROJECT_MOTION_MOVED
                                           ? pt_reproject_tap_valid_moved(params, &T, gc.shape, Ne, hp, &prev_guides[iq])
                                           : pt_reproject_tap_valid(params, &T, &gc, hp, &prev_guides[iq]);
                        if (!ok) continue;
                        pt_reproject_add(&S, pt_reproject_tap_weight(&T, i), hp);
                    }
                }
                pt_reproject_finish(params, &S, &out[4 * ip]);
            }
        }
        std::memcpy(out_rgba, out.data(), 4 * n * sizeof(float));
    } catch (const std::bad_alloc&) {
        return -2;
    }
    return 0;
}

extern "C" int ptsReproject(uint32_t prev_width, uint32_t prev_height, const float* prev_accum,
                            const pt_denoise_guide* prev_guides, const pt_packed_camera* prev_camera, uint32_t width,
                            uint32_t height, const pt_denoise_guide* guides, const pt_packed_camera* camera,
                            const pt_reproject_parameters* params, float* out_rgba)
{
    return Reproject(prev_width, prev_height, prev_accum, prev_guides, prev_camera, width, height, guides, camera,
                     nullptr, 0, params, out_rgba);
}

extern "C" int ptsReprojectMoving(uint32_t prev_width, uint32_t prev_height, const float* prev_accum,
                                  const pt_denoise_guide* prev_guides, const pt_packed_camera* prev_camera,
                                  uint32_t width, uint32_t height, const pt_denoise_guide* guides,
                                  const pt_packed_camera* camera, const pt_shape_motion* motion, uint32_t motion_count,
                                  const pt_reproject_parameters* params, float* out_rgba)
{
    return Reproject(prev_width, prev_height, prev_accum, prev_guides, prev_camera, width, height, guides, camera,
                     motion, motion_count, params, out_rgba);
}

// --- row 9's table: shapes that moved between the two frames ------------------------

static bool TransformFinite(const pt_packed_transform& t)
{
    for (int i = 0; i < 16; i++)
        if (!pt_reproject_finite(t.To[i]) || !pt_reproject_finite(t.From[i])) return false;
    return true;
}

extern "C" int ptsShapeMotion(const pt_packed_shape* prev_shapes, uint32_t prev_count, const pt_packed_shape* shapes,
                              uint32_t count, pt_shape_motion* out)
{
    if ((count && (!shapes || !out)) || (prev_count && !prev_shapes)) return -1;
    for (uint32_t i = 0; i < count; i++) {
        pt_shape_motion m;
        std::memset(&m, 0, sizeof m);
        const pt_packed_shape& c = shapes[i];
        if (i >= prev_count || prev_shapes[i].Type != c.Type || prev_shapes[i].MeshRootNodeIndex != c.MeshRootNodeIndex ||
            !TransformFinite(prev_shapes[i].Transform) || !TransformFinite(c.Transform)) {
            m.Flags = PT_SHAPE_MOTION_NO_HISTORY;
        } else if (std::memcmp(&prev_shapes[i].Transform, &c.Transform, sizeof c.Transform) == 0) {
            m.Point[0] = m.Point[5] = m.Point[10] = 1.0f;
            m.Normal[0] = m.Normal[4] = m.Normal[8] = 1.0f;
        } else {
            const float* Tp = prev_shapes[i].Transform.To;
            const float* Fp = prev_shapes[i].Transform.From;
            const float* Tc = c.Transform.To;
            const float* Fc = c.Transform.From;
            m.Flags = PT_SHAPE_MOTION_MOVED;
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 4; k++)
                    m.Point[4 * r + k] = ((Tp[r] * Fc[4 * k] + Tp[4 + r] * Fc[4 * k + 1]) + Tp[8 + r] * Fc[4 * k + 2]) +
                                         Tp[12 + r] * Fc[4 * k + 3];
            // Normal = transpose of the linear part of To_cur From_prev.
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++)
                    m.Normal[3 * r + k] = (Tc[k] * Fp[4 * r] + Tc[4 + k] * Fp[4 * r + 1]) + Tc[8 + k] * Fp[4 * r + 2];
        }
        out[i] = m;
    }
    return 0;
}

extern "C" int ptsCentralCameraRay(const pt_packed_camera* camera, uint32_t x, uint32_t y, uint32_t width,
                                   uint32_t height, float origin[3], float velocity[3])
{
    if (!camera || !origin || !velocity || width == 0 || height == 0) return -1;
    pt3 O, V;
    if (!pt_reproject_central_ray(camera, x, y, width, height, &O, &V)) return -1;
    origin[0] = O.x; origin[1] = O.y; origin[2] = O.z;
    velocity[0] = V.x; velocity[1] = V.y; velocity[2] = V.z;
    return 0;
}
