// reproject.cpp — ptsReproject (include/pt_scene.h): temporal reprojection
// of an accumulator into a new view on the host.  The
// CPU path for saved frames and the second implementation the device kernel
// (csrc/hip/reproject.hip) is compared with: the same definition, the same
// per-pixel and per-tap arithmetic (include/pt_reproject.h), the same tap
// order.  Single-threaded.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_reproject.h"

#include <cstring>
#include <new>
#include <vector>

extern "C" int ptsReproject(uint32_t prev_width, uint32_t prev_height, const float* prev_accum,
                            const pt_denoise_guide* prev_guides, const pt_packed_camera* prev_camera, uint32_t width,
                            uint32_t height, const pt_denoise_guide* guides, const pt_packed_camera* camera,
                            const pt_reproject_parameters* params, float* out_rgba)
{
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
                if (pt_reproject_locate(camera, prev_camera, x, y, width, height, prev_width, prev_height, gc.shape,
                                        gc.time, &T)) {
                    for (int i = 0; i < 4; i++) {
                        const int64_t qx = T.x0 + (i & 1), qy = T.y0 + (i >> 1);
                        if (qx < 0 || qy < 0 || qx >= (int64_t)prev_width || qy >= (int64_t)prev_height) continue;
                        const size_t iq = (size_t)qy * prev_width + (size_t)qx;
                        const float* hp = prev_accum + 4 * iq;
                        if (!pt_reproject_tap_valid(params, &T, &gc, hp, &prev_guides[iq])) continue;
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
