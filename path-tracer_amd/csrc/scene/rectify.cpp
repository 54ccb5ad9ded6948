// rectify.cpp — ptsRectifyHistory (include/pt_scene.h): validation of a
// carried history against the new frame's samples on
// the host.  The CPU path for saved frames and the second implementation the
// device kernel (csrc/hip/rectify.hip) is compared with: the same definition,
// the same per-pixel and per-tap arithmetic (include/pt_rectify.h), the same
// window order.  Where the kernel stages a tile's window records once, this
// forms a tap's record when it visits the tap: the same function on the same
// inputs.  Single-threaded.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_rectify.h"

#include <cstring>
#include <new>
#include <vector>

extern "C" int ptsRectifyHistory(uint32_t width, uint32_t height, const float* history, const float* current,
                                 const pt_denoise_guide* guides, const pt_rectify_parameters* params, float* out_rgba)
{
    if (!history || !current || !guides || !params || !out_rgba) return -1;
    if (width == 0 || height == 0) return -1;
    if (history == current || out_rgba == current) return -1;
    if (!pt_rectify_parameters_ok(params)) return -1;
    const size_t n = (size_t)width * height;
    const int64_t R = (int64_t)params->Radius;
    try {
        std::vector<float> out(4 * n);
        std::vector<pt_rectify_record> window((size_t)((2 * R + 1) * (2 * R + 1)));
        for (uint32_t y = 0; y < height; y++) {
            for (uint32_t x = 0; x < width; x++) {
                const size_t ip = (size_t)y * width + x;
                const pt_denoise_guide& gc = guides[ip];
                size_t k = 0;
                for (int64_t qy = (int64_t)y - R; qy <= (int64_t)y + R; qy++) {
                    for (int64_t qx = (int64_t)x - R; qx <= (int64_t)x + R; qx++, k++) {
                        const int inside = qx >= 0 && qy >= 0 && qx < (int64_t)width && qy < (int64_t)height;
                        const size_t iq = inside ? (size_t)qy * width + (size_t)qx : ip;
                        pt_rectify_stage(inside, current + 4 * iq, &guides[iq], &window[k]);
                    }
                }
                pt_rectify_sums A;
                pt_rectify_begin(&A);
                for (const pt_rectify_record& r : window)
                    if (pt_rectify_member(params, gc.shape, gc.normal, r.member_shape, r.normal))
                        pt_rectify_add_colour(&A, r.c);
                if (!pt_rectify_tested(params, history + 4 * ip, A.m, &out[4 * ip])) continue;
                float mu[3];
                pt_rectify_mean(&A, mu);
                for (const pt_rectify_record& r : window)
                    if (pt_rectify_member(params, gc.shape, gc.normal, r.member_shape, r.normal))
                        pt_rectify_add_deviation(&A, mu, r.c);
                pt_rectify_clip(params, history + 4 * ip, &A, mu, &out[4 * ip]);
            }
        }
        // history may be out_rgba: nothing was written before this copy.
        std::memmove(out_rgba, out.data(), 4 * n * sizeof(float));
    } catch (const std::bad_alloc&) {
        return -2;
    }
    return 0;
}
