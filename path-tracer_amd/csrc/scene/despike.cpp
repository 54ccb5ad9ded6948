// despike.cpp — ptsDespike (include/pt_scene.h): the neighbourhood firefly
// clamp on the host.  The CPU path for saved frames and
// the second implementation the device kernel (csrc/hip/despike.hip) is
// compared with: the same definition, the same per-pixel and per-tap
// arithmetic (include/pt_despike.h), the same window order.  Where the kernel
// stages a tile's window records once, this forms a tap's record when it
// visits the tap: the same function on the same inputs.  Single-threaded.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_despike.h"

extern "C" int ptsDespike(uint32_t width, uint32_t height, const float* accum, const pt_denoise_guide* guides,
                          const pt_despike_parameters* params, float* out_rgba)
{
    if (!accum || !guides || !params || !out_rgba) return -1;
    if (width == 0 || height == 0) return -1;
    if (out_rgba == accum) return -1;
    if (!pt_despike_parameters_ok(params)) return -1;
    const int64_t R = (int64_t)params->Radius;
    for (uint32_t y = 0; y < height; y++) {
        for (uint32_t x = 0; x < width; x++) {
            const size_t ip = (size_t)y * width + x;
            pt_despike_record centre;
            pt_despike_stage(1, accum + 4 * ip, &guides[ip], &centre);
            pt_despike_top T;
            pt_despike_begin(&T);
            for (int64_t qy = (int64_t)y - R; qy <= (int64_t)y + R; qy++) {
                for (int64_t qx = (int64_t)x - R; qx <= (int64_t)x + R; qx++) {
                    if (qx == (int64_t)x && qy == (int64_t)y) continue;
                    const int inside = qx >= 0 && qy >= 0 && qx < (int64_t)width && qy < (int64_t)height;
                    const size_t iq = inside ? (size_t)qy * width + (size_t)qx : ip;
                    pt_despike_record r;
                    pt_despike_stage(inside, accum + 4 * iq, &guides[iq], &r);
                    pt_despike_insert(&T, pt_despike_member(params, centre.member_shape, centre.normal,
                                                            r.member_shape, r.normal), r.v);
                }
            }
            pt_despike_decide(params, accum + 4 * ip, centre.v, &T, out_rgba + 4 * ip);
        }
    }
    return 0;
}
