// visibility.cpp — ptsAmbientOcclusionRays (include/pt_scene.h): the sample
// rays of one pixel of the ambient-occlusion image on
// the host, from the arithmetic the device kernel (csrc/hip/occlusion.hip)
// runs (include/pt_visibility.h).  The tests hold it against their numpy
// restatement, and trace its rays to form the image the device must give.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_visibility.h"

extern "C" int ptsAmbientOcclusionRays(const pt_ambient_occlusion_parameters* params, uint32_t x, uint32_t y,
                                       const float origin[3], const float velocity[3], float time,
                                       const float normal[3], float* out_origins, uint32_t* out_velocities,
                                       float* out_duration)
{
    if (!params || !origin || !velocity || !normal || !out_origins || !out_velocities) return -1;
    if (!pt_visibility_parameters_ok(params)) return -1;
    const pt3 O = v3(origin[0], origin[1], origin[2]), V = v3(velocity[0], velocity[1], velocity[2]);
    const pt_visibility_frame F = pt_visibility_make_frame(v3(normal[0], normal[1], normal[2]), V);
    uint32_t state = pt_visibility_seed(x, y, params->Seed);
    for (uint32_t k = 0; k < params->Samples; k++) {
        pt3 RO;
        out_velocities[k] = pt_visibility_ray(&F, O, V, time, &state, &RO);
        out_origins[3 * k] = RO.x; out_origins[3 * k + 1] = RO.y; out_origins[3 * k + 2] = RO.z;
    }
    if (out_duration) *out_duration = pt_visibility_duration(params->Radius);
    return 0;
}
