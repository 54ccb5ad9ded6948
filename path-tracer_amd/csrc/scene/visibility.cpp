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

// The gathered visibility of DESIGN.md §6 row 15 on the host, from the same
// header: the rays visibility_gather_kernel traces, point-major, and the
// records from any one-bit-per-ray answer over them.

extern "C" int ptsGatherVisibilityRays(const pt_visibility_gather_parameters* params, uint32_t n, const float* points,
                                       const float* normals, float* out_origins, uint32_t* out_velocities,
                                       float* out_durations)
{
    if (!params || (n && (!points || !normals || !out_origins || !out_velocities || !out_durations))) return -1;
    if (!pt_visibility_gather_parameters_ok(params, n)) return -1;
    const uint32_t S = params->Samples;
    const float duration = pt_visibility_duration(params->Radius);
    for (uint32_t i = 0; i < n; i++) {
        const pt3 P = v3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
        const pt_visibility_frame F =
            pt_visibility_gather_frame(v3(normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]));
        const uint32_t s0 = pt_visibility_gather_seed(params->FirstIndex + i, params->Seed);
        for (uint32_t k = 0; k < S; k++) {
            const size_t ray = (size_t)i * S + k;
            pt3 RO;
            out_velocities[ray] = pt_visibility_gather_ray(&F, P, params->Offset, s0, k, &RO);
            out_origins[3 * ray] = RO.x; out_origins[3 * ray + 1] = RO.y; out_origins[3 * ray + 2] = RO.z;
            out_durations[ray] = duration;
        }
    }
    return 0;
}

extern "C" int ptsGatherVisibilityReduce(uint32_t samples, uint32_t n, const uint32_t* packed,
                                         const uint64_t* occluded_bits, pt_visibility_record* out)
{
    if (samples < 1u || samples > PT_AMBIENT_OCCLUSION_MAX_SAMPLES || (samples & (samples - 1u)) != 0u) return -1;
    if (n > PT_VISIBILITY_GATHER_MAX_POINTS || (n && (!packed || !occluded_bits || !out))) return -1;
    for (uint32_t i = 0; i < n; i++) {
        // Ray i S + k is bit (i S + k) % 64 of word (i S + k) / 64; S divides 64.
        const size_t ray = (size_t)i * samples;
        out[i] = pt_visibility_reduce(samples, packed + ray, occluded_bits[ray >> 6] >> (ray & 63u));
    }
    return 0;
}

extern "C" uint32_t ptsVisibilitySkip(uint32_t state, uint32_t steps) { return pt_visibility_skip(state, steps); }

// The sky light gathered at points of DESIGN.md §6 row 16 on the host, from the
// same header: the rays and first wavelengths sky_gather_kernel uses, and the
// records from any one-bit-per-ray answer and per-ray contributions.  The sky
// evaluation itself is the device's: this library has no texture sampler.

extern "C" int ptsSkyGatherRays(const pt_sky_gather_parameters* params, uint32_t n, const float* points,
                                const float* normals, float* out_origins, uint32_t* out_velocities,
                                float* out_durations, float* out_lambda0)
{
    if (!params || (n && (!points || !out_origins || !out_velocities || !out_durations || !out_lambda0))) return -1;
    if (!pt_sky_gather_parameters_ok(params, n)) return -1;
    const bool cosine = params->Lobe == PT_SKY_GATHER_COSINE;
    if (n && cosine && !normals) return -1;
    const uint32_t S = params->Samples;
    const float duration = pt_visibility_duration(params->Radius);
    for (uint32_t i = 0; i < n; i++) {
        const pt3 P = v3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
        const pt3 N = cosine ? v3(normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2])
                             : v3(0, 0, 0);
        const uint32_t s0 = pt_visibility_gather_seed(params->FirstIndex + i, params->Seed);
        for (uint32_t k = 0; k < S; k++) {
            const size_t ray = (size_t)i * S + k;
            pt3 RO;
            out_velocities[ray] = pt_sky_gather_ray(params->Lobe, N, P, params->Offset, s0, k, &RO);
            out_origins[3 * ray] = RO.x; out_origins[3 * ray + 1] = RO.y; out_origins[3 * ray + 2] = RO.z;
            out_durations[ray] = duration;
            out_lambda0[ray] = pt_sky_gather_lambda0(s0, k);
        }
    }
    return 0;
}

extern "C" int ptsSkyGatherReduce(uint32_t samples, uint32_t n, const uint32_t* packed, const uint64_t* occluded_bits,
                                  const float* contributions, pt_sky_record* out)
{
    if (samples < 1u || samples > PT_AMBIENT_OCCLUSION_MAX_SAMPLES || (samples & (samples - 1u)) != 0u) return -1;
    if (n > PT_VISIBILITY_GATHER_MAX_POINTS || (n && (!packed || !occluded_bits || !contributions || !out))) return -1;
    for (uint32_t i = 0; i < n; i++) {
        // Ray i S + k is bit (i S + k) % 64 of word (i S + k) / 64; S divides 64.
        const size_t ray = (size_t)i * samples;
        out[i] = pt_sky_gather_reduce(samples, packed + ray, occluded_bits[ray >> 6] >> (ray & 63u),
                                      contributions + 3 * ray);
    }
    return 0;
}

extern "C" int ptsSkyGatherBasis(uint32_t n, const uint32_t* packed, float* out)
{
    if (n && (!packed || !out)) return -1;
    for (uint32_t i = 0; i < n; i++) pt_sky_gather_basis(pt_reproject_unpack_unit(packed[i]), out + 9 * (size_t)i);
    return 0;
}
