// probe.hip — test probes of the numerics convention, of the texture
// sampler and of the traversal's slab test on the device (ptEvalNumerics,
// ptSampleTextures, ptEvalSlabTest; no reference counterpart).  A translation
// unit of its own, compiled with the product's flags: the probes see the code
// generation the kernels see, and the kernels' own objects do not change.
// Every function under test is called as the kernels call it (include/pt_fp.h
// through pt_numerics.h, pt_device.hpp, traverse.hpp); nothing is restated
// here.
#include "traverse.hpp"
#include "kernels.hpp"
#include "../../../include/pt_numerics.h"

namespace ptd {

// One thread per element: loads the operand words the op reads, evaluates,
// stores outputs(op) result words.  op is uniform across the launch.
__global__ __launch_bounds__(256) void numerics_probe_kernel(uint32_t op, uint32_t n, const uint32_t* a,
                                                             const uint32_t* b, const uint32_t* c, uint32_t* out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t operands = pt_numerics_operands(op), outputs = pt_numerics_outputs(op);
    const uint32_t ua = a[i];
    const uint32_t ub = operands > 1 ? b[i] : 0u;
    const uint32_t uc = operands > 2 ? c[i] : 0u;
    uint32_t r[3] = {0u, 0u, 0u};
    if (!pt_numerics_eval(op, ua, ub, uc, r)) {
        const float fa = pt_u2f(ua), fb = pt_u2f(ub), fc = pt_u2f(uc);
        if (op == PT_NUM_PACK_UNIT_VECTOR) {
            r[0] = PackUnitVector(v3(fa, fb, fc));
        } else if (op == PT_NUM_UNPACK_UNIT_VECTOR) {
            const pt3 V = UnpackUnitVector(ua);
            r[0] = pt_f2u(V.x); r[1] = pt_f2u(V.y); r[2] = pt_f2u(V.z);
        } else if (op == PT_NUM_FAST_RCP) {
            r[0] = pt_f2u(FastRcp(fa));
        } else if (op == PT_NUM_XDIV) {
            r[0] = pt_f2u(XDiv(fa, fb, RecipForDiv(fb)));
        }
    }
    for (uint32_t k = 0; k < outputs; k++) out[(size_t)i * outputs + k] = r[k];
}

// One thread per sample: SampleTexture of texture index[i] (checked against
// the scene's texture count on the host) at uv[i].  UNIT selects the texel
// wrap: the two-select form of the lean shade kernel, or the remainder.
template <bool UNIT>
__global__ __launch_bounds__(256) void sample_textures_kernel(dscene S, uint32_t n, const uint32_t* index,
                                                              const float2* uv, float4* rgba)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float2 t = uv[i];
    const pt4 v = SampleTexture<UNIT>(S, index[i], v2(t.x, t.y));
    rgba[i] = make_float4(v.x, v.y, v.z, v.w);
}

// One thread per case: the level ray as SetLevelRay sets it (its reciprocal
// and its `exact` flag under S.fast_div, the only field of S that is read),
// then the case's box as both children of IntersectBoxPair, with the
// arguments TlasStep and the BLAS steps pass.
__global__ __launch_bounds__(256) void slab_probe_kernel(dscene S, uint32_t n, const float* origin,
                                                         const float* velocity, const float* reach,
                                                         const float* box_min, const float* box_max, uint32_t* entry,
                                                         uint32_t* exact)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t k = 3 * (size_t)i;
    lane_state L;
    SetLevelRay(S, L, v3(origin[k], origin[k + 1], origin[k + 2]), v3(velocity[k], velocity[k + 1], velocity[k + 2]));
    const float4 b0 = make_float4(box_min[k], box_min[k + 1], box_min[k + 2], 0.0f);
    const float4 b1 = make_float4(box_max[k], box_max[k + 1], box_max[k + 2], 0.0f);
    float TA, TB;
    IntersectBoxPair(L.O, L.V, L.Y, reach[i], b0, b1, b0, b1, L.exact, TA, TB);
    entry[i] = pt_f2u(TA);
    exact[i] = L.exact ? 1u : 0u;
}

}  // namespace ptd

hipError_t pt_launch_numerics_probe(uint32_t op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                    uint32_t* out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u)), block(256);
    hipLaunchKernelGGL(ptd::numerics_probe_kernel, grid, block, 0, st, op, n, a, b, c, out);
    return hipGetLastError();
}

hipError_t pt_launch_sample_textures(const ptd::dscene& S, uint32_t n, const uint32_t* index, const float2* uv,
                                     bool unit_wrap, float4* rgba, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u)), block(256);
    if (unit_wrap) hipLaunchKernelGGL(ptd::sample_textures_kernel<true>, grid, block, 0, st, S, n, index, uv, rgba);
    else hipLaunchKernelGGL(ptd::sample_textures_kernel<false>, grid, block, 0, st, S, n, index, uv, rgba);
    return hipGetLastError();
}

hipError_t pt_launch_slab_probe(const ptd::dscene& S, uint32_t n, const float* origin, const float* velocity,
                                const float* reach, const float* box_min, const float* box_max, uint32_t* entry,
                                uint32_t* exact, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)n + 255u) / 256u)), block(256);
    hipLaunchKernelGGL(ptd::slab_probe_kernel, grid, block, 0, st, S, n, origin, velocity, reach, box_min, box_max, entry,
                       exact);
    return hipGetLastError();
}
