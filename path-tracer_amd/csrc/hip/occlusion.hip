// occlusion.hip — the any-hit query (no reference counterpart; DESIGN.md §6
// row 14): whether anything lies within a ray's duration, one bit per ray, and
// the ambient-occlusion / sky-visibility image built on it, and the same lobe
// gathered at caller-given points (row 15), and the sky's light gathered at
// such points as spherical harmonics (row 16); with their launchers.
//
// The any-hit traversal is Trace() stopped at the first step that leaves an
// accepted intersection in the lane (Hit.ShapeIndex set).  Until that step
// Hit.Time is still the ray's duration, so every box, face and shape test up
// to it runs with the operands of the closest-hit traversal of the same ray,
// in the same order, with the same pushes (those dropped at depth 32
// included): the any-hit traversal is a prefix of the closest-hit one, and
//   occluded(ray) == (ptTraceRays(ray).shape_material != 0xFFFFFFFF)
// for every ray, duration, stack format and scene.  The loops below are
// written around LaneStep / MeshStep as they stand (traverse.hpp): no test is
// restated here, so each shape's own rule at t == duration holds.
#include "extend.hpp"
#include "variants.hpp"
#include "../../../include/pt_reproject.h"
#include "../../../include/pt_guides.h"
#include "../../../include/pt_visibility.h"

namespace ptd {

// The ray of the ptOccludedRays arrays (ptTraceRays' inputs, nothing stored).
struct ray_source_query {
    const float* origins;
    const uint32_t* vel;
    const float* dur;
    PT_DEV bool load(uint32_t i, pt3& O, pt3& V, float& D) const
    {
        O = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
        V = UnpackUnitVector(vel[i]);
        D = dur[i];
        return true;
    }
};

// A lane's world ray, kept in its registers: what TlasStep restores when the
// lane leaves a BLAS.
struct ray_source_held {
    pt3 O, V;
    PT_DEV bool load(uint32_t, pt3& WO, pt3& WV, float& D) const
    {
        WO = O;
        WV = V;
        D = PT_HIT_TIME_LIMIT;
        return true;
    }
};

// Whether anything lies on (O, V) within D.  The lane's stack starts empty
// (LaneBegin / MeshBegin zero the depths; an entry is put before it is read,
// spill rows included).  MESH: the mesh-only loop of a dscene::single_mesh
// scene, in ExtendRay's two passes; its "hit" is MeshHit (the loop carries the
// hit's face, not its shape).  Of the general loop's hit only Shape is read
// afterwards: Prim, C, HA and HB are dead and the compiler drops them.
template <bool SPILL, int CAP, class E, bool MESH, class Src, class Stats>
PT_DEV bool AnyHit(const dscene& S, tstack<SPILL, CAP, E>& st, const Src& src, uint32_t slot, pt3 O, pt3 V, float D,
                   Stats& ss)
{
    lane_state Ln;
    if constexpr (MESH) {
        MeshBegin(S, Ln, O, V, D);
        if (Ln.exact) {
            while (!MeshHit(Ln) && !MeshStep<true>(S, Ln, st)) {}
        } else {
            while (!MeshHit(Ln) && !MeshStep<false>(S, Ln, st)) {}
        }
        return MeshHit(Ln);   // (the mesh-only loop keeps the hit's face, not Shape: no MeshEnd needed)
    } else {
        LaneBegin(S, Ln, O, V, D);
        if (S.g.ShapeCount != 0) {
            while (Ln.Shape == SHAPE_INDEX_NONE && !LaneStep<SPILL, CAP, Src, Stats, true, E>(S, Ln, st, src, slot, ss)) {}
        }
    }
    return Ln.Shape != SHAPE_INDEX_NONE;
}

// One ray per thread; each wave ballots "occluded" and its first lane stores
// the word (ray i: word i / 64, bit i % 64).  Lanes at and beyond n trace
// nothing and vote 0, so the last word's tail bits are 0 and every word of the
// mask is written.
//
// (Occupancy: 8 waves per SIMD declared.  A 256-thread block is one wave per
// SIMD, so 8 resident blocks per CU are the most the wave slots hold, and the
// LDS allows them: 10 KB (u16 stack) or 20 KB (u32 stack, or u16 + node cache)
// per block of 160 KB.  What is left to decide is the 64-VGPR budget of 8
// waves: the general loop's instantiations take 53-55 VGPRs (extend's 66-68:
// 7 waves), the mesh-only ones 42-62, none with scratch
// (profiles/occlusion/resources.txt), so the bound costs nothing and the
// general loop gains the wave extend's registers deny it.)
template <bool SPILL, int CAP, class E, bool NC, bool MESH>
__global__ __launch_bounds__(256, 8) void occlusion_kernel(dscene S, ray_source_query src, uint32_t n, uint32_t* spill,
                                                           uint32_t spill_stride, unsigned long long* mask)
{
    __shared__ E smem[CAP * 256];
    __shared__ float4 ncache[NC ? 4 * PT_NODE_CACHE_PAIRS : 1];
    const uint32_t ncn = NC ? NodeCacheFill(S, ncache) : 0u;
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    bool occluded = false;
    if (slot < n) {
        tstack<SPILL, CAP, E> st;
        st.lds = &smem[threadIdx.x];
        st.spill = spill + slot;
        st.stride = spill_stride;
        st.nc = ncache;
        st.ncn = ncn;
        pt3 O, V;
        float D;
        src.load(slot, O, V, D);
        no_stats ns;
        occluded = AnyHit<SPILL, CAP, E, MESH>(S, st, src, slot, O, V, D, ns);
    }
    const unsigned long long word = __ballot(occluded);
    if ((threadIdx.x & 63u) == 0 && slot < n) mask[slot >> 6] = word;
}

PT_DEV uint32_t OccWaveSum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

PT_DEV uint32_t OccWaveMax(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

// Diagnostic twin (extend_stats_kernel's counters, out[] in its order): the
// general LaneStep with per-lane counters and the same early exit.
template <bool SPILL, int CAP, class E>
__global__ __launch_bounds__(256) void occlusion_stats_kernel(dscene S, ray_source_query src, uint32_t n,
                                                              uint32_t* spill, uint32_t spill_stride,
                                                              unsigned long long* out, uint32_t* steps)
{
    __shared__ E smem[CAP * 256];
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    tstack<SPILL, CAP, E> st;
    st.lds = &smem[threadIdx.x];
    st.spill = spill + slot;
    st.stride = spill_stride;
    lane_stats ss;
    uint32_t ray = 0;
    if (slot < n) {
        ray = 1;
        pt3 O, V;
        float D;
        src.load(slot, O, V, D);
        AnyHit<SPILL, CAP, E, false>(S, st, src, slot, O, V, D, ss);
        if (steps) steps[slot] = ss.steps;
    }
    uint32_t v[14] = {OccWaveSum(ray), OccWaveSum(ss.steps), OccWaveMax(ss.steps) * 64u, OccWaveSum(ss.internals),
                      OccWaveSum(ss.leaves), OccWaveSum(ss.faces), OccWaveSum(ss.pops), OccWaveSum(ss.shapes), 1u,
                      OccWaveSum(ss.uniq[0]), OccWaveSum(ss.uniq[1]), OccWaveSum(ss.uniq[2]), OccWaveSum(ss.uniq[3]),
                      OccWaveSum(ss.uniq[4])};
    if ((threadIdx.x & 63u) == 0)
        for (int i = 0; i < 14; i++) atomicAdd(&out[i], (unsigned long long)v[i]);
}

// --- ambient occlusion / sky visibility (include/pt_visibility.h) -----------------

struct ambient_args {
    uint32_t camera;
    uint32_t w, h;
    uint32_t tiles_x;
    uint32_t samples;
    uint32_t seed;
    float duration;
};

// A lane per pixel, looping over the pixel's samples: the pixel's count is a
// register of its lane, so the image needs no reduction and no atomics, the
// primary trace runs once per pixel, and the lanes of a wave (a 16 x 4 patch
// of one surface, usually) trace sample k together, which are rays of one
// cosine lobe from neighbouring points.  Pixels map in 16 x 16 tiles like
// guides_kernel's; the primary trace and the samples' any-hit traces share the
// lane's stack column, each from an empty stack.
template <bool SPILL, int CAP, class E>
__global__ __launch_bounds__(256) void ambient_occlusion_kernel(dscene S, ambient_args P, uint32_t* spill,
                                                                uint32_t spill_stride, float4* __restrict__ out)
{
    __shared__ E smem[CAP * 256];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t t = i >> 8, l = i & 255u;
    const uint32_t ty = t / P.tiles_x;
    const uint32_t x = (t - ty * P.tiles_x) * 16 + (l & 15u);
    const uint32_t y = ty * 16 + (l >> 4);
    if (x >= P.w || y >= P.h) return;
    tstack<SPILL, CAP, E> st;
    st.lds = &smem[threadIdx.x];
    st.spill = spill + i;
    st.stride = spill_stride;

    const float Sf = (float)P.samples;
    float4* const px = out + ((size_t)y * P.w + x);
    pt3 O, V;
    const bool known = pt_reproject_central_ray(&S.cameras[P.camera], x, y, P.w, P.h, &O, &V);
    lane_state Ln;
    LaneBegin(S, Ln, O, V, PT_HIT_TIME_LIMIT);
    no_stats ns;
    {
        const ray_source_held cur{O, V};
        if (known && S.g.ShapeCount != 0)
            while (!LaneStep<SPILL, CAP, ray_source_held, no_stats, true, E>(S, Ln, st, cur, i, ns)) {}
    }
    if (Ln.Shape == SHAPE_INDEX_NONE) {
        *px = make_float4(Sf, Sf, Sf, Sf);
        return;
    }
    // The guide record's normal (guides_kernel): compact hit -> attributes ->
    // the packed normal's round trip.
    const float4 h = CompactHit(Ln, S.vidx21 != 0);
    const float2 c = make_float2(Ln.C.y, Ln.C.z);
    uint32_t Material;
    pt3 Nrm, TX;
    pt2 UV;
    HitAttributesRecord(S, Ln.Shape, h, c, Material, Nrm, TX, UV);
    const pt3 Nq = UnpackUnitVector(PackUnitVector(Nrm));
    const pt_visibility_frame F = pt_visibility_make_frame(Nq, V);
    uint32_t state = pt_visibility_seed(x, y, P.seed);
    uint32_t u = 0;
    for (uint32_t k = 0; k < P.samples; k++) {
        pt3 RO;
        const pt3 RV = pt_reproject_unpack_unit(pt_visibility_ray(&F, O, V, h.x, &state, &RO));
        const ray_source_held cur{RO, RV};
        u += AnyHit<SPILL, CAP, E, false>(S, st, cur, i, RO, RV, P.duration, ns) ? 0u : 1u;
    }
    const float uf = (float)u;
    *px = make_float4(uf, uf, uf, Sf);
}

// --- visibility gathered at caller-given points --------------

struct gather_args {
    const float* points;    // 3 floats per point
    const float* normals;   // 3 floats per point
    uint32_t n;             // points of this launch; n << shift lanes are live
    uint32_t shift;         // log2 of the samples per point
    uint32_t seed;
    uint32_t first;         // stream index of point 0
    float offset;
    float duration;
};

// A lane per (point, sample): the S lanes of a point are an aligned segment of
// one wave (S is a power of two up to 64), so the point's mask is that
// segment of the wave's ballot and its bent vector log2 S rounds of
// __shfl_xor within it: no LDS, no atomics, one result whatever the order of
// the lanes' arrival.  There is no primary trace to share, so a list of points
// fills n S lanes where a lane per point would fill n.  Every lane reaches the
// node-cache fill's barrier, the ballot and the shuffles: lanes at and beyond
// n S trace nothing, vote 0 and add zeros in segments of their own.  Across the
// trace a lane keeps its ray (ray_source_held) and the packed word; the
// velocity is unpacked again for the sum.
template <bool SPILL, int CAP, class E, bool NC, bool MESH>
__global__ __launch_bounds__(256, 8) void visibility_gather_kernel(dscene S, gather_args P, uint32_t* spill,
                                                                   uint32_t spill_stride, float4* __restrict__ out)
{
    __shared__ E smem[CAP * 256];
    __shared__ float4 ncache[NC ? 4 * PT_NODE_CACHE_PAIRS : 1];
    const uint32_t ncn = NC ? NodeCacheFill(S, ncache) : 0u;
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t samples = 1u << P.shift;
    const uint32_t point = g >> P.shift, k = g & (samples - 1u);
    const bool live = point < P.n;
    bool occluded = false;
    uint32_t word = 0;
    if (live) {
        tstack<SPILL, CAP, E> st;
        st.lds = &smem[threadIdx.x];
        st.spill = spill + g;
        st.stride = spill_stride;
        st.nc = ncache;
        st.ncn = ncn;
        const float* p = P.points + 3 * (size_t)point;
        const float* nrm = P.normals + 3 * (size_t)point;
        const pt_visibility_frame F = pt_visibility_gather_frame(v3(nrm[0], nrm[1], nrm[2]));
        pt3 RO;
        word = pt_visibility_gather_ray(&F, v3(p[0], p[1], p[2]), P.offset,
                                        pt_visibility_gather_seed(P.first + point, P.seed), k, &RO);
        const ray_source_held cur{RO, pt_reproject_unpack_unit(word)};
        no_stats ns;
        occluded = AnyHit<SPILL, CAP, E, MESH>(S, st, cur, g, cur.O, cur.V, P.duration, ns);
    }
    const unsigned long long ballot = __ballot(occluded);
    pt3 b = live && !occluded ? pt_reproject_unpack_unit(word) : v3(0, 0, 0);
    for (uint32_t o = 1; o < samples; o <<= 1) {
        b.x = b.x + __shfl_xor(b.x, (int)o, 64);
        b.y = b.y + __shfl_xor(b.y, (int)o, 64);
        b.z = b.z + __shfl_xor(b.z, (int)o, 64);
    }
    if (live && k == 0) {
        const unsigned long long segment = ballot >> (threadIdx.x & 63u);
        const unsigned long long mask = P.shift == 6u ? segment : segment & ((1ull << samples) - 1ull);
        const float Sf = (float)samples;
        out[2 * (size_t)point] = make_float4(b.x, b.y, b.z, Sf - (float)__popcll(mask));
        reinterpret_cast<uint4*>(out)[2 * (size_t)point + 1] =
            make_uint4((uint32_t)mask, (uint32_t)(mask >> 32), __float_as_uint(Sf), 0u);
    }
}

// --- sky light gathered at caller-given points ----------------

struct sky_gather_args {
    const float* points;    // 3 floats per point
    const float* normals;   // 3 floats per point; not read (may be null) with lobe SPHERE
    uint32_t n;             // points of this launch; n << shift lanes are live
    uint32_t shift;         // log2 of the samples per point
    uint32_t seed;
    uint32_t first;         // stream index of point 0
    float offset;
    float duration;
    uint32_t lobe;          // PT_SKY_GATHER_COSINE / PT_SKY_GATHER_SPHERE
};

// visibility_gather_kernel's shape: a lane per (point, sample), a point an
// aligned segment of one wave, every lane at the node-cache fill's barrier,
// the ballot and the shuffles.  After the trace the open lanes alone look the
// sky up along their ray (texture sample, four parametric spectra, four
// observer values: EscapeContribution of a fresh path); occluded and dead lanes
// hold a zero contribution, and every lane forms the 27 products with its
// basis, so a zero carries the sign the definition gives it.  The 27 sums
// take log2 S rounds of __shfl_xor within the segment, after which every lane
// of the segment holds the whole record as 8 float4: lane k < 8 stores the
// float4s j with j % S == k (with S >= 8, one each), constant register indices
// under a predicate, so nothing is indexed dynamically.
template <bool SPILL, int CAP, class E, bool NC, bool MESH>
__global__ __launch_bounds__(256, 8) void sky_gather_kernel(dscene S, sky_gather_args P, uint32_t* spill,
                                                            uint32_t spill_stride, float4* __restrict__ out)
{
    __shared__ E smem[CAP * 256];
    __shared__ float4 ncache[NC ? 4 * PT_NODE_CACHE_PAIRS : 1];
    const uint32_t ncn = NC ? NodeCacheFill(S, ncache) : 0u;
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t samples = 1u << P.shift;
    const uint32_t point = g >> P.shift, k = g & (samples - 1u);
    const bool live = point < P.n;
    bool occluded = false;
    uint32_t word = 0;
    if (live) {
        tstack<SPILL, CAP, E> st;
        st.lds = &smem[threadIdx.x];
        st.spill = spill + g;
        st.stride = spill_stride;
        st.nc = ncache;
        st.ncn = ncn;
        const float* p = P.points + 3 * (size_t)point;
        pt3 Nrm = v3(0, 0, 0);
        if (P.lobe == PT_SKY_GATHER_COSINE) {
            const float* nrm = P.normals + 3 * (size_t)point;
            Nrm = v3(nrm[0], nrm[1], nrm[2]);
        }
        pt3 RO;
        word = pt_sky_gather_ray(P.lobe, Nrm, v3(p[0], p[1], p[2]), P.offset,
                                 pt_visibility_gather_seed(P.first + point, P.seed), k, &RO);
        const ray_source_held cur{RO, pt_reproject_unpack_unit(word)};
        no_stats ns;
        occluded = AnyHit<SPILL, CAP, E, MESH>(S, st, cur, g, cur.O, cur.V, P.duration, ns);
    }
    const unsigned long long ballot = __ballot(occluded);
    const pt3 V = pt_reproject_unpack_unit(word);
    pt3 Ck = v3(0, 0, 0);
    if (live && !occluded) {
        const float L0 = pt_sky_gather_lambda0(pt_visibility_gather_seed(P.first + point, P.seed), k);
        Ck = EscapeContribution(S, V, PathLambda(L0), v4s(1.0f), 4.0f);
    }
    float Y[9];
    pt_sky_gather_basis(V, Y);
    float r[32];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        r[3 * i] = Ck.x * Y[i];
        r[3 * i + 1] = Ck.y * Y[i];
        r[3 * i + 2] = Ck.z * Y[i];
    }
    for (uint32_t o = 1; o < samples; o <<= 1) {
#pragma unroll
        for (int e = 0; e < 27; e++) r[e] = r[e] + __shfl_xor(r[e], (int)o, 64);
    }
    const unsigned long long segment = ballot >> (threadIdx.x & 63u & ~(samples - 1u));
    const unsigned long long mask = P.shift == 6u ? segment : segment & ((1ull << samples) - 1ull);
    const float Sf = (float)samples;
    r[27] = Sf - (float)__popcll(mask);
    r[28] = __uint_as_float((uint32_t)mask);
    r[29] = __uint_as_float((uint32_t)(mask >> 32));
    r[30] = Sf;
    r[31] = __uint_as_float(0u);
    if (live && k < 8u) {
        float4* const rec = out + 8 * (size_t)point;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++)
            if ((j & (samples - 1u)) == k) rec[j] = make_float4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
    }
}

}  // namespace ptd

// --- launchers (called from rt_probe.hip and rt_post.hip) --------------------------

using ptv::Blocks;

// The one selection of an occlusion_kernel instantiation: the stack entry
// width, the spill, the node cache and the mesh-only loop follow the scene as
// extend's do (LaunchExtend).
hipError_t pt_launch_occluded_rays(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                   const float* dur, uint32_t* spill, unsigned long long* mask, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const ptd::ray_source_query src{origins, vel, dur};
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        const bool cache = S.node_cache && ptv::HasOcclusionNodeCache<E>(spill != nullptr);
        ptv::SelectFlags(
            [&](auto SPILL, auto NC, auto MESH) {
                if constexpr (!NC || ptv::HasOcclusionNodeCache<E>(SPILL))
                    hipLaunchKernelGGL((ptd::occlusion_kernel<SPILL, PT_EXTEND_CAP, E, NC, MESH>), dim3(Blocks(n)),
                                       dim3(256), 0, st, S, src, n, spill, n, mask);
            },
            spill != nullptr, cache, S.single_mesh != 0);
    });
    return hipGetLastError();
}

// visibility_gather_kernel's instantiation is occlusion_kernel's, chosen the same way.
hipError_t pt_launch_gather_visibility(const ptd::dscene& S, uint32_t n, const float* points, const float* normals,
                                       const pt_visibility_gather_parameters* p, uint32_t first_index, uint32_t* spill,
                                       float4* out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    ptd::gather_args P;
    P.points = points;
    P.normals = normals;
    P.n = n;
    P.shift = 0;
    while ((1u << P.shift) < p->Samples) P.shift++;
    P.seed = p->Seed;
    P.first = first_index;
    P.offset = p->Offset;
    P.duration = pt_visibility_duration(p->Radius);
    const uint32_t lanes = n << P.shift;
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        const bool cache = S.node_cache && ptv::HasOcclusionNodeCache<E>(spill != nullptr);
        ptv::SelectFlags(
            [&](auto SPILL, auto NC, auto MESH) {
                if constexpr (!NC || ptv::HasOcclusionNodeCache<E>(SPILL))
                    hipLaunchKernelGGL((ptd::visibility_gather_kernel<SPILL, PT_EXTEND_CAP, E, NC, MESH>),
                                       dim3(Blocks(lanes)), dim3(256), 0, st, S, P, spill, lanes, out);
            },
            spill != nullptr, cache, S.single_mesh != 0);
    });
    return hipGetLastError();
}

// sky_gather_kernel's instantiation is occlusion_kernel's, chosen the same way.
hipError_t pt_launch_gather_sky_light(const ptd::dscene& S, uint32_t n, const float* points, const float* normals,
                                      const pt_sky_gather_parameters* p, uint32_t first_index, uint32_t* spill,
                                      float4* out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    ptd::sky_gather_args P;
    P.points = points;
    P.normals = normals;
    P.n = n;
    P.shift = 0;
    while ((1u << P.shift) < p->Samples) P.shift++;
    P.seed = p->Seed;
    P.first = first_index;
    P.offset = p->Offset;
    P.duration = pt_visibility_duration(p->Radius);
    P.lobe = p->Lobe;
    const uint32_t lanes = n << P.shift;
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        const bool cache = S.node_cache && ptv::HasOcclusionNodeCache<E>(spill != nullptr);
        ptv::SelectFlags(
            [&](auto SPILL, auto NC, auto MESH) {
                if constexpr (!NC || ptv::HasOcclusionNodeCache<E>(SPILL))
                    hipLaunchKernelGGL((ptd::sky_gather_kernel<SPILL, PT_EXTEND_CAP, E, NC, MESH>),
                                       dim3(Blocks(lanes)), dim3(256), 0, st, S, P, spill, lanes, out);
            },
            spill != nullptr, cache, S.single_mesh != 0);
    });
    return hipGetLastError();
}

hipError_t pt_launch_occluded_rays_stats(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                         const float* dur, uint32_t* spill, unsigned long long* out, uint32_t* steps,
                                         hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const ptd::ray_source_query src{origins, vel, dur};
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        ptv::SelectFlags(
            [&](auto SPILL) {
                hipLaunchKernelGGL((ptd::occlusion_stats_kernel<SPILL, PT_EXTEND_CAP, E>), dim3(Blocks(n)), dim3(256),
                                   0, st, S, src, n, spill, n, out, steps);
            },
            spill != nullptr);
    });
    return hipGetLastError();
}

hipError_t pt_launch_ambient_occlusion(const ptd::dscene& S, uint32_t camera_index, uint32_t w, uint32_t h,
                                       const pt_ambient_occlusion_parameters* p, uint32_t* spill, float4* out,
                                       hipStream_t st)
{
    ptd::ambient_args P;
    P.camera = camera_index;
    P.w = w;
    P.h = h;
    P.tiles_x = (w + 15) / 16;
    P.samples = p->Samples;
    P.seed = p->Seed;
    P.duration = pt_visibility_duration(p->Radius);
    const uint32_t tiles = P.tiles_x * ((h + 15) / 16);
    if (tiles == 0) return hipSuccess;
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        ptv::SelectFlags(
            [&](auto SPILL) {
                hipLaunchKernelGGL((ptd::ambient_occlusion_kernel<SPILL, PT_EXTEND_CAP, E>), dim3(tiles), dim3(256), 0,
                                   st, S, P, spill, tiles * 256, out);
            },
            spill != nullptr);
    });
    return hipGetLastError();
}
