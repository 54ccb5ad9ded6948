// extend.hip — the extend kernels: Trace() of every ray -> hit record
// (basic_trace.glsl:7-16, scene.glsl.inc:304-611), for the renderer's slots
// and for the arrays of the ray-query API, with the traversal statistics and
// the length table's classes; and their launchers.
#include "extend.hpp"
#include "variants.hpp"

namespace ptd {

// (The mesh-only instantiations without the node cache declare 8 waves per
// SIMD: left at MINW the compiler gave them 75-78 VGPRs, 6 waves, where 58-63
// hold the loop without a spill; C3 extend on the two 32-bit stack formats
// 0.3142-0.3149 -> 0.3036-0.3038 and 0.3313-0.3328 -> 0.3228-0.3243 ms.  The
// one with the cache takes 56 either way.)
template <class Src, bool SPILL, int MINW, int CAP, class E = uint32_t, bool NC = false, bool MESH = false,
          bool TRAIN = false, bool RUN = false>
__global__ __launch_bounds__(256, (MESH && !NC) ? 8 : MINW) void extend_kernel(dscene S, Src src, uint32_t n,
                                                                               uint32_t* spill, uint32_t spill_stride)
{
    __shared__ E smem[CAP * 256];
    __shared__ float4 ncache[NC ? 4 * PT_NODE_CACHE_PAIRS : 1];
    if constexpr (kRendererSource<Src>) {
        if (src.L.stop && *src.L.stop) return;   // a guarded round past the frame's target
    }
    const uint32_t ncn = NC ? NodeCacheFill(S, ncache) : 0u;
    // Tile order: the slot renderer dispatches the tiles whose waves took
    // longest in the previous round first (tile_order_kernel), so the
    // kernel's tail holds short blocks; each wave records its own time.
    // RUN: the order lists block-map units (ExtendTile), keyed by their own
    // waves' times.
    uint32_t tile = blockIdx.x;
    bool timed = false;
    if constexpr (kRendererSource<Src>) {
        if (src.L.order) {
            tile = src.L.order[blockIdx.x];
            timed = true;
        }
    }
    ExtendTile<Src, SPILL, CAP, E, MESH, TRAIN, RUN>(S, src, n, spill, spill_stride, smem, tile, timed, ncache, ncn);
}

// The length table's finalize (LENGTH order), one block after a call's
// training rounds.  A key's mean steps in 1/16 (steps are capped at 255: 4 096
// values); the classes are cut at the count-weighted 1/7 .. 6/7 quantiles of
// the means -- bound j = the first mean whose keys, with those below, hold
// j/7 of the rays -- and a key's class is the number of bounds below its mean.
// Keys without a sample take the middle class.  A count above 2^16 is shifted
// down with its sum until it fits, so the words never overflow and old rounds
// fade; everything is integer arithmetic on order-independent sums, so the
// classes are the same on every run.
constexpr uint32_t LEN_MEAN_BINS = 4096;
__global__ __launch_bounds__(1024) void length_classes_kernel(uint32_t* sum, uint32_t* cnt, uint8_t* cls)
{
    __shared__ unsigned long long hist[LEN_MEAN_BINS];
    __shared__ unsigned long long part[1024];
    __shared__ uint32_t bound[PT_RAYKEY_CLASSES - 1];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < LEN_MEAN_BINS; i += 1024) hist[i] = 0;
    if (t < PT_RAYKEY_CLASSES - 1) bound[t] = LEN_MEAN_BINS;
    __syncthreads();
    auto mean = [](uint32_t s, uint32_t c) { return min((s << 4) / c, LEN_MEAN_BINS - 1u); };   // c < 2^16, s <= 255 c
    for (uint32_t i = t; i < PT_RAYKEY_COUNT; i += 1024) {
        uint32_t c = cnt[i], s = sum[i];
        if (c > 65535u) {
            const uint32_t sh = 16u - (uint32_t)__clz(c);
            c >>= sh;
            s >>= sh;
            cnt[i] = c;
        }
        s = min(s, 255u * c);   // a sum that wrapped in a very long call
        sum[i] = s;
        if (c) atomicAdd(&hist[mean(s, c)], (unsigned long long)c);
    }
    __syncthreads();
    // Thread t owns bins 4 t .. 4 t + 3; a block scan of the threads' sums.
    unsigned long long h[4], own = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) { h[k] = hist[4 * t + k]; own += h[k]; }
    part[t] = own;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const unsigned long long v = t >= o ? part[t - o] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const unsigned long long total = part[1023];
    unsigned long long before = part[t] - own;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const unsigned long long after = before + h[k];
        for (uint32_t j = 1; j < PT_RAYKEY_CLASSES; j++)
            if (before * PT_RAYKEY_CLASSES < j * total && after * PT_RAYKEY_CLASSES >= j * total) bound[j - 1] = 4 * t + k;
        before = after;
    }
    __syncthreads();
    for (uint32_t i = t; i < PT_RAYKEY_COUNT; i += 1024) {
        const uint32_t c = cnt[i];   // this thread's own writes above
        uint32_t k = PT_RAYKEY_CLASSES / 2;
        if (c) {
            const uint32_t m = mean(sum[i], c);
            k = 0;
            for (uint32_t j = 0; j < PT_RAYKEY_CLASSES - 1; j++) k += m > bound[j] ? 1u : 0u;
        }
        cls[i] = (uint8_t)k;
    }
}

PT_DEV uint32_t WaveSum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

PT_DEV uint32_t WaveMax(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

// Diagnostic extend: the same traversal with per-lane counters, reduced per
// wave into out[]: {rays, lane steps, wave steps x 64, internal nodes, BLAS
// leaves, faces tested, stack pops, TLAS leaves (shapes), waves, then the
// internal-BLAS wave steps by distinct node count 1, 2, 3-4, 5-8, >8}.  SIMD
// efficiency of the traversal loop = lane steps / (wave steps x 64).
template <class Src, bool SPILL, int CAP, class E = uint32_t>
__global__ __launch_bounds__(256) void extend_stats_kernel(dscene S, Src src, uint32_t n, uint32_t* spill,
                                                           uint32_t spill_stride, unsigned long long* out,
                                                           uint32_t* steps)
{
    __shared__ E smem[CAP * 256];
    uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    tstack<SPILL, CAP, E> st;
    st.lds = &smem[threadIdx.x];
    st.spill = spill + slot;
    st.stride = spill_stride;
    lane_stats ss;
    pt3 O, V;
    float D;
    uint32_t ray = 0;
    if (slot < n && src.load(slot, O, V, D)) {
        ray = 1;
        lane_state Ln;
        LaneBegin(S, Ln, O, V, D);
        if (S.g.ShapeCount != 0)
            while (!LaneStep<SPILL, CAP, Src, lane_stats, true, E>(S, Ln, st, src, slot, ss)) {}
        src.store(slot, Ln, S.vidx21 != 0);
    }
    if (steps && slot < n) steps[slot] = ss.steps;   // per position (0: no ray)
    uint32_t v[14] = {WaveSum(ray), WaveSum(ss.steps), WaveMax(ss.steps) * 64u, WaveSum(ss.internals),
                      WaveSum(ss.leaves), WaveSum(ss.faces), WaveSum(ss.pops), WaveSum(ss.shapes), 1u,
                      WaveSum(ss.uniq[0]), WaveSum(ss.uniq[1]), WaveSum(ss.uniq[2]), WaveSum(ss.uniq[3]),
                      WaveSum(ss.uniq[4])};
    if ((threadIdx.x & 63u) == 0)
        for (int i = 0; i < 14; i++) atomicAdd(&out[i], (unsigned long long)v[i]);
}

}  // namespace ptd

// --- launchers (called from rt_rounds.hip and rt_probe.hip) ----------------------

using ptv::Blocks;

uint32_t pt_extend_stack_cap() { return PT_EXTEND_CAP; }

// The one selection of an extend_kernel instantiation, for the render launch,
// the training launch and the ray query.  n: rays (the spill stride and the
// bound of the ray index); blocks: the launch's 256-ray blocks (the
// renderer's tiles).  MESH: the mesh-only loop (dscene::single_mesh scenes;
// every variant has one); the statistics, preview and fused round kernels
// stay on the general LaneStep.
template <class Src>
static hipError_t LaunchExtend(const ptd::dscene& S, const Src& src, uint32_t n, uint32_t blocks, uint32_t* spill,
                               bool train, bool run, hipStream_t st)
{
    constexpr bool renderer = ptd::kRendererSource<Src>;
    if (train && !ptv::HasTrain(renderer, S.single_mesh != 0, spill != nullptr)) return hipErrorNotSupported;
    if (run && !ptv::HasRunMap(renderer, S.single_mesh != 0, spill != nullptr)) return hipErrorNotSupported;
    if (n == 0 || blocks == 0) return hipSuccess;
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        const bool cache = S.node_cache && ptv::HasNodeCache<E>(spill != nullptr);
        ptv::SelectFlags(
            [&](auto SPILL, auto NC, auto MESH, auto TRAIN, auto RUN) {
                if constexpr ((!NC || ptv::HasNodeCache<E>(SPILL)) && (!TRAIN || ptv::HasTrain(renderer, MESH, SPILL)) &&
                              (!RUN || ptv::HasRunMap(renderer, MESH, SPILL)))
                    hipLaunchKernelGGL(
                        (ptd::extend_kernel<Src, SPILL, PT_EXTEND_MINW, PT_EXTEND_CAP, E, NC, MESH, TRAIN, RUN>),
                        dim3(blocks), dim3(256), 0, st, S, src, n, spill, n);
            },
            spill != nullptr, cache, S.single_mesh != 0, train, run);
    });
    return hipGetLastError();
}

bool pt_length_train_supported(const ptd::dscene& S, bool spill) { return ptv::HasTrain(true, S.single_mesh != 0, spill); }

bool pt_block_map_run_supported(const ptd::dscene& S, bool spill) { return ptv::HasRunMap(true, S.single_mesh != 0, spill); }

hipError_t pt_launch_extend(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, uint32_t* spill,
                            hipStream_t st, bool train, const uint32_t* units, uint32_t unit_count)
{
    if (train && (!L.len_sum || !L.len_cnt || !L.len_cam)) return hipErrorNotSupported;
    if (!units) return LaunchExtend(S, ptd::ray_source_slots{L, F}, L.n, L.tile_count, spill, train, false, st);
    // RUN: the kernel's order is the unit order, one block per unit.
    ptd::dslots U = L;
    U.order = const_cast<uint32_t*>(units);
    return LaunchExtend(S, ptd::ray_source_slots{U, F}, L.n, unit_count, spill, train, true, st);
}

hipError_t pt_launch_trace_rays_extend(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                       const float* dur, float4* hit, float2* hc, uint32_t* spill, hipStream_t st)
{
    return LaunchExtend(S, ptd::ray_source_arrays{origins, vel, dur, hit, hc}, n, Blocks(n), spill, false, false, st);
}

hipError_t pt_launch_trace_rays(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                const float* dur, float4* hit, float2* hc, float4* rec, float2* uv, uint32_t* spill,
                                hipStream_t st)
{
    hipError_t e = pt_launch_trace_rays_extend(S, n, origins, vel, dur, hit, hc, spill, st);
    if (e != hipSuccess) return e;
    return pt_launch_finalize(S, n, hit, hc, rec, uv, st);
}

// The same LDS stack capacity and entry width as the render kernel.
template <class Src>
static hipError_t LaunchExtendStats(const ptd::dscene& S, const Src& src, uint32_t n, uint32_t* spill,
                                    unsigned long long* out, uint32_t* steps, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    ptv::SelectStackEntry(S.stack16 != 0, [&](auto entry) {
        using E = typename decltype(entry)::type;
        ptv::SelectFlags(
            [&](auto SPILL) {
                hipLaunchKernelGGL((ptd::extend_stats_kernel<Src, SPILL, PT_EXTEND_CAP, E>), dim3(Blocks(n)), dim3(256),
                                   0, st, S, src, n, spill, n, out, steps);
            },
            spill != nullptr);
    });
    return hipGetLastError();
}

hipError_t pt_launch_trace_rays_stats(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                      const float* dur, float4* hit, float2* hc, uint32_t* spill,
                                      unsigned long long* out, uint32_t* steps, hipStream_t st)
{
    return LaunchExtendStats(S, ptd::ray_source_arrays{origins, vel, dur, hit, hc}, n, spill, out, steps, st);
}

hipError_t pt_launch_extend_stats(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, uint32_t* spill,
                                  unsigned long long* out, uint32_t* steps, hipStream_t st)
{
    return LaunchExtendStats(S, ptd::ray_source_slots{L, F}, L.n, spill, out, steps, st);
}

hipError_t pt_launch_length_classes(uint32_t* sum, uint32_t* cnt, uint8_t* cls, hipStream_t st)
{
    hipLaunchKernelGGL(ptd::length_classes_kernel, dim3(1), dim3(1024), 0, st, sum, cnt, cls);
    return hipGetLastError();
}
