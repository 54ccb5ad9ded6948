// kernels.hip — the small utility kernels of the renderer and their
// launchers: tile order, guard, vertex decode, atlas tiling, stream merge,
// unowned rows and the numerics checks.  The wavefront integrator itself is
// extend.hip (Trace), shade.hip (raygen, Scatter) and rounds.hip (both fused).
#include "pt_device.hpp"
#include "kernels.hpp"
#include "variants.hpp"

namespace ptd {

// One longest-first counting sort by the whole block: item(i), i < n, names
// the i-th thing to order and time(x) gives its time; out[0, n) receives the
// items over 512 log-spaced buckets (16 per octave), longest first.
template <class Item, class Time>
PT_DEV void SortLongestFirst(uint32_t n, uint32_t* out, uint32_t* count, uint32_t* wsum, Item item, Time time)
{
    __syncthreads();   // a sort before this one is done with count[]
    for (uint32_t i = threadIdx.x; i < 512; i += 1024) count[i] = 0;
    __syncthreads();
    auto key = [&](uint32_t x) -> uint32_t {
        uint32_t c = time(x);
        if (c < 16) return 511u;                               // untimed / trivial: last
        uint32_t e = 31u - __clz(c);                           // octave
        uint32_t m = (c >> (e - 4)) & 15u;                     // 16 steps inside it
        uint32_t k = min(e * 16u + m, 511u);
        return 511u - k;                                       // longest first
    };
    for (uint32_t i = threadIdx.x; i < n; i += 1024) atomicAdd(&count[key(item(i))], 1u);
    __syncthreads();
    // Exclusive scan of the 512 buckets: eight waves scan 64 each with
    // shuffles, then add the totals of the waves before them (a serial scan
    // by one thread was most of this kernel's 11 us).
    uint32_t c = 0, incl = 0;
    if (threadIdx.x < 512) {
        c = count[threadIdx.x];
        incl = c;
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
            if ((threadIdx.x & 63u) >= (uint32_t)o) incl += t;
        }
        if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
    }
    __syncthreads();
    if (threadIdx.x < 512) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wsum[w];
        count[threadIdx.x] = before + incl - c;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const uint32_t x = item(i);
        out[atomicAdd(&count[key(x)], 1u)] = x;
    }
}

// Longest-first dispatch order for the next round: tiles by their slowest
// wave's time, descending.  Any order gives the same results; only the
// kernels' tails change.
//
// Tile groups (ptSetBasicRendererSplit; include/pt_blockmap.h): group g of K
// owns the tiles t = g, g + K, ... and its segment order[start, start + count)
// of the dispatch order, which it sorts on its own stream; K = 1 is the whole
// frame.
//
// UNITS (the RUN block map): the group owns whole runs of four tiles, and a
// second block of the same launch sorts its segment of the unit order, which
// extend then dispatches by: unit (run u, quarter j) by the longest of the
// quarter-j waves of the run's tiles, each timed by the block that traced it.
// Shade keeps the tile order.
template <bool UNITS>
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint32_t* cost, uint32_t* order, uint32_t tiles,
                                                          uint32_t groups, uint32_t group, uint32_t start,
                                                          uint32_t* units, uint32_t ustart)
{
    __shared__ uint32_t count[512];
    __shared__ uint32_t wsum[8];
    auto tile_time = [&](uint32_t t) {
        return max(max(cost[4 * t], cost[4 * t + 1]), max(cost[4 * t + 2], cost[4 * t + 3]));
    };
    if constexpr (!UNITS) {
        SortLongestFirst(pt_tile_group_count(tiles, groups, group), order + start, count, wsum,
                         [&](uint32_t i) { return pt_tile_group_tile(tiles, groups, group, i); }, tile_time);
    } else {
        // Two blocks, one order each, so that the launch takes one sort's time.
        constexpr uint32_t G = PT_BLOCK_MAP_RUN_GRANULE;
        if (blockIdx.x == 0)
            SortLongestFirst(pt_group_tile_count(tiles, groups, group, G), order + start, count, wsum,
                             [&](uint32_t i) { return pt_group_tile(groups, group, i, G); }, tile_time);
        else
            SortLongestFirst(pt_group_unit_count(tiles, groups, group, G), units + ustart, count, wsum,
                             [&](uint32_t i) { return pt_group_unit(groups, group, i, G); },
                             [&](uint32_t x) {
                                 uint32_t c = 0;
                                 for (uint32_t w = 0; w < 4; w++) {
                                     const uint32_t t = pt_unit_tile(x, w, G);
                                     if (t < tiles) c = max(c, cost[4 * t + pt_unit_quarter(x, w, G)]);
                                 }
                                 return c;
                             });
    }
}

// Guarded rounds (ptRenderFrame's last rounds, enqueued without a read-back
// between them): before each, the paths completed since the Reset -- the sum
// of the per-wave done words, as ptGetStats adds them -- against the frame's
// target.  Reached: flags[0] = 1, and this and every later launch of the
// frame returns at once (dslots.stop); else the round runs and flags[1]
// counts it.  So the frame still ends at the first round whose total reaches
// the target.
__global__ __launch_bounds__(1024) void guard_kernel(const uint32_t* done, uint32_t words, unsigned long long target,
                                                     uint32_t* flags)
{
    __shared__ unsigned long long part[1024];
    unsigned long long s = 0;
    for (uint32_t i = threadIdx.x; i < words; i += 1024) s += done[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t h = 512; h > 0; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0 && flags[0] == 0u) {
        if (part[0] >= target) flags[0] = 1u;
        else flags[1] += 1u;
    }
}

// Mesh vertices decoded once per upload for HitAttributes: the octahedral
// normal (UnpackUnitVector) and the half-float UV, the functions the hit
// reconstruction applied per hit before, so every hit sees the same bits.
__global__ __launch_bounds__(256) void vertex_decode_kernel(const uint2* v, uint32_t n, float4* attr, float* vv)
{
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint2 V = v[i];
    pt3 N = UnpackUnitVector(V.x);
    attr[i] = make_float4(N.x, N.y, N.z, pt_half_to_float(V.y & 0xFFFF));
    vv[i] = pt_half_to_float(V.y >> 16);
}

// Row-major packed atlas -> the device's 4x2-texel block layout (AtlasIndex):
// one thread per destination texel, so the stores are contiguous.
__global__ __launch_bounds__(256) void atlas_tile_kernel(const float4* src, float4* dst, uint32_t w, uint32_t h,
                                                         uint64_t texels)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < texels; i += (uint64_t)gridDim.x * 256) {
        uint64_t plane = (uint64_t)w * h;
        uint64_t layer = i / plane, r = i - layer * plane;
        uint32_t blk = (uint32_t)(r >> 3), in = (uint32_t)(r & 7u);
        uint32_t by = blk / (w >> 2), bx = blk - by * (w >> 2);
        uint32_t x = bx * 4 + (in & 3u), y = by * 2 + (in >> 2);
        dst[i] = src[layer * plane + (uint64_t)y * w + x];
    }
}

// Path streams' merge (ptMergeBasicRendererStreams): for every pixel of the
// renderer's bands, accum = ((accx[0] + accx[1]) + accx[2]) ... in stream
// order; the streams' own accumulators keep running.
__global__ __launch_bounds__(256) void merge_streams_kernel(float4* accum, float4* accx, uint32_t width, uint32_t height,
                                                            uint32_t rank, uint32_t nranks, uint32_t streams)
{
    const size_t frame = (size_t)width * height;
    for (uint32_t y = blockIdx.y; y < height; y += gridDim.y) {
        if (((y >> 4) % nranks) != rank) continue;
        for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < width; x += gridDim.x * 256) {
            const size_t p = (size_t)y * width + x;
            float4 v = accx[p];
            for (uint32_t k = 1; k < streams; k++) {
                float4 a = accx[(size_t)k * frame + p];
                v.x = v.x + a.x; v.y = v.y + a.y; v.z = v.z + a.z; v.w = v.w + a.w;
            }
            accum[p] = v;
        }
    }
}

__global__ __launch_bounds__(256) void zero_unowned_kernel(float4* accum, uint32_t width, uint32_t height,
                                                           uint32_t rank, uint32_t nranks)
{
    for (uint32_t y = blockIdx.y; y < height; y += gridDim.y) {
        if (((y >> 4) % nranks) == rank) continue;
        for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < width; x += gridDim.x * 256)
            accum[(size_t)y * width + x] = make_float4(0, 0, 0, 0);
    }
}

// Exhaustive check of FastRcp: every bit pattern d = i (i < 2^32); counts
// d in FastRcpRange whose FastRcp(d) differs from 1.0f / d in any bit.
__global__ __launch_bounds__(256) void rcp_check_kernel(unsigned long long* mismatches)
{
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long bad = 0;
    for (; i < (1ull << 32); i += stride) {
        float d = __uint_as_float((uint32_t)i);
        if (!FastRcpRange(d)) continue;
        bad += __float_as_uint(FastRcp(d)) != __float_as_uint(1.0f / d);
    }
    if (bad) atomicAdd(mismatches, bad);
}

// Checks XDiv against IEEE division on device-generated operands: counts
// mismatching bit patterns (test infrastructure for the convention).
__global__ __launch_bounds__(256) void xdiv_check_kernel(uint64_t n, uint32_t seed, unsigned long long* mismatches)
{
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long bad = 0;
    for (; i < n; i += stride) {
        uint32_t s = (uint32_t)i * 2654435761u ^ seed;
        uint32_t ra = pt_random(&s), rb = pt_random(&s), rc = pt_random(&s);
        // exponents spread over +-2^40 around 1, random signs and mantissas
        float a = pt_u2f(((87u + (ra >> 26) + (rc & 15)) << 23) | (ra & 0x7fffffu) | ((rc >> 31) << 31));
        float b = pt_u2f(((107u + ((rb >> 27) & 31)) << 23) | (rb & 0x7fffffu) | (((rc >> 30) & 1u) << 31));
        if ((rc & 0xff0) == 0) a = 0.0f;
        if ((rc & 0xff00) == 0) b = 0.0f;
        float y = RecipForDiv(b);
        float q = XDiv(a, b, y);
        float e = a / b;
        if (pt_f2u(q) != pt_f2u(e) && !(q != q && e != e)) bad++;
    }
    if (bad) atomicAdd(mismatches, bad);
}

}  // namespace ptd

// --- launchers (called from the rt_*.hip host files) -----------------------------

using ptv::Blocks;

hipError_t pt_launch_vertex_decode(const uint2* v, uint32_t n, float4* attr, float* vv, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::vertex_decode_kernel, dim3(Blocks(n)), dim3(256), 0, st, v, n, attr, vv);
    return hipGetLastError();
}

hipError_t pt_launch_guard(const uint32_t* done, uint32_t words, uint64_t target, uint32_t* flags, hipStream_t st)
{
    hipLaunchKernelGGL(ptd::guard_kernel, dim3(1), dim3(1024), 0, st, done, words, (unsigned long long)target, flags);
    return hipGetLastError();
}

hipError_t pt_launch_tile_order(const ptd::dslots& L, hipStream_t st, uint32_t groups, uint32_t group, uint32_t granule,
                                uint32_t* units)
{
    if (!L.order || L.tile_count == 0 || groups == 0 || group >= groups) return hipSuccess;
    if (granule == PT_BLOCK_MAP_RUN_GRANULE) {
        if (!units) return hipErrorInvalidValue;
        hipLaunchKernelGGL(ptd::tile_order_kernel<true>, dim3(2), dim3(1024), 0, st, L.tilecost, L.order, L.tile_count,
                           groups, group, pt_group_tile_start(L.tile_count, groups, group, granule), units,
                           pt_group_unit_start(L.tile_count, groups, group, granule));
    } else {
        hipLaunchKernelGGL(ptd::tile_order_kernel<false>, dim3(1), dim3(1024), 0, st, L.tilecost, L.order, L.tile_count,
                           groups, group, pt_tile_group_start(L.tile_count, groups, group), (uint32_t*)nullptr, 0u);
    }
    return hipGetLastError();
}

hipError_t pt_launch_atlas_tile(const float4* src, float4* dst, uint32_t w, uint32_t h, uint32_t layers, hipStream_t st)
{
    uint64_t texels = (uint64_t)w * h * layers;
    if (texels == 0) return hipSuccess;
    uint64_t blocks = (texels + 255) / 256;
    hipLaunchKernelGGL(ptd::atlas_tile_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, src,
                       dst, w, h, texels);
    return hipGetLastError();
}

hipError_t pt_launch_merge_streams(float4* accum, float4* accx, uint32_t width, uint32_t height, uint32_t rank,
                                   uint32_t nranks, uint32_t streams, hipStream_t st)
{
    if (streams <= 1 || width == 0 || height == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::merge_streams_kernel, dim3(Blocks(width), height < 32768u ? height : 32768u), dim3(256), 0,
                       st, accum, accx, width, height, rank, nranks, streams);
    return hipGetLastError();
}

hipError_t pt_launch_zero_unowned(float4* accum, uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks,
                                  hipStream_t st)
{
    if (nranks <= 1 || width == 0 || height == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::zero_unowned_kernel, dim3(Blocks(width), height < 32768u ? height : 32768u), dim3(256), 0,
                       st, accum, width, height, rank, nranks);
    return hipGetLastError();
}

hipError_t pt_launch_rcp_check(unsigned long long* mismatches, hipStream_t st)
{
    hipLaunchKernelGGL(ptd::rcp_check_kernel, dim3(8192), dim3(256), 0, st, mismatches);
    return hipGetLastError();
}

hipError_t pt_launch_xdiv_check(uint64_t n, uint32_t seed, unsigned long long* mismatches, hipStream_t st)
{
    hipLaunchKernelGGL(ptd::xdiv_check_kernel, dim3(4096), dim3(256), 0, st, n, seed, mismatches);
    return hipGetLastError();
}
