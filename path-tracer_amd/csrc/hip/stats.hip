// stats.hip — frame statistics of one accumulator or of a pair (no reference
// counterpart), the same classes and pair rule counted per
// 16 x 16 tile (row 10; tile_statistics_kernel below), and the sample-buffer
// add that combines two halves on the device.
//
// Frame statistics: one pass, 16 B per pixel and accumulator, float4 loads.  The
// classes, the bins and the pair rule are include/pt_stats.h's, shared with
// the host implementation (csrc/scene/stats.cpp).  Everything written is an
// integer count or a min/max of float bit patterns, so the order in which
// the atomics land does not show: two launches, the host and the numpy
// restatement agree bit for bit.
//
//   - a block of 16 waves strides over the linear pixel index, two pixels per
//     thread and step (two loads in flight); the grid is one block per CU
//     (STATS_BLOCKS_PER_CU), not sized from the image;
//   - each wave owns a private copy of the histograms in LDS (16 waves x
//     {luminance, noise} x 256 bins x 4 B = 32 KB), updated with LDS atomics;
//     at block end one thread per bin sums the sixteen copies and adds the
//     bin to the result with one global atomic, skipping empty bins;
//   - the class counters and the four min/max values stay in registers, are
//     reduced across the wave with shuffles, across the block with LDS
//     atomics, and leave the block as one global atomic each.
//     Atomics on one address are served one after the other, about 50 ns
//     each: the first version of this kernel, 256-thread blocks, 4 per CU,
//     each wave sending its own values, put 4096 of them on every counter
//     and took 0.21 ms whatever the image size.  One block per
//     CU leaves 256 per address;
//   - UNIFORM: when every active lane of a wave falls in the same bin (a
//     constant sky, a denoised frame) the 64 LDS atomics on one address
//     serialise; the first active lane adds the lane count instead.
//
// The minima are kept as the complement of the bit pattern and raised with
// atomicMax, so that the all-zero struct the runtime clears is "no value
// yet" for all four; the runtime turns them back (rt_post.hip).
#include "pt_device.hpp"
#include "kernels.hpp"
#include "../../../include/pt_stats.h"

namespace ptd {

constexpr uint32_t STATS_BLOCK = 1024;
constexpr uint32_t STATS_WAVES = STATS_BLOCK / 64;
constexpr uint32_t STATS_BLOCKS_PER_CU = 1;

PT_DEV uint32_t WaveSum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

PT_DEV uint32_t WaveMax(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t u = (uint32_t)__shfl_xor((int)v, o);
        v = v > u ? v : u;
    }
    return v;
}

// hist[bin] += 1 for the calling lanes (any subset of the wave).
template <bool UNIFORM>
PT_DEV void HistogramAdd(uint32_t* hist, int bin)
{
    if (UNIFORM) {
        const int first = __builtin_amdgcn_readfirstlane(bin);        // the first active lane's bin
        const unsigned long long active = __ballot(1), same = __ballot(bin == first);
        if (same == active) {
            if ((int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&hist[first], (uint32_t)__popcll(active));
            return;
        }
    }
    atomicAdd(&hist[bin], 1u);
}

struct stats_lane {
    uint32_t filled = 0, empty = 0, nonfinite = 0, dark = 0, noisy = 0, skipped = 0;
    uint32_t min_y = 0, max_y = 0, min_w = 0, max_w = 0;   // minima: complement of the bits (0 = none)
};

template <bool PAIR, bool UNIFORM>
PT_DEV void StatsPixel(float4 a, float4 b, uint32_t* lum, uint32_t* noise, stats_lane& L)
{
    float4 p = a;
    if (PAIR) {
        p = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        float Ya = 0.0f, Yb = 0.0f, r = 0.0f;
        if (pt_stats_classify(a.x, a.y, a.z, a.w, &Ya) == PT_STATS_FILLED &&
            pt_stats_classify(b.x, b.y, b.z, b.w, &Yb) == PT_STATS_FILLED) {
            if (pt_stats_pair_noise(Ya, Yb, &r)) {
                L.noisy++;
                HistogramAdd<UNIFORM>(noise, pt_stats_bin(r));
            } else {
                L.skipped++;
            }
        }
    }
    float Y = 0.0f;
    const int c = pt_stats_classify(p.x, p.y, p.z, p.w, &Y);
    if (c == PT_STATS_NONFINITE) { L.nonfinite++; return; }
    if (c == PT_STATS_EMPTY) { L.empty++; return; }
    L.filled++;
    const uint32_t wb = pt_f2u(p.w);                                   // w > 0: orders as its bits
    L.min_w = L.min_w > ~wb ? L.min_w : ~wb;
    L.max_w = L.max_w > wb ? L.max_w : wb;
    if (Y > 0.0f) {
        const uint32_t yb = pt_f2u(Y);
        L.min_y = L.min_y > ~yb ? L.min_y : ~yb;
        L.max_y = L.max_y > yb ? L.max_y : yb;
        HistogramAdd<UNIFORM>(lum, pt_stats_bin(Y));
    } else {
        L.dark++;
    }
}

// The block's scalars in LDS, in the order of stats_lane.
enum { B_FILLED, B_EMPTY, B_NONFINITE, B_DARK, B_NOISY, B_SKIPPED, B_MIN_Y, B_MAX_Y, B_MIN_W, B_MAX_W, B_COUNT };

PT_DEV void AddCounter(uint32_t* dst, uint32_t lane_value, bool leader)
{
    const uint32_t s = WaveSum(lane_value);
    if (leader && s) atomicAdd(dst, s);
}

PT_DEV void RaiseBits(uint32_t* dst, uint32_t lane_value, bool leader)
{
    const uint32_t m = WaveMax(lane_value);
    if (leader && m) atomicMax(dst, m);
}

template <bool PAIR, bool UNIFORM>
__global__ __launch_bounds__(STATS_BLOCK) void frame_statistics_kernel(const float4* __restrict__ A,
                                                                       const float4* __restrict__ B, uint64_t n,
                                                                       pt_frame_statistics* __restrict__ S)
{
    constexpr uint32_t HISTS = PAIR ? 2 : 1;
    __shared__ uint32_t hist[STATS_WAVES][HISTS][PT_STATS_BINS];
    __shared__ uint32_t block[B_COUNT];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    for (uint32_t k = tid; k < STATS_WAVES * HISTS * PT_STATS_BINS; k += STATS_BLOCK) (&hist[0][0][0])[k] = 0;
    if (tid < B_COUNT) block[tid] = 0;
    __syncthreads();
    uint32_t* lum = hist[wave][0];
    uint32_t* noise = hist[wave][HISTS - 1];

    stats_lane L;
    const uint64_t half = (uint64_t)gridDim.x * STATS_BLOCK;           // pixels the grid covers with one load each
    for (uint64_t i = (uint64_t)blockIdx.x * STATS_BLOCK + tid; i < n; i += 2 * half) {
        // The second pixel of the step; past the end the first is loaded again
        // (and not counted), so that both loads are unconditional float4 loads.
        const bool second = i + half < n;
        const uint64_t j = second ? i + half : i;
        const float4 zero = make_float4(0, 0, 0, 0);
        const float4 a0 = A[i], a1 = A[j];
        const float4 b0 = PAIR ? B[i] : zero, b1 = PAIR ? B[j] : zero;
        StatsPixel<PAIR, UNIFORM>(a0, b0, lum, noise, L);
        if (second) StatsPixel<PAIR, UNIFORM>(a1, b1, lum, noise, L);
    }

    // Lanes -> wave (shuffles) -> block (LDS atomics, one per wave and value).
    const bool leader = (tid & 63u) == 0;
    AddCounter(&block[B_FILLED], L.filled, leader);
    AddCounter(&block[B_EMPTY], L.empty, leader);
    AddCounter(&block[B_NONFINITE], L.nonfinite, leader);
    AddCounter(&block[B_DARK], L.dark, leader);
    RaiseBits(&block[B_MIN_Y], L.min_y, leader);
    RaiseBits(&block[B_MAX_Y], L.max_y, leader);
    RaiseBits(&block[B_MIN_W], L.min_w, leader);
    RaiseBits(&block[B_MAX_W], L.max_w, leader);
    if (PAIR) {
        AddCounter(&block[B_NOISY], L.noisy, leader);
        AddCounter(&block[B_SKIPPED], L.skipped, leader);
    }
    __syncthreads();

    // Block -> result: one global atomic per value and per populated bin.
    if (tid < HISTS * PT_STATS_BINS) {
        const uint32_t h = tid / PT_STATS_BINS, bin = tid % PT_STATS_BINS;
        uint32_t s = 0;
        for (uint32_t w = 0; w < STATS_WAVES; w++) s += hist[w][h][bin];
        if (s) atomicAdd(h == 0 ? &S->luminance_histogram[bin] : &S->noise_histogram[bin], s);
    } else if (tid - HISTS * PT_STATS_BINS < B_COUNT) {
        const uint32_t k = tid - HISTS * PT_STATS_BINS, v = block[k];
        uint64_t* const counters[6] = {&S->filled, &S->empty, &S->nonfinite, &S->dark, &S->noise_pixels,
                                       &S->noise_skipped};
        float* const ranges[4] = {&S->min_luminance, &S->max_luminance, &S->min_samples, &S->max_samples};
        if (v && k < B_MIN_Y) atomicAdd(reinterpret_cast<unsigned long long*>(counters[k]), (unsigned long long)v);
        else if (v) atomicMax(reinterpret_cast<unsigned int*>(ranges[k - B_MIN_Y]), v);
    }
}

// Per-tile statistics: one 256-thread block per 16 x 16
// tile, one pixel per thread (thread t: column t & 15, row t >> 4, so a wave
// reads four 256-byte row pieces).  The pixel rule is pt_stats.h's
// pt_tile_stats_pixel, the host's.  No atomics: each count is the popcount of
// a wave ballot, min and max of the .w bits are wave reductions (the minimum
// as the maximum of the complement, 0 = no filled lane), the four waves'
// partial results meet in LDS and thread 0 writes the 32-byte record with two
// 16-byte stores.  Threads outside the image load nothing and count nowhere.
constexpr uint32_t TILE_STATS_WAVES = 4;
enum { T_FILLED, T_EMPTY, T_NONFINITE, T_PAIR, T_OVER, T_MIN_W, T_MAX_W, T_COUNT };

template <bool PAIR>
__global__ __launch_bounds__(256) void tile_statistics_kernel(const float4* __restrict__ A,
                                                              const float4* __restrict__ B, uint32_t width,
                                                              uint32_t height, uint32_t tiles_x, float threshold,
                                                              pt_tile_statistics* __restrict__ out)
{
    __shared__ uint32_t part[TILE_STATS_WAVES][T_COUNT];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t x = tx * PT_TILE_SIZE + (tid & 15u), y = ty * PT_TILE_SIZE + (tid >> 4);
    uint32_t flags = 0, wb = 0;
    if (x < width && y < height) {
        const size_t i = (size_t)y * width + x;
        const float4 a4 = A[i];
        const float4 b4 = PAIR ? B[i] : make_float4(0, 0, 0, 0);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
        flags = pt_tile_stats_pixel(a, b, PAIR, threshold, &wb);
    }
    const bool filled = (flags & PT_TILE_PX_FILLED) != 0;
    const uint32_t n_filled = (uint32_t)__popcll(__ballot(filled));
    const uint32_t n_empty = (uint32_t)__popcll(__ballot((flags & PT_TILE_PX_EMPTY) != 0));
    const uint32_t n_nonfinite = (uint32_t)__popcll(__ballot((flags & PT_TILE_PX_NONFINITE) != 0));
    const uint32_t n_pair = PAIR ? (uint32_t)__popcll(__ballot((flags & PT_TILE_PX_PAIR) != 0)) : 0u;
    const uint32_t n_over = PAIR ? (uint32_t)__popcll(__ballot((flags & PT_TILE_PX_OVER) != 0)) : 0u;
    const uint32_t min_w = WaveMax(filled ? ~wb : 0u), max_w = WaveMax(filled ? wb : 0u);
    if ((tid & 63u) == 0) {
        part[wave][T_FILLED] = n_filled;
        part[wave][T_EMPTY] = n_empty;
        part[wave][T_NONFINITE] = n_nonfinite;
        part[wave][T_PAIR] = n_pair;
        part[wave][T_OVER] = n_over;
        part[wave][T_MIN_W] = min_w;
        part[wave][T_MAX_W] = max_w;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t v[T_COUNT];
        for (uint32_t k = 0; k < T_COUNT; k++) v[k] = part[0][k];
        for (uint32_t w = 1; w < TILE_STATS_WAVES; w++) {
            for (uint32_t k = 0; k < T_MIN_W; k++) v[k] += part[w][k];
            v[T_MIN_W] = v[T_MIN_W] > part[w][T_MIN_W] ? v[T_MIN_W] : part[w][T_MIN_W];
            v[T_MAX_W] = v[T_MAX_W] > part[w][T_MAX_W] ? v[T_MAX_W] : part[w][T_MAX_W];
        }
        // filled > 0: the complement of the largest complement is the smallest
        // .w; no filled pixel: both stay 0 (0.0f).
        const uint32_t lo = v[T_FILLED] ? ~v[T_MIN_W] : 0u, hi = v[T_FILLED] ? v[T_MAX_W] : 0u;
        uint4* rec = reinterpret_cast<uint4*>(out + tile);
        rec[0] = make_uint4(v[T_FILLED], v[T_EMPTY], v[T_NONFINITE], v[T_PAIR]);
        rec[1] = make_uint4(v[T_OVER], lo, hi, 0u);
    }
}

// dst += src, each component in binary32 (numpy's a + b).
__global__ __launch_bounds__(256) void accumulate_kernel(float4* __restrict__ dst, const float4* __restrict__ src,
                                                         uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = dst[i], b = src[i];
    dst[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

}  // namespace ptd

uint32_t pt_frame_statistics_grid(uint64_t n, uint32_t cu_count)
{
    const uint64_t need = (n + 2 * ptd::STATS_BLOCK - 1) / (2 * ptd::STATS_BLOCK);
    const uint64_t cap = (uint64_t)(cu_count ? cu_count : 1) * ptd::STATS_BLOCKS_PER_CU;
    return (uint32_t)(need < cap ? (need ? need : 1) : cap);
}

hipError_t pt_launch_frame_statistics(const float4* a, const float4* b, uint64_t n, uint32_t cu_count, bool uniform,
                                      pt_frame_statistics* out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const dim3 grid(pt_frame_statistics_grid(n, cu_count)), block(ptd::STATS_BLOCK);
    if (b) {
        if (uniform) hipLaunchKernelGGL((ptd::frame_statistics_kernel<true, true>), grid, block, 0, st, a, b, n, out);
        else hipLaunchKernelGGL((ptd::frame_statistics_kernel<true, false>), grid, block, 0, st, a, b, n, out);
    } else {
        if (uniform) hipLaunchKernelGGL((ptd::frame_statistics_kernel<false, true>), grid, block, 0, st, a, b, n, out);
        else hipLaunchKernelGGL((ptd::frame_statistics_kernel<false, false>), grid, block, 0, st, a, b, n, out);
    }
    return hipGetLastError();
}

hipError_t pt_launch_tile_statistics(const float4* a, const float4* b, uint32_t width, uint32_t height,
                                     float threshold, pt_tile_statistics* out, hipStream_t st)
{
    const uint32_t tiles_x = (width + PT_TILE_SIZE - 1) / PT_TILE_SIZE, tiles_y = (height + PT_TILE_SIZE - 1) / PT_TILE_SIZE;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
    if (tiles == 0) return hipSuccess;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)tiles), block(256);
    if (b) hipLaunchKernelGGL(ptd::tile_statistics_kernel<true>, grid, block, 0, st, a, b, width, height, tiles_x, threshold, out);
    else hipLaunchKernelGGL(ptd::tile_statistics_kernel<false>, grid, block, 0, st, a, b, width, height, tiles_x, threshold, out);
    return hipGetLastError();
}

hipError_t pt_launch_accumulate(float4* dst, const float4* src, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::accumulate_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}
