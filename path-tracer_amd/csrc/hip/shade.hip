// shade.hip — raygen and the shade kernels: GenerateNewPath for every slot
// (ResetBasicRenderer, basic_scatter.glsl:330-336), Scatter() + accumulate +
// regenerate per tile (basic_scatter.glsl:44-360) or per outcome class, the
// state restore, the path record conversions and the trace record's finalize
// (it rebuilds a hit's attributes as ShadeSlot does); and their launchers.
#include "shade.hpp"
#include "variants.hpp"

namespace ptd {

// One block per tile (the slot count is a multiple of 256): TileOrder needs
// every thread of the block, so no thread returns early.

__global__ __launch_bounds__(256) void raygen_kernel(dscene S, dslots L, dframe F, dparams Pm)
{
    uint32_t s = blockIdx.x * 256 + threadIdx.x;
    uint32_t x, y, stream;
    bool valid = SlotPixel(F, s, x, y, stream);
    pt3 O = v3s(0), V = v3s(0);
    if (valid) {
        rng G;
        G.State = pt_seed(x, y, StreamSeed(Pm.seed, stream));
        GenerateNewPath(S, L, F, Pm, G, s, x, y, O, V);
        StreamAccum(F, stream)[(size_t)y * F.width + x] = make_float4(0, 0, 0, 0);
    }
    // Every ray is a camera ray (LENGTH order: key 0, the tile's whole count).
    if (L.len_order) TileOrderStoreRay<true>(L, s, valid, true, O, V, L.pos[s] & 255u);
    else TileOrderStoreRay(L, s, valid, true, O, V, L.pos[s] & 255u);
}

// State write (ptWriteBasicRendererState): the restored rays of one tile,
// given by slot, go to their TileOrder positions like a shade's new rays;
// every position of the tile gets a miss record (no trace of the restored
// rays exists until the next extend, which overwrites it).  The order does
// not change any result (TileOrder).
__global__ __launch_bounds__(256) void restore_rays_kernel(dslots L, dframe F, const float4* rays, uint32_t tile0)
{
    const uint32_t s = (tile0 + blockIdx.x) * 256 + threadIdx.x;
    uint32_t x, y;
    const bool valid = SlotPixel(F, s, x, y);
    const float4 r = rays[s - tile0 * 256];
    const pt3 V = UnpackUnitVector(__float_as_uint(r.w));
    L.hit[s] = make_float4(0.0f, __uint_as_float(SHAPE_INDEX_NONE), 0.0f, 0.0f);
    L.uv[s] = make_float2(0.0f, 0.0f);
    // LENGTH order: a restored ray counts as a continuing one (the state does
    // not say which rays start a path).
    if (L.len_order) TileOrderStoreKeyed<true>(L, s, TileOrderLengthKey(L, valid, false, v3(r.x, r.y, r.z), V), r, 0u);
    else TileOrderStoreKeyed(L, s, TileOrderKey(valid, V), r, 0u);
}

// Record forms of the live paths (GreyRecord, StorePathVertex).  Only slots
// of pixels inside the image hold paths.
__global__ __launch_bounds__(256) void grey_check_kernel(dslots L, dframe F, uint32_t* count)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    uint32_t x, y;
    bool bad = false;
    if (s < L.n && SlotPixel(F, s, x, y)) {
        const float4 p = L.prob[s];
        const uint2 a = L.act[s];
        const uint32_t b = __float_as_uint(p.x);
        bad = b != __float_as_uint(p.y) || b != __float_as_uint(p.z) || b != __float_as_uint(p.w) ||
              (a.x & a.y) != 0xFFFFFFFFu;
    }
    const uint64_t m = __ballot(bad);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(count, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(256) void grey_convert_kernel(dslots L, dframe F, float* prob1, bool to_grey)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    uint32_t x, y;
    if (s >= L.n || !SlotPixel(F, s, x, y)) return;
    if (to_grey) {
        prob1[s] = L.prob[s].x;
    } else {
        const float c = prob1[s];
        L.prob[s] = make_float4(c, c, c, c);
        L.act[s] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    }
}

// Compact hit -> the reference's packed trace record (StoreTraceHit,
// basic.glsl.inc:142-157): {time, shape<<16|material, packed normal, packed
// tangent} + uv.  Used by the ray-query API and the state readback.
__global__ __launch_bounds__(256) void finalize_kernel(dscene S, uint32_t n, const float4* hit, const float2* hc,
                                                       float4* rec, float2* uv)
{
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 h = hit[i];
    uint32_t Shape = __float_as_uint(h.y);
    if (Shape == SHAPE_INDEX_NONE) {
        rec[i] = make_float4(0, __uint_as_float(0xFFFFFFFFu), 0, 0);
        uv[i] = make_float2(0, 0);
        return;
    }
    float2 c = hc[i];
    uint32_t Material;
    pt3 N, TX;
    pt2 UV;
    HitAttributesRecord(S, Shape, h, c, Material, N, TX, UV);
    rec[i] = make_float4(h.x, __uint_as_float((Shape << 16) | Material), __uint_as_float(PackUnitVector(N)),
                         __uint_as_float(PackUnitVector(TX)));
    uv[i] = make_float2(UV.x, UV.y);
}

// The launch-summed counters of the shade statistics build (bsdf.hpp
// ShadeMark): a block's LDS counts cleared before its tile and added after.
#if PT_SHADE_STATS
__device__ unsigned long long g_shade_stats[2 * 32];
PT_DEV void ShadeStatsBegin()
{
    if (threadIdx.x < 64) ShadeStatLds()[threadIdx.x] = 0;
    __syncthreads();
}
PT_DEV void ShadeStatsEnd()
{
    __syncthreads();
    if (threadIdx.x < 2 * SM_COUNT) atomicAdd(&g_shade_stats[threadIdx.x], (unsigned long long)ShadeStatLds()[threadIdx.x]);
}
#else
PT_DEV void ShadeStatsBegin() {}
PT_DEV void ShadeStatsEnd() {}
#endif

template <uint32_t MATS, bool COMPACT, bool LEN = false>
__global__ __launch_bounds__(256, ShadeMinWaves<MATS>()) void shade_kernel(dscene S, dslots L, dframe F,
                                                                                    dparams Pm)
{
    // Tiles in extend's longest-first order too: tiles with long traversals
    // also shade more hits (C5 shade -3 %).
    if (L.stop && *L.stop) return;   // a guarded round past the frame's target
    ShadeStatsBegin();
    ShadeTile<MATS, COMPACT, LEN>(S, L, F, Pm, L.order ? L.order[blockIdx.x] : blockIdx.x);
    ShadeStatsEnd();
}

// Class-pure shade (round 5).  Every position of a round
// goes to the global list of its outcome class (extend's ShadeOrder classes:
// hit diffuse / metal / translucent / other material, miss), and
// shade_classq_kernel gives each block 256 entries of one class, so every
// wave shades one class with that class's BSDF code alone (ShadeSlot's CLS).
// A new ray stays at the position it replaces: TileOrder needs a tile's 256
// new rays together, which a class-pure block does not hold; the slot <->
// position map is unchanged, so the results are identical.  Used inside tile
// groups (rt_rounds.hip ClassLists), where the lists' latency and the gathers'
// extra bytes overlap the other groups' launches: C2 +6 %, C5 +6 %; on one
// stream the lists cost more than the lanes gain.
//
// class_list_kernel builds the lists between extend and shade.  A block
// lists CQ_TILES tiles: one wave scans the (tile, wave word) counts of every
// class and takes the block's run of each class's list with one atomic per
// class, lanes 0..C-1 at once (a tile per block instead: 4096 atomics per
// address per C2 round, serialised, 26 us).  Block 0 clears the other
// parity's counters for the next round.
constexpr uint32_t CQ_TILES = 16;
__global__ __launch_bounds__(256) void class_list_kernel(dslots L, uint32_t mat_classes, uint32_t* counts,
                                                         uint32_t* next_counts, uint32_t* list, uint32_t capk,
                                                         uint32_t tiles_all, uint32_t groups, uint32_t group)
{
    // L.tile_count tiles of tile group `group` (all tiles: groups = 1).
    if (L.stop && *L.stop) return;   // a guarded round past the frame's target
    auto TILE = [&](uint32_t j) { return pt_tile_group_tile(tiles_all, groups, group, j); };
    constexpr uint32_t C = PT_OUTCOME_CLASSES;
    static_assert(CQ_SUB == 1 && 4 * CQ_TILES <= 64, "one list per class; one wave scans the block's counts");
    __shared__ uint64_t om_s[CQ_TILES * 4 * C];
    __shared__ uint32_t off[C][4 * CQ_TILES];
    __shared__ uint32_t base[C];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t tile0 = blockIdx.x * CQ_TILES;
    const uint32_t ntiles = L.tile_count - tile0 < CQ_TILES ? L.tile_count - tile0 : CQ_TILES;
    if (blockIdx.x == 0 && t < C) next_counts[t] = 0u;
    for (uint32_t i = t; i < ntiles * 4 * C; i += 256)
        om_s[i] = L.outcome[(size_t)TILE(tile0 + i / (4 * C)) * (4 * C) + i % (4 * C)];
    __syncthreads();
    auto mask = [&](uint32_t j, uint32_t c, uint32_t k) -> uint64_t {
        const uint64_t* om = om_s + j * (4 * C);
        if (mat_classes) return om[4 * c + k];
        const uint64_t miss = om[4 * (C - 1) + k];
        return c == C - 1 ? miss : c == 0 ? ~miss : 0ull;
    };
    if (t < 64) {
        const uint32_t j = t >> 2, k = t & 3u;
        uint32_t total = 0;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t n = j < ntiles ? (uint32_t)__popcll(mask(j, c, k)) : 0u;
            uint32_t x = n;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
                if ((int)lane >= o) x += y;
            }
            off[c][t] = x - n;
            const uint32_t xt = (uint32_t)__shfl((int)x, 63, 64);
            if (lane == c) total = xt;
        }
        if (lane < C) base[lane] = total ? atomicAdd(&counts[lane], total) : 0u;
    }
    __syncthreads();
    for (uint32_t j = 0; j < ntiles; j++) {
        const uint32_t q = TILE(tile0 + j) * 256 + t;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            const uint64_t m = mask(j, c, w);
            if ((m >> lane) & 1ull) {
                const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                list[(size_t)c * capk + base[c] + off[c][4 * j + w] + r] = q;
            }
        }
    }
}

template <uint32_t MATS, bool COMPACT>
__global__ __launch_bounds__(256, ShadeMinWaves<MATS>()) void shade_classq_kernel(dscene S, dslots L, dframe F,
                                                                                         dparams Pm,
                                                                                         const uint32_t* counts,
                                                                                         const uint32_t* list,
                                                                                         uint32_t capk)
{
    constexpr uint32_t C = PT_OUTCOME_CLASSES;
    if (L.stop && *L.stop) return;   // a guarded round past the frame's target
    // Sub-list starts and class totals from the CQ_SUB x C counters
    // (uniform scalar loads; no barrier).
    uint32_t pre[C][CQ_SUB], tot[C];
#pragma unroll
    for (uint32_t k = 0; k < C; k++) {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t j = 0; j < CQ_SUB; j++) { pre[k][j] = x; x += counts[k * CQ_SUB + j]; }
        tot[k] = x;
    }
    uint32_t c = C, i0 = 0, n = 0, start = 0;
#pragma unroll
    for (uint32_t k = 0; k < C; k++) {
        const uint32_t nk = tot[k];
        const uint32_t bk = (nk + 255u) / 256u;
        if (c == C && blockIdx.x < start + bk) { c = k; i0 = (blockIdx.x - start) * 256u; n = nk; }
        start += bk;
    }
    if (c == C) return;   // whole block: past every list
    const uint32_t i = i0 + threadIdx.x;
    const bool in = i < n;
    uint32_t sub = 0, first = 0;   // the last sub-list starting at or before i
#pragma unroll
    for (uint32_t k = 0; k < C; k++) {
        if (k != c) continue;
#pragma unroll
        for (uint32_t j = 1; j < CQ_SUB; j++)
            if (pre[k][j] <= i) { sub = j; first = pre[k][j]; }
    }
    const uint32_t q = in ? list[((size_t)c * CQ_SUB + sub) * capk + (i - first)] : 0u;
    const uint32_t s = (q & ~255u) | L.slotof[q];
    uint32_t x = 0, y = 0, stream = 0;
    const bool valid = in && SlotPixel(F, s, x, y, stream);
    const uint32_t p16 = (q & 255u) << 8;
    pt3 O = v3s(0), V = v3s(0);
    bool completed = false;
    uint32_t cstate = 0;
    pt3 csample = v3s(0.0f);
    bool cactnone = false;
    switch (c) {
    case 0:
        ShadeSlot<MATS, COMPACT, PT_MATS_DIFFUSE>(S, L, F, Pm, s, p16, x, y, stream, valid, O, V, completed, cstate,
                                                  csample, cactnone);
        break;
    case 1:
        ShadeSlot<MATS, COMPACT, PT_MATS_METAL>(S, L, F, Pm, s, p16, x, y, stream, valid, O, V, completed, cstate,
                                                csample, cactnone);
        break;
    case 2:
        ShadeSlot<MATS, COMPACT, PT_MATS_TRANSLUCENT>(S, L, F, Pm, s, p16, x, y, stream, valid, O, V, completed,
                                                      cstate, csample, cactnone);
        break;
    case PT_OUTCOME_CLASSES - 1:
        ShadeSlot<MATS, COMPACT, 0u>(S, L, F, Pm, s, p16, x, y, stream, valid, O, V, completed, cstate, csample,
                                     cactnone);
        break;
    default:
        ShadeSlot<MATS, COMPACT>(S, L, F, Pm, s, p16, x, y, stream, valid, O, V, completed, cstate, csample, cactnone);
        break;
    }
    const uint64_t cm = __ballot(completed);
    const uint32_t words = L.n / 64;
    if ((threadIdx.x & 63u) == 0 && cm && words)
        atomicAdd(&L.done[((blockIdx.x * 256u + threadIdx.x) >> 6) % words], (uint32_t)__popcll(cm));
    if constexpr (COMPACT) CompletionQueue(S, L, F, Pm, s, completed, cm, cstate, csample, cactnone, O, V);
    if (valid) {
        L.ray[q] = make_float4(O.x, O.y, O.z, __uint_as_float(PackUnitVector(V)));
        L.pos[s] = (uint16_t)(((q & 255u) << 8) | (q & 255u));
    }
}

}  // namespace ptd

// --- launchers (called from rt_rounds.hip; finalize from rt_renderer.hip) --------

using ptv::Blocks;

hipError_t pt_launch_raygen(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                            hipStream_t st)
{
    if (L.n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::raygen_kernel, dim3(Blocks(L.n)), dim3(256), 0, st, S, L, F, P);
    return hipGetLastError();
}

hipError_t pt_launch_restore_rays(const ptd::dslots& L, const ptd::dframe& F, const float4* rays, uint32_t tile0,
                                  uint32_t tiles, hipStream_t st)
{
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::restore_rays_kernel, dim3(tiles), dim3(256), 0, st, L, F, rays, tile0);
    return hipGetLastError();
}

hipError_t pt_launch_grey_check(const ptd::dslots& L, const ptd::dframe& F, uint32_t* count, hipStream_t st)
{
    if (L.n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::grey_check_kernel, dim3(Blocks(L.n)), dim3(256), 0, st, L, F, count);
    return hipGetLastError();
}

hipError_t pt_launch_grey_convert(const ptd::dslots& L, const ptd::dframe& F, float* prob1, bool to_grey,
                                  hipStream_t st)
{
    if (L.n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::grey_convert_kernel, dim3(Blocks(L.n)), dim3(256), 0, st, L, F, prob1, to_grey);
    return hipGetLastError();
}

hipError_t pt_launch_finalize(const ptd::dscene& S, uint32_t n, const float4* hit, const float2* hc, float4* rec,
                              float2* uv, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::finalize_kernel, dim3(Blocks(n)), dim3(256), 0, st, S, n, hit, hc, rec, uv);
    return hipGetLastError();
}

// Shade instantiations by material-type mask: the smallest superset of the
// scene's mask is launched (one of variants.hpp's MATS_*).
uint32_t pt_shade_mats(uint32_t scene_mats)
{
    // Diffuse meshes without sky light sampling whose textures lie in the
    // unit square of the atlas (the Viking Room, C3): the lean instantiation,
    // which has no sky lobe and no analytic shapes and wraps texel
    // coordinates with two selects (pt_device.hpp Texel).
    if ((scene_mats & ~ptv::MATS_D) == 0) return ptv::MATS_D;
    scene_mats = (scene_mats & ~(uint32_t)PT_MATS_TEXWRAP) | PT_MATS_SCENE;
    if ((scene_mats & ~ptv::MATS_DS) == 0) return ptv::MATS_DS;
    if ((scene_mats & ~ptv::MATS_DM) == 0) return ptv::MATS_DM;
    if (!(scene_mats & PT_MATS_OPENPBR)) return ptv::MATS_A;
    return ptv::MATS_AO;
}

bool pt_length_order_supported(uint32_t scene_mats) { return ptv::HasLengthShade(pt_shade_mats(scene_mats)); }
bool pt_class_lists_supported(uint32_t scene_mats) { return ptv::HasClassListShade(pt_shade_mats(scene_mats)); }

// LEN (L.len_order): the instantiation that keys a tile's new rays by camera /
// length class.
hipError_t pt_launch_shade(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                           uint32_t scene_mats, bool compact, hipStream_t st)
{
    if (L.n == 0 || L.tile_count == 0) return hipSuccess;
    if (L.len_order && (!pt_length_order_supported(scene_mats) || !L.len_cam)) return hipErrorNotSupported;
    ptv::SelectShadeMats(scene_mats, [&](auto mats) {
        constexpr uint32_t MATS = decltype(mats)::value;
        ptv::SelectFlags(
            [&](auto COMPACT, auto LEN) {
                if constexpr (!LEN || ptv::HasLengthShade(MATS))
                    hipLaunchKernelGGL((ptd::shade_kernel<MATS, COMPACT, LEN>), dim3(L.tile_count), dim3(256), 0, st, S,
                                       L, F, P);
            },
            compact, L.len_order != 0);
    });
    return hipGetLastError();
}

// Blocks past the lists return.
hipError_t pt_launch_shade_classq(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F,
                                  const ptd::dparams& P, uint32_t scene_mats, bool compact, uint32_t* counts,
                                  uint32_t* next_counts, uint32_t* list, hipStream_t st, uint32_t tiles_all,
                                  uint32_t groups, uint32_t group)
{
    if (L.n == 0 || L.tile_count == 0) return hipSuccess;
    if (!pt_class_lists_supported(scene_mats)) return hipErrorNotSupported;
    const uint32_t capk = pt_classq_sub_capacity(L.tile_count);
    hipLaunchKernelGGL(ptd::class_list_kernel, dim3((L.tile_count + ptd::CQ_TILES - 1) / ptd::CQ_TILES), dim3(256), 0,
                       st, L, S.mat_classes, counts, next_counts, list, capk, tiles_all ? tiles_all : L.tile_count,
                       groups, group);
    ptv::SelectShadeMats(scene_mats, [&](auto mats) {
        constexpr uint32_t MATS = decltype(mats)::value;
        ptv::SelectFlags(
            [&](auto COMPACT) {
                if constexpr (ptv::HasClassListShade(MATS))
                    hipLaunchKernelGGL((ptd::shade_classq_kernel<MATS, COMPACT>),
                                       dim3(L.tile_count + ptd::PT_OUTCOME_CLASSES), dim3(256), 0, st, S, L, F, P,
                                       counts, list, capk);
            },
            compact);
    });
    return hipGetLastError();
}

#if PT_SHADE_STATS
// Experiment build only (tools/shade_stats.py): the launch-summed shade
// branch counters {waves, lanes} x SM_COUNT; reset clears them.
extern "C" int ptShadeStatsRead(unsigned long long* out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(ptd::g_shade_stats), sizeof(ptd::g_shade_stats)) != hipSuccess)
        return -1;
    if (reset) {
        unsigned long long z[2 * 32] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_shade_stats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return (int)ptd::SM_COUNT;
}
#endif
