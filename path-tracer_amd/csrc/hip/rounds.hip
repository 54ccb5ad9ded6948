// rounds.hip — the fused round kernels: extend + shade of a tile in one block
// (extend.hpp, shade.hpp), one round or a batch of rounds per launch; and
// their launchers.
#include "extend.hpp"
#include "shade.hpp"
#include "variants.hpp"

#include <map>
#include <mutex>
#include <tuple>

namespace ptd {

// One round (extend + shade) of a tile per block, for partitions whose tiles
// all fit on the GPU at once (a rank's share of a strongly scaled frame):
// a tile is shaded as soon as its own rays are traced, so the shading of
// most tiles runs beside the few long traversals that end the round instead
// of after them, and one launch replaces two.  Same per-tile work and order
// as extend_kernel then shade_kernel, so the results are identical.
template <uint32_t MATS, int CAP, class E>
__global__ __launch_bounds__(256, ShadeMinWaves<MATS>()) void round_kernel(
    dscene S, dslots L, dframe F, dparams Pm)
{
    __shared__ E smem[CAP * 256];
    if (L.stop && *L.stop) return;   // a guarded round past the frame's target
    const uint32_t tile = L.order ? L.order[blockIdx.x] : blockIdx.x;
    ExtendTile<ray_source_slots, false, CAP, E>(S, ray_source_slots{L, F}, L.n, nullptr, 0, smem, tile,
                                                 L.order != nullptr);
    // The tile's hits and outcome masks (global, written by all four waves)
    // are complete and visible to the block after the barrier.
    __syncthreads();
    ShadeTile<MATS>(S, L, F, Pm, tile);
}

// Round batches: Pm.rounds rounds of one tile per block.  A slot's round
// depends only on its own previous round (its ray, path record and pixel;
// the seed is the round's FrameIndex), so tiles need no grid-wide barrier
// between rounds: a block runs its tile's extend and shade Pm.rounds times
// with the seeds of consecutive Run(1) calls (seed_step 1) or of one Run(R)
// (seed_step 0), and the launch has one tail per batch instead of two per
// round.  Barriers between the phases make the tile's hits (extend -> shade)
// and new rays (shade -> next extend, TileOrder positions) visible to the
// block's other waves.  The block's whole time is the tile's cost for the
// next batch's longest-first order.
template <uint32_t MATS, int CAP, class E>
__global__ __launch_bounds__(256, ShadeMinWaves<MATS>()) void rounds_kernel(
    dscene S, dslots L, dframe F, dparams Pm)
{
    __shared__ E smem[CAP * 256];
    const uint32_t tile = L.order ? L.order[blockIdx.x] : blockIdx.x;
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    dparams P = Pm;
    for (uint32_t i = 0; i < Pm.rounds; i++) {
        ExtendTile<ray_source_slots, false, CAP, E>(S, ray_source_slots{L, F}, L.n, nullptr, 0, smem, tile, false);
        __syncthreads();
        ShadeTile<MATS>(S, L, F, P, tile);
        __syncthreads();
        P.seed += Pm.seed_step;
    }
    if (L.order && (threadIdx.x & 63u) == 0)
        L.tilecost[tile * 4 + (threadIdx.x >> 6)] = (uint32_t)(__builtin_amdgcn_s_memtime() - t0);
}

}  // namespace ptd

// --- launchers (called from rt_rounds.hip) ---------------------------------------

// The default extend variant's LDS stack without spill, one instantiation of
// each kernel per shade material mask and stack entry width.  batch: the
// rounds_kernel instantiation, else the round_kernel one.
static const void* RoundKernelFor(uint32_t scene_mats, bool stack16, bool batch)
{
    return ptv::SelectShadeMats(scene_mats, [&](auto mats) {
        return ptv::SelectStackEntry(stack16, [&](auto entry) {
            constexpr uint32_t MATS = decltype(mats)::value;
            using E = typename decltype(entry)::type;
            return batch ? reinterpret_cast<const void*>(&ptd::rounds_kernel<MATS, PT_EXTEND_CAP, E>)
                         : reinterpret_cast<const void*>(&ptd::round_kernel<MATS, PT_EXTEND_CAP, E>);
        });
    });
}

static hipError_t LaunchRoundKernel(const void* k, const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F,
                                    const ptd::dparams& P, hipStream_t st)
{
    void* args[] = {const_cast<ptd::dscene*>(&S), const_cast<ptd::dslots*>(&L), const_cast<ptd::dframe*>(&F),
                    const_cast<ptd::dparams*>(&P)};
    return hipLaunchKernel(k, dim3(L.tile_count), dim3(256), args, 0, st);
}

// Capacity = the tiles the GPU holds at once (blocks per CU at the round
// kernel's occupancy x CUs); a larger partition runs extend + shade.
uint32_t pt_round_capacity(uint32_t scene_mats, bool stack16, uint32_t cu_count)
{
    // Blocks per CU of the round kernel instantiation, cached per (device,
    // shade mask, stack entry width); renderers may be created from several
    // host threads and on several devices.
    static std::mutex mu;
    static std::map<std::tuple<int, uint32_t, bool>, int> per_cu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    uint32_t m = pt_shade_mats(scene_mats);
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_tuple(dev, m, stack16);
    auto it = per_cu.find(key);
    if (it == per_cu.end()) {
        int c = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, RoundKernelFor(scene_mats, stack16, false), 256, 0) !=
            hipSuccess)
            c = 0;
        it = per_cu.emplace(key, c).first;
    }
    return (uint32_t)it->second * cu_count;
}

hipError_t pt_launch_round(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                           uint32_t scene_mats, hipStream_t st)
{
    if (L.n == 0 || L.tile_count == 0) return hipSuccess;
    if (L.spill) return hipErrorNotSupported;
    return LaunchRoundKernel(RoundKernelFor(scene_mats, S.stack16 != 0, false), S, L, F, P, st);
}

// Round batches need the round kernel's condition: no spilled stack.
bool pt_rounds_available(const ptd::dslots& L)
{
    return !L.spill;
}

hipError_t pt_launch_rounds(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                            uint32_t scene_mats, hipStream_t st)
{
    if (L.n == 0 || L.tile_count == 0 || P.rounds == 0) return hipSuccess;
    if (!pt_rounds_available(L)) return hipErrorNotSupported;
    return LaunchRoundKernel(RoundKernelFor(scene_mats, S.stack16 != 0, true), S, L, F, P, st);
}
