// variants.hpp — which instantiations of the kernel templates exist, and how a
// launcher picks one (host code of extend.hip, shade.hip and rounds.hip).
// Every choice is written here once: a launcher selects through these
// dispatchers, instantiates under these conditions, and the runtime's
// "supported" questions (kernels.hpp) are answered from the same conditions.
#pragma once

#include "kernels.hpp"

#include <type_traits>
#include <utility>

// Extend occupancy: min waves per SIMD and LDS stack entries per thread
// (entries beyond the LDS capacity spill to a global buffer).  Compile-time
// only (tools/build_variant.py -DPT_EXTEND_MINW=.. -DPT_EXTEND_CAP=..); the
// round kernels share PT_EXTEND_CAP.  Measured alternatives (4/24, 6/16,
// 4/32, 8/16, 8/12) were all slower on C3.
#ifndef PT_EXTEND_MINW
#define PT_EXTEND_MINW 5
#endif
#ifndef PT_EXTEND_CAP
#define PT_EXTEND_CAP 20
#endif

namespace ptv {

inline uint32_t Blocks(uint32_t n) { return (n + 255) / 256; }

// f(std::bool_constant<flags>...): run-time flags as compile-time ones.
template <class F, bool... Bs>
void SelectFlags(F&& f, std::integer_sequence<bool, Bs...>)
{
    f(std::bool_constant<Bs>{}...);
}
template <class F, bool... Bs, class... Rest>
void SelectFlags(F&& f, std::integer_sequence<bool, Bs...>, bool flag, Rest... rest)
{
    if (flag) SelectFlags(f, std::integer_sequence<bool, Bs..., true>{}, rest...);
    else SelectFlags(f, std::integer_sequence<bool, Bs..., false>{}, rest...);
}
template <class F, class... Flags>
void SelectFlags(F&& f, bool flag, Flags... rest)
{
    SelectFlags(f, std::integer_sequence<bool>{}, flag, rest...);
}

// --- shade material masks ---------------------------------------------------------

// The instantiated masks of shade_kernel, round_kernel and rounds_kernel:
// pt_shade_mats (shade.hip) maps a scene's mask to the smallest superset.
constexpr uint32_t MATS_D = PT_MATS_DIFFUSE;
constexpr uint32_t MATS_DS = PT_MATS_DIFFUSE | PT_MATS_SCENE;
constexpr uint32_t MATS_DM = PT_MATS_DIFFUSE | PT_MATS_METAL | PT_MATS_SCENE;
constexpr uint32_t MATS_A = PT_MATS_ALL | PT_MATS_SCENE;
constexpr uint32_t MATS_AO = PT_MATS_ALL | PT_MATS_OPENPBR | PT_MATS_SCENE;

// f(std::integral_constant<uint32_t, MATS>) for the scene's shade mask.
template <class F>
auto SelectShadeMats(uint32_t scene_mats, F&& f)
{
    switch (pt_shade_mats(scene_mats)) {
    case MATS_D: return f(std::integral_constant<uint32_t, MATS_D>{});
    case MATS_DS: return f(std::integral_constant<uint32_t, MATS_DS>{});
    case MATS_DM: return f(std::integral_constant<uint32_t, MATS_DM>{});
    case MATS_A: return f(std::integral_constant<uint32_t, MATS_A>{});
    default: return f(std::integral_constant<uint32_t, MATS_AO>{});
    }
}

// The masks whose tile shade has a LENGTH instantiation (one-mesh diffuse
// scenes), and those whose shade has a class-list instantiation (more than one
// material type).
constexpr bool HasLengthShade(uint32_t shade_mats) { return shade_mats == MATS_D || shade_mats == MATS_DS; }
constexpr bool HasClassListShade(uint32_t shade_mats) { return shade_mats == MATS_DM || shade_mats == MATS_A; }

// --- extend -------------------------------------------------------------------------

template <class E>
struct stack_entry { using type = E; };

// f(stack_entry<E>): scenes whose stack entries all fit 16 bits
// (dscene::stack16) run a u16 stack.
template <class F>
auto SelectStackEntry(bool stack16, F&& f)
{
    return stack16 ? f(stack_entry<uint16_t>{}) : f(stack_entry<uint32_t>{});
}

// The LDS node cache rides beside the unspilled u16 stack only (with the u32
// stack's 20 KB it would cost occupancy).
template <class E>
constexpr bool HasNodeCache(bool spill) { return sizeof(E) == 2 && !spill; }

// The training instantiations (ExtendRay's TRAIN) count the steps of the
// renderer's mesh-only loop, unspilled.
constexpr bool HasTrain(bool renderer_source, bool mesh, bool spill) { return renderer_source && mesh && !spill; }

// The RUN block map's instantiations (ExtendTile's RUN) exist where LENGTH
// order can run, which gives a run's quarters one predicted length each: the
// renderer's mesh-only loop, unspilled, with and without TRAIN.
constexpr bool HasRunMap(bool renderer_source, bool mesh, bool spill) { return HasTrain(renderer_source, mesh, spill); }

// --- occlusion ----------------------------------------------------------------------

// The any-hit kernel (occlusion.hip) takes extend's stack entry, spill and
// mesh-only choices as they are.  Its LDS node cache rides where extend's
// does; PT_OCCLUSION_NODE_CACHE=0 (tools/build_variant.py) builds it without,
// for the comparison in DESIGN.md §6 row 14.
#ifndef PT_OCCLUSION_NODE_CACHE
#define PT_OCCLUSION_NODE_CACHE 1
#endif
template <class E>
constexpr bool HasOcclusionNodeCache(bool spill) { return PT_OCCLUSION_NODE_CACHE != 0 && HasNodeCache<E>(spill); }

}  // namespace ptv
