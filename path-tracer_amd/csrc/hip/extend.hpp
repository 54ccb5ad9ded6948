// extend.hpp — one tile of extend: the ray sources, ExtendRay, ExtendTile and
// the LDS node cache's fill.  Used by the extend kernels (extend.hip) and the
// fused round kernels (rounds.hip).
#pragma once

#include "path.hpp"

#include <type_traits>

namespace ptd {

// Ray sources of the extend kernel: the renderer's slots, or the arrays of
// the ray-query API.

struct ray_source_slots {
    dslots L;
    dframe F;
    // s is a ray POSITION (TileOrder), not a slot.
    PT_DEV bool load(uint32_t s, pt3& O, pt3& V, float& D) const
    {
        if (!PositionValid(F, s)) return false;
        float4 r = L.ray[s];
        O = v3(r.x, r.y, r.z);
        V = UnpackUnitVector(__float_as_uint(r.w));
        D = PT_HIT_TIME_LIMIT;
        return true;
    }
    PT_DEV void store(uint32_t s, const lane_state& Ln, bool vidx21) const
    {
        L.hit[s] = CompactHit(Ln, vidx21);
        L.uv[s] = make_float2(Ln.C.y, Ln.C.z);
    }
    // ShadeOrder: each wave, once all its rays are traced, stores one ballot
    // per outcome class (one word per 64 positions and class; no atomics,
    // no barrier).
    // Single-material scenes store the miss class only (ShadePosition reads
    // nothing else for them).
    PT_DEV void outcome(uint32_t q, uint32_t cls, bool classes) const
    {
        uint64_t* m = L.outcome + (size_t)(q >> 8) * (4 * PT_OUTCOME_CLASSES) + ((q >> 6) & 3u);
        if (!classes) {
            uint64_t b = __ballot(cls == PT_OUTCOME_CLASSES - 1);
            if ((q & 63u) == 0) m[4 * (PT_OUTCOME_CLASSES - 1)] = b;
            return;
        }
#pragma unroll
        for (uint32_t c = 0; c < PT_OUTCOME_CLASSES; c++) {
            uint64_t b = __ballot(cls == c);
            if ((q & 63u) == 0) m[4 * c] = b;
        }
    }
};

struct ray_source_arrays {
    PT_DEV void outcome(uint32_t, uint32_t, bool) const {}
    const float* origins;
    const uint32_t* vel;
    const float* dur;
    float4* hit;
    float2* hc;
    PT_DEV bool load(uint32_t i, pt3& O, pt3& V, float& D) const
    {
        O = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
        V = UnpackUnitVector(vel[i]);
        D = dur[i];
        return true;
    }
    PT_DEV void store(uint32_t i, const lane_state& Ln, bool vidx21) const
    {
        hit[i] = CompactHit(Ln, vidx21);
        hc[i] = make_float2(Ln.C.y, Ln.C.z);
    }
};

template <class Src>
constexpr bool kRendererSource = std::is_same<Src, ray_source_slots>::value;

// Extend: one ray per thread, LaneStep run to completion.  (A persistent
// variant with per-wave dynamic ray fetch was measured 1.6x slower on C3: the
// refill bookkeeping cost more than the idle lanes it recovered.  Persistent
// waves claiming 64-ray chunks from a launch-wide counter, each ray traced to
// completion, were 1.5x slower too (extend 0.592 vs 0.387 ms): a CU's waves
// then trace unrelated chunks, losing the L1 reuse of a tile's four waves,
// and the dispatcher already balances the 8100 one-tile blocks.)
//
// One ray: Trace() by LaneStep to completion, the compact hit stored, and
// the ray's ShadeOrder outcome class ballotted (positions outside the image:
// class 0, shade skips them).
//
// MESH (a dscene::single_mesh scene): the mesh-only loop instead, one pass
// for the lanes whose ray takes the exact fast division and one for the
// others (usually none); each lane's ray is traced as before, only beside
// other lanes.  The loops carry the hit's time and face; MeshEnd forms the
// rest of the record once, after them.
//
// TRAIN (the renderer's mesh-only loop in LENGTH order, on the table's
// training rounds): the lane counts its steps and adds them, capped at 255,
// and 1 to its ray key's sum and count (integer atomics without a return:
// the sums do not depend on the order).  Positions below the tile's camera
// count are skipped (TileOrderLengthKey).
template <bool SPILL, int CAP, class E, bool MESH = false, bool TRAIN = false, class Src>
PT_DEV void ExtendRay(const dscene& S, const Src& src, tstack<SPILL, CAP, E>& st, uint32_t slot)
{
    static_assert(!TRAIN || (MESH && kRendererSource<Src>), "training counts the mesh-only loop's steps");
    pt3 O, V;
    float D;
    uint32_t cls = 0;
    if (src.load(slot, O, V, D)) {
        lane_state Ln;
        if constexpr (MESH && TRAIN) {
            uint32_t steps = 0;
            MeshBegin(S, Ln, O, V, D);
            if (Ln.exact) {
                while (!MeshStep<true>(S, Ln, st)) steps++;
            } else {
                while (!MeshStep<false>(S, Ln, st)) steps++;
            }
            MeshEnd<sizeof(E) == 2>(S, Ln);
            if ((slot & 255u) >= src.L.len_cam[slot >> 8]) {
                // The ray again from its record: nothing of it stays live over the loop.
                const float4 r = src.L.ray[slot];
                const pt3 W = UnpackUnitVector(__float_as_uint(r.w));
                const uint32_t key = pt_ray_key(r.x, r.y, r.z, W.x, W.y, W.z, &src.L.len_bounds);
                atomicAdd(&src.L.len_sum[key], min(steps, 255u));
                atomicAdd(&src.L.len_cnt[key], 1u);
            }
        } else if constexpr (MESH) {
            MeshBegin(S, Ln, O, V, D);
            if (Ln.exact) {
                while (!MeshStep<true>(S, Ln, st)) {}
            } else {
                while (!MeshStep<false>(S, Ln, st)) {}
            }
            MeshEnd<sizeof(E) == 2>(S, Ln);
        } else {
            LaneBegin(S, Ln, O, V, D);
            no_stats ns;
            if (S.g.ShapeCount != 0) {
                while (!LaneStep<SPILL, CAP, Src, no_stats, true, E>(S, Ln, st, src, slot, ns)) {}
            }
        }
        src.store(slot, Ln, S.vidx21 != 0);
        if (Ln.Shape == SHAPE_INDEX_NONE) {
            cls = 4;
        } else if (S.mat_classes) {
            uint32_t T = S.material[32 * (size_t)S.shapes[Ln.Shape].MaterialIndex];
            cls = T == PT_MATERIAL_TYPE_BASIC_DIFFUSE ? 0u
                : T == PT_MATERIAL_TYPE_BASIC_METAL ? 1u
                : T == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT ? 2u : 3u;
        }
    }
    src.outcome(slot, cls, S.mat_classes != 0);
}

// One block of extend.  Thread i traces the ray at position tile*256 + i; RUN
// (the renderer's RUN block map, include/pt_blockmap.h): `tile` is a unit, and
// wave w traces the unit's quarter of the w-th tile of its run -- or nothing,
// in a short run.  The outcome words, the wave's time, the camera count and
// the stack column all follow the position or the thread as before.
template <class Src, bool SPILL, int CAP, class E, bool MESH = false, bool TRAIN = false, bool RUN = false>
PT_DEV void ExtendTile(const dscene& S, const Src& src, uint32_t n, uint32_t* spill, uint32_t spill_stride, E* smem,
                       uint32_t tile, bool timed, const float4* nc = nullptr, uint32_t ncn = 0)
{
    static_assert(!RUN || (MESH && !SPILL && kRendererSource<Src>), "the RUN block map rides the renderer's mesh-only loop");
    uint64_t t0 = timed ? __builtin_amdgcn_s_memtime() : 0;
    uint32_t slot = tile * 256 + threadIdx.x;
    uint32_t first = 0;   // RUN: the wave's first position, in a scalar register
    if constexpr (RUN) {
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        first = pt_unit_tile(tile, wave, PT_BLOCK_MAP_RUN_GRANULE) * 256 +
                pt_unit_quarter(tile, wave, PT_BLOCK_MAP_RUN_GRANULE) * 64;
        slot = first + (threadIdx.x & 63u);
    }
    if (slot >= n) return;
    tstack<SPILL, CAP, E> st;
    st.lds = &smem[threadIdx.x];
    st.spill = spill + slot;
    st.stride = spill_stride;
    st.nc = nc;
    st.ncn = ncn;
    ExtendRay<SPILL, CAP, E, MESH, TRAIN>(S, src, st, slot);
    if constexpr (kRendererSource<Src>) {
        if (timed && (threadIdx.x & 63u) == 0)
            src.L.tilecost[RUN ? first >> 6 : tile * 4 + (threadIdx.x >> 6)] = (uint32_t)(__builtin_amdgcn_s_memtime() - t0);
    }
}

// The LDS node cache's fill: nodes [0, S.node_cache) of the scene (the top
// child pairs, NodeCacheLayout), 16 B per thread and load, then a barrier
// before any lane traverses.
PT_DEV uint32_t NodeCacheFill(const dscene& S, float4* nc)
{
    const uint32_t nodes = min(S.node_cache, 2u * PT_NODE_CACHE_PAIRS);
    for (uint32_t i = threadIdx.x; i < 2 * nodes; i += 256) nc[i] = S.mesh_nodes[i];
    __syncthreads();
    return nodes;
}

}  // namespace ptd
