// shade.hpp — one tile of shade: the occupancy floors of the shade
// instantiations, ShadeSlot, the completion queue and ShadeTile.  Used by the
// shade kernels (shade.hip) and the fused round kernels (rounds.hip).
#pragma once

#include "path.hpp"

namespace ptd {

#ifndef PT_SHADE_DIFFUSE_MINW
#define PT_SHADE_DIFFUSE_MINW 5
#endif
// Occupancy floor of the other shade instantiations (metal / translucent /
// medium code compiled in): 5 waves per SIMD (96 VGPRs, a few spills of
// rarely live values) beat the compiler's 106-108 VGPRs at 4 waves: C5
// shade 0.190 -> 0.179 ms, C2 0.111 -> 0.104 ms.
#ifndef PT_SHADE_OTHER_MINW
#define PT_SHADE_OTHER_MINW 5
#endif
// The OpenPBR instantiation (opt-in) carries the layered sampler as well:
// 160 VGPRs (3 waves/SIMD) unbounded; a 4-wave floor caps it at 128 with
// 84 B of spills and is faster (OpenPBR test scene at 1080p: shade 0.523 vs
// 0.568 ms, profiles/r02_next).
#ifndef PT_SHADE_OPENPBR_MINW
#define PT_SHADE_OPENPBR_MINW 4
#endif
template <uint32_t MATS>
constexpr int ShadeMinWaves()
{
    return (MATS & ~(uint32_t)PT_MATS_SCENE) == PT_MATS_DIFFUSE ? PT_SHADE_DIFFUSE_MINW
         : (MATS & PT_MATS_OPENPBR) ? PT_SHADE_OPENPBR_MINW : PT_SHADE_OTHER_MINW;
}
// A completed path (basic_scatter.glsl:344-359): its Sample accumulated into
// the pixel (alpha counts the sample) and a new camera path generated with
// the slot's RNG continuing from Scatter's draws.
PT_DEV void CompletePath(const dscene& S, const dslots& L, const dframe& F, const dparams& Pm, rng& G, uint32_t s,
                         uint32_t x, uint32_t y, uint32_t stream, pt3 Sample, bool act_none, pt3& O, pt3& V)
{
    float4* A = &StreamAccum(F, stream)[(size_t)y * F.width + x];
    float4 Val = make_float4(Sample.x, Sample.y, Sample.z, 1.0f);
    if (Pm.render_flags & PT_RENDER_FLAG_ACCUMULATE) {
        float4 Old = *A;
        Val.x = Val.x + Old.x; Val.y = Val.y + Old.y; Val.z = Val.z + Old.z; Val.w = Val.w + Old.w;
    }
    *A = Val;
    GenerateNewPath(S, L, F, Pm, G, s, x, y, O, V, act_none);
}

// Shade one slot (basic_scatter.glsl:main): load its path and its ray's hit
// (at position p16 >> 8), Scatter, store the continuing path or complete it.
// COMPACT: a completed path is left to the block's completion queue (its RNG
// state, Sample and empty-stack flag in cstate / csample / cactnone); else it
// is completed here and its new camera ray returned in O, V.
template <uint32_t MATS, bool COMPACT, uint32_t CLS = 0xFFFFFFFFu>
PT_DEV void ShadeSlot(const dscene& S, const dslots& L, const dframe& F, const dparams& Pm, uint32_t s, uint32_t p16,
                      uint32_t x, uint32_t y, uint32_t stream, bool valid, pt3& O, pt3& V, bool& completed,
                      uint32_t& cstate, pt3& csample, bool& cactnone)
{
    if (valid) {
        ShadeMark(SM_ENTRY);
        rng G;
        G.State = pt_seed(x, y, StreamSeed(Pm.seed, stream));

        // LoadPath (basic.glsl.inc:159-198).  Grey record form (StorePathVertex):
        // one Probability float, and the empty stack without a load.
        const bool grey = pt_grey_mats(MATS) && L.prob1 != nullptr;
        path P;
        float4 thr = L.thr[s];
        uint2 act;
        if (grey) {
            P.Probability = v4s(L.prob1[s]);
            act = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        } else {
            float4 prob = L.prob[s];
            P.Probability = v4(prob.x, prob.y, prob.z, prob.w);
            act = L.act[s];
        }
        P.Throughput = v4(thr.x, thr.y, thr.z, thr.w);
        P.Sample = v3s(0.0f);          // always 0 between rounds (StorePathVertex)
        P.Lambda0 = L.lam[s];
        P.Active[0] = act.x & 0xFFFF; P.Active[1] = act.x >> 16;
        P.Active[2] = act.y & 0xFFFF; P.Active[3] = act.y >> 16;
        for (int I = 0; I < 4; I++)
            if (P.Active[I] == 0xFFFF) P.Active[I] = SHAPE_INDEX_NONE;

        // LoadTraceResult (basic.glsl.inc:99-131).  The extend kernel leaves a
        // compact hit at the ray's position; the trace record's attributes
        // (Trace, scene.glsl.inc:535-608) are rebuilt here and go through the
        // same octahedral snorm16 quantisation as the reference's
        // StoreTraceHit / LoadTraceResult.
        uint32_t q = RayPos(L, s, p16);
        float4 r = L.ray[q];
        O = v3(r.x, r.y, r.z);
        V = UnpackUnitVector(__float_as_uint(r.w));
        float4 h = L.hit[q];
        uint32_t HitShape = __float_as_uint(h.y), HitMaterial = 0;
        float HitTime = PT_HIT_TIME_LIMIT;
        uint32_t PN = 0, PTg = 0;
        pt2 UV = v2(0, 0);
        if (HitShape != SHAPE_INDEX_NONE) {
            ShadeMark(SM_HIT);
#if PT_SHADE_STATS
            {
                const int32_t Ty = S.shapes[HitShape].Type;
                if (Ty == PT_SHAPE_TYPE_MESH_INSTANCE) ShadeMark(SM_MESH_HIT);
                else if (Ty == PT_SHAPE_TYPE_SPHERE) ShadeMark(SM_SPHERE_HIT);
                else if (Ty == PT_SHAPE_TYPE_PLANE) ShadeMark(SM_PLANE_HIT);
                else ShadeMark(SM_CUBE_HIT);
            }
#endif
            float2 c = L.uv[q];
            pt3 N, TX;
            HitAttributesRecord(S, HitShape, h, c, HitMaterial, N, TX, UV, /*uv_if_textured=*/true,
                                /*prims=*/(MATS & PT_MATS_PRIMS) != 0);
            HitMaterial &= 0xFFFFu;
            HitShape &= 0xFFFFu;
            HitTime = h.x;
            PN = PackUnitVector(N);
            PTg = PackUnitVector(TX);
        }

        if (Scatter<MATS, CLS>(S, G, Pm.termination_probability, P, O, V, HitShape, HitMaterial, HitTime, PN, PTg, UV)) {
            // StorePathVertex of a continuing path: Scatter changes Sample only
            // on escape (which terminates the path) and never Lambda0, so lam
            // is unchanged; the active-shape stack is written when it moved.
            ShadeMark(SM_CONTINUE);
            L.thr[s] = make_float4(P.Throughput.x, P.Throughput.y, P.Throughput.z, P.Throughput.w);
            if (grey) {
                L.prob1[s] = P.Probability.x;
            } else {
                L.prob[s] = make_float4(P.Probability.x, P.Probability.y, P.Probability.z, P.Probability.w);
                uint2 na = make_uint2((P.Active[1] << 16) | P.Active[0], (P.Active[3] << 16) | P.Active[2]);
                if ((na.x != act.x) | (na.y != act.y)) L.act[s] = na;
            }
        } else {
            ShadeMark(SM_COMPLETED);
            completed = true;
            if constexpr (COMPACT) {
                cstate = G.State;
                csample = P.Sample;
                cactnone = (act.x & act.y) == 0xFFFFFFFFu;
            } else {
                CompletePath(S, L, F, Pm, G, s, x, y, stream, P.Sample, (act.x & act.y) == 0xFFFFFFFFu, O, V);
            }
        }
    }
}

// Completion queue (COMPACT shade).  Paths that end at a surface (a sky
// sample below the horizon, roulette, a failed BSDF sample) are scattered over
// the tile's hit waves, so the completion work -- accumulate, then a new
// camera path (GenerateNewPath) -- ran in nearly every wave at a third of its
// lanes (C2: 99 % of waves, 25 lanes).  Here the completed slots of the block
// (cm: this wave's ballot) are queued in LDS in thread order, the first
// threads of the block complete them in full waves, and the new rays come
// back through LDS to their slots' threads.  The same operations on the same
// values: bit-identical.
PT_DEV void CompletionQueue(const dscene& S, const dslots& L, const dframe& F, const dparams& Pm, uint32_t s,
                            bool completed, uint64_t cm, uint32_t cstate, pt3 csample, bool cactnone, pt3& O, pt3& V)
{
    __shared__ uint32_t cq_slot[256], cq_rng[256], cq_count[4];
    __shared__ float cq_f[6][256];
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(cm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cm, 0u));
    if ((threadIdx.x & 63u) == 0) cq_count[w] = (uint32_t)__popcll(cm);
    __syncthreads();
    uint32_t qi = below, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t c = cq_count[k];
        qi += k < w ? c : 0u;
        total += c;
    }
    if (completed) {
        cq_slot[qi] = s | (cactnone ? 0x80000000u : 0u);   // slots < 2^31 (renderer creation)
        cq_rng[qi] = cstate;
        cq_f[0][qi] = csample.x; cq_f[1][qi] = csample.y; cq_f[2][qi] = csample.z;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < total) {
        const uint32_t e = cq_slot[t];
        const uint32_t s2 = e & 0x7FFFFFFFu;
        uint32_t x2, y2, stream2;
        (void)SlotPixel(F, s2, x2, y2, stream2);
        rng G2;
        G2.State = cq_rng[t];
        pt3 O2, V2;
        CompletePath(S, L, F, Pm, G2, s2, x2, y2, stream2, v3(cq_f[0][t], cq_f[1][t], cq_f[2][t]),
                     (e & 0x80000000u) != 0, O2, V2);
        cq_f[0][t] = O2.x; cq_f[1][t] = O2.y; cq_f[2][t] = O2.z;   // each thread rewrites only its own entry
        cq_f[3][t] = V2.x; cq_f[4][t] = V2.y; cq_f[5][t] = V2.z;
    }
    __syncthreads();
    if (completed) {
        O = v3(cq_f[0][qi], cq_f[1][qi], cq_f[2][qi]);
        V = v3(cq_f[3][qi], cq_f[4][qi], cq_f[5][qi]);
    }
}

// One tile of shade (basic_scatter.glsl:main for the tile's 256 slots).
// COMPACT: completion queue, for scenes whose paths also end at surfaces
// (ShadeCompact, rt_rounds.hip).
// LEN: the tile's new rays in LENGTH order (TileOrderLengthKey).
template <uint32_t MATS, bool COMPACT = false, bool LEN = false>
PT_DEV void ShadeTile(const dscene& S, const dslots& L, const dframe& F, const dparams& Pm, uint32_t tile)
{
    // One block per tile, no early exit (TileOrder).  ShadeOrder: thread u
    // shades the slot whose ray sits at ShadePosition(u), so the waves of a
    // tile run the surface path or the escape path, mostly not both; path
    // state is read and written by slot (gathers within the tile's records).
    // The position is the ray's own (slotof inverts TileOrder's slot ->
    // position map), so the ray / hit / uv records load from it directly,
    // beside the slotof lookup instead of after a pos[s] lookup.
    const uint32_t base = tile * 256;
    const uint64_t* om = L.outcome + (size_t)tile * (4 * PT_OUTCOME_CLASSES);
    const uint32_t pq = S.mat_classes ? ShadePosition(om, threadIdx.x)
                                      : ShadePosition2(om + 4 * (PT_OUTCOME_CLASSES - 1), threadIdx.x);
    const uint32_t s = base | L.slotof[base | pq];
    const uint32_t p16 = pq << 8;   // RayPos(s, p16) == base | pq (shade -1 % vs gathering pos[s])
    uint32_t x, y, stream;
    bool valid = SlotPixel(F, s, x, y, stream);
    pt3 O = v3s(0), V = v3s(0);
    bool completed = false;
    uint32_t cstate = 0;
    pt3 csample = v3s(0.0f);
    bool cactnone = false;
    ShadeSlot<MATS, COMPACT>(S, L, F, Pm, s, p16, x, y, stream, valid, O, V, completed, cstate, csample, cactnone);
    // Completed paths per wave (ptGetStats): one counter word per 64 slots,
    // updated by the wave's first lane (no atomics: a wave owns its word).
    uint64_t cm = __ballot(completed);
    if ((threadIdx.x & 63u) == 0) L.done[(base | threadIdx.x) >> 6] += (uint32_t)__popcll(cm);
    if constexpr (COMPACT) CompletionQueue(S, L, F, Pm, s, completed, cm, cstate, csample, cactnone, O, V);
    TileOrderStoreRay<LEN>(L, s, valid, completed, O, V, p16 >> 8);
}

}  // namespace ptd
