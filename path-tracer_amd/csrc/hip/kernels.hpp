// kernels.hpp — launch interface between the host files (rt_*.hip) and the kernel sources
// (extend.hip, shade.hip, rounds.hip, kernels.hip and the post-process files).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/pt_packed.h"
#include "../../../include/pt_api.h"
#include "../../../include/pt_raykey.h"
#include "../../../include/pt_blockmap.h"

namespace ptd {

struct dscene;

// ShadeOrder outcome classes of a traced ray (extend.hpp ExtendRay).
constexpr uint32_t PT_OUTCOME_CLASSES = 5;   // hit: diffuse, metal, translucent, other material; miss

// Per-slot state, SoA of 16-byte records.
struct dslots {
    float4* ray;        // origin.xyz, packed velocity
    float4* hit;        // compact hit: time, shape index, primitive index, coords.x
    float2* uv;         // compact hit: coords.y, coords.z
    float4* thr;        // throughput[4]
    float4* prob;       // probability[4]
    float* prob1;       // grey record form (non-null): the path's Probability, whose four components
                        // are equal, as one float; prob and act are then not read (GreyRecord, path.hpp)
    float* lam;         // normalized lambda0 (a live path's Sample is always 0: StorePathVertex)
    uint2* act;         // active-shape stack (2 x u16 pairs)
    uint16_t* pos;      // per slot: position of its current ray (high byte) and of
                        // its last traced hit (low byte) within its tile (TileOrder)
    uint8_t* slotof;    // per position: the slot (within the tile) whose ray sits there
    uint64_t* outcome;  // ShadeOrder, per tile [class][4 words]: bit t set iff the ray at position t
                        // ended in that class (extend): hit diffuse / metal / translucent / other, miss
    uint32_t* tilecost; // per tile and wave: the wave's extend time (s_memtime ticks)
    uint32_t* order;    // extend's block -> tile map (longest previous extend first), or null
    uint32_t* done;     // per wave of 64 slots: paths completed by shade since the last Reset (ptGetStats)
    uint32_t* spill;    // traversal stack spill: (needed - LDS capacity) rows x n
    const uint32_t* stop = nullptr;   // guarded rounds (ptRenderFrame's last rounds): set -> the launch returns
    uint32_t n;
    uint32_t tile_count;    // n / 256: one block per tile
    // Ray order LENGTH (TileOrder, path.hpp; include/pt_raykey.h).  All
    // null / zero in OCTANT order.
    uint32_t len_order = 0;             // 1: a tile's new camera rays first, then continuing rays by length class
    const uint8_t* len_cls = nullptr;   // the scene's class per ray key (0..6); null until the table is trained
    uint16_t* len_cam = nullptr;        // per tile: its camera rays, which sit at the tile's first positions
    uint32_t* len_sum = nullptr;        // a training extend adds every continuing ray's steps to its key's sum
    uint32_t* len_cnt = nullptr;        // ... and 1 to its count
    pt_raykey_bounds len_bounds{};      // the key's grid over the scene's world bounds
};

struct dframe {
    float4* accum;      // width x height, XYZ sum + count
    uint32_t width, height;
    uint32_t rank, nranks;
    uint32_t tiles_x;
    uint32_t tiles_x_magic;   // ceil(2^32 / tiles_x): t / tiles_x = umulhi(t, magic)
                              // for t * tiles_x < 2^32 (checked at renderer creation)
    // Path streams (ptCreateBasicRendererStreams): the renderer's tiles are
    // `streams` copies of its owned tiles, stream k's seeds offset by k << 24
    // and its paths accumulated in accx[k] (one stream: in accum itself).
    uint32_t streams;         // 1: one path per owned pixel
    uint32_t stream_tiles;    // tiles per stream
    uint32_t stream_magic;    // ceil(2^32 / stream_tiles) (streams > 1)
    float4* accx;             // streams x width x height (streams > 1)
};

struct dparams {
    uint32_t camera_index;
    uint32_t render_flags;
    float termination_probability;
    uint32_t seed;
    // Round batches (rounds_kernel): rounds per launch, and the seed step
    // between them (1: consecutive Run(1) calls, 0: one Run(R)).
    uint32_t rounds = 1;
    uint32_t seed_step = 0;
};

}  // namespace ptd

hipError_t pt_launch_raygen(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                            hipStream_t st);
// train: the training instantiation (LENGTH order; L.len_sum, len_cnt and
// len_cam set), which pt_length_train_supported has for the scene.
// units: the RUN block map (include/pt_blockmap.h) -- one block per entry of
// this segment of the unit order, `unit_count` of them, instead of one per
// tile of L.order; for the scenes pt_block_map_run_supported accepts.
hipError_t pt_launch_extend(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, uint32_t* spill,
                            hipStream_t st, bool train = false, const uint32_t* units = nullptr,
                            uint32_t unit_count = 0);
bool pt_block_map_run_supported(const ptd::dscene& S, bool spill);
// Ray order LENGTH: the scenes whose extend has a training instantiation (the
// mesh-only loop without a spilled stack) and the shade masks whose tile shade
// has a LENGTH instantiation (pt_launch_shade takes it when L.len_order is
// set); the renderer keeps OCTANT order elsewhere.
bool pt_length_train_supported(const ptd::dscene& S, bool spill);
bool pt_length_order_supported(uint32_t scene_mats);
// The table's finalize (one block): per-key mean steps in fixed point, the
// classes from the count-weighted 1/7 .. 6/7 quantiles of the means, the
// middle class for keys without a sample; counts above 2^16 are halved with
// their sums until they fit.
hipError_t pt_launch_length_classes(uint32_t* sum, uint32_t* cnt, uint8_t* cls, hipStream_t st);
hipError_t pt_launch_extend_stats(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, uint32_t* spill,
                                  unsigned long long* out, uint32_t* steps, hipStream_t st);
// Material-type mask of a scene (shade kernel specialisation).
enum : uint32_t {
    PT_MATS_DIFFUSE = 1,
    PT_MATS_METAL = 2,
    PT_MATS_TRANSLUCENT = 4,
    PT_MATS_SCATTER = 8,
    PT_MATS_ALL = 15,
    PT_MATS_OPENPBR = 16,     // OpenPBR shapes shaded (ptSetBasicRendererOpenPBR); instantiated as ALL | OPENPBR
    PT_MATS_PRIMS = 32,       // some shape is a plane, sphere or cube (else every shape is a mesh instance)
    PT_MATS_SKY = 64,         // SkyboxSamplingProbability != 0 (sky light sampling can be drawn)
    PT_MATS_SCENE = PT_MATS_PRIMS | PT_MATS_SKY,
    PT_MATS_TEXWRAP = 128,    // some texture's atlas placement lies outside [0, 1] (host mask only: no lean kernel)
};
uint32_t pt_shade_mats(uint32_t scene_mats);
// Grey record form (path.hpp GreyRecord): the shade mask keeps every path's
// Probability wavelength-uniform and its active-shape stack empty.
constexpr bool pt_grey_mats(uint32_t shade_mats) { return !(shade_mats & (PT_MATS_TRANSLUCENT | PT_MATS_OPENPBR)); }
// Record-form conversions of a renderer's live paths (between rounds):
// counts the valid slots whose Probability components differ or whose stack
// is not empty (a path that cannot take the grey form); converts every valid
// slot's record to the grey form (to_grey) or back to the four-float form.
// State write: rays[i] = the restored ray of slot tile0 * 256 + i, for
// `tiles` tiles; stored at their TileOrder positions, every hit a miss.
hipError_t pt_launch_restore_rays(const ptd::dslots& L, const ptd::dframe& F, const float4* rays, uint32_t tile0,
                                  uint32_t tiles, hipStream_t st);
hipError_t pt_launch_grey_check(const ptd::dslots& L, const ptd::dframe& F, uint32_t* count, hipStream_t st);
hipError_t pt_launch_grey_convert(const ptd::dslots& L, const ptd::dframe& F, float* prob1, bool to_grey,
                                  hipStream_t st);
// Preview base-colour tables: the 16 sample constants of ObserveUnderD65
// (preview.hip), filled once per preview context.
constexpr uint32_t PT_OBSERVE_TABLE_FLOATS = 16 * 5;
hipError_t pt_launch_observe_table(float* table, hipStream_t st);
hipError_t pt_launch_preview(const ptd::dscene& S, const pt_preview_parameters* p, uint32_t* spill, float4* out,
                             pt_preview_aov* aov, uint32_t* query, const float* observe_table, hipStream_t st);
uint32_t pt_preview_stack_cap();
hipError_t pt_launch_resolve(const float4* accum, uint32_t n, float brightness, uint32_t mode, float white, float4* out,
                             uint32_t* out8, hipStream_t st);
// Denoiser (denoise.hip).  Guides: one central camera ray per pixel of a
// w x h frame -> 2 float4 per pixel ({normal, time}, {albedo, shape}: a
// pt_denoise_guide); spill as for the preview (pt_guides_stack_cap).
hipError_t pt_launch_denoise_guides(const ptd::dscene& S, uint32_t camera_index, uint32_t w, uint32_t h,
                                    uint32_t* spill, float4* guides, const float* observe_table, hipStream_t st);
// The guides that follow mirrors and smooth glass (DESIGN.md §6 row 13;
// include/pt_guides.h): the same launch shape and spill rows, a chain of up to
// max_bounces + 1 traces per pixel.  max_bounces <= PT_GUIDE_MAX_BOUNCES.
hipError_t pt_launch_denoise_guides_specular(const ptd::dscene& S, uint32_t camera_index, uint32_t max_bounces,
                                             uint32_t w, uint32_t h, uint32_t* spill, float4* guides,
                                             const float* observe_table, hipStream_t st);
uint32_t pt_guides_stack_cap();
// One a-trous iteration (step 2^iteration) in -> out.  accumulator: `in` is
// a sample buffer's accumulator (iteration 0), else a filtered image.
// lattice: the LDS-staged residue-class kernel, else the global gather; both
// compute the same bits.
hipError_t pt_launch_denoise(const float4* in, bool accumulator, const float4* guides, uint32_t w, uint32_t h,
                             const pt_denoise_parameters* p, uint32_t iteration, bool lattice, float4* out,
                             hipStream_t st);
// Iterations = 0: out = the accumulator's mean, .w = 1 (zeros where empty).
hipError_t pt_launch_denoise_mean(const float4* accum, uint32_t n, float4* out, hipStream_t st);
// The pair filter.  Prepare: accumulators a, b -> the
// working image {c_0, prefiltered variance} (.w = -1 where a + b is empty);
// final (Iterations = 0): c_0 in the sample-buffer form instead.  Then one
// iteration (step 2^iteration) in -> out between working images; last: out
// in the sample-buffer form (.w = 1, zeros where empty).
hipError_t pt_launch_denoise_pair_prepare(const float4* a, const float4* b, const float4* guides, uint32_t w,
                                          uint32_t h, bool final, float4* out, hipStream_t st);
hipError_t pt_launch_denoise_pair(const float4* in, const float4* guides, uint32_t w, uint32_t h,
                                  const pt_denoise_pair_parameters* p, uint32_t iteration, bool last, bool lattice,
                                  float4* out, hipStream_t st);
// Frame statistics (stats.hip) of accumulator a, or of
// a + b with the noise fields from the pair (b != nullptr), added into *out,
// which the caller has cleared: counts as they are, the two minima as the
// complement of their bit patterns, pixels untouched.  uniform: the
// one-atomic-per-wave shortcut for waves whose lanes share a bin (same
// result).  pt_frame_statistics_grid: the blocks launched for n pixels.
uint32_t pt_frame_statistics_grid(uint64_t n, uint32_t cu_count);
hipError_t pt_launch_frame_statistics(const float4* a, const float4* b, uint64_t n, uint32_t cu_count, bool uniform,
                                      pt_frame_statistics* out, hipStream_t st);
// Per-tile statistics (stats.hip): one record per 16 x 16
// tile of a, or of a + b with the pair counts (b != nullptr), written to out
// (ceil(width / 16) * ceil(height / 16) records, row-major).  One block per
// tile; every record is written whole, so out needs no clearing.
hipError_t pt_launch_tile_statistics(const float4* a, const float4* b, uint32_t width, uint32_t height,
                                     float threshold, pt_tile_statistics* out, hipStream_t st);
// Temporal reprojection (reproject.hip): the
// previous accumulator (wp x hp) resampled into the current view (w x h) ->
// out.  The cameras are copied into the launch.  motion == nullptr: row 8.
// Otherwise row 9: motion, motion_count records in device memory (a valid
// address even for an empty table), is read per pixel through the guide's
// shape index.
hipError_t pt_launch_reproject(const float4* prev, const float4* prev_guides, uint32_t wp, uint32_t hp,
                               const pt_packed_camera* prev_camera, const float4* guides, uint32_t w, uint32_t h,
                               const pt_packed_camera* camera, const pt_shape_motion* motion, uint32_t motion_count,
                               const pt_reproject_parameters* p, float4* out, hipStream_t st);
// History validation (rectify.hip): the history hist
// held against the windows of the new accumulator cur under the current
// guides, all w x h -> out.  out may be hist, not cur.  p has passed
// pt_rectify_parameters_ok.
hipError_t pt_launch_rectify(const float4* hist, const float4* cur, const float4* guides, uint32_t w, uint32_t h,
                             const pt_rectify_parameters* p, float4* out, hipStream_t st);
// Firefly clamp (despike.hip): the accumulator src under
// its view's guides, both w x h -> out.  out is not src.  p has passed
// pt_despike_parameters_ok.
hipError_t pt_launch_despike(const float4* src, const float4* guides, uint32_t w, uint32_t h,
                             const pt_despike_parameters* p, float4* out, hipStream_t st);
// dst += src per component.
hipError_t pt_launch_accumulate(float4* dst, const float4* src, uint64_t n, hipStream_t st);
// compact: the completion-queue instantiation (ShadeTile), for scenes whose
// paths also end at surfaces.
hipError_t pt_launch_shade(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                           uint32_t scene_mats, bool compact, hipStream_t st);
// Class-pure shade (shade.hip shade_classq_kernel): per-class lists of the
// round's positions built by class_list_kernel, each class's list CQ_SUB
// sub-lists of pt_classq_sub_capacity words; counts: the PT_OUTCOME_CLASSES x
// CQ_SUB counters of this round (zero at the launch), next_counts: the other
// parity's, cleared for the next round.  L is a tile group's slots (the
// group's tile_count; tiles_all, groups, group: pt_tile_group_tile).  For the
// shade instantiations pt_class_lists_supported accepts.
constexpr uint32_t CQ_SUB = 1;
inline uint32_t pt_classq_sub_capacity(uint32_t tiles) { return (tiles + CQ_SUB - 1) / CQ_SUB * 256; }
bool pt_class_lists_supported(uint32_t scene_mats);
hipError_t pt_launch_shade_classq(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F,
                                  const ptd::dparams& P, uint32_t scene_mats, bool compact, uint32_t* counts,
                                  uint32_t* next_counts, uint32_t* list, hipStream_t st, uint32_t tiles_all = 0,
                                  uint32_t groups = 1, uint32_t group = 0);
hipError_t pt_launch_vertex_decode(const uint2* v, uint32_t n, float4* attr, float* vv, hipStream_t st);
// Tile groups (ptSetBasicRendererSplit; include/pt_blockmap.h): group g of K
// owns the granules g, g + K, ... -- tiles (granule 1), or runs of four tiles
// under the RUN block map (granule 4) -- and its segment of the dispatch
// orders.  The three below are the granule-1 forms (t % K == g), which the
// class-list shade derives a group's tiles from.
__host__ __device__ inline uint32_t pt_tile_group_count(uint32_t tiles, uint32_t groups, uint32_t group)
{
    return group < tiles ? (tiles - group + groups - 1) / groups : 0u;
}
// The i-th tile of a group.
__host__ __device__ inline uint32_t pt_tile_group_tile(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t i)
{
    return group + i * groups;
}
__host__ __device__ inline uint32_t pt_tile_group_start(uint32_t tiles, uint32_t groups, uint32_t group)
{
    uint32_t s = 0;
    for (uint32_t h = 0; h < group; h++) s += pt_tile_group_count(tiles, groups, h);
    return s;
}
// Sorts one group's segment of the tile order L.order longest-first (groups =
// 1: the whole frame) and, for granule 4, the group's segment of the unit
// order `units` in the same launch (a block each): unit (run u, quarter j) keyed by the
// longest quarter-j wave of the run's tiles.
hipError_t pt_launch_tile_order(const ptd::dslots& L, hipStream_t st, uint32_t groups = 1, uint32_t group = 0,
                                uint32_t granule = 1, uint32_t* units = nullptr);
// Guarded rounds (ptRenderFrame): flags[0] := 1 once the done words' sum (the
// paths completed since the Reset, ptGetStats) reaches target; while it is
// 0, flags[1] counts the rounds that run.
hipError_t pt_launch_guard(const uint32_t* done, uint32_t words, uint64_t target, uint32_t* flags, hipStream_t st);
// Fused round (extend + shade per tile in one launch, round_kernel): the
// tiles the GPU can hold at once for this scene (0: not available), and the
// launch (hipErrorNotSupported when the scene needs a spilled stack).
uint32_t pt_round_capacity(uint32_t scene_mats, bool stack16, uint32_t cu_count);
hipError_t pt_launch_round(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                           uint32_t scene_mats, hipStream_t st);
// Round batch: P.rounds rounds (extend + shade) of every tile in one launch,
// each block running its own tile through all of them (rounds_kernel).
hipError_t pt_launch_rounds(const ptd::dscene& S, const ptd::dslots& L, const ptd::dframe& F, const ptd::dparams& P,
                            uint32_t scene_mats, hipStream_t st);
bool pt_rounds_available(const ptd::dslots& L);
// Zeroes the rows of a sample buffer outside a renderer's 16-row bands
// (b % nranks != rank) before a frame-end reduce.
hipError_t pt_launch_zero_unowned(float4* accum, uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks,
                                  hipStream_t st);
// Path streams' merge into the sample buffer's accumulator (owned bands).
hipError_t pt_launch_merge_streams(float4* accum, float4* accx, uint32_t width, uint32_t height, uint32_t rank,
                                   uint32_t nranks, uint32_t streams, hipStream_t st);
// Packed row-major atlas (w x h texels per layer) -> AtlasIndex block layout;
// needs w % 4 == 0 and h % 2 == 0.
hipError_t pt_launch_atlas_tile(const float4* src, float4* dst, uint32_t w, uint32_t h, uint32_t layers, hipStream_t st);
hipError_t pt_launch_rcp_check(unsigned long long* mismatches, hipStream_t st);
hipError_t pt_launch_xdiv_check(uint64_t n, uint32_t seed, unsigned long long* mismatches, hipStream_t st);
// Diagnostic: the traversal counters of ptExtendStats for caller-given rays.
hipError_t pt_launch_trace_rays_stats(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                      const float* dur, float4* hit, float2* hc, uint32_t* spill,
                                      unsigned long long* out, uint32_t* steps, hipStream_t st);
hipError_t pt_launch_trace_rays(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                const float* dur, float4* hit, float2* hc, float4* rec, float2* uv, uint32_t* spill,
                                hipStream_t st);
// ptTraceRays' first launch alone: Trace() of the arrays' rays -> compact hits.
hipError_t pt_launch_trace_rays_extend(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                       const float* dur, float4* hit, float2* hc, uint32_t* spill, hipStream_t st);
// The any-hit query (occlusion.hip) over ptTraceRays'
// inputs: mask word i / 64, bit i % 64 = "something lies within ray i's
// duration"; every one of the (n + 63) / 64 words is written, the last one's
// tail bits 0.  spill as for pt_launch_trace_rays.  The stats form fills
// ptExtendStats' counters (out, cleared by the caller) and, if steps is not
// null, each ray's step count.
hipError_t pt_launch_occluded_rays(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                   const float* dur, uint32_t* spill, unsigned long long* mask, hipStream_t st);
hipError_t pt_launch_occluded_rays_stats(const ptd::dscene& S, uint32_t n, const float* origins, const uint32_t* vel,
                                         const float* dur, uint32_t* spill, unsigned long long* out, uint32_t* steps,
                                         hipStream_t st);
// The ambient-occlusion image (occlusion.hip; include/pt_visibility.h): one
// pixel per thread in 16 x 16 tiles -> out (w x h, {u, u, u, Samples}).  spill:
// (needed - pt_extend_stack_cap()) rows of tiles * 256 columns, or null.  p has
// passed pt_visibility_parameters_ok.
hipError_t pt_launch_ambient_occlusion(const ptd::dscene& S, uint32_t camera_index, uint32_t w, uint32_t h,
                                       const pt_ambient_occlusion_parameters* p, uint32_t* spill, float4* out,
                                       hipStream_t st);
// Visibility gathered at n points (occlusion.hip; include/pt_visibility.h; DESIGN.md
// §6 row 15): one lane per (point, sample), n * Samples <= 2^22 lanes -> out, two
// float4 per point (pt_visibility_record).  Point i draws from stream first_index
// + i.  spill: (needed - pt_extend_stack_cap()) rows of n * Samples columns, or
// null.  p has passed pt_visibility_gather_parameters_ok.
hipError_t pt_launch_gather_visibility(const ptd::dscene& S, uint32_t n, const float* points, const float* normals,
                                       const pt_visibility_gather_parameters* p, uint32_t first_index, uint32_t* spill,
                                       float4* out, hipStream_t st);
// Sky light gathered at n points (occlusion.hip; include/pt_visibility.h; DESIGN.md
// §6 row 16): one lane per (point, sample), n * Samples <= 2^22 lanes -> out,
// eight float4 per point (pt_sky_record).  normals may be null with Lobe SPHERE.
// The other arguments as pt_launch_gather_visibility's.  p has passed
// pt_sky_gather_parameters_ok.
hipError_t pt_launch_gather_sky_light(const ptd::dscene& S, uint32_t n, const float* points, const float* normals,
                                      const pt_sky_gather_parameters* p, uint32_t first_index, uint32_t* spill,
                                      float4* out, hipStream_t st);
hipError_t pt_launch_finalize(const ptd::dscene& S, uint32_t n, const float4* hit, const float2* hc, float4* rec,
                              float2* uv, hipStream_t st);
uint32_t pt_extend_stack_cap();
// Test probes (probe.hip): one numerics operation (include/pt_numerics.h) over
// n operand words, SampleTexture at n caller-given UVs with either wrap, and
// the traversal's slab test (SetLevelRay + IntersectBoxPair) on n rays and
// boxes under a scene of which only fast_div is read.
hipError_t pt_launch_numerics_probe(uint32_t op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                    uint32_t* out, hipStream_t st);
hipError_t pt_launch_sample_textures(const ptd::dscene& S, uint32_t n, const uint32_t* index, const float2* uv,
                                     bool unit_wrap, float4* rgba, hipStream_t st);
hipError_t pt_launch_slab_probe(const ptd::dscene& S, uint32_t n, const float* origin, const float* velocity,
                                const float* reach, const float* box_min, const float* box_max, uint32_t* entry,
                                uint32_t* exact, hipStream_t st);
