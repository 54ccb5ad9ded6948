/*
 * pt_api.h — C ABI of the MI355X wavefront path tracer (libpathtracer.so).
 *
 * Drop-in for the reference's integrator boundary.  Each entry point names the
 * reference interface it replaces (paths relative to the reference root):
 *
 *   ptCreateDevice            src/core/vulkan.hpp  CreateVulkan (device + queue)
 *   ptCreateScene             src/scene/scene.hpp:440  CreateVulkanScene
 *   ptUpdateScene             src/scene/scene.hpp:441  UpdateVulkanScene
 *   ptDestroyScene            src/scene/scene.hpp:442  DestroyVulkanScene
 *   ptCreateSampleBuffer      src/integrator/integrator.hpp:51  CreateSampleBuffer
 *   ptDestroySampleBuffer     src/integrator/integrator.hpp:53  DestroySampleBuffer
 *   ptCreateBasicRenderer     src/integrator/basic.hpp:28  CreateBasicRenderer
 *   ptDestroyBasicRenderer    src/integrator/basic.hpp:29  DestroyBasicRenderer
 *   ptResetBasicRenderer      src/integrator/basic.hpp:31  ResetBasicRenderer
 *   ptRunBasicRenderer        src/integrator/basic.hpp:32  RunBasicRenderer
 *   ptRenderSampleBuffer      src/integrator/integrator.hpp:55-60  RenderSampleBuffer
 *                             (resolve.glsl: XYZ -> sRGB, tone mapping)
 *   ptCreatePreviewRenderContext  src/application/preview_render.hpp:65-70
 *   ptDestroyPreviewRenderContext preview_render.hpp:72-76
 *   ptRenderPreview           preview_render.hpp:85-90  RenderPreview
 *   ptRetrievePreviewQueryResult  preview_render.hpp:78-83
 *   ptBasicRendererParams     src/integrator/basic.hpp:6-26  (the caller-written
 *                             CameraIndex / RenderFlags / PathLengthLimit /
 *                             PathTerminationProbability fields, FrameIndex)
 *
 * Additions (no reference counterpart): sample-buffer readback, explicit
 * synchronisation, a bit-exact ray query (ptTraceRays), slot-state readback,
 * per-kernel timing, pixel-band partitioning, an RCCL frame-end reduce for
 * one-process-per-GPU rendering, a denoiser (guide images + an
 * edge-avoiding a-trous filter) in front of ptRenderSampleBuffer, frame
 * statistics (luminance histogram, automatic exposure, a noise estimate from
 * two half renders), a variance-guided form of the denoiser that takes
 * those two half renders (ptDenoiseSampleBufferPair), and temporal
 * reprojection of an accumulator into a new view (ptReprojectSampleBuffer),
 * which keeps a frame's history across a camera move
 * (ptReprojectSampleBufferMoving: and across an object move), and rounds on a
 * chosen set of 16 x 16 tiles (ptSetBasicRendererActiveTiles) with the
 * per-tile statistics that choose them (ptComputeTileStatistics), and an
 * any-hit occlusion query (ptOccludedRays: one bit per ray, equal to "the
 * closest-hit query hits") with an ambient-occlusion / sky-visibility image
 * built on it (ptRenderAmbientOcclusion), and the same lobe gathered at
 * caller-given points: an occlusion count, mask and bent vector per point
 * (ptGatherVisibility), and the sky's light that reaches such points as nine
 * spherical-harmonic coefficients per CIE XYZ channel (ptGatherSkyLight).
 *
 * Conventions: creators return NULL on failure and set ptGetLastError();
 * other calls return 0 on success or a non-zero status (HIP / RCCL error
 * codes are forwarded).  ptDestroy* accept NULL.  Reset/Run enqueue work on
 * the device's stream and return immediately (the reference records into a
 * command buffer that executes after submit); reads and ptSynchronize block.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stdint.h>
#include "pt_packed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_device pt_device;
typedef struct pt_scene pt_scene;
typedef struct pt_sample_buffer pt_sample_buffer;
typedef struct pt_basic_renderer pt_basic_renderer;
typedef struct pt_comm pt_comm;
typedef struct pt_preview pt_preview;
typedef struct pt_denoise_guides pt_denoise_guides;

/* Mutable renderer state (src/integrator/basic.hpp:18-25).  The caller writes
 * CameraIndex, RenderFlags, PathLengthLimit and PathTerminationProbability
 * before Reset/Run, exactly like application.cpp:104-107.  FrameIndex is the
 * seed schedule: Reset seeds with the current value, Run increments it first
 * and all rounds of one Run share the seed (basic.cpp:285-332). */
typedef struct pt_basic_renderer_params {
    uint32_t FrameIndex;
    uint32_t CameraIndex;
    uint32_t RenderFlags;                 /* PT_RENDER_FLAG_ACCUMULATE | _SAMPLE_JITTER */
    uint32_t PathLengthLimit;             /* unused by the reference integrator */
    float    PathTerminationProbability;
} pt_basic_renderer_params;

/* One trace result (src/integrator/basic.glsl.inc:32-38).  On a miss only
 * shape_material (= 0xFFFFFFFF) is meaningful, as in StoreTraceHit. */
typedef struct pt_hit_record {
    float    time;
    uint32_t shape_material;              /* shape << 16 | material */
    uint32_t packed_normal;               /* octahedral snorm16x2 */
    uint32_t packed_tangent;
    float    u, v;
} pt_hit_record;

/* Per-pixel integrator state (trace_buffer + path_buffer of
 * src/integrator/basic.glsl.inc:23-59), in image order.  Duration is not
 * stored: every producer writes HIT_TIME_LIMIT (scene.glsl.inc:617,
 * basic_scatter.glsl:163,307). */
typedef struct pt_pixel_state {
    float    origin[3];
    uint32_t packed_velocity;
    pt_hit_record hit;
    float    lambda0;
    float    throughput[4];
    float    probability[4];
    float    sample[3];
    uint32_t active01, active23;          /* 4 x u16 active shape stack, 0xFFFF = none */
} pt_pixel_state;

enum {
    PT_KERNEL_RAYGEN  = 0,
    PT_KERNEL_EXTEND  = 1,   /* also ptTraceRays' extend launch, ptOccludedRays' launch, ptGatherVisibility's launches and ptGatherSkyLight's launches */
    PT_KERNEL_SHADE   = 2,
    PT_KERNEL_RESOLVE = 3,
    PT_KERNEL_PREVIEW = 4,
    PT_KERNEL_ROUND   = 5,   /* fused extend + shade of a small partition (one launch per round) */
    PT_KERNEL_ROUNDS  = 6,   /* a round batch: several rounds of every tile in one launch */
    PT_KERNEL_DENOISE = 7,   /* one a-trous iteration of ptDenoiseSampleBuffer; ptDespikeSampleBuffer's launch */
    PT_KERNEL_GUIDES  = 8,   /* ptRenderDenoiseGuides[Specular], ptRenderAmbientOcclusion */
    PT_KERNEL_STATS   = 9,   /* ptComputeFrameStatistics' and ptComputeTileStatistics' passes, ptAccumulateSampleBuffer's add */
    PT_KERNEL_REPROJECT = 10, /* ptReprojectSampleBuffer, ptReprojectSampleBufferMoving, ptRectifyHistory */
    PT_KERNEL_COUNT   = 11,
};

/* resolve_parameters (src/integrator/integrator.hpp:12-48). */
enum {
    PT_TONE_MAPPING_CLAMP    = 0,
    PT_TONE_MAPPING_REINHARD = 1,
    PT_TONE_MAPPING_HABLE    = 2,
    PT_TONE_MAPPING_ACES     = 3,
};

/* preview_render_mode (src/application/preview_render.hpp:3-13). */
enum {
    PT_PREVIEW_RENDER_MODE_BASE_COLOR        = 0,
    PT_PREVIEW_RENDER_MODE_BASE_COLOR_SHADED = 1,
    PT_PREVIEW_RENDER_MODE_NORMAL            = 2,
    PT_PREVIEW_RENDER_MODE_MATERIAL_INDEX    = 3,
    PT_PREVIEW_RENDER_MODE_PRIMITIVE_INDEX   = 4,
    PT_PREVIEW_RENDER_MODE_MESH_COMPLEXITY   = 5,
    PT_PREVIEW_RENDER_MODE_SCENE_COMPLEXITY  = 6,
};

/* preview_parameters (preview_render.hpp:22-33). */
typedef struct pt_preview_parameters {
    pt_packed_transform CameraTransform;
    uint32_t RenderMode;
    float    Brightness;
    uint32_t SelectedShapeIndex;          /* 0xFFFFFFFF = none */
    uint32_t RenderSizeX, RenderSizeY;
    uint32_t MouseX, MouseY;
} pt_preview_parameters;

/* Per-pixel primary-hit AOVs of the preview: Trace()'s hit (scene.glsl.inc:
 * 102-119) for the pixel's primary ray. */
typedef struct pt_preview_aov {
    float    time;
    uint32_t shape_index;                 /* 0xFFFFFFFF on a miss (other fields 0) */
    uint32_t material_index;
    uint32_t primitive_index;
    uint32_t mesh_complexity;             /* BLAS nodes visited (Hit.MeshComplexity) */
    uint32_t scene_complexity;            /* TLAS nodes visited (Hit.SceneComplexity) */
    float    normal[3];                   /* world normal, not quantised */
    float    u, v;
    uint32_t reserved;
} pt_preview_aov;

typedef struct pt_resolve_parameters {
    float    Brightness;                  /* default 1 */
    uint32_t ToneMappingMode;             /* PT_TONE_MAPPING_*, default CLAMP */
    float    ToneMappingWhiteLevel;       /* Reinhard white level, default 1 */
} pt_resolve_parameters;

const char* ptGetLastError(void);

pt_device* ptCreateDevice(int hip_device);
void       ptDestroyDevice(pt_device* device);
int        ptSynchronize(pt_device* device);
int        ptGetDeviceCount(int* count);

pt_scene* ptCreateScene(pt_device* device);
int       ptUpdateScene(pt_device* device, pt_scene* scene, const pt_scene_packs* packs, uint32_t dirty_flags);
void      ptDestroyScene(pt_device* device, pt_scene* scene);
/* Encodings chosen per scene at ptUpdateScene (no effect on results; the
 * wider forms are what larger scenes need, so tests force them on small
 * ones).  Stack format: AUTO = 16-bit entries when every TLAS / BLAS entry
 * fits, else packed 32-bit BLAS words when every node fits, else node
 * indices; WORDS32 / NODE_INDEX force the wider forms.  Hit record: AUTO =
 * the hit face's vertex indices when they fit 21 bits, else its face index;
 * FACE_INDEX forces the latter.  Take effect at the next ptUpdateScene. */
enum {
    PT_STACK_FORMAT_AUTO       = 0,
    PT_STACK_FORMAT_WORDS32    = 1,
    PT_STACK_FORMAT_NODE_INDEX = 2,
    PT_HIT_RECORD_AUTO         = 0,
    PT_HIT_RECORD_FACE_INDEX   = 1,
};
int       ptSetSceneStackFormat(pt_scene* scene, uint32_t format);
int       ptSetSceneHitRecordForm(pt_scene* scene, uint32_t form);
/* The extend kernel's form (no effect on results).  AUTO: a scene that is one
 * mesh instance (one shape, the TLAS root a leaf) is traced by a mesh-only
 * traversal loop, every other scene by the general two-level one; GENERAL
 * forces the latter (tests, A/B timing).  Set takes effect at the next
 * ptUpdateScene; Get reports the form the uploaded scene runs (GENERAL or
 * MESH). */
enum {
    PT_EXTEND_FORM_AUTO    = 0,
    PT_EXTEND_FORM_GENERAL = 1,
    PT_EXTEND_FORM_MESH    = 2,
};
int       ptSetSceneExtendForm(pt_scene* scene, uint32_t form);
int       ptGetSceneExtendForm(pt_scene* scene, uint32_t* form);
/* Traversal stack entries the uploaded scene can need (TLAS depth + deepest
 * BLAS depth, each capped at the reference's Stack[32]); the extend kernel keeps
 * 20 in LDS and spills the rest to a per-ray global buffer. */
int       ptSceneStackNeeded(pt_scene* scene, uint32_t* entries);
/* Whether the uploaded scene's box tests take the exact fast slab division
 * (1: every TLAS and BLAS box coordinate is 0 or has magnitude in
 * [2^-50, 2^40], checked at every ptUpdateScene; 0: a coordinate outside it, so
 * every box test divides, or no packs yet).  Results are the same either way
 * (DESIGN.md §2); tests read it to state which branch they ran. */
int       ptSceneFastDivision(pt_scene* scene, uint32_t* enabled);
/* BLAS child pairs the extend kernel keeps in LDS for the uploaded scene
 * (the top levels of its BLASes, laid out first in the device node array;
 * 0 = no cache: scenes whose stack entries need 32 bits, or no mesh). */
int       ptSceneNodeCache(pt_scene* scene, uint32_t* pairs);

pt_sample_buffer* ptCreateSampleBuffer(pt_device* device, uint32_t width, uint32_t height);
void              ptDestroySampleBuffer(pt_device* device, pt_sample_buffer* buffer);
/* rgba = width*height*4 floats: CIE XYZ sums + sample count, row-major. */
int               ptReadSampleBuffer(pt_device* device, pt_sample_buffer* buffer, float* rgba);
/* Overwrites the accumulator (e.g. to resume accumulation from a saved one). */
int               ptWriteSampleBuffer(pt_device* device, pt_sample_buffer* buffer, const float* rgba);
/* RenderSampleBuffer: resolves the accumulator into the buffer's display
 * image on the device stream (resolve.glsl:112-128). */
int               ptRenderSampleBuffer(pt_device* device, pt_sample_buffer* buffer, const pt_resolve_parameters* params);
/* Display image of the last ptRenderSampleBuffer: the fragment shader's
 * OutColor (rgba32f, alpha 1) ... */
int               ptReadResolvedImage(pt_device* device, pt_sample_buffer* buffer, float* rgba);
/* ... and its 8-bit sRGB encoding as a B8G8R8A8_SRGB swapchain stores it
 * (bytes R,G,B,A per pixel). */
int               ptReadResolvedImageSRGB8(pt_device* device, pt_sample_buffer* buffer, uint8_t* rgba8);

pt_basic_renderer* ptCreateBasicRenderer(pt_device* device, pt_scene* scene, pt_sample_buffer* buffer);
/* Renderer owning only the 16-row pixel bands b with b % nranks == rank. */
pt_basic_renderer* ptCreateBasicRendererPartitioned(pt_device* device, pt_scene* scene, pt_sample_buffer* buffer,
                                                    uint32_t rank, uint32_t nranks);
/* Path streams for a partition too small to fill the GPU:
 * the renderer carries `streams` independent paths per owned pixel, stream k
 * seeded with FrameIndex + (k << 24) -- the sample shards' offsets -- so one
 * launch holds streams x the partition's slots.  With more than one stream
 * each stream accumulates into an accumulator of its own, and
 * ptMergeBasicRendererStreams writes their sum, in stream order, into the
 * sample buffer's owned pixels (call it before reading or exchanging a
 * frame; it may repeat as the rounds go on).  Each stream's state and
 * accumulator equal a one-stream renderer's started at its FrameIndex
 * offset. */
pt_basic_renderer* ptCreateBasicRendererStreams(pt_device* device, pt_scene* scene, pt_sample_buffer* buffer,
                                                uint32_t rank, uint32_t nranks, uint32_t streams);
int                ptMergeBasicRendererStreams(pt_device* device, pt_basic_renderer* renderer);
uint32_t           ptBasicRendererStreams(pt_basic_renderer* renderer);
void               ptDestroyBasicRenderer(pt_device* device, pt_basic_renderer* renderer);
pt_basic_renderer_params* ptBasicRendererParams(pt_basic_renderer* renderer);
int                ptResetBasicRenderer(pt_device* device, pt_basic_renderer* renderer);
int                ptRunBasicRenderer(pt_device* device, pt_basic_renderer* renderer, uint32_t rounds);
uint32_t           ptBasicRendererSlotCount(pt_basic_renderer* renderer);
/* Fused rounds: 0 = never (extend then shade launches), 1 = automatic (one
 * extend+shade launch per round when every tile of the renderer fits on the
 * GPU at once: a rank's share of a strongly scaled frame), 2 = whenever the
 * scene allows (no spilled traversal stack).  Results are identical in every
 * mode.  Default 1. */
int                ptSetBasicRendererFusedRounds(pt_basic_renderer* renderer, int mode);
/* Consecutive rounds: ptRunBasicRendererRounds(d, r, k) is k calls of
 * ptRunBasicRenderer(d, r, 1) -- the application's frame loop, one new
 * FrameIndex per round (application.cpp:100-115) -- with identical results.
 * Round batches run up to R of those rounds in one launch, each tile
 * advancing through them without a grid-wide barrier between rounds (a slot's
 * round depends only on its own previous round).  ptSetBasicRendererRoundBatch:
 * 0 = automatic (16 rounds per launch when every tile of the renderer fits on
 * the GPU at once and fused rounds are automatic, else one round per launch
 * pair), 1 = never, R >= 2 = R whenever the scene allows (no spilled stack).
 * Default 0.  ptRenderFrame runs its Run(1) rounds this way. */
int                ptRunBasicRendererRounds(pt_device* device, pt_basic_renderer* renderer, uint32_t count);
int                ptSetBasicRendererRoundBatch(pt_basic_renderer* renderer, uint32_t rounds);
/* Tile groups on concurrent streams (no reference counterpart: a launch
 * schedule).  Consecutive rounds that run one launch pair per round
 * (ptRunBasicRendererRounds, ptRenderFrame) split the renderer's tiles into K
 * groups (tile t in group t % K); each group runs the batch's rounds on its
 * own HIP stream, so one group's launches fill the CUs another group's
 * kernel tail leaves idle.  The device stream forks before the batch and
 * joins after it, and every wait covers the groups.  Results are identical
 * for every K.  groups: 0 = automatic (3 when the rounds run unfused over at
 * least 2 048 tiles, else 1), 1 = off, 2..PT_MAX_SPLIT = that many (4 takes
 * every hardware queue of the process and measured slower).
 * ptGetBasicRendererSplit reports the K that consecutive rounds use now, the
 * tiles of group 0 (the launches kernel profiling times) and all tiles; any
 * pointer may be NULL.  Default 0.  Under the RUN block map (below) a group
 * owns whole runs of four tiles: runs u % K instead of tiles t % K. */
#define PT_MAX_SPLIT 4
/* Class-pure shade inside tile groups (no reference counterpart: a launch
 * schedule).  In scenes with more than one material type, the rounds of a
 * tile group shade through per-class lists of the round's rays, so that each
 * wave shades one material class. Results are identical.  mode: 0 =
 * automatic (on for such scenes in tile groups), 1 = off.
 * ptGetBasicRendererClassLists sets *used to 1 when consecutive rounds use
 * them now.  Default 0. */
int                ptSetBasicRendererClassLists(pt_basic_renderer* renderer, uint32_t mode);
int                ptGetBasicRendererClassLists(const pt_basic_renderer* renderer, uint32_t* used);
/* Ray order (no reference counterpart: where a tile's 256 new rays sit in the
 * tile's ray records; results are identical in every order).  OCTANT: by
 * direction octant.  LENGTH: new camera rays first, then continuing rays by
 * the traversal length predicted for their ray key (include/pt_raykey.h) from
 * a table the device scene learns on a fixed schedule of training rounds --
 * the first 16 LENGTH rounds after the table was cleared and every 64th after
 * them -- so that short rays share waves (DESIGN.md §4 "Length classes").  The
 * table belongs to the scene: every ptUpdateScene that touches shapes or
 * meshes clears it, Resets and frames keep it, renderers of one scene share
 * it.  LENGTH runs where the mesh-only extend loop and the diffuse tile shade
 * do (a scene that is one mesh instance, no spilled stack, unfused rounds);
 * elsewhere the renderer keeps OCTANT.  AUTO (default) = LENGTH where it runs.
 * ptGetBasicRendererRayOrder: the order set and the order the next unfused
 * rounds use (either pointer may be NULL).
 * ptReadSceneLengthTable (diagnostic; any pointer may be NULL): the class
 * 0..6 of each of the PT_RAYKEY_COUNT keys, whether a finalize has written
 * them since the last clear, and the LENGTH rounds counted since then.
 * ptReadBasicRendererRayPositions (diagnostic): per slot, the position of its
 * current ray (high byte) and of its last traced hit (low byte) within its
 * tile; ptBasicRendererSlotCount entries.  Both reads synchronise. */
enum { PT_RAY_ORDER_AUTO = 0, PT_RAY_ORDER_OCTANT = 1, PT_RAY_ORDER_LENGTH = 2 };
int                ptSetBasicRendererRayOrder(pt_basic_renderer* renderer, uint32_t order);
int                ptGetBasicRendererRayOrder(const pt_basic_renderer* renderer, uint32_t* order, uint32_t* used);
int                ptReadSceneLengthTable(pt_device* device, pt_scene* scene, uint8_t* classes, uint32_t* trained,
                                          uint64_t* rounds);
int                ptReadBasicRendererRayPositions(pt_device* device, pt_basic_renderer* renderer, uint16_t* positions);
int                ptSetBasicRendererSplit(pt_basic_renderer* renderer, uint32_t groups);
int                ptGetBasicRendererSplit(const pt_basic_renderer* renderer, uint32_t* groups, uint32_t* timed_tiles,
                                           uint32_t* tiles);
/* Block map (no reference counterpart: which extend block traces which ray
 * positions; results are identical under every map; include/pt_blockmap.h,
 * DESIGN.md §4 "Block map").  TILE: a block traces one tile's four quarters of
 * 64 positions.  RUN: a block traces one quarter of each of four consecutive
 * tiles, so that under LENGTH order its four waves have one predicted length;
 * tile groups then own whole runs of four tiles and extend is dispatched by an
 * order over (run, quarter) units.  RUN runs where LENGTH order does, in
 * rounds issued as separate launches (not fused rounds or round batches) with
 * no active tile set in place; a renderer set to RUN where it never can (a
 * scene LENGTH order does not run on) refuses its rounds with a message.
 * AUTO (default) = RUN wherever it runs.  ptGetBasicRendererBlockMap: the map
 * set and the map the next rounds use (either pointer may be NULL).
 * ptBlockMap*: the host's view of include/pt_blockmap.h for granule 1 (TILE)
 * or 4 (RUN) -- a group's tiles and units, where its segments of the two
 * orders start, and the tile and quarter wave 0..3 of a unit's block traces
 * (the tile may lie past the last one: the wave then traces nothing).  They
 * return 0 for a granule other than 1 or 4 or groups == 0. */
enum { PT_BLOCK_MAP_AUTO = 0, PT_BLOCK_MAP_TILE = 1, PT_BLOCK_MAP_RUN = 2 };
int                ptSetBasicRendererBlockMap(pt_basic_renderer* renderer, uint32_t map);
int                ptGetBasicRendererBlockMap(const pt_basic_renderer* renderer, uint32_t* map, uint32_t* used);
uint32_t           ptBlockMapGroupTileCount(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule);
uint32_t           ptBlockMapGroupTile(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule, uint32_t i);
uint32_t           ptBlockMapGroupTileStart(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule);
uint32_t           ptBlockMapGroupUnitCount(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule);
uint32_t           ptBlockMapGroupUnit(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule, uint32_t i);
uint32_t           ptBlockMapGroupUnitStart(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule);
uint32_t           ptBlockMapUnitTile(uint32_t unit, uint32_t wave, uint32_t granule);
uint32_t           ptBlockMapUnitQuarter(uint32_t unit, uint32_t wave, uint32_t granule);
/* Active tile set (no reference counterpart): the rounds
 * that follow run on the chosen 16 x 16 tiles only.  A full-frame renderer
 * numbers its tiles row-major: tile (tx, ty) covers the pixels [16 tx, 16 tx +
 * 16) x [16 ty, 16 ty + 16) clipped to the image and has index ty * tiles_x +
 * tx, tiles_x = ceil(width / 16) -- pt_tile_statistics' numbering.
 * mask[t] != 0: tile t takes part; mask == NULL with tiles == 0: every tile
 * (the default).  The mask is copied.
 *   - ptRunBasicRenderer and ptRunBasicRendererRounds advance FrameIndex as
 *     before; their launches cover the active tiles.  Nothing of an inactive
 *     tile is written: slot records, TileOrder words, outcome and done words,
 *     accumulator pixels.  After the same calls from the same state an active
 *     tile's slots and pixels equal an unmasked renderer's bit for bit, in
 *     every scheduling mode (separate launches, fused rounds, round batches,
 *     tile groups).  An all-zero mask launches nothing; an all-ones mask gives
 *     the bits of no mask.
 *   - ptResetBasicRenderer keeps the mask and still restarts every tile's
 *     paths.  State reads and writes cover the whole frame.  (A change of the
 *     path record form after a scene update converts every tile's records.)
 *   - ptGetStats' rays grow by the active tiles' valid slots per round.
 *   - The automatic rules of tile groups and fused rounds count the active
 *     tiles.  Class lists are off while a mask is set
 *     (ptGetBasicRendererClassLists reports 0), and the longest-first re-sort
 *     of the dispatch order rests: active tiles run in natural order.
 *   - Setting or clearing a mask waits for the device.
 * Fails, launching nothing and leaving the set as it was, on a NULL device or
 * renderer, a partitioned or multi-stream renderer, tiles different from the
 * renderer's tile count, or a NULL mask with tiles > 0.  ptRenderFrame fails
 * while a mask is set.  ptGetBasicRendererActiveTiles: the tiles the next
 * round launches and all tiles; either pointer may be NULL. */
int                ptSetBasicRendererActiveTiles(pt_device* device, pt_basic_renderer* renderer, const uint8_t* mask,
                                                 uint32_t tiles);
int                ptGetBasicRendererActiveTiles(const pt_basic_renderer* renderer, uint32_t* active, uint32_t* tiles);
/* OpenPBR shading (opt-in extension, no reference counterpart): 0 (default)
 * = an OpenPBR hit ends its path with no contribution, as in the reference,
 * whose integrator does not compile its OpenPBR BSDF (scene.glsl.inc:685);
 * 1 = shade OpenPBR materials with the layered sampler and medium of
 * src/scene/openpbr.glsl.inc (deviations in DESIGN.md §6). */
int                ptSetBasicRendererOpenPBR(pt_basic_renderer* renderer, int enable);
/* Work done since the last Reset: rays traced (one per owned pixel per round)
 * and paths completed (accumulator sample increments, basic_scatter.glsl:
 * 350-359).  Either pointer may be NULL.  Synchronises the device stream. */
int                ptGetStats(pt_device* device, pt_basic_renderer* renderer, uint64_t* rays, uint64_t* samples);
/* Benchmark-mode frame (no reference entry point: the
 * application loop of application.cpp:100-115 with an spp target): Reset,
 * Run(2), then Run(1) rounds until the paths completed since the Reset reach
 * target_samples (e.g. spp * pixels owned) or max_rounds (>= 2) rounds ran.
 * The frame always ends at the first round whose total reaches the target,
 * as the loop issued one round at a time would (the rounds are batched only
 * where they cannot overshoot, the last few guarded on the device).
 * Blocks until done.  rounds_out / samples_out (either may be NULL): rounds
 * run and paths completed. */
int                ptRenderFrame(pt_device* device, pt_basic_renderer* renderer, uint64_t target_samples,
                                 uint32_t max_rounds, uint32_t* rounds_out, uint64_t* samples_out);
/* out = width*height states in image order; pixels outside the renderer's
 * partition are left untouched.  Stream 0's paths (ptReadBasicRendererStreamState:
 * any stream's). */
int                ptReadBasicRendererState(pt_device* device, pt_basic_renderer* renderer, pt_pixel_state* out);
int                ptReadBasicRendererStreamState(pt_device* device, pt_basic_renderer* renderer, uint32_t stream,
                                                  pt_pixel_state* out);
/* Resume (no reference counterpart; the reference restarts paths on Reset,
 * basic_scatter.glsl:330-336): restores the live path of every owned pixel
 * of stream 0 (or `stream`) from `in` (width*height states in image order, as
 * ptReadBasicRendererState returned them between rounds; other pixels are not
 * read): the next ray and the path record (lambda0, throughput, probability,
 * active shapes).  The trace record is not restored -- the next Run traces
 * the restored ray before it scatters, so it is not needed; the readback shows
 * a miss until then.  With the accumulator (ptWriteSampleBuffer) and
 * FrameIndex restored too, the following Runs equal the uninterrupted
 * render's bit for bit.  Fails, writing nothing, if a sample is non-zero (a
 * live path's is 0 between rounds), a lambda0 lies outside [0, 1] or an
 * active entry is neither 0xFFFF nor a shape of the scene.  Synchronises. */
int                ptWriteBasicRendererState(pt_device* device, pt_basic_renderer* renderer, const pt_pixel_state* in);
int                ptWriteBasicRendererStreamState(pt_device* device, pt_basic_renderer* renderer, uint32_t stream,
                                                   const pt_pixel_state* in);
/* A path stream's own accumulator (width*height*4 floats, as
 * ptReadSampleBuffer): with one stream it is the sample buffer; with several,
 * the per-stream sums ptMergeBasicRendererStreams adds up.  Saving and
 * restoring every stream's accumulator and state resumes a multi-stream
 * render bit for bit. */
int                ptReadBasicRendererStreamAccumulator(pt_device* device, pt_basic_renderer* renderer, uint32_t stream,
                                                        float* rgba);
int                ptWriteBasicRendererStreamAccumulator(pt_device* device, pt_basic_renderer* renderer,
                                                         uint32_t stream, const float* rgba);

/* Diagnostic: the shade variant the renderer runs (chosen on the host from
 * the scene's packs at ptUpdateScene and from the renderer's options; no
 * effect on results).  Mask bits: material types present, a scattering
 * medium, analytic shapes, sky light sampling that matters (the host cannot
 * prove SkyboxSamplingProbability * pdf an exact +0), texture placements
 * outside the unit square. */
enum {
    PT_SHADE_DIFFUSE     = 1,
    PT_SHADE_METAL       = 2,
    PT_SHADE_TRANSLUCENT = 4,
    PT_SHADE_SCATTER     = 8,
    PT_SHADE_OPENPBR     = 16,
    PT_SHADE_PRIMS       = 32,
    PT_SHADE_SKY         = 64,
    PT_SHADE_TEXWRAP     = 128,
};
typedef struct pt_shade_info {
    uint32_t scene_mask;        /* PT_SHADE_* of the scene as the renderer shades it */
    uint32_t kernel_mask;       /* the instantiation launched: the smallest superset built
                                   (PT_SHADE_DIFFUSE alone = the lean diffuse-mesh kernel) */
    uint32_t completion_queue;  /* 1: completed paths restart through the block's queue
                                   (the separate extend / shade launches; fused rounds do not queue) */
    uint32_t grey_records;      /* 1: live paths keep one Probability float and no stack
                                   (as of the last Reset / Run / state write) */
    uint32_t ray_order;         /* PT_RAY_ORDER_OCTANT or PT_RAY_ORDER_LENGTH: the order the next
                                   unfused rounds place new rays in (AUTO resolved, fall-backs applied) */
    uint32_t length_trained;    /* 1: the scene's length table holds trained classes */
    uint32_t block_map;         /* PT_BLOCK_MAP_TILE or PT_BLOCK_MAP_RUN: the map the next rounds' extend
                                   launches use (AUTO resolved, fall-backs applied) */
} pt_shade_info;
int                ptGetBasicRendererShadeInfo(pt_basic_renderer* renderer, pt_shade_info* info);

/* Editor preview (preview_render.glsl:96-178): one primary ray per pixel of
 * RenderSizeX x RenderSizeY through the same Trace() as the integrator.
 * RenderPreview enqueues; the reads synchronise.  The query result is the
 * shape index under (MouseX, MouseY) of the last render (0xFFFFFFFF = sky or
 * no render yet; a mouse position outside the image leaves it unchanged, as
 * the reference's query buffer). */
pt_preview* ptCreatePreviewRenderContext(pt_device* device, pt_scene* scene);
void        ptDestroyPreviewRenderContext(pt_device* device, pt_preview* context);
int         ptRenderPreview(pt_device* device, pt_preview* context, const pt_preview_parameters* params);
int         ptRetrievePreviewQueryResult(pt_device* device, pt_preview* context, uint32_t* hit_shape_index);
/* rgba: RenderSizeX * RenderSizeY * 4 floats (OutColor); aov: one record per pixel. */
int         ptReadPreviewImage(pt_device* device, pt_preview* context, float* rgba);
int         ptReadPreviewAOVs(pt_device* device, pt_preview* context, pt_preview_aov* aov);

/* Denoiser (no reference counterpart; definition, kernel design and measured
 * times in DESIGN.md §6): an edge-avoiding a-trous wavelet filter (Dammertz
 * et al. 2010) over a sample buffer's mean, steered by guide images -- the
 * primary hit's normal, distance, base colour and shape -- taken with the
 * scene's own camera.
 *
 * A guides object holds width x height pt_denoise_guide records
 * (pt_packed.h) and the filter's intermediate image.  ptRenderDenoiseGuides
 * enqueues one ray per pixel: the central ray of GenerateCameraRay
 * (scene.glsl.inc:613-655) for packed camera `camera_index` -- sample
 * position pixel + 0.5, lens point at the lens centre, no random number --
 * with its velocity packed and unpacked as every ray of the integrator is
 * between raygen and extend.  normal, time and shape are those of the ray's
 * pt_hit_record (ptTraceRays); albedo is the preview's BASE_COLOR colour at
 * Brightness 1 without a selection (the sky's colour on a miss).  An unknown
 * camera model gives misses with albedo 0.  Fails, launching nothing, on a
 * NULL handle, a scene of another device or without packs, or
 * camera_index >= the scene's camera count.  Read blocks; Write replaces the
 * records (e.g. guides computed elsewhere). */
pt_denoise_guides* ptCreateDenoiseGuides(pt_device* device, uint32_t width, uint32_t height);
void ptDestroyDenoiseGuides(pt_device* device, pt_denoise_guides* guides);
int  ptRenderDenoiseGuides(pt_device* device, pt_scene* scene, pt_denoise_guides* guides, uint32_t camera_index);
/* Guides that follow perfect mirrors and smooth glass to the surface a pixel
 * shows (the arithmetic is include/pt_guides.h's).  The
 * ray starts as ptRenderDenoiseGuides' does.  A hit on a basic metal or basic
 * translucent material whose roughness at the hit is < 1e-3 (the integrator's
 * HasDirac) is followed, at most max_bounces times: the ray is reflected, or
 * refracted by the material's base index (glass always transmits; total
 * internal reflection reflects), and restarted as basic_scatter restarts a
 * path.  The record is that of the first hit that is not followed: its
 * normal and base colour, time = the summed hit times of the chain, and
 * shape = tag << 16 | shape index, where tag is 1 + the index of the first
 * followed shape (0: seen directly), so that a surface seen directly, in one
 * mirror and in another are three surfaces to every consumer's equality
 * test.  A miss writes the miss record with the sky's colour along the last
 * direction and no tag.  max_bounces = 0 gives ptRenderDenoiseGuides' bits.
 * Known limits: no Fresnel reflection branch and no dispersion; no
 * active-shape stack (nested dielectrics are walked surface by surface);
 * media neither absorb nor scatter the ray; time is a path length, so
 * reprojection reconstructs the virtual image (exact for planar mirrors);
 * ptReprojectSampleBufferMoving gives tagged pixels no history (their shape
 * word is beyond the motion table).  Fails like ptRenderDenoiseGuides, and on
 * max_bounces > PT_GUIDE_MAX_BOUNCES, launching nothing. */
#define PT_GUIDE_MAX_BOUNCES 8
int  ptRenderDenoiseGuidesSpecular(pt_device* device, pt_scene* scene, pt_denoise_guides* guides,
                                   uint32_t camera_index, uint32_t max_bounces);
int  ptReadDenoiseGuides(pt_device* device, pt_denoise_guides* guides, pt_denoise_guide* out);
int  ptWriteDenoiseGuides(pt_device* device, pt_denoise_guides* guides, const pt_denoise_guide* in);
/* Enqueues the filter: dst's accumulator := the denoised mean XYZ of src in
 * .xyz and 1 in .w (0, 0, 0, 0 where src's sample count is not positive), so
 * ptRenderSampleBuffer, ptReadSampleBuffer and the image writers work on dst
 * unchanged.  src is not written.  One launch per iteration (step 2^i),
 * between dst and the guides object's intermediate image (allocated at the
 * first call with Iterations >= 2); two calls on the same inputs give the
 * same bits, and the result equals ptsDenoise's (pt_scene.h) bit for bit.
 * Fails, writing nothing, when src == dst, when src, dst and guides differ in
 * size or device, when Iterations > 8 or when a sigma is not > 0. */
int  ptDenoiseSampleBuffer(pt_device* device, pt_sample_buffer* src, pt_denoise_guides* guides,
                           const pt_denoise_parameters* params, pt_sample_buffer* dst);
/* The filter kernel of each iteration (no effect on results): AUTO = the
 * faster one measured per step size, GATHER = every tap from
 * global memory, LATTICE = one residue class of the step lattice per block,
 * taps staged in LDS. */
enum {
    PT_DENOISE_VARIANT_AUTO    = 0,
    PT_DENOISE_VARIANT_GATHER  = 1,
    PT_DENOISE_VARIANT_LATTICE = 2,
};
int  ptSetDenoiseVariant(pt_denoise_guides* guides, uint32_t variant);
/* The variance-guided filter over two half renders (SVGF's spatial part,
 * Schied et al. 2017; definition in DESIGN.md §6 row 7): a and b are two
 * independent renders of one frame (renderers whose FrameIndex differ by
 * 1 << 24, as for ptComputeFrameStatistics).  The filter works on a + b; its
 * luminance edge-stop is SigmaLuminance standard deviations of the pixel's
 * luminance, estimated from a - b, prefiltered 3x3 and filtered along with
 * the colour, so it stops smoothing where the render has converged and does
 * not depend on the frame's brightness.  Enqueues like ptDenoiseSampleBuffer
 * and leaves dst in the same form; a and b are not written.  One prepare
 * launch plus one per iteration, all counted under PT_KERNEL_DENOISE, between
 * dst and the guides object's intermediate image (needed from Iterations >=
 * 1); honours ptSetDenoiseVariant; two calls on the same inputs give the same
 * bits, and the result equals ptsDenoisePair's (pt_scene.h) bit for bit.
 * Fails, launching and writing nothing, on a NULL argument, when two of a, b
 * and dst are the same buffer, when a, b, dst and guides differ in size or
 * device, when Iterations > 8 or when a sigma is not > 0. */
int  ptDenoiseSampleBufferPair(pt_device* device, pt_sample_buffer* a, pt_sample_buffer* b, pt_denoise_guides* guides,
                               const pt_denoise_pair_parameters* params, pt_sample_buffer* dst);
/* Firefly clamp in front of the denoisers (no reference counterpart;
 * definition, kernel design and measured times in DESIGN.md §6 row 12;
 * arithmetic in pt_despike.h).  src is an accumulator, guides the records of
 * the same view.  A pixel's value is the largest component of its mean
 * colour; where it exceeds Scale times the Rank-th largest value among the
 * pixels of the window around it that show the same surface, plus Floor, the
 * pixel's colour sums are scaled down onto that limit.  Every pixel of dst
 * receives src's pixel, clamped or bit for bit; the sample count is never
 * changed, and a pixel that is not usable (a non-finite component, a count
 * not > 0) or has fewer than MinNeighbours such neighbours keeps its bits.
 * dst stays an accumulator: denoise it, add it to another, or go on
 * rendering into it.  For two half renders call it once per half.  Enqueues
 * one launch (counted under PT_KERNEL_DENOISE) and returns, like
 * ptRectifyHistory.  src and guides are not written; two calls on the same
 * inputs give the same bits, and the result equals ptsDespike's (pt_scene.h)
 * bit for bit.  Fails, launching and writing nothing, on a NULL argument,
 * dst == src (a window reads neighbours another block would have replaced),
 * an object of another device, objects of different sizes, or a parameter
 * outside its range (pt_packed.h). */
int  ptDespikeSampleBuffer(pt_device* device, pt_sample_buffer* src, pt_denoise_guides* guides,
                           const pt_despike_parameters* params, pt_sample_buffer* dst);

/* Temporal reprojection (no reference counterpart; definition, kernel design
 * and measured times in DESIGN.md §6 row 8; arithmetic in pt_reproject.h):
 * carries a frame's history across a camera move or a resize.  prev is the
 * accumulator of the previous view, prev_guides its guide records and
 * *prev_camera the packed camera record they were rendered with (the caller
 * keeps it: the scene has been updated since); guides and *camera are the
 * current view's.  Every pixel of dst receives the bilinear blend of the
 * previous accumulator's taps that still show its surface (same shape, normal
 * and distance within the parameters' bounds), as (mean XYZ * n, n) with n
 * the carried sample count capped at MaxHistory, or 0, 0, 0, 0 where the
 * pixel is disoccluded.  dst is an accumulator: a renderer with
 * PT_RENDER_FLAG_ACCUMULATE adds new samples on top of it.  Call it after the
 * frame's ptResetBasicRenderer, whose raygen clears dst, and before its
 * ptRunBasicRenderer.  Enqueues one launch (PT_KERNEL_REPROJECT) and returns,
 * like ptDenoiseSampleBuffer; both cameras are read during the call.  prev
 * and both guides objects are not
 * written; two calls on the same inputs give the same bits, and the result
 * equals ptsReproject's (pt_scene.h) bit for bit.  Fails, launching and
 * writing nothing, on a NULL argument, prev == dst, prev_guides == guides,
 * an object of another device, prev and prev_guides (or dst and guides) of
 * different sizes, or a parameter outside its range (pt_packed.h). */
int  ptReprojectSampleBuffer(pt_device* device, pt_sample_buffer* prev, pt_denoise_guides* prev_guides,
                             const pt_packed_camera* prev_camera, pt_denoise_guides* guides,
                             const pt_packed_camera* camera, const pt_reproject_parameters* params,
                             pt_sample_buffer* dst);
/* The same across an object move: motion is a table of
 * motion_count records in host memory, one per packed shape (ptsShapeMotion,
 * pt_scene.h, fills it from the two frames' packed shapes).  A hit pixel
 * whose shape's record is PT_SHAPE_MOTION_MOVED looks for its history where
 * that surface point was in the previous frame and expects the normal the
 * shape had there; a shape index >= motion_count or a NO_HISTORY record
 * gives the pixel no history; every other pixel gets
 * ptReprojectSampleBuffer's bits.  The table is read during the call (into a
 * pinned copy) and uploaded, in stream order, into a buffer the device object
 * owns (grown on demand); then one launch (PT_KERNEL_REPROJECT).  A call waits
 * for the previous call's upload, not for its kernel.  motion == NULL with
 * motion_count == 0 means no table: ptReprojectSampleBuffer itself.  Equals
 * ptsReprojectMoving bit for bit.  Fails, launching and writing nothing, on
 * ptReprojectSampleBuffer's errors and on motion == NULL with
 * motion_count > 0. */
int  ptReprojectSampleBufferMoving(pt_device* device, pt_sample_buffer* prev, pt_denoise_guides* prev_guides,
                                   const pt_packed_camera* prev_camera, pt_denoise_guides* guides,
                                   const pt_packed_camera* camera, const pt_shape_motion* motion,
                                   uint32_t motion_count, const pt_reproject_parameters* params,
                                   pt_sample_buffer* dst);
/* History validation (no reference counterpart; definition, kernel design and
 * measured times in DESIGN.md §6 row 11; arithmetic in pt_rectify.h): holds a
 * carried history against the new frame's own samples, so that shading that
 * changed without any geometry changing (a shadow that moved, an edited
 * material or sky) does not keep its weight.  history is an accumulator in
 * (mean * n, n) form, e.g. a reprojection's output; current is the
 * accumulator of the new rounds alone; guides are the current view's.  Every
 * pixel of dst receives the history with its mean colour pulled into
 * mean +- Sigma standard deviations of the current samples of the window
 * around it that show the same surface, and, where it had to be pulled, its
 * count cut to ClampedHistory; a pixel with fewer than MinNeighbours such
 * samples keeps its bits, one without a usable history becomes 0, 0, 0, 0.
 * dst is an accumulator again: adding it to current with
 * ptAccumulateSampleBuffer gives the frame the renderer goes on accumulating
 * into.  dst == history is
 * allowed and is the normal use.  Enqueues one launch (counted under
 * PT_KERNEL_REPROJECT) and returns, like ptReprojectSampleBuffer.  current
 * and guides are not written; two calls on the same inputs give the same
 * bits, and the result equals ptsRectifyHistory's (pt_scene.h) bit for bit.
 * Fails, launching and writing nothing, on a NULL argument, dst == current,
 * history == current, an object of another device, objects of different
 * sizes, or a parameter outside its range (pt_packed.h). */
int  ptRectifyHistory(pt_device* device, pt_sample_buffer* history, pt_sample_buffer* current,
                      pt_denoise_guides* guides, const pt_rectify_parameters* params, pt_sample_buffer* dst);

/* Frame statistics (no reference counterpart; definition, kernel design and
 * measured times in DESIGN.md §6 row 6; helpers that read the result in
 * pt_stats.h): one device pass over sample buffer a, or over a and b, two
 * independent renders of one frame (renderers whose FrameIndex differ by
 * 1 << 24).  With b the luminance part of *out describes a + b, the combined
 * frame, and the noise part the relative half-difference of the pixels
 * filled in both; without b the noise fields are 0.  Neither buffer is
 * written.  Blocks, like ptReadSampleBuffer.  The result holds counts and
 * min/max only and equals ptsFrameStatistics' (pt_scene.h) bit for bit.
 * Fails, launching nothing and leaving *out untouched, on a NULL device, a or
 * out, on b == a, and on a or b of another device or b of another size. */
int  ptComputeFrameStatistics(pt_device* device, pt_sample_buffer* a, pt_sample_buffer* b,
                              pt_frame_statistics* out);
/* Per-tile statistics (no reference counterpart): the
 * classes and the pair rule of the frame statistics counted per 16 x 16 tile
 * in one device pass, the data an active tile set is chosen from.  out holds
 * ceil(width / 16) * ceil(height / 16) records, tile (tx, ty) at ty *
 * ceil(width / 16) + tx (ptSetBasicRendererActiveTiles' numbering).  Without b
 * pair and over are 0; with b the classes and counts describe a + b.  over
 * counts the pair pixels whose relative half-difference r exceeds
 * noise_threshold.  Blocks, like ptComputeFrameStatistics; one launch,
 * counted under PT_KERNEL_STATS.  Equals ptsTileStatistics (pt_scene.h) bit
 * for bit.  Fails, launching nothing and leaving out untouched, on
 * ptComputeFrameStatistics' errors and on a noise_threshold that is NaN or
 * negative. */
int  ptComputeTileStatistics(pt_device* device, pt_sample_buffer* a, pt_sample_buffer* b, float noise_threshold,
                             pt_tile_statistics* out);
/* Enqueues dst's accumulator += src's, each component in binary32: combines
 * two halves without a host round trip.  src is not written.  Fails,
 * launching nothing, on a NULL argument, dst == src, or buffers of different
 * size or of another device. */
int  ptAccumulateSampleBuffer(pt_device* device, pt_sample_buffer* dst, pt_sample_buffer* src);
/* The statistics kernel's histogram update (no effect on results): PLAIN =
 * one LDS atomic per lane, UNIFORM = one per wave when all of its active
 * lanes share a bin, AUTO = the one kept after measuring. */
enum {
    PT_STATS_VARIANT_AUTO    = 0,
    PT_STATS_VARIANT_PLAIN   = 1,
    PT_STATS_VARIANT_UNIFORM = 2,
};
int  ptSetFrameStatisticsVariant(pt_device* device, uint32_t variant);

/* Bit-exact Trace() (scene.glsl.inc:522-611) of n rays: origins (3n floats),
 * packed unit velocities (n), durations (n) -> n hit records. */
int ptTraceRays(pt_device* device, pt_scene* scene, uint32_t n, const float* origins,
                const uint32_t* packed_velocities, const float* durations, pt_hit_record* out);

/* The any-hit (occlusion) query (no reference counterpart; DESIGN.md §6 row
 * 14): for each of ptTraceRays' n rays, whether anything lies within its
 * duration.  mask holds (n + 63) / 64 words; ray i is bit i % 64 of word
 * i / 64, and the bits at and above n in the last word are 0.  Every word is
 * written.  The traversal is Trace() stopped at its first accepted
 * intersection, a prefix of the closest-hit traversal of the same ray, so
 *     occluded(ray) == (ptTraceRays(ray).shape_material != 0xFFFFFFFF)
 * holds exactly, for every ray, duration, stack format and scene.  A hit at
 * exactly `duration` counts or not as the shape's own test decides (a plane,
 * sphere or mesh face at t == duration occludes, a cube does not): it is
 * Trace()'s rule, not one of this query's.  No hit record is formed and there
 * is no finalize pass: one launch, one bit per ray read back.  Blocks, like
 * ptTraceRays, and fails as it does: on a NULL device or scene, on n > 0 with
 * a NULL array, on a scene without packs; n == 0 succeeds and writes nothing.
 * While the device profiles, the launch is timed under PT_KERNEL_EXTEND, as
 * ptTraceRays' extend launch is. */
int ptOccludedRays(pt_device* device, pt_scene* scene, uint32_t n, const float* origins,
                   const uint32_t* packed_velocities, const float* durations, uint64_t* mask);

/* Diagnostic: evaluates the device's exact fast division helper (XDiv: an
 * FMA-corrected reciprocal, no longer on the traversal path since the slab
 * test's reciprocal convention) against IEEE division on n
 * device-generated operand pairs; returns the number of bit mismatches
 * (must be 0). */
int ptCheckFastDivision(pt_device* device, uint64_t n, uint32_t seed, uint64_t* mismatches);

/* Diagnostic: evaluates the device's fast reciprocal (hardware rcp + one
 * FMA Newton step) on every float d with 2^-126 <= |d| < 2^126 against the
 * IEEE quotient 1.0f / d; returns the number of bit mismatches (must be 0). */
int ptCheckFastReciprocal(pt_device* device, uint64_t* mismatches);

/* Test probe: evaluates operation `op` of pt_numerics.h (PT_NUM_*) on the
 * device over n elements, calling the functions of pt_fp.h and pt_device.hpp
 * as the kernels do.  a, b, c are the operand words (a float's bit pattern or
 * the integer itself); an operand the op does not read may be NULL.  out
 * receives n * pt_numerics_outputs(op) words, element i first.  The host's
 * counterpart is the oracle's oracle_fp_eval; tests compare the two bit for
 * bit.  Blocks.  Fails, launching and writing nothing, on a NULL device, an
 * unknown op, or n > 0 with out or a needed operand NULL; n == 0 succeeds. */
int ptEvalNumerics(pt_device* device, uint32_t op, uint32_t n, const uint32_t* a, const uint32_t* b,
                   const uint32_t* c, uint32_t* out);

/* Test probe: SampleTexture (scene.glsl.inc:181-205) of the uploaded scene's
 * texture texture_index[i] at uv[2 i], uv[2 i + 1] -> rgba[4 i ..], n samples.
 * wrap selects the texel wrap: 0 = the signed remainder (every scene), 1 =
 * the two-select form of the lean shade kernel, which is exact only when
 * every atlas placement lies in [0, 1] and is refused for a scene whose mask
 * has PT_SHADE_TEXWRAP.  Blocks.  Fails, launching and writing nothing, on a
 * NULL argument (with n > 0), a scene of another device or without packs,
 * wrap > 1, or a texture index >= the scene's texture count. */
int ptSampleTextures(pt_device* device, pt_scene* scene, uint32_t n, const uint32_t* texture_index,
                     const float* uv, uint32_t wrap, float* rgba);

/* Test probe: the traversal's slab test as the kernels call it, one case per
 * thread.  Case i sets its level ray with SetLevelRay from origin[3 i ..] and
 * velocity[3 i ..] under a scene of which only the box-coordinate gate
 * (scene_gate, 0 or 1: dscene::fast_div) is set, then tests the box
 * box_min[3 i ..], box_max[3 i ..] with IntersectBoxPair (the box as both
 * children) against reach[i].  entry[i] receives the entry time's bit pattern
 * (PT_INFINITY's for a miss), exact[i] the ray's fast-division flag (0 or 1).
 * The host's counterpart is IEEE division: whenever the flag is set the entry
 * time must equal it bit for bit (zeros of either sign aside).  Blocks.
 * Fails, launching and writing nothing, on a NULL device, scene_gate > 1, or
 * n > 0 with a NULL array; n == 0 succeeds. */
int ptEvalSlabTest(pt_device* device, uint32_t n, const float* origin, const float* velocity, const float* reach,
                   const float* box_min, const float* box_max, uint32_t scene_gate, uint32_t* entry, uint32_t* exact);

/* Diagnostic: runs the extend step on the renderer's current rays with
 * traversal counters.  It writes the same hit records the next Run's extend
 * writes first, so the render is not perturbed.  out = {rays, lane steps, wave steps x 64, internal nodes,
 * BLAS leaves, faces tested, stack pops, TLAS leaves, waves, then the internal
 * BLAS wave steps by the number of distinct nodes among the wave's lanes
 * taking them: 1, 2, 3-4, 5-8, more than 8}. */
#define PT_EXTEND_STATS_COUNT 14
int ptExtendStats(pt_device* device, pt_basic_renderer* renderer, uint64_t out[PT_EXTEND_STATS_COUNT]);
/* Diagnostic, same pass: the traversal step count of every ray, per ray
 * POSITION (steps[q], q < width-rounded slot count; 0 where no ray). */
int ptExtendStepCounts(pt_device* device, pt_basic_renderer* renderer, uint32_t* steps);

/* Diagnostic, caller-given rays (the ptTraceRays inputs): the counters of
 * ptExtendStats and, if steps != NULL, each ray's traversal step count. */
int ptTraceRaysStats(pt_device* device, pt_scene* scene, uint32_t n, const float* origins,
                     const uint32_t* packed_velocities, const float* durations,
                     uint64_t out[PT_EXTEND_STATS_COUNT], uint32_t* steps);
/* Diagnostic: the same counters and step counts for ptOccludedRays' any-hit
 * traversal of those rays (the first nine counters are filled).  A ray's
 * any-hit step count is at most its closest-hit one, and equal where the ray
 * is not occluded. */
int ptOccludedRaysStats(pt_device* device, pt_scene* scene, uint32_t n, const float* origins,
                        const uint32_t* packed_velocities, const float* durations,
                        uint64_t out[PT_EXTEND_STATS_COUNT], uint32_t* steps);

/* Ambient occlusion / sky visibility (no reference counterpart; definition in
 * pt_visibility.h and DESIGN.md §6 row 14).  Every pixel of dst takes the
 * primary ray and normal of ptRenderDenoiseGuides for camera camera_index; on
 * a hit, params->Samples cosine-lobe rays of length params->Radius leave the
 * hit point, drawn from the integrator's random stream of that pixel in frame
 * params->Seed, and go through the any-hit traversal of ptOccludedRays.  The
 * pixel becomes (u, u, u, Samples) with u the number of unoccluded rays; a
 * miss, or a camera of unknown model, is (Samples, Samples, Samples, Samples).
 * dst is therefore an accumulator: ptRenderSampleBuffer shows the visible
 * fraction, ptAccumulateSampleBuffer adds images of different seeds, and both
 * denoisers take it.  .y is the value; the image is data, not colour (the
 * three equal components are not CIE XYZ of anything).  Enqueues one launch
 * (counted under PT_KERNEL_GUIDES) and returns, like ptRenderDenoiseGuides;
 * two calls give the same bits.  Fails, launching and writing nothing, on a
 * NULL argument, a scene or buffer of another device, a scene without packs,
 * camera_index out of range, Samples outside 1..64 or a Radius that is not
 * > 0 (a NaN included). */
int ptRenderAmbientOcclusion(pt_device* device, pt_scene* scene, uint32_t camera_index,
                             const pt_ambient_occlusion_parameters* params, pt_sample_buffer* dst);

/* Visibility gathered at caller-given points (no reference counterpart;
 * definition in pt_visibility.h and DESIGN.md §6 row 15): for light probes,
 * vertex or texel bakes and contact shading, where the points are not the
 * pixels of a camera.  points and normals hold 3 floats per point and are
 * used as given (a normal is neither normalised nor quantised).  Point i
 * draws params->Samples rays of row 14's cosine lobe around its normal from
 * the random stream params->FirstIndex + i of frame params->Seed; they start
 * params->Offset along their direction, reach params->Radius and go through
 * ptOccludedRays' any-hit traversal, one lane per (point, sample).  out[i] is
 * the point's pt_visibility_record (pt_packed.h): the occluded bits, the
 * unoccluded count and the bent vector, summed by a fixed tree, so two calls
 * give the same bits.  A point's first S' rays are its rays at Samples = S',
 * and a call on points [a, b) with FirstIndex = a equals that slice of the
 * whole call.  Uploads 24 bytes per point, launches in chunks of whole points
 * and at most 2^22 lanes (each launch counted under PT_KERNEL_EXTEND), reads
 * back 32 bytes per point and blocks.  n == 0 succeeds and touches nothing.
 * Fails, launching and writing nothing, on a NULL argument (the arrays with
 * n > 0), a scene of another device or without packs, Samples not a power of
 * two in 1..64, a Radius that is not > 0 (a NaN included), an Offset that is
 * negative or not finite, n > 2^26 or FirstIndex + n > 2^32. */
int ptGatherVisibility(pt_device* device, pt_scene* scene, uint32_t n, const float* points, const float* normals,
                       const pt_visibility_gather_parameters* params, pt_visibility_record* out);
/* Test probe: ptGatherVisibility with launches of at most max_lanes lanes
 * (64..2^22; ptGatherVisibility passes 2^22), so that a small batch takes
 * several launches.  The records do not depend on max_lanes. */
int ptGatherVisibilityChunked(pt_device* device, pt_scene* scene, uint32_t n, const float* points,
                              const float* normals, const pt_visibility_gather_parameters* params,
                              uint32_t max_lanes, pt_visibility_record* out);

/* Sky light gathered at caller-given points (no reference counterpart;
 * definition in pt_visibility.h and DESIGN.md §6 row 16): every scene is lit by
 * its sky alone, so the first-order lighting of a point is the sky's radiance
 * over the directions that are not blocked.  points (and normals, with
 * params->Lobe == PT_SKY_GATHER_COSINE) hold 3 floats per point and are used
 * as given.  Point i draws params->Samples rays from the random stream
 * params->FirstIndex + i of frame params->Seed: with Lobe COSINE exactly
 * ptGatherVisibility's rays for the same Samples, Radius, Seed, Offset and
 * FirstIndex; with Lobe SPHERE uniform over the sphere, and normals is not read
 * (it may be NULL).  Each ray goes through ptOccludedRays' any-hit traversal,
 * one lane per (point, sample); an open ray contributes what a camera ray
 * leaving the scene along it adds to its pixel (the sky's radiance at four
 * wavelengths of a draw of the same stream, observed to CIE XYZ, in the
 * integrator's units), times the nine real spherical harmonics of bands 0..2
 * along it (z up; pt_sky_gather_basis).  out[i] is the point's pt_sky_record
 * (pt_packed.h): SH[i][c] summed by a fixed tree, so two calls give the same
 * bits; OccludedMask, Unoccluded and Samples as ptGatherVisibility's, and with
 * Lobe COSINE equal to them.
 *
 * Reading a record of S samples, Y0 = 0.28209479:
 *   COSINE: pi * SH[0][c] / (Y0 * S) is the XYZ irradiance from the sky at the
 *           point; SH[0][c] / (Y0 * S) is the pixel value the integrator
 *           converges to for direct sky light on a white Lambertian surface
 *           there.
 *   SPHERE: (4 pi / S) * SH[i][c] are the SH9 coefficients of the visible
 *           sky's radiance around the point (a light probe).
 * Records of other Seeds add, field by field, to a record of more samples.
 *
 * Nesting and partition independence hold as for ptGatherVisibility.  Uploads
 * 12 or 24 bytes per point, launches in chunks of whole points and at most
 * 2^22 lanes (each launch counted under PT_KERNEL_EXTEND), reads back 128
 * bytes per point and blocks.  n == 0 succeeds and touches nothing.  Fails,
 * launching and writing nothing, on a NULL argument (the arrays with n > 0;
 * normals only with Lobe COSINE), a scene of another device or without packs,
 * a Lobe other than the two, or Samples, Radius, Offset, n or FirstIndex
 * outside ptGatherVisibility's ranges. */
int ptGatherSkyLight(pt_device* device, pt_scene* scene, uint32_t n, const float* points, const float* normals,
                     const pt_sky_gather_parameters* params, pt_sky_record* out);
/* Test probe: ptGatherSkyLight with launches of at most max_lanes lanes
 * (64..2^22; ptGatherSkyLight passes 2^22).  The records do not depend on
 * max_lanes. */
int ptGatherSkyLightChunked(pt_device* device, pt_scene* scene, uint32_t n, const float* points,
                            const float* normals, const pt_sky_gather_parameters* params, uint32_t max_lanes,
                            pt_sky_record* out);

/* Per-kernel device time, measured with HIP events on the renderer stream. */
int ptSetProfiling(pt_device* device, int enable);
/* Time only the kernels of every period-th round (default 1; rounds counted
 * across ptRunBasicRenderer calls): each event pair around a kernel costs
 * issue time, so a timed loop can sample its kernels' durations instead of
 * bracketing every launch. */
int ptSetProfilingPeriod(pt_device* device, uint32_t period);
int ptGetKernelStats(pt_device* device, int kernel, uint64_t* launches, double* total_ms);
/* Rounds covered by the timed launches of `kernel` (one per launch, except a
 * round batch, PT_KERNEL_ROUNDS, which covers its rounds): total_ms / rounds
 * is the kernel's time per round. */
int ptGetKernelRounds(pt_device* device, int kernel, uint64_t* rounds);
int ptResetKernelStats(pt_device* device);

/* RCCL communicator over one process per GPU (xGMI).
 *
 * Failure contract: every ptComm* exchange first agrees
 * on its argument checks across the ranks (a one-word all-reduce), so a
 * check that fails on any rank fails the call on every rank and nothing is
 * exchanged.  While a communicator is live, every call that waits for the
 * device stream (ptSynchronize, the reads, ptGetStats, ptRenderFrame,
 * ptUpdateScene, the comm calls' own checks) polls the stream, RCCL's
 * asynchronous error state and the communicator's deadline instead of
 * blocking: on an RCCL error it aborts the device's communicators
 * (ncclCommAbort) and returns PT_ERROR_COMM_ABORTED, at the deadline
 * PT_ERROR_TIMEOUT.  An aborted communicator fails every later call with
 * PT_ERROR_COMM_ABORTED; destroy it (and the process normally exits). */
enum {
    PT_ERROR_COMM_ABORTED = -2,
    PT_ERROR_TIMEOUT      = -3,
};
int      ptCommGetUniqueId(uint8_t id[128]);
pt_comm* ptCommCreate(pt_device* device, int nranks, int rank, const uint8_t id[128]);
void     ptCommDestroy(pt_comm* comm);
/* Deadline of a wait on the device stream while the communicator is live
 * (default 600 s: longer than any frame of the benchmark configurations). */
int      ptCommSetTimeout(pt_comm* comm, double seconds);
/* Frame-end ncclReduce(sum) of the float4 accumulator to `root` (exact: the
 * ranks' pixel bands are disjoint).  Each rank first zeroes the rows outside
 * the bands of the last partitioned renderer created on the buffer, so the
 * root's buffer may be reduced again after further rounds (progressive
 * frames): after every call it holds the sum of the ranks' own bands. */
int      ptCommReduceSampleBuffer(pt_device* device, pt_comm* comm, pt_sample_buffer* buffer, int root);
/* The same frame-end exchange at 1/N of the traffic: every rank's own bands
 * go point-to-point to `root`, which stores them in place (grouped
 * ncclSend/ncclRecv).  Requires the buffer's partition (the last partitioned
 * renderer created on it) to be this communicator's rank of nranks.  After
 * the call the root's buffer holds every rank's bands; other ranks' buffers
 * are unchanged.  Repeatable after further rounds. */
int      ptCommGatherSampleBuffer(pt_device* device, pt_comm* comm, pt_sample_buffer* buffer, int root);
/* Sample sharding (north_star: "pixels/samples shard ... RCCL reduce of the
 * per-pixel radiance and sample-count buffers at frame end"): every rank
 * renders the whole frame with its own RNG stream (a FrameIndex offset per
 * rank) and keeps its own running accumulator; this out-of-place
 * ncclReduce(sum) leaves in `total` on `root` the sum over ranks of their
 * XYZ radiance sums and sample counts, which the resolve averages.  The
 * ranks' own accumulators are unchanged, so the call may repeat after more
 * rounds (progressive frames).  `total` is read only on `root` (may be NULL
 * elsewhere) and must match `buffer`'s size. */
int      ptCommReduceSampleBufferInto(pt_device* device, pt_comm* comm, pt_sample_buffer* buffer,
                                      pt_sample_buffer* total, int root);

#ifdef __cplusplus
}
#endif

#endif /* PT_API_H */
