// runtime.hpp — what the host files of libpathtracer.so (rt_*.hip) share: the
// error state, the device array, the seven handle structs of include/pt_api.h,
// the device wait and launch timing, and the renderer helpers that more than
// one file needs.  Everything that is not a pt* entry point lives in namespace
// ptrt with hidden visibility: the library exports none of it.
//
// The host side replaces the reference's Vulkan integrator host
// (src/integrator/basic.cpp, src/integrator/integrator.cpp:15-87) and scene
// upload (src/scene/scene.cpp:1643-2006) with HIP: device buffers for the
// packed scene, a float4 sample buffer, SoA slot buffers, and kernel launches
// on one stream per device.
#pragma once
#include "pt_device.hpp"
#include "kernels.hpp"
#include "../../../include/pt_api.h"
#include "../../../include/pt_denoise.h"
#include "../../../include/pt_reproject.h"
#include "../../../include/pt_rectify.h"
#include "../../../include/pt_despike.h"
#include "../../../include/pt_guides.h"
#include "../../../include/pt_stats.h"
#include "../../../include/pt_numerics.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace ptrt __attribute__((visibility("hidden"))) {

// Sets the calling thread's ptGetLastError text (rt_device.hip).
void SetError(const char* fmt, ...);

#define PT_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ptrt::SetError("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (int)e_;                                                                  \
        }                                                                                    \
    } while (0)

// A device array that owns its memory: freed when the buffer, or the object
// it is a member of, goes away (with that object's device current and its
// stream idle: the destroy functions see to both before their delete).
template <class T>
struct dbuf {
    T* ptr = nullptr;
    size_t count = 0;
    dbuf() = default;
    dbuf(const dbuf&) = delete;
    dbuf& operator=(const dbuf&) = delete;
    ~dbuf() { release(); }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; count = 0; }
    hipError_t upload(const T* src, size_t n)
    {
        // An empty array still gets one zeroed element, so that kernels which
        // read a first record unconditionally (the TLAS root in LaneBegin)
        // read defined memory in a scene without shapes.
        if (!ptr || n > count) {
            release();
            hipError_t e = hipMalloc(&ptr, std::max<size_t>(n, 1) * sizeof(T));
            if (e != hipSuccess) { ptr = nullptr; return e; }
            count = n;
        }
        if (n == 0) return hipMemset(ptr, 0, sizeof(T));
        return hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t alloc(size_t n)
    {
        if (n <= count && ptr) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&ptr, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) { ptr = nullptr; return e; }
        count = n;
        return hipSuccess;
    }
    // alloc, then the n elements zeroed (like upload: on the null stream).
    hipError_t alloc_zero(size_t n)
    {
        hipError_t e = alloc(n);
        return e != hipSuccess || n == 0 ? e : hipMemset(ptr, 0, n * sizeof(T));
    }
};

struct event_pair { hipEvent_t a, b; int kernel; uint32_t rounds; hipStream_t stream; };

}  // namespace ptrt

struct pt_device {
    int id = 0;
    hipStream_t stream = nullptr;
    uint32_t cu_count = 256;
    bool profiling = false;
    uint32_t profile_period = 1;   // time every period-th Run call
    uint64_t run_tick = 0;
    std::vector<ptrt::event_pair> pending;
    std::vector<ptrt::event_pair> free_events;
    // Live RCCL communicators on this device: while one exists, the blocking
    // calls wait for the stream by polling it together with RCCL's
    // asynchronous error state and a deadline (DeviceWait), so a collective
    // whose peer died returns an error instead of hanging.
    std::vector<pt_comm*> comms;
    bool comm_failed = false;      // a communicator was aborted: waits keep a short deadline
    uint64_t launches[PT_KERNEL_COUNT] = {};
    uint64_t rounds[PT_KERNEL_COUNT] = {};    // rounds the timed launches covered (a batch: its rounds)
    double total_ms[PT_KERNEL_COUNT] = {};
    // Tile-group streams (ptSetBasicRendererSplit): groups 1.. of a batch of
    // rounds run on these, forked from `stream` and joined back into it, so
    // every wait on `stream` covers them.  Created on first use.
    hipStream_t group_stream[PT_MAX_SPLIT - 1] = {};
    hipEvent_t fork_event = nullptr;
    hipEvent_t join_event[PT_MAX_SPLIT - 1] = {};
    // ptComputeFrameStatistics' result on the device: allocated at the first
    // call, cleared on `stream` before every launch.
    ptrt::dbuf<pt_frame_statistics> stats;
    uint32_t stats_variant = PT_STATS_VARIANT_AUTO;
    // ptComputeTileStatistics' records on the device: grown on demand, every
    // record rewritten by each launch.
    ptrt::dbuf<pt_tile_statistics> tile_stats;
    // ptReprojectSampleBufferMoving's motion table on the device: grown on
    // demand, rewritten on `stream` before every launch that reads it, from a
    // pinned copy of the caller's table (so the caller's memory is done with
    // when the call returns); motion_copied: that upload has left the copy.
    ptrt::dbuf<pt_shape_motion> motion;
    pt_shape_motion* motion_host = nullptr;
    size_t motion_host_count = 0;
    hipEvent_t motion_copied = nullptr;
};

struct pt_scene {
    pt_device* dev = nullptr;
    ptd::dscene d{};
    ptrt::dbuf<pt_packed_texture> textures;
    ptrt::dbuf<uint32_t> material;
    ptrt::dbuf<pt_packed_shape> shapes;        // device copy: Pad0 = PT_SHAPE_FLAG_UV when the material reads UVs
    ptrt::dbuf<pt_packed_shape_node> shape_nodes;
    ptrt::dbuf<pt_packed_mesh_face> faces;
    ptrt::dbuf<pt_packed_mesh_vertex> vertices;
    ptrt::dbuf<float4> vertex_attr;            // decoded vertex normals + U (vertex_decode_kernel)
    ptrt::dbuf<float> vertex_v;                // decoded V
    ptrt::dbuf<pt_packed_mesh_node> mesh_nodes;
    ptrt::dbuf<pt_packed_camera> cameras;
    ptrt::dbuf<float> atlas;
    bool atlas_tiled = false;    // atlas in AtlasIndex 4x2-texel blocks
    uint32_t camera_count = 0;
    uint32_t texture_count = 0;  // texture records on the device (ptSampleTextures checks its indices)
    uint32_t stack_needed = 0;   // max traversal stack entries (TLAS + BLAS)
    uint32_t mats = PT_MATS_ALL | PT_MATS_SCENE; // SceneMaterialMask (shade specialisation)
    uint32_t stack_format = PT_STACK_FORMAT_AUTO;   // ptSetSceneStackFormat (applied at the next update)
    uint32_t hit_record = PT_HIT_RECORD_AUTO;       // ptSetSceneHitRecordForm (applied at the next update)
    uint32_t cached_pairs = 0;   // BLAS child pairs at the front of the device node array (NodeCacheLayout)
    bool blas_packable = false;  // BlasWordsPackable / BlasWords16FirstBits of the device node layout
    uint32_t blas16_bits = 0;
    uint32_t extend_form = PT_EXTEND_FORM_AUTO;     // ptSetSceneExtendForm (applied at the next update)
    bool one_mesh = false;       // the uploaded scene is one mesh instance (OneMeshScene; d.mesh_root, d.mesh_from)
    // Traversal-length table (ray order LENGTH; rt_rounds.hip): per ray key
    // the steps and rays the training rounds added and the class made of them.
    // Cleared by every update that touches shapes or meshes; kept across
    // Resets, frames and renderers (a function of the geometry).
    ptrt::dbuf<uint32_t> len_sum, len_cnt;
    ptrt::dbuf<uint8_t> len_cls;
    pt_raykey_bounds len_bounds{};
    bool len_trained = false;    // a finalize has written len_cls since the last clear
    bool len_pending = false;    // training rounds ran since the last finalize
    uint64_t len_rounds = 0;     // LENGTH rounds issued since the last clear (the training schedule's clock)
    ptrt::dbuf<uint32_t> visibility_spill;   // ptRenderAmbientOcclusion's spill rows (deep scenes only; grown on demand)
    bool valid = false;
};

struct pt_sample_buffer {
    pt_device* dev = nullptr;
    uint32_t width = 0, height = 0;
    float4* accum = nullptr;
    ptrt::dbuf<float4> display;      // resolved image (ptRenderSampleBuffer)
    ptrt::dbuf<uint32_t> display8;   // its sRGB8 encoding
    bool resolved = false;
    uint32_t rank = 0, nranks = 1;   // pixel bands of the last partitioned renderer created on it
};

struct pt_preview {
    pt_device* dev = nullptr;
    pt_scene* scene = nullptr;           // non-owning (preview_render.hpp:20)
    uint32_t width = 0, height = 0;
    ptrt::dbuf<float4> image;
    ptrt::dbuf<pt_preview_aov> aov;
    ptrt::dbuf<uint32_t> spill;
    ptrt::dbuf<float> observe;           // ObserveUnderD65's per-sample constants (preview.hip)
    ptrt::dbuf<uint32_t> query;          // the picked shape's index (ptRetrievePreviewQueryResult)
    bool rendered = false;
};

struct pt_denoise_guides {
    pt_device* dev = nullptr;
    uint32_t width = 0, height = 0;
    ptrt::dbuf<float4> records;          // 2 float4 per pixel: a pt_denoise_guide
    ptrt::dbuf<float4> scratch;          // the filter's second image (Iterations >= 2; the pair filter: >= 1)
    ptrt::dbuf<uint32_t> spill;
    ptrt::dbuf<float> observe;           // ObserveUnderD65's per-sample constants (base_color.hpp)
    uint32_t variant = PT_DENOISE_VARIANT_AUTO;
};

struct pt_basic_renderer {
    pt_basic_renderer_params params{};
    pt_device* dev = nullptr;
    pt_scene* scene = nullptr;          // non-owning (basic.hpp:8,21)
    pt_sample_buffer* buffer = nullptr; // non-owning
    uint32_t rank = 0, nranks = 1;
    uint32_t tiles_x = 0;
    ptd::dslots slots{};
    ptrt::dbuf<float4> ray, hit, thr, prob;
    ptrt::dbuf<float> prob1;            // grey record form's Probability (path.hpp StorePathVertex)
    bool grey = false;                  // the live paths are in the grey record form (slots.prob1 set)
    bool grey_blocked = false;          // some live path cannot take it (until the next Reset / state write)
    ptrt::dbuf<uint32_t> grey_count;    // pt_launch_grey_check's result word
    ptrt::dbuf<uint32_t> cq_counts, cq_list;  // class-pure shade lists (ClassLists)
    uint32_t cq_parity[PT_MAX_SPLIT + 1] = {};   // per counter region (NextClassLists)
    uint32_t class_lists = 0;           // ptSetBasicRendererClassLists: 0 automatic, 1 off
    ptrt::dbuf<float> lam;              // lambda0 per slot (Sample is 0 between rounds)
    ptrt::dbuf<float2> uv;
    ptrt::dbuf<uint2> act;
    ptrt::dbuf<uint16_t> pos;           // TileOrder positions (path.hpp)
    ptrt::dbuf<uint8_t> slotof;         // position -> slot within the tile
    ptrt::dbuf<uint64_t> outcome;       // ShadeOrder: outcome-class bits per tile (extend -> shade)
    ptrt::dbuf<uint32_t> tilecost, order;     // longest-first tile order (extend -> tile_order -> extend)
    uint64_t order_tick = 0;            // rounds since creation (tile-order re-sort period)
    ptrt::dbuf<uint32_t> done;          // per wave: completed paths since the last Reset (ptGetStats)
    int fused = 1;                      // fused rounds mode (ptSetBasicRendererFusedRounds)
    int openpbr = 0;                    // shade OpenPBR materials (ptSetBasicRendererOpenPBR)
    uint32_t round_batch = 0;           // rounds per launch of consecutive Run(1) rounds (0: automatic)
    uint32_t split = 0;                 // tile groups of consecutive rounds (ptSetBasicRendererSplit): 0 auto, 1 off
    ptrt::dbuf<uint32_t> guard;         // guarded rounds' {stop, rounds run} (ptRenderFrame)
    uint32_t order_groups = 1;          // the group structure the order array holds (tile_order_kernel)
    // Block map (ptSetBasicRendererBlockMap; include/pt_blockmap.h).  While
    // the order array's groups own whole runs (order_granule 4), `units`
    // holds the dispatch order of extend's (run, quarter) units in the same
    // group segments; under granule 1 it is not kept.
    uint32_t block_map = PT_BLOCK_MAP_AUTO;
    uint32_t order_granule = PT_BLOCK_MAP_TILE_GRANULE;
    ptrt::dbuf<uint32_t> units;
    // Active tile set (ptSetBasicRendererActiveTiles): one byte per tile, empty
    // = every tile.  While set, each group's segment of the order array holds
    // the group's active tiles first, in natural order (WriteOrder), and the
    // rounds' launches cover only those.
    std::vector<uint8_t> mask;
    uint32_t active_tiles = 0;          // tiles set in mask
    uint64_t active_slots = 0;          // their valid slots: the paths of one masked round
    uint32_t group_active[PT_MAX_SPLIT] = {};   // active tiles of each of the order_groups groups
    uint64_t pixels = 0;                // image pixels owned
    uint32_t streams = 1;               // path streams per owned pixel (ptCreateBasicRendererStreams)
    uint32_t stream_tiles = 0;          // tiles per stream
    uint64_t valid_slots = 0;           // streams x pixels: the paths of one round
    ptrt::dbuf<float4> accx;            // streams > 1: each stream's accumulator (streams x width x height)
    uint64_t rays = 0;                  // rays traced since the last Reset
    ptrt::dbuf<uint32_t> spill;
    uint32_t ray_order = PT_RAY_ORDER_AUTO;   // ptSetBasicRendererRayOrder
    ptrt::dbuf<uint16_t> len_cam;       // LENGTH order: camera rays per tile (path.hpp TileOrderLengthKey)
    bool len_cam_stale = true;          // len_cam does not describe the rays in place: zero it before a training round
};

struct pt_comm {
    pt_device* dev = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    double timeout_s = 600.0;     // ptCommSetTimeout
    bool aborted = false;
    int* flag = nullptr;          // device word of the collective argument check (CommAgree)
    int* host_flag = nullptr;     // its pinned host copy: the readback stays an asynchronous copy
                                  // that DeviceWait polls, and outlives a wait that times out
};

namespace ptrt __attribute__((visibility("hidden"))) {

// --- rt_device.hip: the device wait and launch timing ------------------------------

// Aborts every communicator of the device (ncclCommAbort: RCCL stops their
// kernels) after a failed or overdue collective.
void AbortComms(pt_device* dev);

// Waits until the device stream is idle.  With no communicator: one
// hipStreamSynchronize.  With live communicators: polls the stream, each
// communicator's asynchronous error (ncclCommGetAsyncError) and the shortest
// communicator deadline; on an RCCL error or at the deadline every
// communicator is aborted and PT_ERROR_COMM_ABORTED / PT_ERROR_TIMEOUT
// returned.  After an abort, waits give up after 10 s (PT_ERROR_TIMEOUT).
int DeviceWait(pt_device* dev);

#define PT_WAIT(dev)                                    \
    do {                                                \
        if (int w_ = ptrt::DeviceWait(dev)) return w_;  \
    } while (0)

int BeginTimed(pt_device* dev, int kernel, event_pair& ep, bool sampled = true, uint32_t rounds = 1);
int EndTimed(pt_device* dev, event_pair& ep);

// One launch, timed whenever the device profiles (the render loop's launches,
// which are sampled and may cover several rounds, call the two halves).
#define PT_TIMED(dev, KERNEL, launch)                               \
    do {                                                            \
        ptrt::event_pair ep_{};                                     \
        if (int b_ = ptrt::BeginTimed(dev, KERNEL, ep_)) return b_; \
        PT_HIP(launch);                                             \
        if (int d_ = ptrt::EndTimed(dev, ep_)) return d_;           \
    } while (0)

int CollectTimes(pt_device* dev);

// The plain read-backs and writes: the device made current, one asynchronous
// copy on its stream, the wait for it.
inline int CopyAndWait(pt_device* d, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    PT_HIP(hipSetDevice(d->id));
    PT_HIP(hipMemcpyAsync(dst, src, bytes, kind, d->stream));
    PT_WAIT(d);
    return 0;
}
inline int ReadBack(pt_device* d, void* host, const void* device, size_t bytes)
{
    return CopyAndWait(d, host, device, bytes, hipMemcpyDeviceToHost);
}
inline int WriteThrough(pt_device* d, void* device, const void* host, size_t bytes)
{
    return CopyAndWait(d, device, host, bytes, hipMemcpyHostToDevice);
}

// --- the renderer: what its launches take ------------------------------------------

inline ptd::dframe Frame(pt_basic_renderer* r)
{
    ptd::dframe F;
    F.accum = r->buffer->accum;
    F.width = r->buffer->width;
    F.height = r->buffer->height;
    F.rank = r->rank;
    F.nranks = r->nranks;
    F.tiles_x = r->tiles_x;
    F.tiles_x_magic = r->tiles_x > 1 ? (uint32_t)(((1ull << 32) + r->tiles_x - 1) / r->tiles_x) : 0u;
    F.streams = r->streams;
    F.stream_tiles = r->stream_tiles;
    F.stream_magic = r->streams > 1 ? (uint32_t)(((1ull << 32) + r->stream_tiles - 1) / r->stream_tiles) : 0u;
    F.accx = r->accx.ptr;
    return F;
}

inline ptd::dparams Params(pt_basic_renderer* r, uint32_t seed)
{
    ptd::dparams P;
    P.camera_index = r->params.CameraIndex;
    P.render_flags = r->params.RenderFlags;
    P.termination_probability = r->params.PathTerminationProbability;
    P.seed = seed;
    return P;
}

inline bool Spills(const pt_basic_renderer* r) { return r->scene->stack_needed > pt_extend_stack_cap(); }

// Traversal stack entries beyond the kernel's LDS capacity live in a global
// buffer of (needed - capacity) rows x one column per ray.
inline int EnsureSpill(pt_basic_renderer* r)
{
    if (!Spills(r)) { r->slots.spill = nullptr; return 0; }
    size_t rows = r->scene->stack_needed - pt_extend_stack_cap();
    PT_HIP(r->spill.alloc(rows * (size_t)r->slots.n));
    r->slots.spill = r->spill.ptr;
    return 0;
}

inline int CheckReady(pt_basic_renderer* r)
{
    if (!r || !r->scene || !r->buffer) { SetError("renderer: null"); return -1; }
    if (!r->scene->valid) { SetError("renderer: scene has no valid packs (call ptUpdateScene)"); return -1; }
    if (r->params.CameraIndex >= r->scene->camera_count) {
        SetError("renderer: CameraIndex %u >= camera count %u", r->params.CameraIndex, r->scene->camera_count);
        return -1;
    }
    return 0;
}

// --- rt_rounds.hip: what rt_renderer.hip's Reset, state write and getters ask of the
// render loop.  Defined beside the per-round path that tests them every round.

uint32_t ShadeMats(const pt_basic_renderer* r);      // the material mask the renderer shades with
bool GreyForm(const pt_basic_renderer* r);           // live paths take the grey record form
bool ShadeCompact(const pt_basic_renderer* r);       // the shade kernel's completion queue is on
uint32_t SplitGroups(const pt_basic_renderer* r);    // tile groups of consecutive rounds
bool ClassListRounds(const pt_basic_renderer* r);    // rounds shade through class lists
bool LengthOrder(const pt_basic_renderer* r);        // rays are placed by predicted traversal length
bool RunMapPossible(const pt_basic_renderer* r);     // the RUN block map can run on the renderer's scene and ray order
bool RunMap(const pt_basic_renderer* r);             // the next rounds' extend launches take the RUN block map
uint32_t OrderGranule(const pt_basic_renderer* r);   // the granule tile groups own under the map in use (1 or 4)
int SyncRayOrder(pt_basic_renderer* r);              // sets the slots' ray order for the launches that follow

}  // namespace ptrt
