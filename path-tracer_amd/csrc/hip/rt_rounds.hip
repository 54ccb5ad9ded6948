// rt_rounds.hip — host side of libpathtracer.so: the render loop.  What decides a round's
// launches (shade mask, record form, fused rounds, tile groups, class lists, ray
// order, active tiles) and the one path every round is issued through.  The
// per-round functions stay in this file so that they inline into each other.
#include "runtime.hpp"

using namespace ptrt;

// Automatic mode's batch for a renderer whose tiles all fit on the GPU at
// once (RoundFused's condition): one launch per AUTO_BATCH rounds.
constexpr uint32_t AUTO_BATCH = 16;

// Rounds between two longest-first tile-order sorts (C3 / C5 / C2 at 4:
// +3.4 / +4.9 / -1.4 %, at 16: +3.9 / +5.3 / 0 % vs natural order; period 1
// C3 -2.4 %: DESIGN.md §4).
#ifndef PT_TILE_ORDER_PERIOD
#define PT_TILE_ORDER_PERIOD 16   // experiment builds may change it
#endif
constexpr uint32_t TILE_ORDER_PERIOD = PT_TILE_ORDER_PERIOD;

// Material mask the renderer shades with (shade / round instantiation): the
// scene's OpenPBR shapes, and the media they bring, join it only when OpenPBR
// shading is enabled (ptSetBasicRendererOpenPBR); otherwise their hits end
// the path as in the reference.
uint32_t ptrt::ShadeMats(const pt_basic_renderer* r)
{
    uint32_t m = r->scene->mats;
    if (!(m & PT_MATS_OPENPBR)) return m;
    if (!r->openpbr) return m & ~(uint32_t)PT_MATS_OPENPBR;
    return m | PT_MATS_SCATTER;
}

// Whether the live paths take the grey record form.  Decided on the shade
// instantiation's mask (pt_shade_mats), the same mask ShadeSlot tests as MATS:
// a scene mask without glass can still map to an instantiation that has it
// (diffuse + metal + fog -> PT_MATS_ALL), and that kernel reads the
// four-float record.
bool ptrt::GreyForm(const pt_basic_renderer* r) { return pt_grey_mats(pt_shade_mats(ShadeMats(r))); }

// The record form of the renderer's live paths (GreyRecord, path.hpp
// StorePathVertex): grey while the shade mask keeps every Probability
// wavelength-uniform and every active-shape stack empty.  A mask change
// between rounds (a scene update without Reset, ptSetBasicRendererOpenPBR)
// converts the live paths: to the four-float form always; to the grey form
// only if every live path satisfies its invariants (checked on the device:
// paths that crossed into a glass keep a non-empty stack), else the renderer
// stays in the four-float form until the next Reset or state write.
static int SyncRecordForm(pt_device* d, pt_basic_renderer* r)
{
    const bool want = GreyForm(r);
    if (want != r->grey && r->slots.n) {
        const ptd::dframe F = Frame(r);
        if (!want) {
            PT_HIP(pt_launch_grey_convert(r->slots, F, r->prob1.ptr, false, d->stream));
            r->grey = false;
        } else if (!r->grey_blocked) {
            PT_HIP(hipMemsetAsync(r->grey_count.ptr, 0, sizeof(uint32_t), d->stream));
            PT_HIP(pt_launch_grey_check(r->slots, F, r->grey_count.ptr, d->stream));
            PT_WAIT(d);
            uint32_t bad = 0;
            PT_HIP(hipMemcpy(&bad, r->grey_count.ptr, sizeof(bad), hipMemcpyDeviceToHost));
            if (bad == 0) {
                PT_HIP(pt_launch_grey_convert(r->slots, F, r->prob1.ptr, true, d->stream));
                r->grey = true;
            } else {
                r->grey_blocked = true;
            }
        }
    }
    r->slots.prob1 = r->grey ? r->prob1.ptr : nullptr;
    return 0;
}

// RunBasicRenderer (basic.cpp:306-332)
// Fused rounds (round_kernel) when every tile of the launch fits on the GPU
// at once -- a rank's share of a strongly scaled frame -- and the scene needs
// no spilled stack (renderer mode 1); mode 0 never fuses, mode 2 fuses
// whenever the kernel applies (tests and A/B).

// Completion queue of the shade kernel (shade.hpp ShadeTile): worth its
// barriers when paths also end at surfaces -- sky light sampling (a sample
// below the horizon ends the path), roulette, or metal / translucent /
// OpenPBR BSDFs (failed samples) -- so that completions are scattered over
// the hit waves.  Measured (profiles/r04_ab3): C2 shade -3.7 %, C5 -3.0 %;
// C3 (diffuse, no light sampling, no roulette: every completion is an escape,
// already grouped by ShadeOrder) +3 % with it, so it stays off there.
bool ptrt::ShadeCompact(const pt_basic_renderer* r)
{
    const uint32_t m = ShadeMats(r);
    return (m & (PT_MATS_METAL | PT_MATS_TRANSLUCENT | PT_MATS_OPENPBR)) != 0 ||
           r->scene->d.g.SkyboxSamplingProbability > 0.0f || r->params.PathTerminationProbability > 0.0f;
}

// Active tile set (ptSetBasicRendererActiveTiles).  The kernels of a round
// take their tile from order[blockIdx.x] and their grid from tile_count, so a
// round over a subset is a launch whose tile_count is the subset's size over
// an order array that lists the subset first: the view tile groups use.
static bool Masked(const pt_basic_renderer* r) { return !r->mask.empty(); }

// The paths one round traces.
static uint64_t RoundSlots(const pt_basic_renderer* r) { return Masked(r) ? r->active_slots : r->valid_slots; }

// The slots of a single-stream round: with a mask, the active tiles at the
// head of the order array (which must hold one group: EnsureOrderGroups(1)).
static ptd::dslots ActiveSlots(const pt_basic_renderer* r)
{
    ptd::dslots L = r->slots;
    if (Masked(r)) L.tile_count = r->active_tiles;
    return L;
}

static bool RoundFused(const pt_basic_renderer* r, const ptd::dslots& g)
{
    const int mode = r->fused;
    if (mode == 0 || g.spill || g.tile_count == 0) return false;
    uint32_t cap = pt_round_capacity(ShadeMats(r), r->scene->d.stack16 != 0, r->dev->cu_count);
    if (cap == 0) return false;
    return mode == 2 || g.tile_count <= cap;
}

// Class-list region of one tile group of K: classes x CQ_SUB sub-lists of
// the largest group's capacity (group g holds at most ceil(T / K) tiles).
static size_t ClassListStride(uint32_t tiles, uint32_t K)
{
    return (size_t)ptd::PT_OUTCOME_CLASSES * CQ_SUB * pt_classq_sub_capacity((tiles + K - 1) / K);
}

// Class-list buffers: the counters of PT_MAX_SPLIT tile groups (2 parities x
// classes x CQ_SUB each) plus those of single-stream rounds (region
// PT_MAX_SPLIT, kept zero by its own parity), allocated on first use and
// zeroed; the lists sized for the K groups in use (K regions of
// ClassListStride) or for a single-stream round over every tile, whichever
// is larger (about 20 B per slot), grown when K grows.  A growth waits for
// the device stream: the old lists may still be read by queued launches.
static int ClassListBuffers(pt_device* d, pt_basic_renderer* r, uint32_t K)
{
    const size_t nc = (size_t)ptd::PT_OUTCOME_CLASSES * CQ_SUB;
    const uint32_t T = r->slots.tile_count;
    if (!r->cq_counts.ptr) {
        // Zeroed on the device stream (the tile groups' streams fork from it):
        // the null stream is not ordered against these non-blocking streams.
        if (r->cq_counts.alloc((PT_MAX_SPLIT + 1) * 2 * nc) != hipSuccess ||
            hipMemsetAsync(r->cq_counts.ptr, 0, (PT_MAX_SPLIT + 1) * 2 * nc * sizeof(uint32_t), d->stream) != hipSuccess) {
            SetError("class list allocation failed");
            return -1;
        }
    }
    const size_t need = std::max(ClassListStride(T, 1), K * ClassListStride(T, K));
    if (need > r->cq_list.count) {
        if (r->cq_list.ptr) PT_WAIT(d);
        if (r->cq_list.alloc(need) != hipSuccess) {
            SetError("class list allocation failed");
            return -1;
        }
    }
    return 0;
}

// Tile groups on concurrent streams (ptSetBasicRendererSplit).  A batch of
// consecutive rounds over a whole frame ends each extend and shade launch
// with a tail of a few long blocks while most CUs idle.  Split into K groups
// of tiles (t = g, g + K, ...), each running its own sequence of rounds on
// its own stream, the launches of one group fill the CUs another group's
// tail leaves idle.  A slot's round depends only on its own previous round
// and the round's FrameIndex, so the results are those of the unsplit
// rounds, bit for bit.  Measured (bench.py A/B, profiles/r05_split,
// r05_splitk): K = 2 / 3 / 4 against 1 -- C3 +4.8 / +6.8 / -8 %, C2 +17 /
// +17 / -3 %, C5 +15 / +16 / -11 %, C4 +1.3 / +1.7 / -1 %; halving the
// launches on ONE stream costs 14-20 % (tools/exp_two_streams.py), so the
// gain is the overlap.  Four groups take every hardware queue of the
// process (GPU_MAX_HW_QUEUES = 4) and lose.
constexpr uint32_t SPLIT_MIN_TILES = 2048;   // automatic mode: whole frames (C2 has 4 096 tiles)
constexpr uint32_t SPLIT_AUTO_GROUPS = 3;

uint32_t ptrt::SplitGroups(const pt_basic_renderer* r)
{
    // The groups partition every tile of the renderer, masked or not (group
    // t % K); the automatic mode's rules look at the tiles a round launches.
    const ptd::dslots L = ActiveSlots(r);
    if (!L.order || r->slots.tile_count < 2 || r->split == 1) return 1;
    if (r->split >= 2) return std::min(r->split, r->slots.tile_count);
    return (!RoundFused(r, L) && L.tile_count >= SPLIT_MIN_TILES) ? SPLIT_AUTO_GROUPS : 1u;
}

// Class-pure shade inside tile groups (shade.hip shade_classq_kernel):
// scenes with more than one material type whose shade instantiation has a
// class-pure form.  In tile groups the lists' latency and the gathers' extra
// bytes overlap the other groups' launches (C2 +6 %, C5 +6 %); alone on one
// stream they cost more than the lanes gain, so single-stream rounds keep
// the tile-local shade.
static bool ClassLists(const pt_basic_renderer* r)
{
    // class_list_kernel derives a group's tiles arithmetically: off under a mask.
    return r->class_lists != 1 && !Masked(r) && r->scene->d.mat_classes != 0 &&
           pt_class_lists_supported(ShadeMats(r));
}

// Rounds of this renderer shade through class lists (tile groups and
// single-stream rounds alike).
bool ptrt::ClassListRounds(const pt_basic_renderer* r) { return SplitGroups(r) > 1 && ClassLists(r); }

// --- ray order (ptSetBasicRendererRayOrder; DESIGN.md §4 "Length classes") ------
// LENGTH places a tile's new rays by the traversal length their key's class
// predicts (path.hpp TileOrderLengthKey), from the scene's table.  It runs
// where extend has a training instantiation (the mesh-only loop, no spilled
// stack) and the tile shade a LENGTH one; elsewhere the renderer keeps OCTANT
// and reports it.  The fused round kernels and the class-list shade place
// rays as before: class lists never meet LENGTH (their masks differ), and a
// fused round leaves the camera counts stale (len_cam_stale).
//
// Training schedule, counted in the LENGTH rounds issued on the scene since
// its table was cleared: the first LEN_TRAIN_FIRST rounds and every
// LEN_TRAIN_PERIOD-th after them run the training extend; guarded rounds and
// fused rounds never train.  A finalize follows the training rounds of a call
// on the device stream, once every tile group has joined, so the classes
// change only between calls and every run of the same calls sees the same
// classes in the same rounds.  A batch of tile-group rounds that holds the
// first training rounds is cut after them, so that its other rounds already
// use the classes.
constexpr uint64_t LEN_TRAIN_FIRST = 16, LEN_TRAIN_PERIOD = 64;

static bool LengthSupported(const pt_basic_renderer* r)
{
    return pt_length_train_supported(r->scene->d, Spills(r)) && pt_length_order_supported(ShadeMats(r));
}

// AUTO: LENGTH wherever it is supported -- the unfused tile shade of diffuse
// one-mesh scenes (C3, C4), where it measured faster.
bool ptrt::LengthOrder(const pt_basic_renderer* r)
{
    return r->ray_order != PT_RAY_ORDER_OCTANT && LengthSupported(r);
}

// --- block map (ptSetBasicRendererBlockMap; DESIGN.md §4 "Block map") -----------
// RUN gives each extend block one quarter of four neighbouring tiles, which
// under LENGTH order are four waves of one predicted length: the block no
// longer holds three empty wave slots and its LDS while one long wave ends.
// It runs where LENGTH order does and extend has the instantiation, in rounds
// issued as separate launches over every tile: fused rounds and round batches
// trace a tile per block, and an active tile set breaks runs.  Tile groups
// then own whole runs (OrderGranule), so that a run's tiles stay neighbours.
bool ptrt::RunMapPossible(const pt_basic_renderer* r)
{
    return LengthOrder(r) && pt_block_map_run_supported(r->scene->d, Spills(r));
}

// AUTO: RUN wherever it runs (C3 +2.2 %, C4 +4.9 %: DESIGN.md §4 "Block map").
bool ptrt::RunMap(const pt_basic_renderer* r)
{
    return r->block_map != PT_BLOCK_MAP_TILE && RunMapPossible(r) && !Masked(r) && r->round_batch < 2 &&
           !RoundFused(r, ActiveSlots(r));
}

uint32_t ptrt::OrderGranule(const pt_basic_renderer* r)
{
    return RunMap(r) ? PT_BLOCK_MAP_RUN_GRANULE : PT_BLOCK_MAP_TILE_GRANULE;
}

// The order of the launches that follow, in the renderer's slots (every
// round's view is cut from them).
int ptrt::SyncRayOrder(pt_basic_renderer* r)
{
    ptd::dslots& L = r->slots;
    if (!LengthOrder(r)) {
        if (L.len_order) r->len_cam_stale = true;
        L.len_order = 0;
        L.len_cls = nullptr;
        L.len_cam = nullptr;
        L.len_sum = L.len_cnt = nullptr;
        return 0;
    }
    pt_scene* s = r->scene;
    if (!r->len_cam.ptr) {
        PT_HIP(r->len_cam.alloc((size_t)L.tile_count + 1));
        r->len_cam_stale = true;
    }
    if (!L.len_order) r->len_cam_stale = true;
    L.len_order = 1;
    L.len_cls = s->len_trained ? s->len_cls.ptr : nullptr;
    L.len_cam = r->len_cam.ptr;
    L.len_sum = s->len_sum.ptr;
    L.len_cnt = s->len_cnt.ptr;
    L.len_bounds = s->len_bounds;
    return 0;
}

// Whether the next LENGTH round trains (and counts it).
static bool LengthTrainRound(pt_basic_renderer* r)
{
    if (!r->slots.len_order) return false;
    pt_scene* s = r->scene;
    const uint64_t t = s->len_rounds++;
    const bool train = t < LEN_TRAIN_FIRST || t % LEN_TRAIN_PERIOD == 0;
    if (train) s->len_pending = true;
    return train;
}

// After a call's rounds, on the device stream (the tile groups joined).
static int LengthFinalize(pt_device* d, pt_basic_renderer* r)
{
    pt_scene* s = r->scene;
    if (!r->slots.len_order || !s->len_pending) return 0;
    PT_HIP(pt_launch_length_classes(s->len_sum.ptr, s->len_cnt.ptr, s->len_cls.ptr, d->stream));
    s->len_pending = false;
    s->len_trained = true;
    return SyncRayOrder(r);
}

// Rewrites the dispatch order for K groups of tiles (granule 1) or of runs
// (granule 4: the RUN block map, never with an active tile set), each group's
// tiles in its own segment in natural order and, for granule 4, its units in
// theirs; with an active tile set, a segment's active tiles first
// (group_active of them), the inactive ones behind.  Waits for the device
// first: queued launches may still read the arrays.
static int WriteOrder(pt_device* d, pt_basic_renderer* r, uint32_t K, uint32_t granule)
{
    if (!r->slots.order) return 0;
    const uint32_t T = r->slots.tile_count;
    std::vector<uint32_t> order(T), units;
    uint32_t i = 0;
    for (uint32_t g = 0; g < PT_MAX_SPLIT; g++) r->group_active[g] = 0;
    for (uint32_t g = 0; g < K; g++) {
        const uint32_t n = pt_group_tile_count(T, K, g, granule);
        for (uint32_t pass = 0; pass < (Masked(r) ? 2u : 1u); pass++) {
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t t = pt_group_tile(K, g, j, granule);
                if (Masked(r) && (r->mask[t] != 0) != (pass == 0)) continue;
                order[i++] = t;
                if (Masked(r) && pass == 0) r->group_active[g]++;
            }
        }
        if (granule == PT_BLOCK_MAP_RUN_GRANULE)
            for (uint32_t j = 0; j < pt_group_unit_count(T, K, g, granule); j++)
                units.push_back(pt_group_unit(K, g, j, granule));
    }
    PT_WAIT(d);
    PT_HIP(hipMemcpy(r->order.ptr, order.data(), (size_t)T * 4, hipMemcpyHostToDevice));
    if (!units.empty()) PT_HIP(hipMemcpy(r->units.ptr, units.data(), units.size() * 4, hipMemcpyHostToDevice));
    r->order_groups = K;
    r->order_granule = granule;
    return 0;
}

// The dispatch order holds each group's tiles in its own segment; a change of
// K or of the granule restarts it from the natural order of each group.  A
// single-stream round over every tile runs on any group structure (its
// launches cover the whole arrays), but needs the granule of its block map.
static int EnsureOrderGroups(pt_device* d, pt_basic_renderer* r, uint32_t K, uint32_t granule)
{
    if (!r->slots.order) return 0;
    const bool grouped = K > 1 || Masked(r);
    if (r->order_granule == granule && (!grouped || r->order_groups == K)) return 0;
    return WriteOrder(d, r, grouped ? K : r->order_groups, granule);
}

static int EnsureGroupStreams(pt_device* d, uint32_t K)
{
    if (!d->fork_event) PT_HIP(hipEventCreateWithFlags(&d->fork_event, hipEventDisableTiming));
    for (uint32_t g = 0; g + 1 < K; g++) {
        if (!d->group_stream[g]) PT_HIP(hipStreamCreateWithFlags(&d->group_stream[g], hipStreamNonBlocking));
        if (!d->join_event[g]) PT_HIP(hipEventCreateWithFlags(&d->join_event[g], hipEventDisableTiming));
    }
    return 0;
}

// --- the render loop ------------------------------------------------------------
// Every entry point (ptRunBasicRenderer, ptRunBasicRendererRounds,
// ptRenderFrame) issues its rounds through the functions below: BeginRounds
// once per call, then IssueRound per round and view (single-stream rounds,
// the tile groups of SplitRounds, RunGuardedRounds) or IssueBatch per launch
// of the rounds kernel.

// The class-list counters and list of one round.
struct class_lists { uint32_t *counts, *next_counts, *list; };

// Class-list counter regions: g of the K > 1 tile groups a batch runs in, or
// the single-stream region PT_MAX_SPLIT (K = 1: the renderer's rounds outside
// tile groups -- Run(2), single rounds, guarded rounds).  A round takes its
// region's counters of the current parity (zero at the launch), clears the
// other parity's for the next round, and flips the parity.
static int NextClassLists(pt_device* d, pt_basic_renderer* r, uint32_t K, uint32_t g, class_lists& q)
{
    if (int e = ClassListBuffers(d, r, K)) return e;
    const size_t nc = (size_t)ptd::PT_OUTCOME_CLASSES * CQ_SUB;
    const uint32_t region = K > 1 ? g : PT_MAX_SPLIT;
    uint32_t* cnt = r->cq_counts.ptr + region * 2 * nc;
    uint32_t& parity = r->cq_parity[region];
    q.counts = cnt + nc * parity;
    q.next_counts = cnt + nc * (parity ^ 1u);
    q.list = r->cq_list.ptr + (K > 1 ? g * ClassListStride(r->slots.tile_count, K) : 0);
    parity ^= 1u;
    return 0;
}

// A batch in K tile groups starts from zeroed group counters at parity 0
// (the single-stream region keeps itself zero by its own parity).
static int ResetGroupLists(pt_device* d, pt_basic_renderer* r, uint32_t K)
{
    if (int e = ClassListBuffers(d, r, K)) return e;
    PT_HIP(hipMemsetAsync(r->cq_counts.ptr, 0, PT_MAX_SPLIT * 2 * ptd::PT_OUTCOME_CLASSES * CQ_SUB * sizeof(uint32_t),
                          d->stream));
    for (uint32_t g = 0; g < PT_MAX_SPLIT; g++) r->cq_parity[g] = 0;
    return 0;
}

// What the rounds of one call share.
struct round_setup {
    bool idle;          // an active tile set without a tile: nothing to launch
    ptd::dframe F;
    uint32_t mats;      // ShadeMats
    bool compact;       // ShadeCompact
    bool fused;         // a round is one round_kernel launch (single-stream rounds only)
    bool lists;         // an unfused round shades through class lists
    bool run;           // an unfused round's extend takes the RUN block map (RunMap)
};

// Before the rounds of a call that run in K tile groups (1: on the device
// stream alone): the device, the spill buffer, the live paths' record form,
// the order array's group structure (a single-stream round needs one group
// only under a mask: its launches then cover the head of the array) and the
// groups' streams.  A masked renderer without an active tile launches
// nothing: the call still takes its `seeds` seeds.
static int BeginRounds(pt_device* d, pt_basic_renderer* r, uint32_t K, uint64_t seeds, round_setup& S)
{
    S = {};
    PT_HIP(hipSetDevice(d->id));
    S.idle = Masked(r) && r->active_tiles == 0;
    if (S.idle) {
        r->params.FrameIndex += (uint32_t)seeds;
        return 0;
    }
    if (r->block_map == PT_BLOCK_MAP_RUN && !RunMapPossible(r)) {
        SetError("renderer: the RUN block map does not run on this scene and ray order (ptSetBasicRendererBlockMap)");
        return -1;
    }
    if (int e = EnsureSpill(r)) return e;
    if (int e = SyncRecordForm(d, r)) return e;
    S.run = RunMap(r);
    if (int e = EnsureOrderGroups(d, r, K, OrderGranule(r))) return e;
    if (K > 1)
        if (int e = EnsureGroupStreams(d, K)) return e;
    S.F = Frame(r);
    S.mats = ShadeMats(r);
    S.compact = ShadeCompact(r);
    S.fused = K == 1 && RoundFused(r, ActiveSlots(r));
    // A renderer whose tile groups use the lists takes them for every round:
    // a tile-local shade's TileOrder would leave the slots permuted within
    // their tiles against the positions, and the class lists' gathers by slot
    // lose their coherence (C2 -4 % measured, profiles/r05_exp2).
    S.lists = !S.fused && ClassLists(r) && (K > 1 || SplitGroups(r) > 1);
    // Ray order of the call's launches.  Camera counts that do not describe
    // the rays in place (a change of order, fused rounds in between) are
    // zeroed before a round may train: it then trains every ray once.
    if (int e = SyncRayOrder(r)) return e;
    if (r->slots.len_order && r->len_cam_stale && !S.fused) {
        PT_HIP(hipMemsetAsync(r->len_cam.ptr, 0, ((size_t)r->slots.tile_count + 1) * sizeof(uint16_t), d->stream));
        r->len_cam_stale = false;
    }
    return 0;
}

// What the next round does besides its launches: whether kernel timing
// samples it (every profile_period-th round) and whether the tile order is
// re-sorted after it -- tiles keep their relative cost for many rounds, so
// every TILE_ORDER_PERIOD rounds (one small launch per group); a masked
// renderer keeps the natural order (tile_order_kernel permutes whole
// segments).
struct round_tick { bool sampled, sort; };

static round_tick NextRound(const pt_device* d, const pt_basic_renderer* r)
{
    return {d->profiling && d->run_tick % d->profile_period == 0,
            r->slots.order && r->order_tick % TILE_ORDER_PERIOD == 0 && !Masked(r)};
}

// Host bookkeeping of n single rounds that ran, `seeds` of them with a seed
// of their own, each over `slots` paths.
static void RoundsDone(pt_device* d, pt_basic_renderer* r, uint32_t n, uint32_t seeds, uint64_t slots)
{
    r->params.FrameIndex += seeds;
    r->rays += slots * n;
    d->run_tick += n;
    if (r->slots.order) r->order_tick += n;
}

// Longest-first re-sort of the order array's groups g0 .. g1 - 1 on st (and
// of their units, when the groups own runs).
static int Resort(pt_basic_renderer* r, uint32_t g0, uint32_t g1, hipStream_t st)
{
    for (uint32_t g = g0; g < g1; g++)
        PT_HIP(pt_launch_tile_order(r->slots, st, r->order_groups, g, r->order_granule, r->units.ptr));
    return 0;
}

// One round's launches over the view L -- every tile, the active ones, group
// g of K, with or without a guard -- on st: the fused round, or extend and
// then the tile-local or the class-list shade.  timed: kernel timing takes
// the launches (those on the device stream of a sampled round).
static int IssueRound(pt_device* d, pt_basic_renderer* r, const round_setup& S, const ptd::dslots& L,
                      const ptd::dparams& P, hipStream_t st, bool timed, uint32_t K = 1, uint32_t g = 0,
                      bool train = false)
{
    event_pair ep{};
    if (S.fused) {
        if (int e = BeginTimed(d, PT_KERNEL_ROUND, ep, timed)) return e;
        PT_HIP(pt_launch_round(r->scene->d, L, S.F, P, S.mats, st));
        r->len_cam_stale = true;   // the fused shade places rays by octant
        return EndTimed(d, ep);
    }
    if (int e = BeginTimed(d, PT_KERNEL_EXTEND, ep, timed)) return e;
    if (S.run) {
        // The view's units: group g's segment of the unit order, or all of it.
        constexpr uint32_t G = PT_BLOCK_MAP_RUN_GRANULE;
        const uint32_t T = r->slots.tile_count;
        const uint32_t* units = r->units.ptr + (K > 1 ? pt_group_unit_start(T, K, g, G) : 0u);
        PT_HIP(pt_launch_extend(r->scene->d, L, S.F, L.spill, st, train, units,
                                K > 1 ? pt_group_unit_count(T, K, g, G) : pt_unit_count(T, G)));
    } else {
        PT_HIP(pt_launch_extend(r->scene->d, L, S.F, L.spill, st, train));
    }
    if (int e = EndTimed(d, ep)) return e;
    if (int e = BeginTimed(d, PT_KERNEL_SHADE, ep, timed)) return e;
    if (S.lists) {
        class_lists q;
        if (int e = NextClassLists(d, r, K, g, q)) return e;
        PT_HIP(pt_launch_shade_classq(r->scene->d, L, S.F, P, S.mats, S.compact, q.counts, q.next_counts, q.list, st,
                                      r->slots.tile_count, K, g));
    } else {
        PT_HIP(pt_launch_shade(r->scene->d, L, S.F, P, S.mats, S.compact, st));
    }
    return EndTimed(d, ep);
}

// One launch of the rounds kernel: n rounds over L, round i with the seed
// first_seed + i * seed_step.  The profiling period counts rounds: the batch
// is timed when one of its n rounds is a sampled one.  The batch's block
// times order the next batch (natural order under a mask).
static int IssueBatch(pt_device* d, pt_basic_renderer* r, const round_setup& S, const ptd::dslots& L,
                      uint32_t first_seed, uint32_t seed_step, uint32_t n)
{
    ptd::dparams P = Params(r, first_seed);
    P.rounds = n;
    P.seed_step = seed_step;
    const uint64_t t = d->run_tick % d->profile_period;
    const bool sampled = d->profiling && (t == 0 || t + n > d->profile_period);
    d->run_tick += n;
    event_pair ep{};
    if (int e = BeginTimed(d, PT_KERNEL_ROUNDS, ep, sampled, n)) return e;
    PT_HIP(pt_launch_rounds(r->scene->d, L, S.F, P, S.mats, d->stream));
    r->len_cam_stale = true;   // the fused shade places rays by octant
    if (int e = EndTimed(d, ep)) return e;
    if (!Masked(r))
        if (int e = Resort(r, 0, r->order_groups, d->stream)) return e;
    r->rays += RoundSlots(r) * n;
    return 0;
}

// Tile groups on concurrent streams: k consecutive rounds (FrameIndex + 1 ...
// + k) in K > 1 tile groups, after BeginRounds for K.  Group 0 runs on the
// device stream (its launches are the ones profiling times); the others wait
// for everything enqueued before (fork) and the device stream waits for them
// at the end (join), on every path out.  Group g's segment is re-sorted on
// group g's stream.
static int SplitRounds(pt_device* d, pt_basic_renderer* r, const round_setup& S, uint64_t k, uint32_t K)
{
    ptd::dslots G[PT_MAX_SPLIT];
    hipStream_t St[PT_MAX_SPLIT];
    for (uint32_t g = 0; g < K; g++) {
        G[g] = r->slots;
        G[g].order = r->slots.order + pt_group_tile_start(r->slots.tile_count, K, g, r->order_granule);
        G[g].tile_count = Masked(r) ? r->group_active[g] : pt_group_tile_count(r->slots.tile_count, K, g, r->order_granule);
        St[g] = g ? d->group_stream[g - 1] : d->stream;
    }
    if (S.lists)
        if (int e = ResetGroupLists(d, r, K)) return e;
    PT_HIP(hipEventRecord(d->fork_event, d->stream));
    for (uint32_t g = 1; g < K; g++) PT_HIP(hipStreamWaitEvent(St[g], d->fork_event, 0));
    auto rounds = [&]() -> int {
        for (uint64_t i = 0; i < k; i++) {
            const ptd::dparams P = Params(r, r->params.FrameIndex + 1);
            const round_tick tick = NextRound(d, r);
            const bool train = LengthTrainRound(r);   // every group of the round, or none
            for (uint32_t g = 0; g < K; g++) {
                if (G[g].tile_count == 0) continue;   // a group without an active tile
                if (int e = IssueRound(d, r, S, G[g], P, St[g], g == 0 && tick.sampled, K, g, train)) return e;
                if (tick.sort)
                    if (int e = Resort(r, g, g + 1, St[g])) return e;
            }
            RoundsDone(d, r, 1, 1, RoundSlots(r));
        }
        return 0;
    };
    const int rc = rounds();
    for (uint32_t g = 1; g < K; g++) {
        PT_HIP(hipEventRecord(d->join_event[g - 1], St[g]));
        PT_HIP(hipStreamWaitEvent(d->stream, d->join_event[g - 1], 0));
    }
    return rc;
}

// k consecutive Run(1) calls: the same rounds with the same seeds (FrameIndex
// + 1 ... + k), as round batches (rounds_kernel) when the renderer allows
// them, else in tile groups (SplitGroups; two rounds or more), else one
// ptRunBasicRenderer(1) per round.  round_batch: 0 automatic (AUTO_BATCH
// rounds per launch when every tile fits on the GPU at once, where the
// per-round launches cost most: C1 256x256 round 0.0176 -> 0.0055 ms; whole
// frames that do not fit run slower batched -- C3 0.431 vs 0.47-0.53 ms per
// round, C2 -22 %: extend then runs at the shade kernel's occupancy and the
// block's waves wait at the round's barriers), 1 never, R >= 2 always R.
// A scene that needs a spilled stack takes no batches (pt_rounds_available).
static int RunRounds(pt_device* d, pt_basic_renderer* r, uint64_t k)
{
    if (!r || CheckReady(r) != 0) return -1;
    uint32_t B = r->round_batch;
    if (B == 0) B = RoundFused(r, ActiveSlots(r)) && r->fused == 1 ? AUTO_BATCH : 1u;
    const bool batches = B > 1 && !Spills(r);
    const uint32_t K = batches || k < 2 ? 1u : SplitGroups(r);
    round_setup S;
    if (int e = BeginRounds(d, r, K, k, S)) return e;
    if (S.idle) return 0;
    if (batches) {
        const ptd::dslots L = ActiveSlots(r);
        while (k > 0) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(k, B);
            if (int e = IssueBatch(d, r, S, L, r->params.FrameIndex + 1, 1, n)) return e;
            r->params.FrameIndex += n;
            k -= n;
        }
        return 0;
    }
    if (K > 1) {
        // LENGTH order: the table's first training rounds end in a finalize
        // of their own, so that the batch's other rounds run on its classes.
        while (k > 0) {
            uint64_t n = k;
            if (r->slots.len_order && r->scene->len_rounds < LEN_TRAIN_FIRST)
                n = std::min<uint64_t>(k, LEN_TRAIN_FIRST - r->scene->len_rounds);
            if (int e = SplitRounds(d, r, S, n, K)) return e;
            if (int e = LengthFinalize(d, r)) return e;
            k -= n;
        }
        return 0;
    }
    for (uint64_t i = 0; i < k; i++)
        if (int e = ptRunBasicRenderer(d, r, 1)) return e;
    return 0;
}

// n guarded Run(1) rounds (FrameIndex + 1 ... + n) on the device stream:
// each preceded by guard_kernel, the launches of a round past the target
// returning at once.  Untimed, no re-sort.  Returns the rounds that ran in
// *ran; the host's bookkeeping -- the seeds, the rays of every valid slot,
// the ticks and the class-list parity -- follows those rounds, not the n
// issued.  (Never masked: ptRenderFrame refuses an active tile set.)
static int RunGuardedRounds(pt_device* d, pt_basic_renderer* r, uint32_t n, uint64_t target, uint32_t* ran)
{
    round_setup S;
    if (int e = BeginRounds(d, r, 1, 0, S)) return e;
    if (!r->guard.ptr) PT_HIP(r->guard.alloc(2));
    PT_HIP(hipMemsetAsync(r->guard.ptr, 0, 2 * sizeof(uint32_t), d->stream));
    ptd::dslots L = r->slots;
    L.stop = r->guard.ptr;
    const uint32_t base = r->params.FrameIndex;
    uint32_t& parity = r->cq_parity[PT_MAX_SPLIT];
    const uint32_t parity0 = parity;
    for (uint32_t i = 0; i < n; i++) {
        PT_HIP(pt_launch_guard(r->done.ptr, r->slots.n / 64 + 1, target, r->guard.ptr, d->stream));
        if (int e = IssueRound(d, r, S, L, Params(r, base + i + 1), d->stream, false)) return e;
    }
    uint32_t flags[2] = {0, 0};
    PT_WAIT(d);
    PT_HIP(hipMemcpy(flags, r->guard.ptr, sizeof(flags), hipMemcpyDeviceToHost));
    *ran = flags[1];
    if (S.lists) parity = parity0 ^ (*ran & 1u);   // a skipped round left the class-list counters alone
    RoundsDone(d, r, *ran, *ran, r->valid_slots);
    return 0;
}

constexpr double GUARD_PREDICTED = 8.0;   // rounds left, by the last batch's rate, for the guarded end

extern "C" {

int ptRunBasicRenderer(pt_device* d, pt_basic_renderer* r, uint32_t rounds)
{
    if (!d) { SetError("null device"); return -1; }
    if (CheckReady(r) != 0) return -1;
    round_setup S;
    if (int e = BeginRounds(d, r, 1, 1, S)) return e;
    if (S.idle) return 0;
    r->params.FrameIndex += 1;   // the call's one seed, whatever its rounds
    const uint32_t seed = r->params.FrameIndex;
    const ptd::dslots L = ActiveSlots(r);
    // Run(R >= 2) of a renderer whose rounds fuse: the R rounds with the one
    // seed as batches of the rounds kernel (seed_step 0), one launch instead
    // of R -- the application's Run(2) after a restart.  (RunRounds batches
    // for an explicit round_batch without fused rounds too.)
    const uint32_t B = r->round_batch ? r->round_batch : (S.fused && r->fused == 1 ? AUTO_BATCH : 1u);
    if (S.fused && rounds >= 2 && B >= 2 && pt_rounds_available(L)) {
        for (uint32_t left = rounds; left > 0;) {
            const uint32_t n = std::min(left, B);
            if (int e = IssueBatch(d, r, S, L, seed, 0, n)) return e;
            left -= n;
        }
        return 0;
    }
    const ptd::dparams P = Params(r, seed);
    for (uint32_t i = 0; i < rounds; i++) {
        const round_tick tick = NextRound(d, r);
        const bool train = !S.fused && LengthTrainRound(r);
        if (int e = IssueRound(d, r, S, L, P, d->stream, tick.sampled, 1, 0, train)) return e;
        if (tick.sort)
            if (int e = Resort(r, 0, r->order_groups, d->stream)) return e;
        RoundsDone(d, r, 1, 0, RoundSlots(r));
    }
    return LengthFinalize(d, r);
}

int ptRunBasicRendererRounds(pt_device* d, pt_basic_renderer* r, uint32_t count)
{
    if (!d) { SetError("null device"); return -1; }
    if (CheckReady(r) != 0) return -1;
    return RunRounds(d, r, count);
}

// Active tile set.  Setting or clearing it waits for the device and rewrites
// the order array for the current group structure (WriteOrder).
int ptSetBasicRendererActiveTiles(pt_device* d, pt_basic_renderer* r, const uint8_t* mask, uint32_t tiles)
{
    if (!d || !r) { SetError("ptSetBasicRendererActiveTiles: null argument"); return -1; }
    if (r->dev != d) { SetError("ptSetBasicRendererActiveTiles: renderer of another device"); return -1; }
    if (r->nranks != 1 || r->streams != 1) {
        SetError("ptSetBasicRendererActiveTiles: partitioned and multi-stream renderers take no active tile set");
        return -1;
    }
    if (!mask && tiles != 0) { SetError("ptSetBasicRendererActiveTiles: null mask with %u tiles", tiles); return -1; }
    if (mask && tiles != r->slots.tile_count) {
        SetError("ptSetBasicRendererActiveTiles: %u tiles given, the renderer has %u", tiles, r->slots.tile_count);
        return -1;
    }
    if (!mask && !Masked(r)) return 0;
    PT_HIP(hipSetDevice(d->id));
    std::vector<uint8_t> previous;
    const uint32_t previous_tiles = r->active_tiles;
    const uint64_t previous_slots = r->active_slots;
    previous.swap(r->mask);
    r->active_tiles = 0;
    r->active_slots = 0;
    if (mask && tiles) {
        r->mask.assign(mask, mask + tiles);
        const uint32_t w = r->buffer->width, h = r->buffer->height;
        for (uint32_t t = 0; t < tiles; t++) {
            if (!mask[t]) continue;
            const uint32_t ty = t / r->tiles_x, tx = t - ty * r->tiles_x;
            r->active_tiles++;
            r->active_slots += (uint64_t)std::min(16u, w - tx * 16u) * std::min(16u, h - ty * 16u);
        }
    }
    // Groups of tiles: the RUN block map is off while a set is in place, and
    // the next unmasked round restores its runs (EnsureOrderGroups).
    if (int e = WriteOrder(d, r, r->order_groups, PT_BLOCK_MAP_TILE_GRANULE)) {
        // The order array is as it was: so is the set.
        r->mask.swap(previous);
        r->active_tiles = previous_tiles;
        r->active_slots = previous_slots;
        return e;
    }
    return 0;
}

int ptGetBasicRendererActiveTiles(const pt_basic_renderer* r, uint32_t* active, uint32_t* tiles)
{
    if (!r) { SetError("ptGetBasicRendererActiveTiles: null renderer"); return -1; }
    if (active) *active = Masked(r) ? r->active_tiles : r->slots.tile_count;
    if (tiles) *tiles = r->slots.tile_count;
    return 0;
}

// Benchmark-mode frame: Reset, Run(2) as after a restart
// (application.cpp:109-110), then Run(1) rounds -- one new seed each, as the
// application's frame loop issues them (application.cpp:100-115,
// basic.cpp:306-332) -- until the paths completed since the Reset reach
// target_samples (the accumulator's alpha sum) or max_rounds rounds ran.
//
// The frame ends at the reference's round -- the first whose total reaches
// the target -- unconditionally.  A round completes at most one path per
// owned pixel (px), so with `remaining` paths to go the first
// ceil(remaining / px) - 1 rounds cannot reach the target: every batch of
// rounds enqueued without a look at the count is at most ceil(remaining /
// px) long, its last round the first that may reach it.  The count is read
// back between batches.  When the last batch's completion rate says at most
// GUARD_PREDICTED rounds are left, the rounds run guarded instead: a device
// check before each round returns the round's launches at once when the
// target is already reached (RunGuardedRounds), so a rate that changes can
// cost a read-back but never a round.  The guarded end starts with the
// rounds that cannot overshoot, batched, and guards only the rest.  The
// rate decides only how the rounds are issued, never how many run.
// Measured on the C3 1024-spp frame (tools/exp_frame_end.py,
// profiles/r06_frame_end): 16 batches, +1.7 ms (0.16 %) against the same
// 2 760 rounds in one call with no read-back.
int ptRenderFrame(pt_device* d, pt_basic_renderer* r, uint64_t target_samples, uint32_t max_rounds,
                  uint32_t* rounds_out, uint64_t* samples_out)
{
    if (!d || !r) { SetError("null argument"); return -1; }
    if (max_rounds < 2) { SetError("ptRenderFrame: max_rounds must be >= 2"); return -1; }
    if (Masked(r)) { SetError("ptRenderFrame: an active tile set is in place (ptSetBasicRendererActiveTiles)"); return -1; }
    if (int e = ptResetBasicRenderer(d, r)) return e;
    if (int e = ptRunBasicRenderer(d, r, 2)) return e;
    uint32_t rounds = 2;
    uint64_t samples = 0, prev = 0;
    uint32_t last_batch = 0;
    const uint64_t px = std::max<uint64_t>(r->valid_slots, 1);   // paths one round can complete
    // The two rounds of Run(2) complete at most 2 px paths: the first batch
    // needs no read-back.
    if (target_samples > 2 * px) {
        const uint64_t k = std::min<uint64_t>((target_samples - 2 * px + px - 1) / px, max_rounds - rounds);
        if (k >= 1) {
            if (int e = RunRounds(d, r, k)) return e;
            rounds += (uint32_t)k;
            last_batch = rounds;   // the rate below: completions since the Reset per round
        }
    }
    for (;;) {
        if (int e = ptGetStats(d, r, nullptr, &samples)) return e;
        if (samples >= target_samples || rounds >= max_rounds) break;
        const uint64_t remaining = target_samples - samples;
        if (last_batch > 0 && samples > prev) {
            const double rate = (double)(samples - prev) / last_batch;   // completions per round
            const double predicted = (double)remaining / rate;
            if (predicted <= GUARD_PREDICTED) {
                // The last few rounds, with one read-back after them: first
                // the rounds that cannot overshoot, as one batch (its last
                // round may reach the target), then guarded single rounds
                // for the rest the rate predicts -- each returns at once
                // when the target is already reached, so the frame still
                // ends at the first round that reaches it.
                const uint64_t ks = std::min<uint64_t>((remaining + px - 1) / px, max_rounds - rounds);
                if (int e = RunRounds(d, r, ks)) return e;
                rounds += (uint32_t)ks;
                const double left = std::max(predicted - (double)ks, 0.0);
                const uint32_t n = (uint32_t)std::min<uint64_t>((uint64_t)(1.25 * left) + 2, max_rounds - rounds);
                uint32_t ran = 0;
                if (n >= 1)
                    if (int e = RunGuardedRounds(d, r, n, target_samples, &ran)) return e;
                rounds += ran;
                prev = samples;
                last_batch = (uint32_t)ks + ran;
                continue;
            }
        }
        const uint64_t k = std::min<uint64_t>((remaining + px - 1) / px, max_rounds - rounds);   // cannot overshoot
        if (int e = RunRounds(d, r, k)) return e;
        rounds += (uint32_t)k;
        prev = samples;
        last_batch = (uint32_t)k;
    }
    if (rounds_out) *rounds_out = rounds;
    if (samples_out) *samples_out = samples;
    return 0;
}

}  // extern "C"
