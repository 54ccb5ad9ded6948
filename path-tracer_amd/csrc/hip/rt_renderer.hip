// rt_renderer.hip — host side of libpathtracer.so: the basic renderer's creation, Reset,
// settings, counters, and path-state save and restore.  Its rounds are issued by
// rt_rounds.hip, which also answers what the getters here report of them.
#include "runtime.hpp"

using namespace ptrt;

extern "C" {

pt_basic_renderer* ptCreateBasicRendererStreams(pt_device* d, pt_scene* s, pt_sample_buffer* b, uint32_t rank,
                                                uint32_t nranks, uint32_t streams)
{
    if (!d || !s || !b) { SetError("null argument"); return nullptr; }
    if (nranks == 0 || rank >= nranks) { SetError("bad partition %u/%u", rank, nranks); return nullptr; }
    if (streams == 0 || streams > 256) { SetError("bad stream count %u (1..256)", streams); return nullptr; }
    if (hipSetDevice(d->id) != hipSuccess) { SetError("hipSetDevice failed"); return nullptr; }
    pt_basic_renderer* r = new pt_basic_renderer;
    r->dev = d;
    r->scene = s;
    r->buffer = b;
    r->rank = rank;
    r->nranks = nranks;
    r->tiles_x = (b->width + 15) / 16;
    uint32_t bands = (b->height + 15) / 16;
    uint32_t owned = bands > rank ? (bands - rank + nranks - 1) / nranks : 0;
    const uint64_t T = (uint64_t)owned * r->tiles_x;   // tiles per stream
    uint64_t n = T * streams * 256;
    // TileRow's and TileStream's reciprocal divisions are exact while every
    // tile index t has t * divisor < 2^32.
    if (T * r->tiles_x >= (1ull << 32) || (streams > 1 && T * T * streams >= (1ull << 32))) {
        SetError("frame too large");
        delete r;
        return nullptr;
    }
    if (n > 0xFFFFFFFFull / 2) { SetError("too many slots"); delete r; return nullptr; }
    uint32_t ns = (uint32_t)n;
    const size_t tiles = ns / 256, frame_px = (size_t)b->width * b->height;
    // Every array zeroed but the result word, and pos, slotof and order, which
    // get their identity contents below.
    bool ok = r->ray.alloc_zero(ns) == hipSuccess && r->hit.alloc_zero(ns) == hipSuccess &&
              r->thr.alloc_zero(ns) == hipSuccess && r->prob.alloc_zero(ns) == hipSuccess &&
              r->prob1.alloc_zero(ns) == hipSuccess && r->grey_count.alloc(1) == hipSuccess &&
              r->lam.alloc_zero(ns) == hipSuccess && r->uv.alloc_zero(ns) == hipSuccess &&
              r->act.alloc_zero(ns) == hipSuccess && r->pos.alloc(ns) == hipSuccess && r->slotof.alloc(ns) == hipSuccess &&
              r->outcome.alloc_zero(tiles * 4 * ptd::PT_OUTCOME_CLASSES + 1) == hipSuccess &&
              r->tilecost.alloc_zero(tiles * 4 + 1) == hipSuccess && r->order.alloc(tiles + 1) == hipSuccess &&
              r->units.alloc(pt_unit_count((uint32_t)tiles, PT_BLOCK_MAP_RUN_GRANULE) + 1) == hipSuccess &&
              r->done.alloc_zero(ns / 64 + 1) == hipSuccess &&
              (streams == 1 || r->accx.alloc_zero((size_t)streams * frame_px) == hipSuccess);
    if (ok && ns) {
        // Identity TileOrder until the first Reset sorts the rays.
        std::vector<uint16_t> pos(ns);
        std::vector<uint8_t> slotof(ns);
        for (uint32_t i = 0; i < ns; i++) { pos[i] = (uint16_t)(((i & 255u) << 8) | (i & 255u)); slotof[i] = (uint8_t)(i & 255u); }
        std::vector<uint32_t> order(tiles);
        for (uint32_t t = 0; t < tiles; t++) order[t] = t;   // natural order until a round is timed
        ok = hipMemcpy(r->pos.ptr, pos.data(), (size_t)ns * 2, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(r->slotof.ptr, slotof.data(), ns, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(r->order.ptr, order.data(), tiles * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        SetError("renderer slot allocation failed (%u slots)", ns);
        delete r;
        return nullptr;
    }
    r->streams = streams;
    r->stream_tiles = (uint32_t)T;
    r->slots.ray = r->ray.ptr;
    r->slots.hit = r->hit.ptr;
    r->slots.uv = r->uv.ptr;
    r->slots.thr = r->thr.ptr;
    r->slots.prob = r->prob.ptr;
    r->slots.lam = r->lam.ptr;
    r->slots.act = r->act.ptr;
    r->slots.pos = r->pos.ptr;
    r->slots.slotof = r->slotof.ptr;
    r->slots.outcome = r->outcome.ptr;
    r->slots.tilecost = r->tilecost.ptr;
    r->slots.order = ns ? r->order.ptr : nullptr;
    r->slots.done = r->done.ptr;
    r->slots.spill = nullptr;
    r->slots.n = ns;
    r->slots.tile_count = ns / 256;
    for (uint32_t band = rank; band < bands; band += nranks)
        r->pixels += (uint64_t)b->width * std::min<uint32_t>(16u, b->height - band * 16u);
    r->valid_slots = r->pixels * streams;
    b->rank = rank;
    b->nranks = nranks;
    return r;
}

pt_basic_renderer* ptCreateBasicRendererPartitioned(pt_device* d, pt_scene* s, pt_sample_buffer* b, uint32_t rank,
                                                    uint32_t nranks)
{
    return ptCreateBasicRendererStreams(d, s, b, rank, nranks, 1);
}

// The sample buffer's owned pixels := the streams' accumulators summed in
// stream order, ((A0 + A1) + A2) ...; the streams keep accumulating, so a
// later merge gives the new totals.
int ptMergeBasicRendererStreams(pt_device* d, pt_basic_renderer* r)
{
    if (!d || !r || !r->buffer) { SetError("null argument"); return -1; }
    if (r->streams == 1) return 0;
    PT_HIP(hipSetDevice(d->id));
    PT_HIP(pt_launch_merge_streams(r->buffer->accum, r->accx.ptr, r->buffer->width, r->buffer->height, r->rank,
                                   r->nranks, r->streams, d->stream));
    return 0;
}

uint32_t ptBasicRendererStreams(pt_basic_renderer* r) { return r ? r->streams : 0; }

pt_basic_renderer* ptCreateBasicRenderer(pt_device* d, pt_scene* s, pt_sample_buffer* b)
{
    return ptCreateBasicRendererPartitioned(d, s, b, 0, 1);
}

void ptDestroyBasicRenderer(pt_device* d, pt_basic_renderer* r)
{
    if (!r) return;
    if (d) { (void)hipSetDevice(d->id); (void)DeviceWait(d); }
    delete r;
}

pt_basic_renderer_params* ptBasicRendererParams(pt_basic_renderer* r) { return r ? &r->params : nullptr; }
uint32_t ptBasicRendererSlotCount(pt_basic_renderer* r) { return r ? r->slots.n : 0; }

// ResetBasicRenderer (basic.cpp:285-304)
int ptResetBasicRenderer(pt_device* d, pt_basic_renderer* r)
{
    if (!d) { SetError("null device"); return -1; }
    if (CheckReady(r) != 0) return -1;
    PT_HIP(hipSetDevice(d->id));
    // Every live path is replaced: the record form follows the shade mask.
    r->grey = GreyForm(r);
    r->grey_blocked = false;
    r->slots.prob1 = r->grey ? r->prob1.ptr : nullptr;
    // Raygen places every tile's rays in the renderer's order and, in LENGTH
    // order, writes every tile's camera count.
    if (int e = SyncRayOrder(r)) return e;
    r->len_cam_stale = false;
    PT_TIMED(d, PT_KERNEL_RAYGEN,
             pt_launch_raygen(r->scene->d, r->slots, Frame(r), Params(r, r->params.FrameIndex), d->stream));
    PT_HIP(hipMemsetAsync(r->done.ptr, 0, (size_t)(r->slots.n / 64 + 1) * 4, d->stream));
    r->rays = 0;
    return 0;
}

int ptSetBasicRendererRoundBatch(pt_basic_renderer* r, uint32_t rounds)
{
    if (!r) { SetError("ptSetBasicRendererRoundBatch: null renderer"); return -1; }
    r->round_batch = rounds;
    return 0;
}

int ptSetBasicRendererClassLists(pt_basic_renderer* r, uint32_t mode)
{
    if (!r || mode > 1) { SetError("ptSetBasicRendererClassLists: bad argument (0 automatic, 1 off)"); return -1; }
    r->class_lists = mode;
    return 0;
}

int ptGetBasicRendererClassLists(const pt_basic_renderer* r, uint32_t* used)
{
    if (!r || !used) { SetError("ptGetBasicRendererClassLists: null argument"); return -1; }
    *used = ClassListRounds(r) ? 1u : 0u;
    return 0;
}

int ptSetBasicRendererRayOrder(pt_basic_renderer* r, uint32_t order)
{
    if (!r || order > PT_RAY_ORDER_LENGTH) {
        SetError("ptSetBasicRendererRayOrder: bad argument (0 automatic, 1 octant, 2 length)");
        return -1;
    }
    r->ray_order = order;
    return 0;
}

int ptGetBasicRendererRayOrder(const pt_basic_renderer* r, uint32_t* order, uint32_t* used)
{
    if (!r) { SetError("ptGetBasicRendererRayOrder: null renderer"); return -1; }
    if (used && (!r->scene || !r->scene->valid)) {
        SetError("renderer: scene has no valid packs (call ptUpdateScene)");
        return -1;
    }
    if (order) *order = r->ray_order;
    if (used) *used = LengthOrder(r) ? PT_RAY_ORDER_LENGTH : PT_RAY_ORDER_OCTANT;
    return 0;
}

int ptSetBasicRendererBlockMap(pt_basic_renderer* r, uint32_t map)
{
    if (!r || map > PT_BLOCK_MAP_RUN) {
        SetError("ptSetBasicRendererBlockMap: bad argument (0 automatic, 1 tile, 2 run)");
        return -1;
    }
    if (map == PT_BLOCK_MAP_RUN && r->scene && r->scene->valid && !RunMapPossible(r)) {
        SetError("ptSetBasicRendererBlockMap: the RUN block map runs where ray order LENGTH does "
                 "(a one-mesh diffuse scene without a spilled stack, ray order not OCTANT)");
        return -1;
    }
    r->block_map = map;
    return 0;
}

int ptGetBasicRendererBlockMap(const pt_basic_renderer* r, uint32_t* map, uint32_t* used)
{
    if (!r) { SetError("ptGetBasicRendererBlockMap: null renderer"); return -1; }
    if (used && (!r->scene || !r->scene->valid)) {
        SetError("renderer: scene has no valid packs (call ptUpdateScene)");
        return -1;
    }
    if (map) *map = r->block_map;
    if (used) *used = RunMap(r) ? PT_BLOCK_MAP_RUN : PT_BLOCK_MAP_TILE;
    return 0;
}

// The host's view of include/pt_blockmap.h (tests, tools).
static bool MapArgs(uint32_t groups, uint32_t granule)
{
    return groups != 0 && (granule == PT_BLOCK_MAP_TILE_GRANULE || granule == PT_BLOCK_MAP_RUN_GRANULE);
}
uint32_t ptBlockMapGroupTileCount(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    return MapArgs(groups, granule) ? pt_group_tile_count(tiles, groups, group, granule) : 0u;
}
uint32_t ptBlockMapGroupTile(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule, uint32_t i)
{
    return MapArgs(groups, granule) && i < pt_group_tile_count(tiles, groups, group, granule)
               ? pt_group_tile(groups, group, i, granule) : 0u;
}
uint32_t ptBlockMapGroupTileStart(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    return MapArgs(groups, granule) ? pt_group_tile_start(tiles, groups, std::min(group, groups), granule) : 0u;
}
uint32_t ptBlockMapGroupUnitCount(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    return MapArgs(groups, granule) ? pt_group_unit_count(tiles, groups, group, granule) : 0u;
}
uint32_t ptBlockMapGroupUnit(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule, uint32_t i)
{
    return MapArgs(groups, granule) && i < pt_group_unit_count(tiles, groups, group, granule)
               ? pt_group_unit(groups, group, i, granule) : 0u;
}
uint32_t ptBlockMapGroupUnitStart(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    return MapArgs(groups, granule) ? pt_group_unit_start(tiles, groups, std::min(group, groups), granule) : 0u;
}
uint32_t ptBlockMapUnitTile(uint32_t unit, uint32_t wave, uint32_t granule)
{
    return MapArgs(1, granule) && wave < 4 ? pt_unit_tile(unit, wave, granule) : 0u;
}
uint32_t ptBlockMapUnitQuarter(uint32_t unit, uint32_t wave, uint32_t granule)
{
    return MapArgs(1, granule) && wave < 4 ? pt_unit_quarter(unit, wave, granule) : 0u;
}

int ptReadBasicRendererRayPositions(pt_device* d, pt_basic_renderer* r, uint16_t* positions)
{
    if (!d || !r || !positions) { SetError("ptReadBasicRendererRayPositions: null argument"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    PT_WAIT(d);
    if (r->slots.n) PT_HIP(hipMemcpy(positions, r->pos.ptr, (size_t)r->slots.n * 2, hipMemcpyDeviceToHost));
    return 0;
}

int ptSetBasicRendererSplit(pt_basic_renderer* r, uint32_t groups)
{
    if (!r || groups > PT_MAX_SPLIT) {
        SetError("ptSetBasicRendererSplit: bad argument (groups 0..%u)", PT_MAX_SPLIT);
        return -1;
    }
    r->split = groups;
    return 0;
}

int ptGetBasicRendererSplit(const pt_basic_renderer* r, uint32_t* groups, uint32_t* timed_tiles, uint32_t* tiles)
{
    if (!r) { SetError("ptGetBasicRendererSplit: null renderer"); return -1; }
    const uint32_t K = SplitGroups(r);
    if (groups) *groups = K;
    if (timed_tiles) *timed_tiles = pt_group_tile_count(r->slots.tile_count, K, 0, K > 1 ? OrderGranule(r) : 1u);
    if (tiles) *tiles = r->slots.tile_count;
    return 0;
}

int ptSetBasicRendererFusedRounds(pt_basic_renderer* r, int mode)
{
    if (!r || mode < 0 || mode > 2) { SetError("ptSetBasicRendererFusedRounds: bad argument"); return -1; }
    r->fused = mode;
    return 0;
}

int ptSetBasicRendererOpenPBR(pt_basic_renderer* r, int enable)
{
    if (!r || enable < 0 || enable > 1) { SetError("ptSetBasicRendererOpenPBR: bad argument"); return -1; }
    r->openpbr = enable;
    return 0;
}

// Counters of the work done since the last Reset: rays traced (every owned
// pixel's slot traces one ray per round, K3) and paths completed (the
// accumulator increments of basic_scatter.glsl:350-359, counted whether or
// not RENDER_FLAG_ACCUMULATE is set).  Synchronises the device stream.
int ptGetStats(pt_device* d, pt_basic_renderer* r, uint64_t* rays, uint64_t* samples)
{
    if (!d || !r) { SetError("null argument"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    PT_WAIT(d);
    if (rays) *rays = r->rays;
    if (samples) {
        std::vector<uint32_t> w(r->slots.n / 64 + 1);
        PT_HIP(hipMemcpy(w.data(), r->done.ptr, w.size() * 4, hipMemcpyDeviceToHost));
        uint64_t sum = 0;
        for (uint32_t v : w) sum += v;
        *samples = sum;
    }
    return 0;
}

int ptReadBasicRendererStreamState(pt_device* d, pt_basic_renderer* r, uint32_t stream, pt_pixel_state* out)
{
    if (!d || !r || !out) { SetError("null argument"); return -1; }
    if (stream >= r->streams) { SetError("stream %u >= the renderer's %u streams", stream, r->streams); return -1; }
    PT_HIP(hipSetDevice(d->id));
    PT_WAIT(d);
    uint32_t n = r->slots.n;
    std::vector<float4> ray(n), hit(n), thr(n), prob(n);
    std::vector<float> lam(n);
    std::vector<float2> uv(n);
    std::vector<uint2> act(n);
    std::vector<uint16_t> pos(n);
    if (n && r->scene->valid) {
        // The slots hold compact hits; rebuild the reference's packed trace
        // records (normal, tangent, uv, material) for the readback.
        dbuf<float4> rec;
        dbuf<float2> ruv;
        PT_HIP(rec.alloc(n));
        PT_HIP(ruv.alloc(n));
        PT_HIP(pt_launch_finalize(r->scene->d, n, r->hit.ptr, r->uv.ptr, rec.ptr, ruv.ptr, d->stream));
        PT_HIP(hipStreamSynchronize(d->stream));
        PT_HIP(hipMemcpy(hit.data(), rec.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
        PT_HIP(hipMemcpy(uv.data(), ruv.ptr, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    PT_HIP(hipMemcpy(ray.data(), r->ray.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(thr.data(), r->thr.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (r->grey) {
        // Grey record form: the one stored Probability is all four components.
        std::vector<float> p1(n);
        PT_HIP(hipMemcpy(p1.data(), r->prob1.ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) prob[i] = make_float4(p1[i], p1[i], p1[i], p1[i]);
    } else {
        PT_HIP(hipMemcpy(prob.data(), r->prob.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
    }
    PT_HIP(hipMemcpy(lam.data(), r->lam.ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(act.data(), r->act.ptr, (size_t)n * 8, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(pos.data(), r->pos.ptr, (size_t)n * 2, hipMemcpyDeviceToHost));
    uint32_t W = r->buffer->width, H = r->buffer->height;
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    const uint32_t s0 = stream * r->stream_tiles * 256, s1 = s0 + r->stream_tiles * 256;
    for (uint32_t s = s0; s < s1; s++) {
        uint32_t t = (s >> 8) - stream * r->stream_tiles, l = s & 255u, k = t / r->tiles_x, tx = t - k * r->tiles_x;
        uint32_t x = tx * 16 + (l & 15u), y = (r->rank + k * r->nranks) * 16 + (l >> 4);
        if (x >= W || y >= H) continue;
        pt_pixel_state& O = out[(size_t)y * W + x];
        // Ray and hit records live at the slot's TileOrder positions.
        uint32_t qr = (s & ~255u) | (pos[s] >> 8u), qh = (s & ~255u) | (pos[s] & 255u);
        O.origin[0] = ray[qr].x; O.origin[1] = ray[qr].y; O.origin[2] = ray[qr].z;
        O.packed_velocity = bits(ray[qr].w);
        O.hit.time = hit[qh].x;
        O.hit.shape_material = bits(hit[qh].y);
        O.hit.packed_normal = bits(hit[qh].z);
        O.hit.packed_tangent = bits(hit[qh].w);
        O.hit.u = uv[qh].x;
        O.hit.v = uv[qh].y;
        O.lambda0 = lam[s];
        O.throughput[0] = thr[s].x; O.throughput[1] = thr[s].y; O.throughput[2] = thr[s].z; O.throughput[3] = thr[s].w;
        O.probability[0] = prob[s].x; O.probability[1] = prob[s].y; O.probability[2] = prob[s].z; O.probability[3] = prob[s].w;
        O.sample[0] = O.sample[1] = O.sample[2] = 0.0f;   // StorePathVertex (path.hpp)
        O.active01 = act[s].x;
        O.active23 = act[s].y;
    }
    return 0;
}

int ptReadBasicRendererState(pt_device* d, pt_basic_renderer* r, pt_pixel_state* out)
{
    return ptReadBasicRendererStreamState(d, r, 0, out);
}

// Resume: the live path of every owned pixel of one stream from
// a saved pt_pixel_state (what ptReadBasicRendererStreamState returned between
// rounds).  Restored: the next ray (origin, packed velocity) and the path
// record (basic.glsl.inc:159-198: lambda0, throughput, probability, active
// stack).  Not restored: the trace record -- each round traces before it
// scatters (basic_trace.glsl then basic_scatter.glsl), so the next Run's
// extend replaces it before anything reads it; until then the readback
// reports a miss.  Sample must be 0: a live path's Sample is 0 between rounds
// (StorePathVertex, path.hpp).  Checked before anything is written: every
// active-stack entry is 0xFFFF or a shape of the scene, lambda0 lies in
// [0, 1].
int ptWriteBasicRendererStreamState(pt_device* d, pt_basic_renderer* r, uint32_t stream, const pt_pixel_state* in)
{
    if (!d || !in) { SetError("null argument"); return -1; }
    if (CheckReady(r) != 0) return -1;
    if (stream >= r->streams) { SetError("stream %u >= the renderer's %u streams", stream, r->streams); return -1; }
    const uint32_t W = r->buffer->width, H = r->buffer->height;
    const uint32_t shapes = r->scene->d.g.ShapeCount;
    const uint32_t T = r->stream_tiles, s0 = stream * T * 256;
    std::vector<float4> ray((size_t)T * 256), thr((size_t)T * 256), prob((size_t)T * 256);
    std::vector<float> lam((size_t)T * 256);
    std::vector<uint2> act((size_t)T * 256);
    for (uint32_t i = 0; i < T * 256; i++) {
        const uint32_t t = i >> 8, l = i & 255u, k = t / r->tiles_x, tx = t - k * r->tiles_x;
        const uint32_t x = tx * 16 + (l & 15u), y = (r->rank + k * r->nranks) * 16 + (l >> 4);
        ray[i] = make_float4(0, 0, 0, 0);
        thr[i] = prob[i] = make_float4(0, 0, 0, 0);
        lam[i] = 0.0f;
        act[i] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (x >= W || y >= H) continue;
        const pt_pixel_state& S = in[(size_t)y * W + x];
        if (S.sample[0] != 0.0f || S.sample[1] != 0.0f || S.sample[2] != 0.0f) {
            SetError("pixel (%u, %u): a live path's sample is 0 between rounds", x, y);
            return -1;
        }
        if (!(S.lambda0 >= 0.0f && S.lambda0 <= 1.0f)) {   // R01() of basic_scatter.glsl:40 (can round to 1)
            SetError("pixel (%u, %u): lambda0 %g outside [0, 1]", x, y, (double)S.lambda0);
            return -1;
        }
        const uint32_t e[4] = {S.active01 & 0xFFFFu, S.active01 >> 16, S.active23 & 0xFFFFu, S.active23 >> 16};
        for (uint32_t v : e)
            if (v != 0xFFFFu && v >= shapes) {
                SetError("pixel (%u, %u): active shape %u >= the scene's %u shapes", x, y, v, shapes);
                return -1;
            }
        float w;
        std::memcpy(&w, &S.packed_velocity, 4);
        ray[i] = make_float4(S.origin[0], S.origin[1], S.origin[2], w);
        thr[i] = make_float4(S.throughput[0], S.throughput[1], S.throughput[2], S.throughput[3]);
        prob[i] = make_float4(S.probability[0], S.probability[1], S.probability[2], S.probability[3]);
        lam[i] = S.lambda0;
        act[i] = make_uint2(S.active01, S.active23);
    }
    PT_HIP(hipSetDevice(d->id));
    // The written records are four-float ones: the other streams' live paths
    // leave the grey form too; the next Run converts back when it can.
    if (r->grey) PT_HIP(pt_launch_grey_convert(r->slots, Frame(r), r->prob1.ptr, false, d->stream));
    r->grey = false;
    r->grey_blocked = false;
    r->slots.prob1 = nullptr;
    PT_WAIT(d);
    const size_t n = (size_t)T * 256;
    PT_HIP(hipMemcpy(r->thr.ptr + s0, thr.data(), n * 16, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(r->prob.ptr + s0, prob.data(), n * 16, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(r->lam.ptr + s0, lam.data(), n * 4, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(r->act.ptr + s0, act.data(), n * 8, hipMemcpyHostToDevice));
    dbuf<float4> stage;
    PT_HIP(stage.upload(ray.data(), n));
    if (int e = SyncRayOrder(r)) return e;
    if (r->slots.len_order && r->len_cam_stale) {   // the other streams' tiles (BeginRounds)
        PT_HIP(hipMemsetAsync(r->len_cam.ptr, 0, ((size_t)r->slots.tile_count + 1) * sizeof(uint16_t), d->stream));
        r->len_cam_stale = false;
    }
    PT_HIP(pt_launch_restore_rays(r->slots, Frame(r), stage.ptr, s0 / 256, T, d->stream));
    PT_WAIT(d);   // the launch reads stage
    return 0;
}

int ptWriteBasicRendererState(pt_device* d, pt_basic_renderer* r, const pt_pixel_state* in)
{
    return ptWriteBasicRendererStreamState(d, r, 0, in);
}

// A stream's own accumulator (width x height rgba32f; one stream: the sample
// buffer itself), for saving and restoring a multi-stream render.
static float4* StreamAccumulator(pt_basic_renderer* r, uint32_t stream)
{
    return r->streams == 1 ? r->buffer->accum : r->accx.ptr + (size_t)stream * r->buffer->width * r->buffer->height;
}

int ptReadBasicRendererStreamAccumulator(pt_device* d, pt_basic_renderer* r, uint32_t stream, float* rgba)
{
    if (!d || !r || !r->buffer || !rgba) { SetError("null argument"); return -1; }
    if (stream >= r->streams) { SetError("stream %u >= the renderer's %u streams", stream, r->streams); return -1; }
    return ReadBack(d, rgba, StreamAccumulator(r, stream), (size_t)r->buffer->width * r->buffer->height * 16);
}

int ptWriteBasicRendererStreamAccumulator(pt_device* d, pt_basic_renderer* r, uint32_t stream, const float* rgba)
{
    if (!d || !r || !r->buffer || !rgba) { SetError("null argument"); return -1; }
    if (stream >= r->streams) { SetError("stream %u >= the renderer's %u streams", stream, r->streams); return -1; }
    return WriteThrough(d, StreamAccumulator(r, stream), rgba, (size_t)r->buffer->width * r->buffer->height * 16);
}

static_assert(PT_SHADE_DIFFUSE == PT_MATS_DIFFUSE && PT_SHADE_METAL == PT_MATS_METAL &&
              PT_SHADE_TRANSLUCENT == PT_MATS_TRANSLUCENT && PT_SHADE_SCATTER == PT_MATS_SCATTER &&
              PT_SHADE_OPENPBR == PT_MATS_OPENPBR && PT_SHADE_PRIMS == PT_MATS_PRIMS && PT_SHADE_SKY == PT_MATS_SKY &&
              PT_SHADE_TEXWRAP == PT_MATS_TEXWRAP, "pt_api.h shade mask bits");

int ptGetBasicRendererShadeInfo(pt_basic_renderer* r, pt_shade_info* info)
{
    if (!r || !info) { SetError("null argument"); return -1; }
    if (!r->scene || !r->scene->valid) { SetError("renderer: scene has no valid packs (call ptUpdateScene)"); return -1; }
    info->scene_mask = ShadeMats(r);
    info->kernel_mask = pt_shade_mats(ShadeMats(r));
    info->completion_queue = ShadeCompact(r) ? 1u : 0u;
    info->grey_records = r->grey ? 1u : 0u;
    info->ray_order = LengthOrder(r) ? PT_RAY_ORDER_LENGTH : PT_RAY_ORDER_OCTANT;
    info->length_trained = r->scene->len_trained ? 1u : 0u;
    info->block_map = RunMap(r) ? PT_BLOCK_MAP_RUN : PT_BLOCK_MAP_TILE;
    return 0;
}

}  // extern "C"
