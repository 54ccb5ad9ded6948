// rt_post.hip — host side of libpathtracer.so: what works on finished sample buffers:
// preview, denoise guides, the denoisers, reprojection, history validation, the
// firefly clamp, statistics and accumulation.
#include "runtime.hpp"
#include "../../../include/pt_visibility.h"

#include <initializer_list>
#include <string>

using namespace ptrt;

namespace {

// One object of an entry point's device and size checks: an optional object
// that is absent has no label and takes no part.  Objects of the same group
// must have the same size.
struct checked { const char* label; const pt_device* dev; uint32_t w, h; bool buffer; int group; };

checked Obj(const char* label, const pt_sample_buffer* b, int group = 0)
{
    return b ? checked{label, b->dev, b->width, b->height, true, group} : checked{};
}
checked Obj(const char* label, const pt_denoise_guides* g, int group = 0)
{
    return checked{label, g->dev, g->width, g->height, false, group};
}

// After the null and aliasing checks of entry point `what`: every object
// belongs to device d, then every group's objects have one size.
int CheckObjects(const char* what, const pt_device* d, std::initializer_list<checked> objs)
{
    bool buffers = true, device = true, size = true;
    for (const checked& o : objs) {
        if (!o.label) continue;
        buffers &= o.buffer;
        device &= o.dev == d;
        for (const checked& p : objs) size &= !p.label || p.group != o.group || (p.w == o.w && p.h == o.h);
    }
    if (!device) { SetError("%s: %s of another device", what, buffers ? "sample buffer" : "objects"); return -1; }
    if (size) return 0;
    std::string sizes;
    for (const checked& o : objs)
        if (o.label)
            sizes += (sizes.empty() ? "" : ", ") + std::string(o.label) + " " + std::to_string(o.w) + "x" + std::to_string(o.h);
    SetError("%s: size mismatch (%s)", what, sizes.c_str());
    return -1;
}

}  // namespace

extern "C" {

pt_preview* ptCreatePreviewRenderContext(pt_device* d, pt_scene* s)
{
    if (!d || !s) { SetError("null argument"); return nullptr; }
    if (hipSetDevice(d->id) != hipSuccess) { SetError("hipSetDevice failed"); return nullptr; }
    pt_preview* c = new pt_preview;
    c->dev = d;
    c->scene = s;
    uint32_t none = 0xFFFFFFFFu;
    if (c->query.upload(&none, 1) != hipSuccess) {
        SetError("preview query buffer allocation failed");
        delete c;
        return nullptr;
    }
    if (c->observe.alloc(PT_OBSERVE_TABLE_FLOATS) != hipSuccess || pt_launch_observe_table(c->observe.ptr, d->stream) != hipSuccess) {
        SetError("preview table set-up failed");
        delete c;
        return nullptr;
    }
    return c;
}

void ptDestroyPreviewRenderContext(pt_device* d, pt_preview* c)
{
    if (!c) return;
    if (d) (void)hipSetDevice(d->id);
    delete c;
}

// RenderPreview (preview_render.cpp:118-181)
int ptRenderPreview(pt_device* d, pt_preview* c, const pt_preview_parameters* p)
{
    if (!d || !c || !p) { SetError("null argument"); return -1; }
    if (!c->scene->valid) { SetError("preview: scene has no valid packs (call ptUpdateScene)"); return -1; }
    if (p->RenderMode > PT_PREVIEW_RENDER_MODE_SCENE_COMPLEXITY) { SetError("bad preview mode %u", p->RenderMode); return -1; }
    if (p->RenderSizeX == 0 || p->RenderSizeY == 0 || p->RenderSizeX > 32768 || p->RenderSizeY > 32768) {
        SetError("bad preview size %ux%u", p->RenderSizeX, p->RenderSizeY);
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    size_t n = (size_t)p->RenderSizeX * p->RenderSizeY;
    PT_HIP(c->image.alloc(n));
    PT_HIP(c->aov.alloc(n));
    uint32_t need = c->scene->stack_needed, cap = pt_preview_stack_cap();
    uint32_t* spill = nullptr;
    if (need > cap) {
        size_t threads = (size_t)((p->RenderSizeX + 15) / 16) * ((p->RenderSizeY + 15) / 16) * 256;
        PT_HIP(c->spill.alloc((need - cap) * threads));
        spill = c->spill.ptr;
    }
    PT_TIMED(d, PT_KERNEL_PREVIEW,
             pt_launch_preview(c->scene->d, p, spill, c->image.ptr, c->aov.ptr, c->query.ptr, c->observe.ptr, d->stream));
    c->width = p->RenderSizeX;
    c->height = p->RenderSizeY;
    c->rendered = true;
    return 0;
}

// RetrievePreviewQueryResult (preview_render.cpp:96-116)
int ptRetrievePreviewQueryResult(pt_device* d, pt_preview* c, uint32_t* hit_shape_index)
{
    if (!d || !c || !hit_shape_index) { SetError("null argument"); return -1; }
    return ReadBack(d, hit_shape_index, c->query.ptr, sizeof(uint32_t));
}

int ptReadPreviewImage(pt_device* d, pt_preview* c, float* rgba)
{
    if (!d || !c || !rgba) { SetError("null argument"); return -1; }
    if (!c->rendered) { SetError("preview not rendered"); return -1; }
    return ReadBack(d, rgba, c->image.ptr, (size_t)c->width * c->height * sizeof(float4));
}

int ptReadPreviewAOVs(pt_device* d, pt_preview* c, pt_preview_aov* aov)
{
    if (!d || !c || !aov) { SetError("null argument"); return -1; }
    if (!c->rendered) { SetError("preview not rendered"); return -1; }
    return ReadBack(d, aov, c->aov.ptr, (size_t)c->width * c->height * sizeof(pt_preview_aov));
}

// --- denoiser (denoise.hip) ------------------------------------------

pt_denoise_guides* ptCreateDenoiseGuides(pt_device* d, uint32_t w, uint32_t h)
{
    if (!d || w == 0 || h == 0 || w > 32768 || h > 32768) { SetError("bad denoise guides arguments"); return nullptr; }
    if (hipSetDevice(d->id) != hipSuccess) { SetError("hipSetDevice failed"); return nullptr; }
    pt_denoise_guides* g = new pt_denoise_guides;
    g->dev = d;
    g->width = w;
    g->height = h;
    size_t n = (size_t)w * h;
    if (g->records.alloc(2 * n) != hipSuccess ||
        hipMemsetAsync(g->records.ptr, 0, n * sizeof(pt_denoise_guide), d->stream) != hipSuccess ||
        g->observe.alloc(PT_OBSERVE_TABLE_FLOATS) != hipSuccess ||
        pt_launch_observe_table(g->observe.ptr, d->stream) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess) {
        SetError("denoise guides allocation failed (%zu bytes)", n * sizeof(pt_denoise_guide));
        delete g;
        return nullptr;
    }
    return g;
}

void ptDestroyDenoiseGuides(pt_device* d, pt_denoise_guides* g)
{
    if (!g) return;
    if (d) (void)hipSetDevice(d->id);
    delete g;
}

// specular: ptRenderDenoiseGuidesSpecular's launch.  A chain of zero bounces,
// and any chain in a scene none of whose shapes has a metal or translucent
// material (pt_scene::mats: nothing can be followed), is the plain kernel's
// record bit for bit, so those take the plain kernel.
static int RenderGuides(pt_device* d, pt_scene* s, pt_denoise_guides* g, uint32_t camera_index, bool specular,
                        uint32_t max_bounces)
{
    if (!d || !s || !g) { SetError("null argument"); return -1; }
    if (specular && max_bounces > PT_GUIDE_MAX_BOUNCES) {
        SetError("denoise guides: %u bounces, at most %u", max_bounces, (uint32_t)PT_GUIDE_MAX_BOUNCES);
        return -1;
    }
    if (s->dev != d || g->dev != d) { SetError("denoise guides: scene or guides belong to another device"); return -1; }
    if (!s->valid) { SetError("denoise guides: scene has no valid packs (call ptUpdateScene)"); return -1; }
    if (camera_index >= s->camera_count) {
        SetError("denoise guides: camera index %u out of range (%u cameras)", camera_index, s->camera_count);
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    uint32_t need = s->stack_needed, cap = pt_guides_stack_cap();
    uint32_t* spill = nullptr;
    if (need > cap) {
        size_t threads = (size_t)((g->width + 15) / 16) * ((g->height + 15) / 16) * 256;
        PT_HIP(g->spill.alloc((need - cap) * threads));
        spill = g->spill.ptr;
    }
    if (specular && max_bounces != 0 && (s->mats & (PT_MATS_METAL | PT_MATS_TRANSLUCENT)) != 0) {
        PT_TIMED(d, PT_KERNEL_GUIDES,
                 pt_launch_denoise_guides_specular(s->d, camera_index, max_bounces, g->width, g->height, spill,
                                                   g->records.ptr, g->observe.ptr, d->stream));
        return 0;
    }
    PT_TIMED(d, PT_KERNEL_GUIDES,
             pt_launch_denoise_guides(s->d, camera_index, g->width, g->height, spill, g->records.ptr, g->observe.ptr,
                                      d->stream));
    return 0;
}

int ptRenderDenoiseGuides(pt_device* d, pt_scene* s, pt_denoise_guides* g, uint32_t camera_index)
{
    return RenderGuides(d, s, g, camera_index, false, 0);
}

int ptRenderDenoiseGuidesSpecular(pt_device* d, pt_scene* s, pt_denoise_guides* g, uint32_t camera_index,
                                  uint32_t max_bounces)
{
    return RenderGuides(d, s, g, camera_index, true, max_bounces);
}

// --- ambient occlusion / sky visibility (occlusion.hip) --------

// One launch, counted under PT_KERNEL_GUIDES (the same launch shape: a primary
// ray per pixel in 16 x 16 tiles).  The spill rows are the scene's, grown on
// demand (a regrowth frees the old rows, which waits for the device).
int ptRenderAmbientOcclusion(pt_device* d, pt_scene* s, uint32_t camera_index, const pt_ambient_occlusion_parameters* p,
                             pt_sample_buffer* dst)
{
    if (!d || !s || !p || !dst) { SetError("null argument"); return -1; }
    if (s->dev != d || dst->dev != d) { SetError("ambient occlusion: scene or sample buffer of another device"); return -1; }
    if (!s->valid) { SetError("ambient occlusion: scene has no valid packs (call ptUpdateScene)"); return -1; }
    if (camera_index >= s->camera_count) {
        SetError("ambient occlusion: camera index %u out of range (%u cameras)", camera_index, s->camera_count);
        return -1;
    }
    if (!pt_visibility_parameters_ok(p)) {
        SetError("ambient occlusion: Samples %u (1..%u) or Radius %g (> 0) out of range", p->Samples,
                 (uint32_t)PT_AMBIENT_OCCLUSION_MAX_SAMPLES, (double)p->Radius);
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    const uint32_t need = s->stack_needed, cap = pt_extend_stack_cap();
    uint32_t* spill = nullptr;
    if (need > cap) {
        const size_t threads = (size_t)((dst->width + 15) / 16) * ((dst->height + 15) / 16) * 256;
        PT_HIP(s->visibility_spill.alloc((need - cap) * threads));
        spill = s->visibility_spill.ptr;
    }
    PT_TIMED(d, PT_KERNEL_GUIDES,
             pt_launch_ambient_occlusion(s->d, camera_index, dst->width, dst->height, p, spill, dst->accum, d->stream));
    return 0;
}

int ptReadDenoiseGuides(pt_device* d, pt_denoise_guides* g, pt_denoise_guide* out)
{
    if (!d || !g || !out) { SetError("null argument"); return -1; }
    return ReadBack(d, out, g->records.ptr, (size_t)g->width * g->height * sizeof(pt_denoise_guide));
}

int ptWriteDenoiseGuides(pt_device* d, pt_denoise_guides* g, const pt_denoise_guide* in)
{
    if (!d || !g || !in) { SetError("null argument"); return -1; }
    return WriteThrough(d, g->records.ptr, in, (size_t)g->width * g->height * sizeof(pt_denoise_guide));
}

int ptSetDenoiseVariant(pt_denoise_guides* g, uint32_t variant)
{
    if (!g || variant > PT_DENOISE_VARIANT_LATTICE) { SetError("bad denoise variant"); return -1; }
    g->variant = variant;
    return 0;
}

// The kernel of iteration i (step 2^i), of the single-buffer and of the pair
// filter.  Automatic mode takes the lattice kernel at every step: measured at
// 1920x1080 and 3840x2160 it is 1.3 - 2 x faster than the gather at each of
// the steps 1 .. 32, so the choice does not depend on the
// iteration.  For the pair filter that started as this choice carried over,
// then was measured on the pair filter itself, where the lattice is again
// 1.2 - 2 x faster at each of the steps 1 .. 32.
static bool DenoiseLattice(uint32_t variant, uint32_t /*iteration*/)
{
    return variant != PT_DENOISE_VARIANT_GATHER;
}

int ptDenoiseSampleBuffer(pt_device* d, pt_sample_buffer* src, pt_denoise_guides* g, const pt_denoise_parameters* p,
                          pt_sample_buffer* dst)
{
    if (!d || !src || !g || !p || !dst) { SetError("null argument"); return -1; }
    if (src == dst) { SetError("denoise: src and dst are the same sample buffer"); return -1; }
    if (CheckObjects("denoise", d, {Obj("src", src), Obj("guides", g), Obj("dst", dst)})) return -1;
    if (!pt_denoise_parameters_ok(p)) {
        SetError("denoise: bad parameters (Iterations %u > %u or a sigma not > 0)", p->Iterations,
                 (uint32_t)PT_DENOISE_MAX_ITERATIONS);
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    const size_t n = (size_t)g->width * g->height;
    const uint32_t N = p->Iterations;
    if (N >= 2) PT_HIP(g->scratch.alloc(n));
    if (N == 0) {
        PT_HIP(pt_launch_denoise_mean(src->accum, (uint32_t)n, dst->accum, d->stream));
        return 0;
    }
    // Iteration i writes dst when an even number of iterations follow it, so
    // the last one lands in dst; iteration 0 reads src's accumulator.
    const float4* in = src->accum;
    for (uint32_t i = 0; i < N; i++) {
        float4* out = ((N - 1 - i) & 1u) ? g->scratch.ptr : dst->accum;
        PT_TIMED(d, PT_KERNEL_DENOISE,
                 pt_launch_denoise(in, i == 0, g->records.ptr, g->width, g->height, p, i, DenoiseLattice(g->variant, i),
                                   out, d->stream));
        in = out;
    }
    return 0;
}

int ptDenoiseSampleBufferPair(pt_device* d, pt_sample_buffer* a, pt_sample_buffer* b, pt_denoise_guides* g,
                              const pt_denoise_pair_parameters* p, pt_sample_buffer* dst)
{
    if (!d || !a || !b || !g || !p || !dst) { SetError("null argument"); return -1; }
    if (a == b || a == dst || b == dst) { SetError("denoise pair: a, b and dst must be three sample buffers"); return -1; }
    if (CheckObjects("denoise pair", d, {Obj("a", a), Obj("b", b), Obj("guides", g), Obj("dst", dst)})) return -1;
    if (!pt_denoise_pair_parameters_ok(p)) {
        SetError("denoise pair: bad parameters (Iterations %u > %u or a sigma not > 0)", p->Iterations,
                 (uint32_t)PT_DENOISE_MAX_ITERATIONS);
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    const size_t n = (size_t)g->width * g->height;
    const uint32_t N = p->Iterations;
    if (N >= 1) PT_HIP(g->scratch.alloc(n));
    // Image k (0: the prepare launch's, k: iteration k - 1's) is dst when an
    // even number of launches follow it, so the last one lands in dst.
    auto image = [&](uint32_t k) { return ((N - k) & 1u) ? g->scratch.ptr : dst->accum; };
    PT_TIMED(d, PT_KERNEL_DENOISE,
             pt_launch_denoise_pair_prepare(a->accum, b->accum, g->records.ptr, g->width, g->height, N == 0, image(0),
                                            d->stream));
    for (uint32_t i = 0; i < N; i++)
        PT_TIMED(d, PT_KERNEL_DENOISE,
                 pt_launch_denoise_pair(image(i), g->records.ptr, g->width, g->height, p, i, i + 1 == N,
                                        DenoiseLattice(g->variant, i), image(i + 1), d->stream));
    return 0;
}

// --- temporal reprojection (reproject.hip) --------------

// Both entry points: the checks, then with a table (row 9) its stream-ordered
// copy into the device's own buffer, then the launch.  Without one (NULL, 0)
// it is row 8.
static int Reproject(pt_device* d, pt_sample_buffer* prev, pt_denoise_guides* pg, const pt_packed_camera* pc,
                     pt_denoise_guides* g, const pt_packed_camera* c, const pt_shape_motion* motion,
                     uint32_t motion_count, const pt_reproject_parameters* p, pt_sample_buffer* dst)
{
    if (!motion && motion_count) { SetError("reproject: %u motion records at a null pointer", motion_count); return -1; }
    if (!d || !prev || !pg || !pc || !g || !c || !p || !dst) { SetError("null argument"); return -1; }
    if (prev == dst) { SetError("reproject: prev and dst are the same sample buffer"); return -1; }
    if (pg == g) { SetError("reproject: prev_guides and guides are the same object"); return -1; }
    // Two sizes: the previous frame's (group 0) and the new one's (group 1).
    if (CheckObjects("reproject", d, {Obj("prev", prev), Obj("prev_guides", pg), Obj("guides", g, 1), Obj("dst", dst, 1)}))
        return -1;
    if (!pt_reproject_parameters_ok(p)) {
        SetError("reproject: bad parameters (NormalCosine in (-1, 1], DepthTolerance > 0, MinWeight in (0, 1], "
                 "MaxHistory > 0)");
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    // Growing frees the old table; hipFree waits for the launches that read it.
    // An empty table still has a device address: it is what selects row 9.
    if (motion) PT_HIP(d->motion.alloc(motion_count));
    if (motion_count) {
        // The last call's upload may still be queued: it must have read the
        // pinned copy before this call overwrites it.
        if (!d->motion_copied) PT_HIP(hipEventCreateWithFlags(&d->motion_copied, hipEventDisableTiming));
        PT_HIP(hipEventSynchronize(d->motion_copied));
        if (motion_count > d->motion_host_count) {
            if (d->motion_host) (void)hipHostFree(d->motion_host);
            d->motion_host = nullptr;
            d->motion_host_count = 0;
            PT_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->motion_host), (size_t)motion_count * sizeof(pt_shape_motion),
                                 hipHostMallocDefault));
            d->motion_host_count = motion_count;
        }
        std::memcpy(d->motion_host, motion, (size_t)motion_count * sizeof(pt_shape_motion));
        PT_HIP(hipMemcpyAsync(d->motion.ptr, d->motion_host, (size_t)motion_count * sizeof(pt_shape_motion),
                              hipMemcpyHostToDevice, d->stream));
        PT_HIP(hipEventRecord(d->motion_copied, d->stream));
    }
    PT_TIMED(d, PT_KERNEL_REPROJECT,
             pt_launch_reproject(prev->accum, pg->records.ptr, pg->width, pg->height, pc, g->records.ptr, g->width,
                                 g->height, c, motion ? d->motion.ptr : nullptr, motion_count, p, dst->accum,
                                 d->stream));
    return 0;
}

int ptReprojectSampleBuffer(pt_device* d, pt_sample_buffer* prev, pt_denoise_guides* pg, const pt_packed_camera* pc,
                            pt_denoise_guides* g, const pt_packed_camera* c, const pt_reproject_parameters* p,
                            pt_sample_buffer* dst)
{
    return Reproject(d, prev, pg, pc, g, c, nullptr, 0, p, dst);
}

int ptReprojectSampleBufferMoving(pt_device* d, pt_sample_buffer* prev, pt_denoise_guides* pg,
                                  const pt_packed_camera* pc, pt_denoise_guides* g, const pt_packed_camera* c,
                                  const pt_shape_motion* motion, uint32_t motion_count,
                                  const pt_reproject_parameters* p, pt_sample_buffer* dst)
{
    return Reproject(d, prev, pg, pc, g, c, motion, motion_count, p, dst);
}

// --- history validation (rectify.hip) --------------------------

int ptRectifyHistory(pt_device* d, pt_sample_buffer* history, pt_sample_buffer* current, pt_denoise_guides* g,
                     const pt_rectify_parameters* p, pt_sample_buffer* dst)
{
    if (!d || !history || !current || !g || !p || !dst) { SetError("null argument"); return -1; }
    if (history == current || dst == current) {
        SetError("rectify: current is also the history or dst");
        return -1;
    }
    if (CheckObjects("rectify", d, {Obj("history", history), Obj("current", current), Obj("guides", g), Obj("dst", dst)}))
        return -1;
    if (!pt_rectify_parameters_ok(p)) {
        SetError("rectify: bad parameters (Radius in 1..3, MinNeighbours in 1..49, Sigma finite and >= 0, "
                 "ClampedHistory > 0, NormalCosine in (-1, 1])");
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    PT_TIMED(d, PT_KERNEL_REPROJECT,
             pt_launch_rectify(history->accum, current->accum, g->records.ptr, g->width, g->height, p, dst->accum,
                               d->stream));
    return 0;
}

// --- firefly clamp (despike.hip) -------------------------------

int ptDespikeSampleBuffer(pt_device* d, pt_sample_buffer* src, pt_denoise_guides* g, const pt_despike_parameters* p,
                          pt_sample_buffer* dst)
{
    if (!d || !src || !g || !p || !dst) { SetError("null argument"); return -1; }
    if (dst == src) {
        SetError("despike: dst is src");
        return -1;
    }
    if (CheckObjects("despike", d, {Obj("src", src), Obj("guides", g), Obj("dst", dst)})) return -1;
    if (!pt_despike_parameters_ok(p)) {
        SetError("despike: bad parameters (Radius in 1..3, Rank in 1..4, MinNeighbours in Rank..(2 Radius + 1)^2 - 1, "
                 "Scale and Floor finite and >= 0, Floor not -0, NormalCosine in (-1, 1])");
        return -1;
    }
    PT_HIP(hipSetDevice(d->id));
    PT_TIMED(d, PT_KERNEL_DENOISE,
             pt_launch_despike(src->accum, g->records.ptr, g->width, g->height, p, dst->accum, d->stream));
    return 0;
}

// --- frame statistics (stats.hip) ------------------------------

// Automatic mode's histogram update: the wave-uniform shortcut.  Without it a
// constant image runs 19 % (1920x1080) to 37 % (3840x2160) slower than a
// rendered one, far beyond the 1 - 3 % spread of repeated runs; with it the
// constant image is the faster of the two and the rendered one keeps its
// time within that spread.
static bool StatsUniform(uint32_t variant)
{
    return variant != PT_STATS_VARIANT_PLAIN;
}

int ptSetFrameStatisticsVariant(pt_device* d, uint32_t variant)
{
    if (!d || variant > PT_STATS_VARIANT_UNIFORM) { SetError("bad frame statistics variant"); return -1; }
    d->stats_variant = variant;
    return 0;
}

int ptComputeFrameStatistics(pt_device* d, pt_sample_buffer* a, pt_sample_buffer* b, pt_frame_statistics* out)
{
    if (!d || !a || !out) { SetError("null argument"); return -1; }
    if (b == a) { SetError("frame statistics: a and b are the same sample buffer"); return -1; }
    if (CheckObjects("frame statistics", d, {Obj("a", a), Obj("b", b)})) return -1;
    PT_HIP(hipSetDevice(d->id));
    if (hipError_t e = d->stats.alloc(1); e != hipSuccess) {
        SetError("frame statistics allocation failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    const uint64_t n = (uint64_t)a->width * a->height;
    PT_HIP(hipMemsetAsync(d->stats.ptr, 0, sizeof(pt_frame_statistics), d->stream));
    PT_TIMED(d, PT_KERNEL_STATS,
             pt_launch_frame_statistics(a->accum, b ? b->accum : nullptr, n, d->cu_count,
                                        StatsUniform(d->stats_variant), d->stats.ptr, d->stream));
    pt_frame_statistics s;
    PT_HIP(hipMemcpyAsync(&s, d->stats.ptr, sizeof(s), hipMemcpyDeviceToHost, d->stream));
    PT_WAIT(d);
    // The kernel keeps each minimum as the complement of its bit pattern, so
    // that 0 is "no value" for all four fields.
    s.pixels = n;
    s.min_luminance = pt_f2u(s.max_luminance) ? pt_u2f(~pt_f2u(s.min_luminance)) : 0.0f;
    s.min_samples = pt_f2u(s.max_samples) ? pt_u2f(~pt_f2u(s.min_samples)) : 0.0f;
    *out = s;
    return 0;
}

// Per-tile statistics (stats.hip): one launch, one
// read-back of tiles x 32 bytes.
int ptComputeTileStatistics(pt_device* d, pt_sample_buffer* a, pt_sample_buffer* b, float noise_threshold,
                            pt_tile_statistics* out)
{
    if (!d || !a || !out) { SetError("null argument"); return -1; }
    if (b == a) { SetError("tile statistics: a and b are the same sample buffer"); return -1; }
    if (CheckObjects("tile statistics", d, {Obj("a", a), Obj("b", b)})) return -1;
    if (!pt_tile_stats_threshold_ok(noise_threshold)) {
        SetError("tile statistics: the noise threshold is NaN or negative");
        return -1;
    }
    const size_t tiles = (size_t)((a->width + PT_TILE_SIZE - 1) / PT_TILE_SIZE) * ((a->height + PT_TILE_SIZE - 1) / PT_TILE_SIZE);
    if (tiles == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    if (tiles > d->tile_stats.count) {
        // The old records may still be read by a queued copy.
        if (d->tile_stats.ptr) PT_WAIT(d);
        if (hipError_t e = d->tile_stats.alloc(tiles); e != hipSuccess) {
            SetError("tile statistics allocation failed: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    PT_TIMED(d, PT_KERNEL_STATS,
             pt_launch_tile_statistics(a->accum, b ? b->accum : nullptr, a->width, a->height, noise_threshold,
                                       d->tile_stats.ptr, d->stream));
    PT_HIP(hipMemcpyAsync(out, d->tile_stats.ptr, tiles * sizeof(pt_tile_statistics), hipMemcpyDeviceToHost,
                          d->stream));
    PT_WAIT(d);
    return 0;
}

int ptAccumulateSampleBuffer(pt_device* d, pt_sample_buffer* dst, pt_sample_buffer* src)
{
    if (!d || !dst || !src) { SetError("null argument"); return -1; }
    if (dst == src) { SetError("accumulate: dst and src are the same sample buffer"); return -1; }
    if (CheckObjects("accumulate", d, {Obj("dst", dst), Obj("src", src)})) return -1;
    PT_HIP(hipSetDevice(d->id));
    PT_TIMED(d, PT_KERNEL_STATS,
             pt_launch_accumulate(dst->accum, src->accum, (uint64_t)dst->width * dst->height, d->stream));
    return 0;
}

}  // extern "C"
