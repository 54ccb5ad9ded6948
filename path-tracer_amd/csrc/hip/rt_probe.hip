// rt_probe.hip — host side of libpathtracer.so: the test probes: ray queries, traversal
// counters, device numerics, the texture sampler and the slab test, each
// checked against the host by the tests.
#include "runtime.hpp"
#include "../../../include/pt_visibility.h"

using namespace ptrt;

extern "C" {

int ptTraceRays(pt_device* d, pt_scene* s, uint32_t n, const float* origins, const uint32_t* vel, const float* dur,
                pt_hit_record* out)
{
    if (!d || !s || (n && (!origins || !vel || !dur || !out))) { SetError("null argument"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    bool spill = s->stack_needed > pt_extend_stack_cap();
    dbuf<float> d_o, d_t;
    dbuf<uint32_t> d_v, d_spill;
    dbuf<float4> d_hit, d_rec;
    dbuf<float2> d_hc, d_uv;
    hipError_t e = hipSuccess;
    do {
        if ((e = d_o.upload(origins, (size_t)n * 3)) != hipSuccess) break;
        if ((e = d_t.upload(dur, n)) != hipSuccess) break;
        if ((e = d_v.upload(vel, n)) != hipSuccess) break;
        if ((e = d_hit.alloc(n)) != hipSuccess || (e = d_rec.alloc(n)) != hipSuccess) break;
        if ((e = d_hc.alloc(n)) != hipSuccess || (e = d_uv.alloc(n)) != hipSuccess) break;
        if (spill && (e = d_spill.alloc((size_t)(s->stack_needed - pt_extend_stack_cap()) * n)) != hipSuccess) break;
        // The extend launch alone is timed (PT_KERNEL_EXTEND) while the device
        // profiles: the figure ptOccludedRays' launch is held against.
        PT_TIMED(d, PT_KERNEL_EXTEND,
                 pt_launch_trace_rays_extend(s->d, n, d_o.ptr, d_v.ptr, d_t.ptr, d_hit.ptr, d_hc.ptr,
                                             spill ? d_spill.ptr : nullptr, d->stream));
        if ((e = pt_launch_finalize(s->d, n, d_hit.ptr, d_hc.ptr, d_rec.ptr, d_uv.ptr, d->stream)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(d->stream)) != hipSuccess) break;
        std::vector<float4> rec(n);
        std::vector<float2> uv(n);
        if ((e = hipMemcpy(rec.data(), d_rec.ptr, (size_t)n * 16, hipMemcpyDeviceToHost)) != hipSuccess) break;
        if ((e = hipMemcpy(uv.data(), d_uv.ptr, (size_t)n * 8, hipMemcpyDeviceToHost)) != hipSuccess) break;
        for (uint32_t i = 0; i < n; i++) {
            std::memcpy(&out[i].time, &rec[i].x, 4);
            std::memcpy(&out[i].shape_material, &rec[i].y, 4);
            std::memcpy(&out[i].packed_normal, &rec[i].z, 4);
            std::memcpy(&out[i].packed_tangent, &rec[i].w, 4);
            out[i].u = uv[i].x;
            out[i].v = uv[i].y;
        }
    } while (0);
    if (e != hipSuccess) { SetError("ptTraceRays: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

// Diagnostic: ptExtendStats's traversal counters for caller-given rays (the
// ptTraceRays inputs), plus each ray's step count (order-independent: a ray's
// traversal does not depend on its neighbours).
int ptTraceRaysStats(pt_device* d, pt_scene* s, uint32_t n, const float* origins, const uint32_t* vel,
                     const float* dur, uint64_t out[PT_EXTEND_STATS_COUNT], uint32_t* steps)
{
    if (!d || !s || !out || (n && (!origins || !vel || !dur))) { SetError("null argument"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    for (int i = 0; i < PT_EXTEND_STATS_COUNT; i++) out[i] = 0;
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    bool spill = s->stack_needed > pt_extend_stack_cap();
    dbuf<float> d_o, d_t;
    dbuf<uint32_t> d_v, d_spill, d_steps;
    dbuf<float4> d_hit;
    dbuf<float2> d_hc;
    dbuf<unsigned long long> d_out;
    hipError_t e = hipSuccess;
    unsigned long long h[PT_EXTEND_STATS_COUNT] = {};
    do {
        if ((e = d_o.upload(origins, (size_t)n * 3)) != hipSuccess) break;
        if ((e = d_t.upload(dur, n)) != hipSuccess) break;
        if ((e = d_v.upload(vel, n)) != hipSuccess) break;
        if ((e = d_hit.alloc(n)) != hipSuccess || (e = d_hc.alloc(n)) != hipSuccess) break;
        if ((e = d_out.alloc(PT_EXTEND_STATS_COUNT)) != hipSuccess) break;
        if (steps && (e = d_steps.alloc(n)) != hipSuccess) break;
        if (spill && (e = d_spill.alloc((size_t)(s->stack_needed - pt_extend_stack_cap()) * n)) != hipSuccess) break;
        if ((e = hipMemsetAsync(d_out.ptr, 0, sizeof(h), d->stream)) != hipSuccess) break;
        e = pt_launch_trace_rays_stats(s->d, n, d_o.ptr, d_v.ptr, d_t.ptr, d_hit.ptr, d_hc.ptr,
                                       spill ? d_spill.ptr : nullptr, d_out.ptr, steps ? d_steps.ptr : nullptr,
                                       d->stream);
        if (e != hipSuccess) break;
        if ((e = hipMemcpyAsync(h, d_out.ptr, sizeof(h), hipMemcpyDeviceToHost, d->stream)) != hipSuccess) break;
        if (steps && (e = hipMemcpyAsync(steps, d_steps.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream)) != hipSuccess)
            break;
        e = hipStreamSynchronize(d->stream);
    } while (0);
    if (e != hipSuccess) { SetError("ptTraceRaysStats: %s", hipGetErrorString(e)); return (int)e; }
    for (int i = 0; i < PT_EXTEND_STATS_COUNT; i++) out[i] = h[i];
    return 0;
}

// The any-hit query (occlusion.hip): ptTraceRays' inputs, one bit per ray out.
// The launch is timed under PT_KERNEL_EXTEND while the device profiles.
int ptOccludedRays(pt_device* d, pt_scene* s, uint32_t n, const float* origins, const uint32_t* vel, const float* dur,
                   uint64_t* mask)
{
    if (!d || !s || (n && (!origins || !vel || !dur || !mask))) { SetError("null argument"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    const bool spill = s->stack_needed > pt_extend_stack_cap();
    const size_t words = ((size_t)n + 63) / 64;
    dbuf<float> d_o, d_t;
    dbuf<uint32_t> d_v, d_spill;
    dbuf<unsigned long long> d_mask;
    PT_HIP(d_o.upload(origins, (size_t)n * 3));
    PT_HIP(d_t.upload(dur, n));
    PT_HIP(d_v.upload(vel, n));
    PT_HIP(d_mask.alloc(words));
    if (spill) PT_HIP(d_spill.alloc((size_t)(s->stack_needed - pt_extend_stack_cap()) * n));
    PT_TIMED(d, PT_KERNEL_EXTEND,
             pt_launch_occluded_rays(s->d, n, d_o.ptr, d_v.ptr, d_t.ptr, spill ? d_spill.ptr : nullptr, d_mask.ptr,
                                     d->stream));
    PT_HIP(hipMemcpyAsync(mask, d_mask.ptr, words * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    PT_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

// Diagnostic: ptTraceRaysStats' counters and step counts for the any-hit
// traversal of the same rays (the general loop with the early exit).
int ptOccludedRaysStats(pt_device* d, pt_scene* s, uint32_t n, const float* origins, const uint32_t* vel,
                        const float* dur, uint64_t out[PT_EXTEND_STATS_COUNT], uint32_t* steps)
{
    if (!d || !s || !out || (n && (!origins || !vel || !dur))) { SetError("null argument"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    for (int i = 0; i < PT_EXTEND_STATS_COUNT; i++) out[i] = 0;
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    const bool spill = s->stack_needed > pt_extend_stack_cap();
    dbuf<float> d_o, d_t;
    dbuf<uint32_t> d_v, d_spill, d_steps;
    dbuf<unsigned long long> d_out;
    unsigned long long h[PT_EXTEND_STATS_COUNT] = {};
    PT_HIP(d_o.upload(origins, (size_t)n * 3));
    PT_HIP(d_t.upload(dur, n));
    PT_HIP(d_v.upload(vel, n));
    PT_HIP(d_out.alloc(PT_EXTEND_STATS_COUNT));
    if (steps) PT_HIP(d_steps.alloc(n));
    if (spill) PT_HIP(d_spill.alloc((size_t)(s->stack_needed - pt_extend_stack_cap()) * n));
    PT_HIP(hipMemsetAsync(d_out.ptr, 0, sizeof(h), d->stream));
    PT_HIP(pt_launch_occluded_rays_stats(s->d, n, d_o.ptr, d_v.ptr, d_t.ptr, spill ? d_spill.ptr : nullptr, d_out.ptr,
                                         steps ? d_steps.ptr : nullptr, d->stream));
    PT_HIP(hipMemcpyAsync(h, d_out.ptr, sizeof(h), hipMemcpyDeviceToHost, d->stream));
    if (steps) PT_HIP(hipMemcpyAsync(steps, d_steps.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream));
    PT_HIP(hipStreamSynchronize(d->stream));
    for (int i = 0; i < PT_EXTEND_STATS_COUNT; i++) out[i] = h[i];
    return 0;
}

// Visibility gathered at caller-given points (occlusion.hip; DESIGN.md §6 row
// 15).  A launch covers a whole number of points and at most max_lanes lanes,
// which bounds a deep scene's spill rows at (stack_needed - cap) x max_lanes
// words whatever n is.  Each launch is timed under PT_KERNEL_EXTEND.
int ptGatherVisibilityChunked(pt_device* d, pt_scene* s, uint32_t n, const float* points, const float* normals,
                              const pt_visibility_gather_parameters* params, uint32_t max_lanes,
                              pt_visibility_record* out)
{
    if (!d || !s || !params || (n && (!points || !normals || !out))) { SetError("null argument"); return -1; }
    if (s->dev != d) { SetError("ptGatherVisibility: scene of another device"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    if (!pt_visibility_gather_parameters_ok(params, n)) {
        SetError("ptGatherVisibility: Samples %u (a power of two up to 64), Radius %g (> 0), Offset %g (finite, >= 0), "
                 "FirstIndex %u + n %u (n <= 2^26, the sum <= 2^32)",
                 params->Samples, (double)params->Radius, (double)params->Offset, params->FirstIndex, n);
        return -1;
    }
    if (max_lanes < PT_AMBIENT_OCCLUSION_MAX_SAMPLES || max_lanes > PT_VISIBILITY_GATHER_MAX_LANES) {
        SetError("ptGatherVisibilityChunked: max_lanes %u outside 64..2^22", max_lanes);
        return -1;
    }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    const uint32_t chunk = std::min(n, max_lanes / params->Samples);   // points per launch, >= 1
    const bool spill = s->stack_needed > pt_extend_stack_cap();
    dbuf<float> d_p, d_n;
    dbuf<uint32_t> d_spill;
    dbuf<float4> d_out;
    PT_HIP(d_p.upload(points, (size_t)n * 3));
    PT_HIP(d_n.upload(normals, (size_t)n * 3));
    PT_HIP(d_out.alloc((size_t)n * 2));
    if (spill) PT_HIP(d_spill.alloc((size_t)(s->stack_needed - pt_extend_stack_cap()) * chunk * params->Samples));
    for (uint32_t a = 0; a < n; a += chunk) {
        const uint32_t m = std::min(chunk, n - a);
        PT_TIMED(d, PT_KERNEL_EXTEND,
                 pt_launch_gather_visibility(s->d, m, d_p.ptr + (size_t)a * 3, d_n.ptr + (size_t)a * 3, params,
                                             params->FirstIndex + a, spill ? d_spill.ptr : nullptr,
                                             d_out.ptr + (size_t)a * 2, d->stream));
    }
    PT_HIP(hipMemcpyAsync(out, d_out.ptr, (size_t)n * sizeof(pt_visibility_record), hipMemcpyDeviceToHost, d->stream));
    PT_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

int ptGatherVisibility(pt_device* d, pt_scene* s, uint32_t n, const float* points, const float* normals,
                       const pt_visibility_gather_parameters* params, pt_visibility_record* out)
{
    return ptGatherVisibilityChunked(d, s, n, points, normals, params, PT_VISIBILITY_GATHER_MAX_LANES, out);
}

// Sky light gathered at caller-given points (occlusion.hip; DESIGN.md §6 row
// 16): ptGatherVisibilityChunked's upload, whole-point chunks and spill rows;
// eight float4 per point come back.  The normals are uploaded with Lobe COSINE
// only.
int ptGatherSkyLightChunked(pt_device* d, pt_scene* s, uint32_t n, const float* points, const float* normals,
                            const pt_sky_gather_parameters* params, uint32_t max_lanes, pt_sky_record* out)
{
    if (!d || !s || !params || (n && (!points || !out))) { SetError("null argument"); return -1; }
    if (s->dev != d) { SetError("ptGatherSkyLight: scene of another device"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    if (!pt_sky_gather_parameters_ok(params, n)) {
        SetError("ptGatherSkyLight: Samples %u (a power of two up to 64), Radius %g (> 0), Offset %g (finite, >= 0), "
                 "FirstIndex %u + n %u (n <= 2^26, the sum <= 2^32), Lobe %u (0 or 1)",
                 params->Samples, (double)params->Radius, (double)params->Offset, params->FirstIndex, n, params->Lobe);
        return -1;
    }
    const bool cosine = params->Lobe == PT_SKY_GATHER_COSINE;
    if (n && cosine && !normals) { SetError("null argument"); return -1; }
    if (max_lanes < PT_AMBIENT_OCCLUSION_MAX_SAMPLES || max_lanes > PT_VISIBILITY_GATHER_MAX_LANES) {
        SetError("ptGatherSkyLightChunked: max_lanes %u outside 64..2^22", max_lanes);
        return -1;
    }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    const uint32_t chunk = std::min(n, max_lanes / params->Samples);   // points per launch, >= 1
    const bool spill = s->stack_needed > pt_extend_stack_cap();
    dbuf<float> d_p, d_n;
    dbuf<uint32_t> d_spill;
    dbuf<float4> d_out;
    PT_HIP(d_p.upload(points, (size_t)n * 3));
    if (cosine) PT_HIP(d_n.upload(normals, (size_t)n * 3));
    PT_HIP(d_out.alloc((size_t)n * 8));
    if (spill) PT_HIP(d_spill.alloc((size_t)(s->stack_needed - pt_extend_stack_cap()) * chunk * params->Samples));
    for (uint32_t a = 0; a < n; a += chunk) {
        const uint32_t m = std::min(chunk, n - a);
        PT_TIMED(d, PT_KERNEL_EXTEND,
                 pt_launch_gather_sky_light(s->d, m, d_p.ptr + (size_t)a * 3, cosine ? d_n.ptr + (size_t)a * 3 : nullptr,
                                            params, params->FirstIndex + a, spill ? d_spill.ptr : nullptr,
                                            d_out.ptr + (size_t)a * 8, d->stream));
    }
    PT_HIP(hipMemcpyAsync(out, d_out.ptr, (size_t)n * sizeof(pt_sky_record), hipMemcpyDeviceToHost, d->stream));
    PT_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

int ptGatherSkyLight(pt_device* d, pt_scene* s, uint32_t n, const float* points, const float* normals,
                     const pt_sky_gather_parameters* params, pt_sky_record* out)
{
    return ptGatherSkyLightChunked(d, s, n, points, normals, params, PT_VISIBILITY_GATHER_MAX_LANES, out);
}

int ptCheckFastDivision(pt_device* d, uint64_t n, uint32_t seed, uint64_t* mismatches)
{
    if (!d || !mismatches) { SetError("null argument"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    unsigned long long* dm = nullptr;
    PT_HIP(hipMalloc(&dm, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(dm, 0, sizeof(unsigned long long), d->stream);
    if (e == hipSuccess) e = pt_launch_xdiv_check(n, seed, dm, d->stream);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, dm, sizeof(h), hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(dm);
    if (e != hipSuccess) { SetError("ptCheckFastDivision: %s", hipGetErrorString(e)); return (int)e; }
    *mismatches = h;
    return 0;
}

int ptCheckFastReciprocal(pt_device* d, uint64_t* mismatches)
{
    if (!d || !mismatches) { SetError("null argument"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    unsigned long long* dm = nullptr;
    PT_HIP(hipMalloc(&dm, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(dm, 0, sizeof(unsigned long long), d->stream);
    if (e == hipSuccess) e = pt_launch_rcp_check(dm, d->stream);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, dm, sizeof(h), hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(dm);
    if (e != hipSuccess) { SetError("ptCheckFastReciprocal: %s", hipGetErrorString(e)); return (int)e; }
    *mismatches = h;
    return 0;
}

int ptEvalNumerics(pt_device* d, uint32_t op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                   uint32_t* out)
{
    if (!d) { SetError("null argument"); return -1; }
    const uint32_t operands = pt_numerics_operands(op), outputs = pt_numerics_outputs(op);
    if (operands == 0) { SetError("ptEvalNumerics: unknown op %u", op); return -1; }
    if (n && (!out || !a || (operands > 1 && !b) || (operands > 2 && !c))) { SetError("null argument"); return -1; }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    dbuf<uint32_t> d_a, d_b, d_c, d_out;
    hipError_t e = hipSuccess;
    do {
        if ((e = d_a.upload(a, n)) != hipSuccess) break;
        if (operands > 1 && (e = d_b.upload(b, n)) != hipSuccess) break;
        if (operands > 2 && (e = d_c.upload(c, n)) != hipSuccess) break;
        if ((e = d_out.alloc((size_t)n * outputs)) != hipSuccess) break;
        if ((e = pt_launch_numerics_probe(op, n, d_a.ptr, d_b.ptr, d_c.ptr, d_out.ptr, d->stream)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(d->stream)) != hipSuccess) break;
        e = hipMemcpy(out, d_out.ptr, (size_t)n * outputs * sizeof(uint32_t), hipMemcpyDeviceToHost);
    } while (0);
    if (e != hipSuccess) { SetError("ptEvalNumerics: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

int ptSampleTextures(pt_device* d, pt_scene* s, uint32_t n, const uint32_t* texture_index, const float* uv,
                     uint32_t wrap, float* rgba)
{
    if (!d || !s || (n && (!texture_index || !uv || !rgba))) { SetError("null argument"); return -1; }
    if (s->dev != d) { SetError("ptSampleTextures: scene of another device"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs"); return -1; }
    if (wrap > 1) { SetError("ptSampleTextures: wrap %u", wrap); return -1; }
    if (wrap == 1 && (s->mats & PT_MATS_TEXWRAP)) {
        SetError("ptSampleTextures: the two-select wrap needs every atlas placement inside [0, 1]");
        return -1;
    }
    for (uint32_t i = 0; i < n; i++)
        if (texture_index[i] >= s->texture_count) {
            SetError("ptSampleTextures: texture index %u >= texture count %u", texture_index[i], s->texture_count);
            return -1;
        }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    dbuf<uint32_t> d_index;
    dbuf<float2> d_uv;
    dbuf<float4> d_rgba;
    hipError_t e = hipSuccess;
    do {
        if ((e = d_index.upload(texture_index, n)) != hipSuccess) break;
        if ((e = d_uv.upload(reinterpret_cast<const float2*>(uv), n)) != hipSuccess) break;
        if ((e = d_rgba.alloc(n)) != hipSuccess) break;
        if ((e = pt_launch_sample_textures(s->d, n, d_index.ptr, d_uv.ptr, wrap == 1, d_rgba.ptr, d->stream)) != hipSuccess)
            break;
        if ((e = hipStreamSynchronize(d->stream)) != hipSuccess) break;
        e = hipMemcpy(rgba, d_rgba.ptr, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
    } while (0);
    if (e != hipSuccess) { SetError("ptSampleTextures: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

int ptEvalSlabTest(pt_device* d, uint32_t n, const float* origin, const float* velocity, const float* reach,
                   const float* box_min, const float* box_max, uint32_t scene_gate, uint32_t* entry, uint32_t* exact)
{
    if (!d || (n && (!origin || !velocity || !reach || !box_min || !box_max || !entry || !exact))) {
        SetError("null argument");
        return -1;
    }
    if (scene_gate > 1) { SetError("ptEvalSlabTest: scene_gate %u", scene_gate); return -1; }
    if (n == 0) return 0;
    PT_HIP(hipSetDevice(d->id));
    ptd::dscene S{};
    S.fast_div = scene_gate;
    dbuf<float> d_o, d_v, d_r, d_lo, d_hi;
    dbuf<uint32_t> d_entry, d_exact;
    PT_HIP(d_o.upload(origin, (size_t)n * 3));
    PT_HIP(d_v.upload(velocity, (size_t)n * 3));
    PT_HIP(d_r.upload(reach, n));
    PT_HIP(d_lo.upload(box_min, (size_t)n * 3));
    PT_HIP(d_hi.upload(box_max, (size_t)n * 3));
    PT_HIP(d_entry.alloc(n));
    PT_HIP(d_exact.alloc(n));
    PT_HIP(pt_launch_slab_probe(S, n, d_o.ptr, d_v.ptr, d_r.ptr, d_lo.ptr, d_hi.ptr, d_entry.ptr, d_exact.ptr, d->stream));
    PT_HIP(hipMemcpyAsync(entry, d_entry.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    PT_HIP(hipMemcpyAsync(exact, d_exact.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    PT_HIP(hipStreamSynchronize(d->stream));
    return 0;
}

static int ExtendStats(pt_device* d, pt_basic_renderer* r, uint64_t* out, uint32_t* steps_out, const char* what)
{
    if (!d || (!out && !steps_out)) { SetError("null argument"); return -1; }
    if (CheckReady(r) != 0) return -1;
    PT_HIP(hipSetDevice(d->id));
    if (int e = EnsureSpill(r)) return e;
    unsigned long long* dm = nullptr;
    uint32_t* ds = nullptr;
    PT_HIP(hipMalloc(&dm, PT_EXTEND_STATS_COUNT * sizeof(unsigned long long)));
    hipError_t e = steps_out ? hipMalloc(&ds, (size_t)r->slots.n * 4) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(dm, 0, PT_EXTEND_STATS_COUNT * sizeof(unsigned long long), d->stream);
    if (e == hipSuccess)
        e = pt_launch_extend_stats(r->scene->d, r->slots, Frame(r), r->slots.spill, dm, ds, d->stream);
    unsigned long long h[PT_EXTEND_STATS_COUNT] = {};
    if (e == hipSuccess) e = hipMemcpyAsync(h, dm, sizeof(h), hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess && ds) e = hipMemcpyAsync(steps_out, ds, (size_t)r->slots.n * 4, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    (void)hipFree(dm);
    if (ds) (void)hipFree(ds);
    if (e != hipSuccess) { SetError("%s: %s", what, hipGetErrorString(e)); return (int)e; }
    if (out)
        for (int i = 0; i < PT_EXTEND_STATS_COUNT; i++) out[i] = h[i];
    return 0;
}

int ptExtendStats(pt_device* d, pt_basic_renderer* r, uint64_t out[PT_EXTEND_STATS_COUNT])
{
    return ExtendStats(d, r, out, nullptr, "ptExtendStats");
}

int ptExtendStepCounts(pt_device* d, pt_basic_renderer* r, uint32_t* steps)
{
    return ExtendStats(d, r, nullptr, steps, "ptExtendStepCounts");
}

}  // extern "C"
