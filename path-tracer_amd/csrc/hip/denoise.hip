// denoise.hip — the denoiser in front of the tone mapper (no reference
// counterpart): guide images taken with the scene's own camera,
// and the edge-avoiding a-trous filter (Dammertz et al. 2010) over an
// accumulator-shaped image.
//
// Guides: one primary ray per pixel, the central ray of GenerateCameraRay
// (include/pt_reproject.h's pt_reproject_central_ray, the one reprojection
// inverts), through the same Trace() as the extend kernel and the same hit
// attribute code as ptTraceRays' records; pixels map in 16x16 tiles like the
// preview kernel.
//
// Filter: one launch per iteration between two float4 images.  The per-tap
// arithmetic is include/pt_denoise.h's, shared with the host implementation
// (csrc/scene/denoise.cpp); taps run dy outer, dx inner, sums left to right,
// no atomics.  Two kernels, one per memory strategy, computing the same bits:
//   gather   every tap read from global memory (25 x 48 B per pixel);
//   lattice  a block owns a 16x16 set of pixels of ONE residue class of the
//            step lattice (x = rx, y = ry mod step), so its taps fall in a
//            20x20 lattice window whatever the step is; the window is staged
//            in LDS once (400 x 48 B) and the 25 taps read LDS.
// Each is a template over a filter policy, which says what an image record
// is and what a tap does with it: single_filter (row 5: colour, .w = 1, or 0
// for an empty pixel) and pair_filter (a working image
// {colour, luminance variance}, behind one prepare launch that forms the
// combined frame of two half renders and its prefiltered variance).  The
// policy is resolved at compile time; the loops exist once.
#include <type_traits>
#include "pt_device.hpp"
#include "traverse.hpp"
#include "kernels.hpp"
#include "base_color.hpp"
#include "../../../include/pt_denoise.h"
#include "../../../include/pt_reproject.h"
#include "../../../include/pt_guides.h"

namespace ptd {

// --- guides ---------------------------------------------------------------------

struct guide_args {
    uint32_t camera;
    uint32_t w, h;
    uint32_t tiles_x;
};

struct ray_source_guides {
    const dscene* S;
    const guide_args* P;
    PT_DEV bool pixel(uint32_t i, uint32_t& x, uint32_t& y) const
    {
        uint32_t t = i >> 8, l = i & 255u;
        uint32_t ty = t / P->tiles_x;
        x = (t - ty * P->tiles_x) * 16 + (l & 15u);
        y = ty * 16 + (l >> 4);
        return x < P->w && y < P->h;
    }
    PT_DEV bool load(uint32_t i, pt3& O, pt3& V, float& D) const
    {
        uint32_t x, y;
        pixel(i, x, y);
        D = PT_HIT_TIME_LIMIT;
        // The packed velocity's round trip every ray of the integrator takes
        // between raygen and extend is part of it.  False: unknown model.
        return pt_reproject_central_ray(&S->cameras[P->camera], x, y, P->w, P->h, &O, &V);
    }
};

// The launch record of the SPECULAR instantiation; the
// plain one keeps guide_args.
struct guide_args_specular : guide_args {
    uint32_t max_bounces;
};

// A bounced lane's world ray, kept in its registers: what TlasStep restores
// when the lane leaves a BLAS (ray_source_guides::load would hand it the
// camera ray again).
struct ray_source_lane {
    pt3 O, V;
    PT_DEV bool load(uint32_t, pt3& WO, pt3& WV, float& D) const
    {
        WO = O;
        WV = V;
        D = PT_HIT_TIME_LIMIT;
        return true;
    }
};

PT_DEV void StoreGuideMiss(const dscene& S, const observe_table& Tb, bool known, pt3 V, float4* __restrict__ rec)
{
    pt3 A = v3s(0);
    if (known) A = XYZToSRGB(ObserveUnderD65(Tb, SampleSkyboxSpectrum(S, V)));
    rec[0] = make_float4(0, 0, 0, 0);
    rec[1] = make_float4(A.x, A.y, A.z, __uint_as_float(0xFFFFFFFFu));
}

// The chain of include/pt_guides.h for one pixel: up to max_bounces + 1 traces
// through the same LaneBegin / LaneStep, each from an empty stack (LaneBegin
// zeroes both depths; an entry is always put before it is read, spill rows
// included).  A lane whose chain ended leaves the loop and waits for the
// wave's longest chain.
template <int CAP>
PT_DEV void GuideChain(const dscene& S, const observe_table& Tb, tstack<true, CAP>& st, uint32_t i, bool known, pt3 O,
                       pt3 V, uint32_t max_bounces, float4* __restrict__ rec)
{
    const bool trace = known && S.g.ShapeCount != 0;
    float total = 0.0f;
    uint32_t tag = 0;
    for (uint32_t b = 0; b <= PT_GUIDE_MAX_BOUNCES; b++) {
        lane_state Ln;
        LaneBegin(S, Ln, O, V, PT_HIT_TIME_LIMIT);
        const ray_source_lane cur{O, V};
        complexity_stats cx;
        if (trace)
            while (!LaneStep<true, CAP>(S, Ln, st, cur, i, cx)) {}
        if (Ln.Shape == SHAPE_INDEX_NONE) {
            StoreGuideMiss(S, Tb, known, V, rec);
            return;
        }
        float4 h = CompactHit(Ln, S.vidx21 != 0);
        float2 c = make_float2(Ln.C.y, Ln.C.z);
        uint32_t Material;
        pt3 N, TX;
        pt2 UV;
        HitAttributesRecord(S, Ln.Shape, h, c, Material, N, TX, UV);
        const pt3 Nq = UnpackUnitVector(PackUnitVector(N));
        total = pt_guide_total(total, h.x, b);
        const uint32_t Type = MUint(S, Material, 0);
        float Roughness = 1.0f;
        if (pt_guide_candidate(Type)) Roughness = MaterialTexturableValue(S, Material, pt_guide_roughness_word(Type), UV);
        if (!pt_guide_followed(Type, Roughness, b, max_bounces)) {
            pt3 A = XYZToSRGB(MaterialBaseColor(S, Tb, Material, UV));
            rec[0] = make_float4(Nq.x, Nq.y, Nq.z, total);
            rec[1] = make_float4(A.x, A.y, A.z, __uint_as_float(pt_guide_shape_word(tag, Ln.Shape)));
            return;
        }
        tag = pt_guide_tag(tag, Ln.Shape);
        const pt3 TXq = UnpackUnitVector(PackUnitVector(TX));
        const pt3 W = pt_guide_direction(Type, MFloat(S, Material, PT_BASIC_TRANSLUCENT_IOR), Nq, TXq, V);
        pt_guide_restart(&O, &V, h.x, W);
    }
}

// A guide record as two float4: {normal, time}, {albedo, shape bits}.
// SPECULAR: the chain through mirrors and smooth glass (GuideChain); the plain
// instantiation holds no trace of it.
template <int CAP, bool SPECULAR = false>
__global__ __launch_bounds__(256) void guides_kernel(dscene S,
                                                     std::conditional_t<SPECULAR, guide_args_specular, guide_args> P,
                                                     uint32_t* spill, uint32_t spill_stride,
                                                     float4* __restrict__ out,
                                                     const observe_table* __restrict__ observe)
{
    __shared__ uint32_t smem[CAP * 256];
    const observe_table& Tb = *observe;
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    ray_source_guides src{&S, &P};
    uint32_t x, y;
    if (!src.pixel(i, x, y)) return;
    tstack<true, CAP> st;
    st.lds = &smem[threadIdx.x];
    st.spill = spill ? spill + i : nullptr;
    st.stride = spill_stride;

    pt3 O, V;
    float D;
    const bool known = src.load(i, O, V, D);
    if constexpr (SPECULAR) {
        GuideChain<CAP>(S, Tb, st, i, known, O, V, P.max_bounces, out + 2 * ((size_t)y * P.w + x));
        return;
    }
    lane_state Ln;
    LaneBegin(S, Ln, O, V, D);
    complexity_stats cx;
    if (known && S.g.ShapeCount != 0)
        while (!LaneStep<true, CAP>(S, Ln, st, src, i, cx)) {}

    size_t p = (size_t)y * P.w + x;
    if (Ln.Shape == SHAPE_INDEX_NONE) {
        pt3 A = v3s(0);
        if (known) A = XYZToSRGB(ObserveUnderD65(Tb, SampleSkyboxSpectrum(S, V)));
        out[2 * p] = make_float4(0, 0, 0, 0);
        out[2 * p + 1] = make_float4(A.x, A.y, A.z, __uint_as_float(0xFFFFFFFFu));
        return;
    }
    // The ptTraceRays record (finalize_kernel): compact hit -> attributes ->
    // {time, shape << 16 | material, packed normal}; the guide unpacks it.
    float4 h = CompactHit(Ln, S.vidx21 != 0);
    float2 c = make_float2(Ln.C.y, Ln.C.z);
    uint32_t Material;
    pt3 N, TX;
    pt2 UV;
    HitAttributesRecord(S, Ln.Shape, h, c, Material, N, TX, UV);
    uint32_t ShapeMaterial = (Ln.Shape << 16) | Material;
    pt3 Nq = UnpackUnitVector(PackUnitVector(N));
    pt3 A = XYZToSRGB(MaterialBaseColor(S, Tb, Material, UV));
    out[2 * p] = make_float4(Nq.x, Nq.y, Nq.z, h.x);
    out[2 * p + 1] = make_float4(A.x, A.y, A.z, __uint_as_float(ShapeMaterial >> 16));
}

// --- filter ---------------------------------------------------------------------

// The geometry of one iteration, shared by the single-buffer and the pair filter.
struct filter_grid {
    uint32_t w, h;
    uint32_t step;
    // lattice variant: residue classes and 16x16 lattice tiles per class
    uint32_t ncx, ncy;
};

struct denoise_args : filter_grid {
    pt_denoise_sigmas sg;
};

struct pair_args : filter_grid {
    pt_denoise_pair_sigmas sg;
};

// FIRST: the input is the accumulator (XYZ sums, sample count); the filter's
// c_0 is formed on load.
template <bool FIRST>
PT_DEV float4 LoadColor(const float4* __restrict__ in, size_t i)
{
    float4 v = in[i];
    if (!FIRST) return v;
    if (v.w > 0.0f) return make_float4(v.x / v.w, v.y / v.w, v.z / v.w, 1.0f);
    return make_float4(0, 0, 0, 0);
}

PT_DEV pt_denoise_pixel MakePixel(float4 c, float4 ga, float4 gb)
{
    pt_denoise_pixel p;
    p.c.x = c.x; p.c.y = c.y; p.c.z = c.z;
    p.n.x = ga.x; p.n.y = ga.y; p.n.z = ga.z;
    p.t = ga.w;
    p.a.x = gb.x; p.a.y = gb.y; p.a.z = gb.z;
    p.shape = __float_as_uint(gb.w);
    return p;
}

struct tap_sums { float x, y, z, w; };

// One tap that lies inside the image: skipped when empty or of another shape.
PT_DEV void Tap(tap_sums& A, const pt_denoise_pixel& p, float4 c, float4 ga, float4 gb, int dx, int dy,
                const pt_denoise_sigmas& sg)
{
    if (!(c.w > 0.0f) || __float_as_uint(gb.w) != p.shape) return;
    pt_denoise_pixel q = MakePixel(c, ga, gb);
    float hk = pt_denoise_k(dx + 2) * pt_denoise_k(dy + 2);
    float w = pt_denoise_weight(hk, &p, &q, &sg);
    A.x = A.x + w * q.c.x;
    A.y = A.y + w * q.c.y;
    A.z = A.z + w * q.c.z;
    A.w = A.w + w;
}

// LDS window: 20 rows of 20 records in three 16-B arrays (colour, {normal,
// time}, {albedo, shape}), row stride 32 records = 512 B.  A wave reads 4
// window rows x 16 consecutive records per tap with ds_read_b128, whose
// 16-lane groups each take 8 + 4 + 4 lanes of two neighbouring rows; a row
// stride that is a multiple of the 256-B bank row puts those pieces on
// disjoint 16-B slots (a packed 320-B stride would overlap them).
constexpr uint32_t DN_WIN = 20;
constexpr uint32_t DN_ROW = 32;

// The block of the lattice variant: tile (tile_x, tile_y) of the residue
// class (rx, ry).  Neighbouring blocks take neighbouring residues of the same
// lattice tile: their strided window loads share cache lines.
struct lattice_block {
    uint32_t tile_x, tile_y, rx, ry;
    PT_DEV explicit lattice_block(const filter_grid& P)
    {
        tile_x = blockIdx.x / P.ncx; rx = blockIdx.x - tile_x * P.ncx;
        tile_y = blockIdx.y / P.ncy; ry = blockIdx.y - tile_y * P.ncy;
    }
    // Window record r (row-major over DN_WIN x DN_WIN): its LDS slot, and its
    // pixel index when it lies inside the image.
    PT_DEV bool record(const filter_grid& P, uint32_t r, uint32_t& slot, size_t& iq) const
    {
        const uint32_t wy = r / DN_WIN, wx = r - wy * DN_WIN;
        slot = wy * DN_ROW + wx;
        // lattice coordinates of the record; the window starts 2 before the tile
        const int64_t lx = (int64_t)(tile_x * 16 + wx) - 2, ly = (int64_t)(tile_y * 16 + wy) - 2;
        const int64_t qx = (int64_t)rx + lx * (int64_t)P.step, qy = (int64_t)ry + ly * (int64_t)P.step;
        if (!(lx >= 0 && ly >= 0 && qx < (int64_t)P.w && qy < (int64_t)P.h)) return false;
        iq = (size_t)qy * P.w + (size_t)qx;
        return true;
    }
    // The thread's own pixel: its LDS slot, and its index when inside the image.
    PT_DEV bool pixel(const filter_grid& P, uint32_t& slot, size_t& ip) const
    {
        const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
        slot = (ty + 2) * DN_ROW + tx + 2;
        const uint64_t x = (uint64_t)rx + (uint64_t)(tile_x * 16 + tx) * P.step;
        const uint64_t y = (uint64_t)ry + (uint64_t)(tile_y * 16 + ty) * P.step;
        if (x >= P.w || y >= P.h) return false;
        ip = (size_t)y * P.w + (size_t)x;
        return true;
    }
};

// Iterations = 0: the accumulator's mean, .w = 1 (0, 0, 0, 0 where empty).
__global__ __launch_bounds__(256) void denoise_mean_kernel(const float4* __restrict__ accum, uint32_t n,
                                                           float4* __restrict__ out)
{
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = LoadColor<true>(accum, i);
}

// --- the variance-guided filter over two half renders --------
//
// Working image between the launches: one float4 {c.xyz, v} per pixel, v the
// variance of the pixel's luminance.  v is never negative (a square, or sums
// of products of squares and non-negative weights, or NaN), so an empty pixel
// is marked by .w = -1 and a pixel is filled iff !(.w < 0).  The last launch
// writes the sample-buffer form instead: .w = 1, or 0, 0, 0, 0 where empty.

PT_DEV float4 PairEmpty(bool final) { return make_float4(0, 0, 0, final ? 0.0f : -1.0f); }

// The working record of pixel i before the prefilter: {c_0, raw variance}.
PT_DEV float4 PairBegin(const float4* __restrict__ A, const float4* __restrict__ B, size_t i)
{
    const float4 a = A[i], b = B[i];
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    const pt_denoise_pair_start s = pt_denoise_pair_begin(av, bv);
    if (!s.filled) return PairEmpty(false);
    return make_float4(s.c.x, s.c.y, s.c.z, s.v);
}

// Prepare: c_0 and the 3x3-prefiltered variance v_0.  The block stages the
// 18x18 records around its 16x16 pixels in LDS, so the divisions behind a
// pixel's c_0 and raw variance are done once (1.27 x per pixel with the halo)
// and not once per tap (9 x), and A and B are read once; row stride as below.
// FINAL (Iterations = 0): c_0 straight in the sample-buffer form, no prefilter.
constexpr uint32_t PP_WIN = 18;
constexpr uint32_t PP_ROW = 32;

template <bool FINAL>
__global__ __launch_bounds__(256) void denoise_pair_prepare_kernel(const float4* __restrict__ A,
                                                                   const float4* __restrict__ B,
                                                                   const float4* __restrict__ guides, uint32_t w,
                                                                   uint32_t h, float4* __restrict__ out)
{
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t x = blockIdx.x * 16 + tx, y = blockIdx.y * 16 + ty;
    if constexpr (FINAL) {
        if (x >= w || y >= h) return;
        const size_t ip = (size_t)y * w + x;
        const float4 c = PairBegin(A, B, ip);
        out[ip] = c.w < 0.0f ? PairEmpty(true) : make_float4(c.x, c.y, c.z, 1.0f);
    } else {
        __shared__ float4 sc[PP_WIN * PP_ROW];
        __shared__ uint32_t ss[PP_WIN * PP_ROW];
        for (uint32_t r = threadIdx.x; r < PP_WIN * PP_WIN; r += 256) {
            const uint32_t wy = r / PP_WIN, wx = r - wy * PP_WIN;
            const int64_t qx = (int64_t)(blockIdx.x * 16 + wx) - 1, qy = (int64_t)(blockIdx.y * 16 + wy) - 1;
            float4 c = PairEmpty(false);       // outside the image: skipped like an empty pixel
            uint32_t shape = 0;
            if (qx >= 0 && qy >= 0 && qx < (int64_t)w && qy < (int64_t)h) {
                const size_t iq = (size_t)qy * w + (size_t)qx;
                c = PairBegin(A, B, iq);
                shape = __float_as_uint(guides[2 * iq + 1].w);
            }
            sc[wy * PP_ROW + wx] = c;
            ss[wy * PP_ROW + wx] = shape;
        }
        __syncthreads();
        if (x >= w || y >= h) return;
        const size_t ip = (size_t)y * w + x;
        const uint32_t ic = (ty + 1) * PP_ROW + tx + 1;
        const float4 cp = sc[ic];
        if (cp.w < 0.0f) { out[ip] = PairEmpty(false); return; }
        const uint32_t shape = ss[ic];
        float sv = 0.0f, sk = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const uint32_t iq = (uint32_t)((int)ic + dy * (int)PP_ROW + dx);
                const float v = sc[iq].w;
                if (v < 0.0f || ss[iq] != shape) continue;
                const float k = pt_denoise_k3(dx + 1) * pt_denoise_k3(dy + 1);
                sv = sv + k * v;
                sk = sk + k;
            }
        }
        out[ip] = make_float4(cp.x, cp.y, cp.z, sv / sk);
    }
}

struct pair_sums { float x, y, z, w, v; };

// One tap that lies inside the image: skipped when empty or of another shape.
PT_DEV void PairTap(pair_sums& A, const pt_denoise_pixel& p, float D, float4 c, float4 ga, float4 gb, int dx, int dy,
                    const pt_denoise_pair_sigmas& sg)
{
    if (c.w < 0.0f || __float_as_uint(gb.w) != p.shape) return;
    pt_denoise_pixel q = MakePixel(c, ga, gb);
    float hk = pt_denoise_k(dx + 2) * pt_denoise_k(dy + 2);
    float w = pt_denoise_pair_weight(hk, &p, &q, D, &sg);
    A.x = A.x + w * q.c.x;
    A.y = A.y + w * q.c.y;
    A.z = A.z + w * q.c.z;
    A.w = A.w + w;
    A.v = A.v + (w * w) * c.w;
}

template <bool LAST>
PT_DEV float4 PairResult(const pair_sums& A)
{
    return make_float4(A.x / A.w, A.y / A.w, A.z / A.w, LAST ? 1.0f : A.v / (A.w * A.w));
}

// --- the two filters as policies, and the two kernels over them --------------------
//
// A policy F gives: args (a filter_grid with the filter's sigmas), sums and
// centre (the running sums, and what is set up once per centre pixel); load
// (an image record as the taps see it); outside (the record stored for a
// window slot outside the image, which the tap skips like an empty pixel);
// empty / empty_result (the test on a centre record, and what an empty centre
// writes); setup, tap and result.  Everything is static and inlined: a kernel
// instantiation holds no trace of the other filter.

// FIRST: iteration 0, which reads the accumulator.
template <bool FIRST>
struct single_filter {
    using args = denoise_args;
    using sums = tap_sums;
    struct centre {};
    static PT_DEV float4 load(const float4* __restrict__ in, size_t i) { return LoadColor<FIRST>(in, i); }
    static PT_DEV float4 outside() { return make_float4(0, 0, 0, 0); }
    static PT_DEV bool empty(float4 c) { return !(c.w > 0.0f); }
    static PT_DEV float4 empty_result() { return make_float4(0, 0, 0, 0); }
    static PT_DEV centre setup(const args&, float4) { return {}; }
    static PT_DEV void tap(sums& A, const pt_denoise_pixel& p, centre, float4 c, float4 ga, float4 gb, int dx, int dy,
                           const args& P)
    {
        Tap(A, p, c, ga, gb, dx, dy, P.sg);
    }
    static PT_DEV float4 result(const sums& A) { return make_float4(A.x / A.w, A.y / A.w, A.z / A.w, 1.0f); }
};

// LAST: the last iteration, which writes the sample-buffer form.  The
// variance rides in the colour record's .w, so the lattice kernel's LDS
// footprint is the single filter's.
template <bool LAST>
struct pair_filter {
    using args = pair_args;
    using sums = pair_sums;
    using centre = float;       // D, the centre's luminance scale
    static PT_DEV float4 load(const float4* __restrict__ in, size_t i) { return in[i]; }
    static PT_DEV float4 outside() { return PairEmpty(false); }
    static PT_DEV bool empty(float4 c) { return c.w < 0.0f; }
    static PT_DEV float4 empty_result() { return PairEmpty(LAST); }
    static PT_DEV centre setup(const args& P, float4 cp) { return pt_denoise_pair_scale(&P.sg, cp.w); }
    static PT_DEV void tap(sums& A, const pt_denoise_pixel& p, centre D, float4 c, float4 ga, float4 gb, int dx, int dy,
                           const args& P)
    {
        PairTap(A, p, D, c, ga, gb, dx, dy, P.sg);
    }
    static PT_DEV float4 result(const sums& A) { return PairResult<LAST>(A); }
};

template <class F>
__global__ __launch_bounds__(256) void filter_gather_kernel(const float4* __restrict__ in,
                                                            const float4* __restrict__ guides, typename F::args P,
                                                            float4* __restrict__ out)
{
    const uint32_t x = blockIdx.x * 16 + (threadIdx.x & 15u), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= P.w || y >= P.h) return;
    const size_t ip = (size_t)y * P.w + x;
    const float4 cp = F::load(in, ip);
    if (F::empty(cp)) { out[ip] = F::empty_result(); return; }
    const pt_denoise_pixel p = MakePixel(cp, guides[2 * ip], guides[2 * ip + 1]);
    const typename F::centre C = F::setup(P, cp);
    typename F::sums A{};
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)P.step;
        if (qy < 0 || qy >= (int64_t)P.h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)P.step;
            if (qx < 0 || qx >= (int64_t)P.w) continue;
            const size_t iq = (size_t)qy * P.w + (size_t)qx;
            F::tap(A, p, C, F::load(in, iq), guides[2 * iq], guides[2 * iq + 1], dx, dy, P);
        }
    }
    out[ip] = F::result(A);
}

template <class F>
__global__ __launch_bounds__(256) void filter_lattice_kernel(const float4* __restrict__ in,
                                                             const float4* __restrict__ guides, typename F::args P,
                                                             float4* __restrict__ out)
{
    __shared__ float4 sc[DN_WIN * DN_ROW], sa[DN_WIN * DN_ROW], sb[DN_WIN * DN_ROW];
    const lattice_block blk(P);
    for (uint32_t r = threadIdx.x; r < DN_WIN * DN_WIN; r += 256) {
        uint32_t slot;
        size_t iq;
        float4 c = F::outside(), ga = make_float4(0, 0, 0, 0), gb = ga;
        if (blk.record(P, r, slot, iq)) {
            c = F::load(in, iq);
            ga = guides[2 * iq];
            gb = guides[2 * iq + 1];
        }
        sc[slot] = c;
        sa[slot] = ga;
        sb[slot] = gb;
    }
    __syncthreads();
    uint32_t ic;
    size_t ip;
    if (!blk.pixel(P, ic, ip)) return;
    const float4 cp = sc[ic];
    if (F::empty(cp)) { out[ip] = F::empty_result(); return; }
    const pt_denoise_pixel p = MakePixel(cp, sa[ic], sb[ic]);
    const typename F::centre C = F::setup(P, cp);
    typename F::sums A{};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const uint32_t iq = (uint32_t)((int)ic + dy * (int)DN_ROW + dx);
            F::tap(A, p, C, sc[iq], sa[iq], sb[iq], dx, dy, P);
        }
    }
    out[ip] = F::result(A);
}

}  // namespace ptd

uint32_t pt_guides_stack_cap() { return 20; }

hipError_t pt_launch_denoise_guides(const ptd::dscene& S, uint32_t camera_index, uint32_t w, uint32_t h,
                                    uint32_t* spill, float4* guides, const float* observe_table, hipStream_t st)
{
    ptd::guide_args P;
    P.camera = camera_index;
    P.w = w;
    P.h = h;
    P.tiles_x = (w + 15) / 16;
    uint32_t tiles = P.tiles_x * ((h + 15) / 16);
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::guides_kernel<20>, dim3(tiles), dim3(256), 0, st, S, P, spill, tiles * 256, guides,
                       reinterpret_cast<const ptd::observe_table*>(observe_table));
    return hipGetLastError();
}

hipError_t pt_launch_denoise_guides_specular(const ptd::dscene& S, uint32_t camera_index, uint32_t max_bounces,
                                             uint32_t w, uint32_t h, uint32_t* spill, float4* guides,
                                             const float* observe_table, hipStream_t st)
{
    if (max_bounces > PT_GUIDE_MAX_BOUNCES) return hipErrorInvalidValue;
    ptd::guide_args_specular P;
    P.camera = camera_index;
    P.w = w;
    P.h = h;
    P.tiles_x = (w + 15) / 16;
    P.max_bounces = max_bounces;
    uint32_t tiles = P.tiles_x * ((h + 15) / 16);
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL((ptd::guides_kernel<20, true>), dim3(tiles), dim3(256), 0, st, S, P, spill, tiles * 256, guides,
                       reinterpret_cast<const ptd::observe_table*>(observe_table));
    return hipGetLastError();
}

// Iteration `iteration`'s geometry and the launch grid of its kernel variant.
static dim3 FilterGrid(ptd::filter_grid& P, uint32_t w, uint32_t h, uint32_t iteration, bool lattice)
{
    P.w = w;
    P.h = h;
    P.step = 1u << iteration;
    P.ncx = P.step < w ? P.step : w;
    P.ncy = P.step < h ? P.step : h;
    if (!lattice) return dim3((w + 15) / 16, (h + 15) / 16);
    // 16x16 lattice tiles of the largest residue class (rx = ry = 0); the
    // smaller classes leave their last tiles partly or wholly idle.
    uint32_t lw = (w + P.step - 1) / P.step, lh = (h + P.step - 1) / P.step;
    return dim3(P.ncx * ((lw + 15) / 16), P.ncy * ((lh + 15) / 16));
}

// One iteration of filter F<flag>: P holds the sigmas already; the geometry
// and the kernel of the memory strategy are chosen here.
template <template <bool> class F>
static hipError_t LaunchFilter(const float4* in, const float4* guides, typename F<true>::args& P, uint32_t w,
                               uint32_t h, uint32_t iteration, bool flag, bool lattice, float4* out, hipStream_t st)
{
    if (w == 0 || h == 0) return hipSuccess;
    const dim3 grid = FilterGrid(P, w, h, iteration, lattice);
    void (*kernel)(const float4*, const float4*, typename F<true>::args, float4*) =
        lattice ? (flag ? ptd::filter_lattice_kernel<F<true>> : ptd::filter_lattice_kernel<F<false>>)
                : (flag ? ptd::filter_gather_kernel<F<true>> : ptd::filter_gather_kernel<F<false>>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, in, guides, P, out);
    return hipGetLastError();
}

hipError_t pt_launch_denoise(const float4* in, bool accumulator, const float4* guides, uint32_t w, uint32_t h,
                             const pt_denoise_parameters* p, uint32_t iteration, bool lattice, float4* out,
                             hipStream_t st)
{
    ptd::denoise_args P;
    P.sg = pt_denoise_iteration_sigmas(p, iteration);
    return LaunchFilter<ptd::single_filter>(in, guides, P, w, h, iteration, accumulator, lattice, out, st);
}

hipError_t pt_launch_denoise_mean(const float4* accum, uint32_t n, float4* out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ptd::denoise_mean_kernel, dim3((n + 255) / 256), dim3(256), 0, st, accum, n, out);
    return hipGetLastError();
}

hipError_t pt_launch_denoise_pair_prepare(const float4* a, const float4* b, const float4* guides, uint32_t w,
                                          uint32_t h, bool final, float4* out, hipStream_t st)
{
    if (w == 0 || h == 0) return hipSuccess;
    dim3 grid((w + 15) / 16, (h + 15) / 16);
    if (final) hipLaunchKernelGGL(ptd::denoise_pair_prepare_kernel<true>, grid, dim3(256), 0, st, a, b, guides, w, h, out);
    else hipLaunchKernelGGL(ptd::denoise_pair_prepare_kernel<false>, grid, dim3(256), 0, st, a, b, guides, w, h, out);
    return hipGetLastError();
}

hipError_t pt_launch_denoise_pair(const float4* in, const float4* guides, uint32_t w, uint32_t h,
                                  const pt_denoise_pair_parameters* p, uint32_t iteration, bool last, bool lattice,
                                  float4* out, hipStream_t st)
{
    ptd::pair_args P;
    P.sg = pt_denoise_pair_make_sigmas(p);
    return LaunchFilter<ptd::pair_filter>(in, guides, P, w, h, iteration, last, lattice, out, st);
}
