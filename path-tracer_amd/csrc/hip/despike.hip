// despike.hip — the neighbourhood firefly clamp in front of the denoisers (no
// reference counterpart).  One 256-thread block per
// 16x16 tile, mapped as rectify_kernel maps pixels.  The block stages the
// (16 + 2R)^2 window records of its tile into LDS once (include/pt_despike.h's
// pt_despike_stage: the guide's normal, the shape word with "not a member
// whatever the centre" coded in it, and the value v = the largest component
// of Src.xyz / Src.w, divided and compared there, once per pixel), and after
// one barrier every thread walks its window once out of LDS in row-major
// order: membership from the staged normal and shape words, a non-member's
// value replaced by -inf, and a sorted insertion into four registers of which
// the Rank-th is read at the end.  The per-pixel and per-tap arithmetic is
// pt_despike.h's, shared with the host implementation (csrc/scene/despike.cpp).
// No atomics; one 16-byte store per pixel.
//
// LDS layout.  A tap needs five words.  Derived from the documented LDS rules,
// not measured against the alternatives:
//  * normal.xyz and the shape word are one 16-byte slot, read by one 16-byte
//    read, laid out as rectify.hip lays out its planes: DESPIKE_STRIDE = 32
//    slots to a row.  A 16-byte read is served in four groups of 16 lanes and
//    each group holds the tile's sixteen columns once over two adjacent rows;
//    a row stride that is a multiple of 16 slots (256 B, all 64 banks) puts
//    both rows' slots on the residues one row's would have: sixteen distinct
//    slots, every bank once, for any tap offset.  32 is the smallest such
//    stride that holds Radius 3's 22 columns.
//  * the value is a plane of 4-byte words of its own.  Packing all five words
//    into a 32-byte record costs a second 16-byte read per tap (4 + 4 LDS
//    cycles a wave against 4 + 2 here), and splitting them as 12 bytes of
//    normal beside 8 of shape and value is worse still: a 12-byte read runs
//    at half a 16-byte read's rate (8 cycles) before the second is counted.
//    A 4-byte read is served in two groups of 32 lanes, rows ty and ty + 1 of
//    the tile, over 32 banks.  Sixteen consecutive words of one row and
//    sixteen of the next fall on distinct banks when the row stride is 16
//    modulo 32 words; DESPIKE_VALUE_STRIDE = 48 is the smallest such stride
//    >= 22.  (32 words would put both rows of a group on the same banks,
//    two-way throughout; counted over 64 banks it is rows ty and ty + 2 that
//    meet, and 48 = 3 * 16 clears that reading as well: rows ty .. ty + 3
//    start at 0, 48, 32 and 16 modulo 64.)
// Radius is a template parameter: a window row unrolls into 2R + 1 pairs of
// reads at constant offsets that are in flight together, and the rows stay a
// loop (rectify.hip's header: unrolling them too lifts every read above its
// use and costs occupancy).
//
// A record outside the image is written without a global load.  A thread
// whose own pixel lies outside the image takes part in the staging, reaches
// the barrier, and stores nothing.  dst is never src (refused by the caller):
// another block's window reads the pixels this one stores.
#include "pt_device.hpp"
#include "kernels.hpp"
#include "../../../include/pt_despike.h"

namespace ptd {

constexpr uint32_t DESPIKE_STRIDE = 32;         // 16-byte slots per surface row: a multiple of 16, >= 16 + 2 * 3
constexpr uint32_t DESPIKE_VALUE_STRIDE = 48;   // words per value row: 16 modulo 32, >= 16 + 2 * 3

struct despike_args {
    pt_despike_parameters params;
    uint32_t w, h;
};

// A record read from LDS, pinned as four live registers at the point of the
// read.  Without it the compiler takes the 16-byte read apart (the normal is
// used only behind the shape test) and pairs the words again across records
// as 8-byte reads of two 4-byte halves, at a quarter of the rate.
__device__ __forceinline__ uint4 whole_record(uint4 v)
{
    asm("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
}

template <int R>
__global__ __launch_bounds__(256) void despike_kernel(const float4* __restrict__ src,
                                                      const float4* __restrict__ guides, despike_args P,
                                                      float4* __restrict__ out)
{
    constexpr uint32_t W = 16 + 2 * R;
    static_assert(R >= 1 && R <= PT_DESPIKE_MAX_RADIUS && W <= DESPIKE_STRIDE && W <= DESPIKE_VALUE_STRIDE, "window");
    // Bit patterns, not floats: the shape word travels untouched.
    __shared__ uint4 surface[W * DESPIKE_STRIDE];       // normal.xyz, member_shape
    __shared__ float value[W * DESPIKE_VALUE_STRIDE];   // v

    const int64_t ox = (int64_t)blockIdx.x * 16 - R, oy = (int64_t)blockIdx.y * 16 - R;
    for (uint32_t i = threadIdx.x; i < W * W; i += 256) {
        const uint32_t rx = i % W, ry = i / W;          // rx, ry < W: inside both planes
        const int64_t qx = ox + rx, qy = oy + ry;
        const int inside = qx >= 0 && qy >= 0 && qx < (int64_t)P.w && qy < (int64_t)P.h;
        float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        pt_denoise_guide g;
        g.normal[0] = 0.0f; g.normal[1] = 0.0f; g.normal[2] = 0.0f;
        g.shape = PT_SHAPE_INDEX_NONE;
        if (inside) {
            // 0 <= qx < w, 0 <= qy < h: inside src and guides.
            const size_t iq = (size_t)qy * P.w + (size_t)qx;
            const float4 v = src[iq], ga = guides[2 * iq];
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
            g.normal[0] = ga.x; g.normal[1] = ga.y; g.normal[2] = ga.z;
            g.shape = reinterpret_cast<const uint32_t*>(guides)[8 * iq + 7];
        }
        pt_despike_record r;
        pt_despike_stage(inside, c, &g, &r);
        surface[ry * DESPIKE_STRIDE + rx] = make_uint4(__float_as_uint(r.normal[0]), __float_as_uint(r.normal[1]),
                                                       __float_as_uint(r.normal[2]), r.member_shape);
        value[ry * DESPIKE_VALUE_STRIDE + rx] = r.v;
    }
    __syncthreads();

    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t x = blockIdx.x * 16 + tx, y = blockIdx.y * 16 + ty;
    if (x >= P.w || y >= P.h) return;
    const size_t ip = (size_t)y * P.w + x;
    const float4 sv = src[ip];
    const float S[4] = {sv.x, sv.y, sv.z, sv.w};

    // Tap (dy, dx) of this thread is surface slot first + dy * DESPIKE_STRIDE + dx
    // and value word vfirst + dy * DESPIKE_VALUE_STRIDE + dx: rows ty .. ty + 2R
    // < W, columns tx .. tx + 2R < W.
    const uint32_t first = ty * DESPIKE_STRIDE + tx, vfirst = ty * DESPIKE_VALUE_STRIDE + tx;
    const uint4 sc = surface[first + R * DESPIKE_STRIDE + R];
    const float cn[3] = {__uint_as_float(sc.x), __uint_as_float(sc.y), __uint_as_float(sc.z)};
    const uint32_t cshape = sc.w;
    const float cv = value[vfirst + R * DESPIKE_VALUE_STRIDE + R];

    pt_despike_top T;
    pt_despike_begin(&T);
#pragma unroll 1
    for (int dy = 0; dy <= 2 * R; dy++) {
        // A window row's reads first, so that they are in flight together.
        uint4 a[2 * R + 1];
        float v[2 * R + 1];
#pragma unroll
        for (int dx = 0; dx <= 2 * R; dx++) {
            a[dx] = whole_record(surface[first + dy * DESPIKE_STRIDE + dx]);
            v[dx] = value[vfirst + dy * DESPIKE_VALUE_STRIDE + dx];
        }
#pragma unroll
        for (int dx = 0; dx <= 2 * R; dx++) {
            const float qn[3] = {__uint_as_float(a[dx].x), __uint_as_float(a[dx].y), __uint_as_float(a[dx].z)};
            int member = pt_despike_member(&P.params, cshape, cn, a[dx].w, qn);
            if (dx == R) member = member && dy != R;        // the centre is no neighbour of itself
            pt_despike_insert(&T, member, v[dx]);
        }
    }
    float r[4];
    pt_despike_decide(&P.params, S, cv, &T, r);
    out[ip] = make_float4(r[0], r[1], r[2], r[3]);
}

}  // namespace ptd

hipError_t pt_launch_despike(const float4* src, const float4* guides, uint32_t w, uint32_t h,
                             const pt_despike_parameters* p, float4* out, hipStream_t st)
{
    if (w == 0 || h == 0) return hipSuccess;
    ptd::despike_args P;
    P.params = *p;
    P.w = w; P.h = h;
    const dim3 grid((w + 15) / 16, (h + 15) / 16), block(256);
    if (p->Radius == 1) hipLaunchKernelGGL(ptd::despike_kernel<1>, grid, block, 0, st, src, guides, P, out);
    else if (p->Radius == 2) hipLaunchKernelGGL(ptd::despike_kernel<2>, grid, block, 0, st, src, guides, P, out);
    else hipLaunchKernelGGL(ptd::despike_kernel<3>, grid, block, 0, st, src, guides, P, out);
    return hipGetLastError();
}
