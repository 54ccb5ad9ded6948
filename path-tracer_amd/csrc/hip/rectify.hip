// rectify.hip — validation of a carried history against the new frame's
// samples (no reference counterpart).  One 256-thread
// block per 16x16 tile, mapped as reproject_kernel and guides_kernel map
// pixels.  The block stages the (16 + 2R)^2 window records of its tile into
// LDS once (include/pt_rectify.h's pt_rectify_stage: the colour Cur.xyz /
// Cur.w divided there, the shape word, the normal; "not a member whatever the
// centre" coded in the shape word), and after one barrier every thread runs
// the definition's two window passes out of LDS, every tap a 16-byte read (the
// centre's own surface record, once per thread, is not one): the first
// decides membership, counts and sums, and keeps the membership as a bit
// mask; the second reads the colour half alone.  The per-pixel and per-tap
// arithmetic is pt_rectify.h's, shared with the host implementation
// (csrc/scene/rectify.cpp); taps run in row-major window order, sums left to
// right, no atomics, plain vector stores.
//
// LDS layout: a record's two 16-byte halves lie in two planes of 16-byte
// slots, RECTIFY_STRIDE = 32 slots to a row.  A 16-byte LDS read is served in
// four groups of 16 lanes, and each group holds the sixteen columns of the
// tile exactly once, spread over two adjacent rows (lanes 0-3, 12-15 of one
// row with 4-11 of the next, and so on).  With one slot per record in a plane
// the sixteen columns are sixteen consecutive slots, and with a row stride
// that is a multiple of 16 slots (256 B, one bank row) the second row's slots
// fall on the same residues as the first's would: sixteen distinct slots, all
// 64 banks once, no conflict for any tap offset.  The natural strides 18, 20
// and 22 put the second row 2, 4 or 6 slots off and make up to 6 of the 16
// lanes collide two-way; an interleaved 32-byte record would use every other
// slot and collide two-way everywhere.  32 is the smallest such stride that
// holds the 22 columns of Radius 3.  Radius is a template parameter: a
// window row unrolls into 2R + 1 reads at constant offsets that are in flight
// together, and the rows stay a loop.  Unrolling the rows as well lets the
// compiler lift all 49 reads of Radius 3 above their use: 215 VGPRs and two
// waves per SIMD, against the figures in DESIGN.md §6 row 11.
//
// A record outside the image is written without a global load.  A thread
// whose own pixel lies outside the image takes part in the staging, reaches
// the barrier, and stores nothing.  dst may be the history: a thread reads
// the history at its own pixel only, before it stores there.
#include "pt_device.hpp"
#include "kernels.hpp"
#include "../../../include/pt_rectify.h"

namespace ptd {

constexpr uint32_t RECTIFY_STRIDE = 32;     // 16-byte slots per LDS row: a multiple of 16, >= 16 + 2 * 3

struct rectify_args {
    pt_rectify_parameters params;
    uint32_t w, h;
};

template <int R>
__global__ __launch_bounds__(256) void rectify_kernel(const float4* hist, const float4* __restrict__ cur,
                                                      const float4* __restrict__ guides, rectify_args P, float4* out)
{
    constexpr uint32_t W = 16 + 2 * R;
    static_assert(R >= 1 && R <= PT_RECTIFY_MAX_RADIUS && W <= RECTIFY_STRIDE, "window");
    // Bit patterns, not floats: the shape words travel untouched.
    __shared__ uint4 colour[W * RECTIFY_STRIDE];    // c.xyz, member_shape
    __shared__ uint4 surface[W * RECTIFY_STRIDE];   // normal.xyz, shape

    const int64_t ox = (int64_t)blockIdx.x * 16 - R, oy = (int64_t)blockIdx.y * 16 - R;
    for (uint32_t i = threadIdx.x; i < W * W; i += 256) {
        const uint32_t rx = i % W, ry = i / W;          // rx, ry < W <= RECTIFY_STRIDE: inside both planes
        const int64_t qx = ox + rx, qy = oy + ry;
        const int inside = qx >= 0 && qy >= 0 && qx < (int64_t)P.w && qy < (int64_t)P.h;
        float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        pt_denoise_guide g;
        g.normal[0] = 0.0f; g.normal[1] = 0.0f; g.normal[2] = 0.0f;
        g.shape = PT_SHAPE_INDEX_NONE;
        if (inside) {
            // 0 <= qx < w, 0 <= qy < h: inside cur and guides.
            const size_t iq = (size_t)qy * P.w + (size_t)qx;
            const float4 v = cur[iq], ga = guides[2 * iq];
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
            g.normal[0] = ga.x; g.normal[1] = ga.y; g.normal[2] = ga.z;
            g.shape = reinterpret_cast<const uint32_t*>(guides)[8 * iq + 7];
        }
        pt_rectify_record r;
        pt_rectify_stage(inside, c, &g, &r);
        const uint32_t s = ry * RECTIFY_STRIDE + rx;
        colour[s] = make_uint4(__float_as_uint(r.c[0]), __float_as_uint(r.c[1]), __float_as_uint(r.c[2]),
                               r.member_shape);
        surface[s] = make_uint4(__float_as_uint(r.normal[0]), __float_as_uint(r.normal[1]),
                                __float_as_uint(r.normal[2]), r.shape);
    }
    __syncthreads();

    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t x = blockIdx.x * 16 + tx, y = blockIdx.y * 16 + ty;
    if (x >= P.w || y >= P.h) return;
    const size_t ip = (size_t)y * P.w + x;
    const float4 hv = hist[ip];
    const float H[4] = {hv.x, hv.y, hv.z, hv.w};

    // Tap (dy, dx) of this thread is slot first + dy * RECTIFY_STRIDE + dx:
    // rows ty .. ty + 2R < W, columns tx .. tx + 2R < W.
    const uint32_t first = ty * RECTIFY_STRIDE + tx;
    const uint4 sc = surface[first + R * RECTIFY_STRIDE + R];
    const float cn[3] = {__uint_as_float(sc.x), __uint_as_float(sc.y), __uint_as_float(sc.z)};
    const uint32_t cshape = sc.w;

    pt_rectify_sums A;
    pt_rectify_begin(&A);
    uint64_t members = 0;
#pragma unroll 1
    for (int dy = 0; dy <= 2 * R; dy++) {
        // A window row's reads first, so that they are in flight together.
        // A tap also looks at the surface half's shape word, which repeats
        // what the colour half's says of a pixel outside the image: that
        // keeps the read 16 bytes wide (a 12-byte LDS read runs at half the
        // rate of a 16-byte one).
        uint4 a[2 * R + 1], b[2 * R + 1];
#pragma unroll
        for (int dx = 0; dx <= 2 * R; dx++) {
            a[dx] = colour[first + dy * RECTIFY_STRIDE + dx];
            b[dx] = surface[first + dy * RECTIFY_STRIDE + dx];
        }
#pragma unroll
        for (int dx = 0; dx <= 2 * R; dx++) {
            const float qn[3] = {__uint_as_float(b[dx].x), __uint_as_float(b[dx].y), __uint_as_float(b[dx].z)};
            if (pt_rectify_member(&P.params, cshape, cn, a[dx].w, qn) && b[dx].w != PT_RECTIFY_NOT_A_MEMBER) {
                const float c[3] = {__uint_as_float(a[dx].x), __uint_as_float(a[dx].y), __uint_as_float(a[dx].z)};
                pt_rectify_add_colour(&A, c);
                members |= 1ull << (dy * (2 * R + 1) + dx);
            }
        }
    }
    float r[4];
    if (pt_rectify_tested(&P.params, H, A.m, r)) {
        float mu[3];
        pt_rectify_mean(&A, mu);
#pragma unroll 1
        for (int dy = 0; dy <= 2 * R; dy++) {
            uint4 a[2 * R + 1];
#pragma unroll
            for (int dx = 0; dx <= 2 * R; dx++) a[dx] = colour[first + dy * RECTIFY_STRIDE + dx];
#pragma unroll
            for (int dx = 0; dx <= 2 * R; dx++) {
                // A member's shape word is never the code; as above, for the read's width.
                if (!(members >> (dy * (2 * R + 1) + dx) & 1ull) || a[dx].w == PT_RECTIFY_NOT_A_MEMBER) continue;
                const float c[3] = {__uint_as_float(a[dx].x), __uint_as_float(a[dx].y), __uint_as_float(a[dx].z)};
                pt_rectify_add_deviation(&A, mu, c);
            }
        }
        pt_rectify_clip(&P.params, H, &A, mu, r);
    }
    out[ip] = make_float4(r[0], r[1], r[2], r[3]);
}

}  // namespace ptd

hipError_t pt_launch_rectify(const float4* hist, const float4* cur, const float4* guides, uint32_t w, uint32_t h,
                             const pt_rectify_parameters* p, float4* out, hipStream_t st)
{
    if (w == 0 || h == 0) return hipSuccess;
    ptd::rectify_args P;
    P.params = *p;
    P.w = w; P.h = h;
    const dim3 grid((w + 15) / 16, (h + 15) / 16), block(256);
    if (p->Radius == 1) hipLaunchKernelGGL(ptd::rectify_kernel<1>, grid, block, 0, st, hist, cur, guides, P, out);
    else if (p->Radius == 2) hipLaunchKernelGGL(ptd::rectify_kernel<2>, grid, block, 0, st, hist, cur, guides, P, out);
    else hipLaunchKernelGGL(ptd::rectify_kernel<3>, grid, block, 0, st, hist, cur, guides, P, out);
    return hipGetLastError();
}
