// denoise.cpp — ptsDenoise (include/pt_scene.h): the edge-avoiding a-trous
// filter of DESIGN.md §6 on the host.  The CPU path for saved accumulators
// and the second implementation the device kernels (csrc/hip/denoise.hip) are
// compared with: the same definition, the same per-tap arithmetic
// (include/pt_denoise.h), the same tap order.  Single-threaded.
// ptsDenoisePair is the same for the variance-guided filter over two half
// renders and ptDenoiseSampleBufferPair.  The 5x5 loop
// is one template; the two filters are its policies, as on the device.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_denoise.h"

#include <cstring>
#include <new>
#include <vector>

namespace {

struct px4 { float x, y, z, w; };   // w: 1 = pixel has a colour, 0 = empty

pt_denoise_pixel Pixel(const px4& c, const pt_denoise_guide& g)
{
    pt_denoise_pixel p;
    p.c = {c.x, c.y, c.z};
    p.n = {g.normal[0], g.normal[1], g.normal[2]};
    p.t = g.time;
    p.a = {g.albedo[0], g.albedo[1], g.albedo[2]};
    p.shape = g.shape;
    return p;
}

struct pair_px { float x, y, z, v; bool filled; };   // colour, variance of its luminance

// The two filters as policies of the one loop below: the image record (px),
// whether it is empty, its colour, what is set up once per centre pixel, and
// what a tap adds to the sums.
struct single_filter {
    using px = px4;
    using sigmas = pt_denoise_sigmas;
    struct sums { float x, y, z, w; };
    static bool empty(const px& c) { return !(c.w > 0.0f); }
    static px empty_px() { return {0, 0, 0, 0}; }
    static px4 colour(const px& c) { return c; }
    static float setup(const sigmas&, const px&) { return 0.0f; }
    static void tap(sums& A, float h, const pt_denoise_pixel& p, const pt_denoise_pixel& q, float, const px&,
                    const sigmas& sg)
    {
        const float w = pt_denoise_weight(h, &p, &q, &sg);
        A.x = A.x + w * q.c.x;
        A.y = A.y + w * q.c.y;
        A.z = A.z + w * q.c.z;
        A.w = A.w + w;
    }
    static px result(const sums& A) { return {A.x / A.w, A.y / A.w, A.z / A.w, 1.0f}; }
};

// The variance-guided filter over two half renders.
struct pair_filter {
    using px = pair_px;
    using sigmas = pt_denoise_pair_sigmas;
    struct sums { float x, y, z, w, v; };
    static bool empty(const px& c) { return !c.filled; }
    static px empty_px() { return {0, 0, 0, 0, false}; }
    static px4 colour(const px& c) { return {c.x, c.y, c.z, 1.0f}; }
    static float setup(const sigmas& sg, const px& c) { return pt_denoise_pair_scale(&sg, c.v); }
    static void tap(sums& A, float h, const pt_denoise_pixel& p, const pt_denoise_pixel& q, float D, const px& c,
                    const sigmas& sg)
    {
        const float w = pt_denoise_pair_weight(h, &p, &q, D, &sg);
        A.x = A.x + w * q.c.x;
        A.y = A.y + w * q.c.y;
        A.z = A.z + w * q.c.z;
        A.w = A.w + w;
        A.v = A.v + (w * w) * c.v;
    }
    static px result(const sums& A) { return {A.x / A.w, A.y / A.w, A.z / A.w, A.v / (A.w * A.w), true}; }
};

// One a-trous iteration of filter F, in -> out.
template <class F>
void Iterate(uint32_t W, uint32_t H, const typename F::px* in, const pt_denoise_guide* guides,
             const typename F::sigmas& sg, uint32_t step, typename F::px* out)
{
    for (uint32_t y = 0; y < H; y++) {
        for (uint32_t x = 0; x < W; x++) {
            const size_t ip = (size_t)y * W + x;
            if (F::empty(in[ip])) { out[ip] = F::empty_px(); continue; }
            const pt_denoise_pixel p = Pixel(F::colour(in[ip]), guides[ip]);
            const float C = F::setup(sg, in[ip]);
            typename F::sums A{};
            for (int dy = -2; dy <= 2; dy++) {
                const int64_t qy = (int64_t)y + (int64_t)dy * step;
                if (qy < 0 || qy >= (int64_t)H) continue;
                for (int dx = -2; dx <= 2; dx++) {
                    const int64_t qx = (int64_t)x + (int64_t)dx * step;
                    if (qx < 0 || qx >= (int64_t)W) continue;
                    const size_t iq = (size_t)qy * W + (size_t)qx;
                    if (F::empty(in[iq]) || guides[iq].shape != p.shape) continue;
                    const pt_denoise_pixel q = Pixel(F::colour(in[iq]), guides[iq]);
                    const float h = pt_denoise_k(dx + 2) * pt_denoise_k(dy + 2);
                    F::tap(A, h, p, q, C, in[iq], sg);
                }
            }
            out[ip] = F::result(A);
        }
    }
}

// c_0 and the prefiltered variance v_0 of S = A + B.
void PairPrepare(uint32_t W, uint32_t H, const float* A, const float* B, const pt_denoise_guide* guides, pair_px* out)
{
    const size_t n = (size_t)W * H;
    std::vector<float> raw(n);
    for (size_t i = 0; i < n; i++) {
        const pt_denoise_pair_start s = pt_denoise_pair_begin(A + 4 * i, B + 4 * i);
        out[i] = {s.c.x, s.c.y, s.c.z, 0.0f, s.filled != 0};
        raw[i] = s.v;
    }
    for (uint32_t y = 0; y < H; y++) {
        for (uint32_t x = 0; x < W; x++) {
            const size_t ip = (size_t)y * W + x;
            if (!out[ip].filled) continue;
            float sv = 0.0f, sk = 0.0f;
            for (int dy = -1; dy <= 1; dy++) {
                const int64_t qy = (int64_t)y + dy;
                if (qy < 0 || qy >= (int64_t)H) continue;
                for (int dx = -1; dx <= 1; dx++) {
                    const int64_t qx = (int64_t)x + dx;
                    if (qx < 0 || qx >= (int64_t)W) continue;
                    const size_t iq = (size_t)qy * W + (size_t)qx;
                    if (!out[iq].filled || guides[iq].shape != guides[ip].shape) continue;
                    const float k = pt_denoise_k3(dx + 1) * pt_denoise_k3(dy + 1);
                    sv = sv + k * raw[iq];
                    sk = sk + k;
                }
            }
            out[ip].v = sv / sk;
        }
    }
}

}  // namespace

extern "C" int ptsDenoisePair(uint32_t width, uint32_t height, const float* accum_a, const float* accum_b,
                              const pt_denoise_guide* guides, const pt_denoise_pair_parameters* params,
                              float* out_rgba)
{
    if (!accum_a || !accum_b || !guides || !params || !out_rgba || width == 0 || height == 0) return -1;
    if (accum_a == accum_b) return -1;
    if (!pt_denoise_pair_parameters_ok(params)) return -1;
    const size_t n = (size_t)width * height;
    try {
        std::vector<pair_px> a(n), b(params->Iterations ? n : 0);
        PairPrepare(width, height, accum_a, accum_b, guides, a.data());
        const pt_denoise_pair_sigmas sg = pt_denoise_pair_make_sigmas(params);
        for (uint32_t i = 0; i < params->Iterations; i++) {
            Iterate<pair_filter>(width, height, a.data(), guides, sg, 1u << i, b.data());
            a.swap(b);
        }
        for (size_t i = 0; i < n; i++) {
            float* o = out_rgba + 4 * i;
            if (a[i].filled) { o[0] = a[i].x; o[1] = a[i].y; o[2] = a[i].z; o[3] = 1.0f; }
            else { o[0] = o[1] = o[2] = o[3] = 0.0f; }
        }
    } catch (const std::bad_alloc&) {
        return -2;
    }
    return 0;
}

extern "C" int ptsDenoise(uint32_t width, uint32_t height, const float* accum_rgba, const pt_denoise_guide* guides,
                          const pt_denoise_parameters* params, float* out_rgba)
{
    if (!accum_rgba || !guides || !params || !out_rgba || width == 0 || height == 0) return -1;
    if (!pt_denoise_parameters_ok(params)) return -1;
    const size_t n = (size_t)width * height;
    try {
        std::vector<px4> a(n), b(params->Iterations ? n : 0);
        for (size_t i = 0; i < n; i++) {
            const float* s = accum_rgba + 4 * i;
            if (s[3] > 0.0f) a[i] = {s[0] / s[3], s[1] / s[3], s[2] / s[3], 1.0f};
            else a[i] = {0, 0, 0, 0};
        }
        for (uint32_t i = 0; i < params->Iterations; i++) {
            Iterate<single_filter>(width, height, a.data(), guides, pt_denoise_iteration_sigmas(params, i), 1u << i,
                                   b.data());
            a.swap(b);
        }
        std::memcpy(out_rgba, a.data(), n * sizeof(px4));
    } catch (const std::bad_alloc&) {
        return -2;
    }
    return 0;
}
