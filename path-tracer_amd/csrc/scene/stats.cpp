// stats.cpp — ptsFrameStatistics (include/pt_scene.h): the frame statistics
// of DESIGN.md §6 row 6 on the host.  The CPU path for saved accumulators and
// the second implementation the device kernel (csrc/hip/stats.hip) is
// compared with: the same classes, bins and pair rule (include/pt_stats.h).
// The ptsStats* functions export pt_stats.h's double helpers to callers that
// cannot include the header (the Python mirror).  Single-threaded.
#include "../../../include/pt_scene.h"
#include "../../../include/pt_stats.h"

#include <cstring>

namespace {

struct px4 { float x, y, z, w; };

}  // namespace

extern "C" int ptsFrameStatistics(uint32_t width, uint32_t height, const float* accum_a, const float* accum_b,
                                  pt_frame_statistics* out)
{
    if (!accum_a || !out || width == 0 || height == 0 || accum_a == accum_b) return -1;
    const size_t n = (size_t)width * height;
    const px4* A = reinterpret_cast<const px4*>(accum_a);
    const px4* B = reinterpret_cast<const px4*>(accum_b);
    pt_frame_statistics s;
    std::memset(&s, 0, sizeof(s));
    s.pixels = n;
    uint32_t min_y = 0xFFFFFFFFu, max_y = 0, min_w = 0xFFFFFFFFu, max_w = 0;
    for (size_t i = 0; i < n; i++) {
        px4 p = A[i];
        if (B) {
            const px4 a = A[i], b = B[i];
            p = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
            float Ya = 0.0f, Yb = 0.0f, r = 0.0f;
            if (pt_stats_classify(a.x, a.y, a.z, a.w, &Ya) == PT_STATS_FILLED &&
                pt_stats_classify(b.x, b.y, b.z, b.w, &Yb) == PT_STATS_FILLED) {
                if (pt_stats_pair_noise(Ya, Yb, &r)) {
                    s.noise_pixels++;
                    s.noise_histogram[pt_stats_bin(r)]++;
                } else {
                    s.noise_skipped++;
                }
            }
        }
        float Y = 0.0f;
        switch (pt_stats_classify(p.x, p.y, p.z, p.w, &Y)) {
        case PT_STATS_NONFINITE: s.nonfinite++; break;
        case PT_STATS_EMPTY: s.empty++; break;
        default:
            s.filled++;
            // Positive floats order as their bit patterns.
            min_w = pt_umin(min_w, pt_f2u(p.w));
            max_w = max_w > pt_f2u(p.w) ? max_w : pt_f2u(p.w);
            if (Y > 0.0f) {
                s.luminance_histogram[pt_stats_bin(Y)]++;
                min_y = pt_umin(min_y, pt_f2u(Y));
                max_y = max_y > pt_f2u(Y) ? max_y : pt_f2u(Y);
            } else {
                s.dark++;
            }
        }
    }
    if (max_y) { s.min_luminance = pt_u2f(min_y); s.max_luminance = pt_u2f(max_y); }
    if (max_w) { s.min_samples = pt_u2f(min_w); s.max_samples = pt_u2f(max_w); }
    *out = s;
    return 0;
}

// Per-tile statistics: the pixel rule is pt_stats.h's
// pt_tile_stats_pixel, shared with the device kernel.
extern "C" int ptsTileStatistics(uint32_t width, uint32_t height, const float* accum_a, const float* accum_b,
                                 float noise_threshold, pt_tile_statistics* out)
{
    if (!accum_a || !out || width == 0 || height == 0 || accum_a == accum_b) return -1;
    if (!pt_tile_stats_threshold_ok(noise_threshold)) return -1;
    const uint32_t tiles_x = (width + PT_TILE_SIZE - 1) / PT_TILE_SIZE, tiles_y = (height + PT_TILE_SIZE - 1) / PT_TILE_SIZE;
    for (uint32_t ty = 0; ty < tiles_y; ty++) {
        for (uint32_t tx = 0; tx < tiles_x; tx++) {
            pt_tile_statistics s;
            std::memset(&s, 0, sizeof(s));
            uint32_t min_w = 0xFFFFFFFFu, max_w = 0;
            const uint32_t x1 = pt_umin(width, (tx + 1) * PT_TILE_SIZE), y1 = pt_umin(height, (ty + 1) * PT_TILE_SIZE);
            for (uint32_t y = ty * PT_TILE_SIZE; y < y1; y++) {
                for (uint32_t x = tx * PT_TILE_SIZE; x < x1; x++) {
                    const size_t i = ((size_t)y * width + x) * 4;
                    uint32_t wb = 0;
                    const uint32_t f = pt_tile_stats_pixel(accum_a + i, accum_b ? accum_b + i : accum_a + i,
                                                           accum_b != nullptr, noise_threshold, &wb);
                    s.filled += (f & PT_TILE_PX_FILLED) != 0;
                    s.empty += (f & PT_TILE_PX_EMPTY) != 0;
                    s.nonfinite += (f & PT_TILE_PX_NONFINITE) != 0;
                    s.pair += (f & PT_TILE_PX_PAIR) != 0;
                    s.over += (f & PT_TILE_PX_OVER) != 0;
                    if (f & PT_TILE_PX_FILLED) {
                        min_w = pt_umin(min_w, wb);
                        max_w = max_w > wb ? max_w : wb;
                    }
                }
            }
            if (s.filled) { s.min_count = pt_u2f(min_w); s.max_count = pt_u2f(max_w); }
            out[(size_t)ty * tiles_x + tx] = s;
        }
    }
    return 0;
}

extern "C" int ptsStatsBin(float v) { return pt_stats_bin(v); }
extern "C" double ptsStatsBinEdge(int bin) { return bin < 0 || bin > PT_STATS_BINS ? 0.0 : pt_stats_bin_edge(bin); }
extern "C" int ptsStatsPercentileBin(const uint32_t* histogram, double q)
{
    return histogram ? pt_stats_percentile_bin(histogram, q) : -1;
}
extern "C" double ptsStatsLogAverage(const uint32_t* histogram, double q_lo, double q_hi)
{
    return histogram ? pt_stats_log_average(histogram, q_lo, q_hi) : 0.0;
}
extern "C" double ptsStatsAutoBrightness(const pt_frame_statistics* stats, double key, double q_lo, double q_hi)
{
    return stats ? pt_stats_auto_brightness(stats, key, q_lo, q_hi) : 1.0;
}
extern "C" double ptsStatsNoise(const pt_frame_statistics* stats, double q)
{
    return stats ? pt_stats_noise(stats, q) : (double)INFINITY;
}
