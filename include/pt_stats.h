/*
 * pt_stats.h — frame statistics: the pixel classes and
 * the histogram binning, written once for the device kernel
 * (csrc/hip/stats.hip), the host implementation (csrc/scene/stats.cpp) and C
 * callers, and the small double-precision helpers that read a
 * pt_frame_statistics (percentiles, log-average luminance, automatic
 * Brightness, the noise figure).
 *
 * The per-pixel part is integer work on IEEE binary32 bit patterns plus one
 * division and, for a pair, one add, one subtract and one more division; it
 * holds no sum of floats and no transcendental, so counts accumulated in any
 * order agree bit for bit.  The helpers are host arithmetic: no kernel calls
 * them.
 */
#ifndef PT_STATS_H
#define PT_STATS_H

#include "pt_fp.h"
#include "pt_packed.h"

/* --- per pixel ---------------------------------------------------------------- */

enum {
    PT_STATS_NONFINITE = 0,
    PT_STATS_EMPTY     = 1,
    PT_STATS_FILLED    = 2,
};

PT_HD int pt_stats_finite(float v) { return (pt_f2u(v) & 0x7F800000u) != 0x7F800000u; }

/* The class of accumulator pixel (x, y, z, w); *Y = y / w for a filled one. */
PT_HD int pt_stats_classify(float x, float y, float z, float w, float* Y)
{
    if (!(pt_stats_finite(x) && pt_stats_finite(y) && pt_stats_finite(z) && pt_stats_finite(w)))
        return PT_STATS_NONFINITE;
    if (!(w > 0.0f)) return PT_STATS_EMPTY;
    *Y = y / w;
    return PT_STATS_FILLED;
}

/* 256 quarter-octave bins, linear in the mantissa: exponent and the two top
 * mantissa bits, 1.0 opening bin 128.  Denormals and everything below 2^-32
 * (0 included) fall in bin 0; 2^32 and above, +inf included, in bin 255.
 * v is not negative and not NaN. */
PT_HD int pt_stats_bin(float v)
{
    if (!(v > 0.0f)) return 0;
    int b = (int)(pt_f2u(v) >> 21) - 380;
    return b < 0 ? 0 : (b > PT_STATS_BINS - 1 ? PT_STATS_BINS - 1 : b);
}

/* The noise figure of a pixel filled in both halves: 1 and *r when
 * s = Y_A + Y_B > 0 and r = |Y_A - Y_B| / s is finite, else 0 (skipped). */
PT_HD int pt_stats_pair_noise(float Ya, float Yb, float* r)
{
    float s = Ya + Yb;
    if (!(s > 0.0f)) return 0;
    float q = pt_abs(Ya - Yb) / s;
    if (!pt_stats_finite(q)) return 0;
    *r = q;
    return 1;
}

/* --- per tile --------------------------------------------- */

/* One pixel's share of its tile's pt_tile_statistics: bit flags, and the
 * classified accumulator's .w bits for a filled pixel.  has_b == 0: the class
 * of a alone, no pair.  Otherwise the class of a + b and the pair rule on the
 * two halves, as pt_frame_statistics counts them. */
enum {
    PT_TILE_PX_FILLED    = 1,
    PT_TILE_PX_EMPTY     = 2,
    PT_TILE_PX_NONFINITE = 4,
    PT_TILE_PX_PAIR      = 8,
    PT_TILE_PX_OVER      = 16,
};

PT_HD uint32_t pt_tile_stats_pixel(const float a[4], const float b[4], int has_b, float noise_threshold,
                                   uint32_t* w_bits)
{
    float p[4] = {a[0], a[1], a[2], a[3]};
    uint32_t flags = 0;
    if (has_b) {
        float Ya = 0.0f, Yb = 0.0f, r = 0.0f;
        for (int k = 0; k < 4; k++) p[k] = a[k] + b[k];
        if (pt_stats_classify(a[0], a[1], a[2], a[3], &Ya) == PT_STATS_FILLED &&
            pt_stats_classify(b[0], b[1], b[2], b[3], &Yb) == PT_STATS_FILLED && pt_stats_pair_noise(Ya, Yb, &r)) {
            flags |= PT_TILE_PX_PAIR;
            if (r > noise_threshold) flags |= PT_TILE_PX_OVER;
        }
    }
    float Y = 0.0f;
    const int c = pt_stats_classify(p[0], p[1], p[2], p[3], &Y);
    *w_bits = 0;
    if (c == PT_STATS_NONFINITE) return flags | PT_TILE_PX_NONFINITE;
    if (c == PT_STATS_EMPTY) return flags | PT_TILE_PX_EMPTY;
    *w_bits = pt_f2u(p[3]);            /* w > 0: orders as its bits */
    return flags | PT_TILE_PX_FILLED;
}

/* A usable threshold: not NaN and not negative (+infinity: nothing is over). */
PT_HD int pt_tile_stats_threshold_ok(float noise_threshold) { return noise_threshold >= 0.0f; }

/* --- reading the result (host, double) ------------------------------------------ */

/* Lower edge of bin b, 0 <= b <= 256 (256: the upper edge of the last bin):
 * (1 + (b & 3) / 4) * 2^((b >> 2) - 32). */
PT_HD double pt_stats_bin_edge(int b) { return ldexp(1.0 + 0.25 * (double)(b & 3), (b >> 2) - 32); }

/* The smallest bin whose cumulative count reaches ceil(q * total), 0 < q <= 1;
 * -1 on an empty histogram. */
PT_HD int pt_stats_percentile_bin(const uint32_t* hist, double q)
{
    uint64_t total = 0, run = 0;
    for (int b = 0; b < PT_STATS_BINS; b++) total += hist[b];
    if (total == 0) return -1;
    double want = ceil(q * (double)total);
    for (int b = 0; b < PT_STATS_BINS; b++) {
        run += hist[b];
        if (run > 0 && (double)run >= want) return b;
    }
    return PT_STATS_BINS - 1;
}

/* 2^(sum n_b log2 c_b / sum n_b) over the bins from the q_lo to the q_hi
 * percentile bin inclusive, c_b = sqrt(edge(b) edge(b + 1)) the bin's
 * geometric centre; 0 when no pixel lies there. */
PT_HD double pt_stats_log_average(const uint32_t* hist, double q_lo, double q_hi)
{
    int lo = pt_stats_percentile_bin(hist, q_lo), hi = pt_stats_percentile_bin(hist, q_hi);
    if (lo < 0 || hi < lo) return 0.0;
    double sum = 0.0, count = 0.0;
    for (int b = lo; b <= hi; b++) {
        sum += (double)hist[b] * log2(sqrt(pt_stats_bin_edge(b) * pt_stats_bin_edge(b + 1)));
        count += (double)hist[b];
    }
    return count > 0.0 ? exp2(sum / count) : 0.0;
}

/* The Brightness (a linear scale in front of the tone curve, resolve.glsl:118)
 * that puts the log-average luminance at `key`; 1 for a frame without a
 * binned pixel.  Usual arguments: key 0.18, q_lo 0.01, q_hi 0.99. */
PT_HD double pt_stats_auto_brightness(const pt_frame_statistics* s, double key, double q_lo, double q_hi)
{
    double avg = pt_stats_log_average(s->luminance_histogram, q_lo, q_hi);
    return avg > 0.0 ? key / avg : 1.0;
}

/* An upper bound of the relative noise of a share q of the pair pixels: the
 * upper edge of the noise histogram's q percentile bin.  +infinity without a
 * pair pixel: nothing is known then. */
PT_HD double pt_stats_noise(const pt_frame_statistics* s, double q)
{
    int b = pt_stats_percentile_bin(s->noise_histogram, q);
    return b < 0 ? (double)INFINITY : pt_stats_bin_edge(b + 1);
}

#endif /* PT_STATS_H */
