/*
 * pt_raykey.h — the key of a ray in the traversal-length table (TileOrder's
 * LENGTH mode, path.hpp; DESIGN.md §4 "Length classes").
 *
 * A ray's key is the cell of its origin in an 8 x 8 x 8 grid over the scene's
 * world bounds (origins outside are clamped to the border cells) times the
 * bin of its direction in an 8 x 8 octahedral map: 32 768 keys.  The device
 * scene keeps, per key, the mean traversal steps of the rays that had it and
 * a length class 0..6 made from those means; shade places a tile's new rays
 * by class so that short rays share waves.
 *
 * Any deterministic function is correct here: the order of a tile's rays
 * never changes a result.  The key uses adds, multiplies, compares and
 * conversions, and one division (the octahedral normalisation); NaN and
 * infinite inputs land in a border cell or bin.  Shared by the device code
 * and the host library (ptRayKey), plain C++ like pt_fp.h.
 */
#ifndef PT_RAYKEY_H
#define PT_RAYKEY_H

#include "pt_fp.h"

#define PT_RAYKEY_CELLS   8u      /* per axis */
#define PT_RAYKEY_DIRS    8u      /* per octahedral axis */
#define PT_RAYKEY_COUNT   32768u  /* 8^3 cells x 8^2 direction bins */
#define PT_RAYKEY_CLASSES 7u      /* length classes of a continuing ray */

/* The grid: cell = (o - lo) * scale per axis.  scale = cells / extent, or 0
 * for an axis without extent (a flat scene: every origin in cell 0 there). */
typedef struct pt_raykey_bounds {
    float lo[3];
    float scale[3];
} pt_raykey_bounds;

/* The one place the grid divides: once per scene update, on the host. */
static inline pt_raykey_bounds pt_raykey_make_bounds(const float lo[3], const float hi[3])
{
    pt_raykey_bounds B;
    for (int k = 0; k < 3; k++) {
        const float e = hi[k] - lo[k];
        B.lo[k] = lo[k];
        B.scale[k] = (e > 0.0f && e < PT_INFINITY && lo[k] > -PT_INFINITY) ? (float)PT_RAYKEY_CELLS / e : 0.0f;
        if (!(B.lo[k] > -PT_INFINITY && B.lo[k] < PT_INFINITY)) B.lo[k] = 0.0f;
    }
    return B;
}

/* x in [0, n) as an index: NaN and negatives give 0, large values n - 1. */
PT_HD uint32_t pt_raykey_bin(float x, uint32_t n)
{
    const float hi = (float)(n - 1u);
    x = x >= 0.0f ? x : 0.0f;   /* NaN compares false */
    x = x <= hi ? x : hi;
    return (uint32_t)x;
}

PT_HD uint32_t pt_ray_key(float ox, float oy, float oz, float vx, float vy, float vz, const pt_raykey_bounds* B)
{
    const uint32_t cx = pt_raykey_bin((ox - B->lo[0]) * B->scale[0], PT_RAYKEY_CELLS);
    const uint32_t cy = pt_raykey_bin((oy - B->lo[1]) * B->scale[1], PT_RAYKEY_CELLS);
    const uint32_t cz = pt_raykey_bin((oz - B->lo[2]) * B->scale[2], PT_RAYKEY_CELLS);
    /* Octahedral map: project on |x| + |y| + |z| = 1, fold the lower half
     * over the diagonals.  The zero vector divides by zero: NaN, bin 0. */
    const float inv = 1.0f / (pt_abs(vx) + pt_abs(vy) + pt_abs(vz));
    float u = vx * inv, v = vy * inv;
    if (vz < 0.0f) {
        const float fu = (1.0f - pt_abs(v)) * (vx < 0.0f ? -1.0f : 1.0f);
        const float fv = (1.0f - pt_abs(u)) * (vy < 0.0f ? -1.0f : 1.0f);
        u = fu;
        v = fv;
    }
    const float half = 0.5f * (float)PT_RAYKEY_DIRS;
    const uint32_t bu = pt_raykey_bin(u * half + half, PT_RAYKEY_DIRS);
    const uint32_t bv = pt_raykey_bin(v * half + half, PT_RAYKEY_DIRS);
    return (((cz * PT_RAYKEY_CELLS + cy) * PT_RAYKEY_CELLS + cx) * PT_RAYKEY_DIRS + bv) * PT_RAYKEY_DIRS + bu;
}

#endif /* PT_RAYKEY_H */
