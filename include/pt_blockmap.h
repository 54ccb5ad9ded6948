/*
 * pt_blockmap.h — which ray positions one extend block traces, and which
 * tiles a tile group owns (DESIGN.md §4 "Block map").
 *
 * A tile is 256 ray positions in four quarters of 64, one wave each.  Under
 * LENGTH order (pt_raykey.h) quarter 0 holds a tile's camera rays and
 * shortest class and quarter 3 its longest, so a block that traces one tile
 * keeps its four wave slots and its LDS until the one long wave ends.
 *
 * Granule 1 (TILE): a unit is a tile; wave w of its block traces quarter w.
 *
 * Granule 4 (RUN): a run is four consecutive tiles 4u .. 4u + 3 of the
 * renderer's row-major tile index (the last run may be short).  A unit is
 * (run u, quarter j), index 4u + j; wave w of its block traces quarter j of
 * tile 4u + w -- four waves of one predicted length from neighbouring tiles.
 * A wave whose tile does not exist traces nothing.
 *
 * Tile groups (ptSetBasicRendererSplit): group g of K owns the granules g,
 * g + K, ... -- tiles for granule 1 (t % K == g, as ever), whole runs for
 * granule 4 -- and one segment of the tile order and of the unit order, the
 * groups' segments in group order.
 *
 * Any assignment that gives every position to exactly one wave is correct:
 * which block traces a position never changes a result.  Shared by the device
 * code and the host library (ptBlockMap*), plain C++ like pt_raykey.h.
 */
#ifndef PT_BLOCKMAP_H
#define PT_BLOCKMAP_H

#include "pt_fp.h"

#define PT_BLOCK_MAP_TILE_GRANULE 1u
#define PT_BLOCK_MAP_RUN_GRANULE  4u

/* Granules (tiles or runs) of `tiles` tiles. */
PT_HD uint32_t pt_granule_count(uint32_t tiles, uint32_t granule) { return (tiles + granule - 1u) / granule; }

/* Granules group `group` of `groups` owns. */
PT_HD uint32_t pt_group_granules(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    const uint32_t n = pt_granule_count(tiles, granule);
    return group < n ? (n - group + groups - 1u) / groups : 0u;
}

/* Tiles of a group: its granules, the frame's last one possibly short. */
PT_HD uint32_t pt_group_tile_count(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    const uint32_t own = pt_group_granules(tiles, groups, group, granule);
    if (own == 0u) return 0u;
    const uint32_t last = group + (own - 1u) * groups;          /* the group's last granule */
    const uint32_t end = last * granule + granule;
    return own * granule - (end > tiles ? end - tiles : 0u);
}

/* The i-th tile of a group, i < pt_group_tile_count. */
PT_HD uint32_t pt_group_tile(uint32_t groups, uint32_t group, uint32_t i, uint32_t granule)
{
    return (group + (i / granule) * groups) * granule + i % granule;
}

/* Where a group's segment of the tile order starts. */
PT_HD uint32_t pt_group_tile_start(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    uint32_t s = 0;
    for (uint32_t h = 0; h < group; h++) s += pt_group_tile_count(tiles, groups, h, granule);
    return s;
}

/* Units: `granule` per granule (granule 1: the tiles; granule 4: four
 * quarters per run, also of a short run). */
PT_HD uint32_t pt_unit_count(uint32_t tiles, uint32_t granule) { return pt_granule_count(tiles, granule) * granule; }

PT_HD uint32_t pt_group_unit_count(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    return pt_group_granules(tiles, groups, group, granule) * granule;
}

/* The i-th unit of a group, i < pt_group_unit_count. */
PT_HD uint32_t pt_group_unit(uint32_t groups, uint32_t group, uint32_t i, uint32_t granule)
{
    return (group + (i / granule) * groups) * granule + i % granule;
}

/* Where a group's segment of the unit order starts. */
PT_HD uint32_t pt_group_unit_start(uint32_t tiles, uint32_t groups, uint32_t group, uint32_t granule)
{
    uint32_t s = 0;
    for (uint32_t h = 0; h < group; h++) s += pt_group_unit_count(tiles, groups, h, granule);
    return s;
}

/* The tile and the quarter wave `wave` (0..3) of a unit's block traces.  The
 * tile may lie past the frame's last (a short run): that wave traces nothing. */
PT_HD uint32_t pt_unit_tile(uint32_t unit, uint32_t wave, uint32_t granule)
{
    return granule == PT_BLOCK_MAP_RUN_GRANULE ? (unit & ~3u) + wave : unit;
}
PT_HD uint32_t pt_unit_quarter(uint32_t unit, uint32_t wave, uint32_t granule)
{
    return granule == PT_BLOCK_MAP_RUN_GRANULE ? (unit & 3u) : wave;
}

#endif /* PT_BLOCKMAP_H */
