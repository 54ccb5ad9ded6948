"""CPU: the block map's arithmetic (include/pt_blockmap.h) through the host
library's ptBlockMap* functions.

Granule 1 (TILE): a unit is a tile and groups own tiles t % K -- the lists
tile groups have always had.  Granule 4 (RUN): a unit is (run of four
consecutive tiles, quarter) and groups own whole runs.  Under both, for tile
counts 1..41 and K 1..4: every (tile, quarter) of a group's tiles is traced by
exactly one wave of one unit of that group, no wave of a unit traces anything
else, and the groups' segments tile the tile order and the unit order."""
from __future__ import annotations

import pytest

TILE, RUN = 1, 4   # PT_BLOCK_MAP_TILE_GRANULE, PT_BLOCK_MAP_RUN_GRANULE


@pytest.fixture(scope="module")
def L(pt):
    return pt._native.hip_lib()


def group_tiles(L, T, K, g, granule):
    return [L.ptBlockMapGroupTile(T, K, g, granule, i) for i in range(L.ptBlockMapGroupTileCount(T, K, g, granule))]


def group_units(L, T, K, g, granule):
    return [L.ptBlockMapGroupUnit(T, K, g, granule, i) for i in range(L.ptBlockMapGroupUnitCount(T, K, g, granule))]


@pytest.mark.parametrize("granule", [TILE, RUN])
def test_every_quarter_in_exactly_one_unit_of_its_group(L, granule):
    for T in range(1, 42):
        for K in range(1, 5):
            all_tiles, all_units = [], []
            tile_start = unit_start = 0
            for g in range(K):
                tiles, units = group_tiles(L, T, K, g, granule), group_units(L, T, K, g, granule)
                where = (T, K, g, granule)
                # the segments follow each other in group order
                assert L.ptBlockMapGroupTileStart(T, K, g, granule) == tile_start, where
                assert L.ptBlockMapGroupUnitStart(T, K, g, granule) == unit_start, where
                tile_start += len(tiles)
                unit_start += len(units)
                assert all(t < T for t in tiles) and len(set(tiles)) == len(tiles), where
                assert len(set(units)) == len(units), where
                traced = []
                for u in units:
                    for w in range(4):
                        t, q = L.ptBlockMapUnitTile(u, w, granule), L.ptBlockMapUnitQuarter(u, w, granule)
                        assert q < 4, where
                        if t >= T:
                            assert granule == RUN and t // 4 == (T - 1) // 4, where   # only a short last run
                            continue
                        traced.append((t, q))
                    assert L.ptBlockMapUnitTile(u, 0, granule) < T, where   # no unit without a ray
                assert sorted(traced) == sorted((t, q) for t in tiles for q in range(4)), where
                all_tiles += tiles
                all_units += units
            units_total = T if granule == TILE else 4 * ((T + 3) // 4)
            assert sorted(all_tiles) == list(range(T)), (T, K, granule)
            assert sorted(all_units) == list(range(units_total)), (T, K, granule)
            assert L.ptBlockMapGroupTileStart(T, K, K, granule) == T
            assert L.ptBlockMapGroupUnitStart(T, K, K, granule) == units_total


def test_granule_1_is_t_mod_k(L):
    for T in range(1, 42):
        for K in range(1, 5):
            for g in range(K):
                want = list(range(g, T, K))
                assert group_tiles(L, T, K, g, TILE) == want
                assert group_units(L, T, K, g, TILE) == want   # a unit is a tile ...
            for t in range(T):
                for w in range(4):       # ... whose wave w traces quarter w
                    assert (L.ptBlockMapUnitTile(t, w, TILE), L.ptBlockMapUnitQuarter(t, w, TILE)) == (t, w)


def test_granule_4_groups_own_whole_runs(L):
    """Group g of K owns runs g, g + K, ...: four consecutive tiles each, in
    order; wave w of unit (u, j) traces quarter j of tile 4 u + w."""
    for T in range(1, 42):
        for K in range(1, 5):
            for g in range(K):
                want = [t for u in range(g, (T + 3) // 4, K) for t in range(4 * u, min(4 * u + 4, T))]
                assert group_tiles(L, T, K, g, RUN) == want
                assert group_units(L, T, K, g, RUN) == [4 * u + j for u in range(g, (T + 3) // 4, K) for j in range(4)]
    for u in range(11):
        for j in range(4):
            for w in range(4):
                assert (L.ptBlockMapUnitTile(4 * u + j, w, RUN), L.ptBlockMapUnitQuarter(4 * u + j, w, RUN)) == (4 * u + w, j)


def test_bad_arguments_answer_zero(L):
    assert L.ptBlockMapGroupTileCount(9, 0, 0, TILE) == 0 and L.ptBlockMapGroupTileCount(9, 2, 0, 3) == 0
    assert L.ptBlockMapGroupUnitCount(9, 2, 5, RUN) == 0      # a group past the last
    assert L.ptBlockMapGroupTile(9, 2, 0, RUN, 99) == 0 and L.ptBlockMapGroupUnit(9, 2, 0, RUN, 99) == 0
    assert L.ptBlockMapUnitTile(5, 4, RUN) == 0 and L.ptBlockMapUnitQuarter(5, 0, 2) == 0
    assert L.ptSetBasicRendererBlockMap(None, 0) != 0 and L.ptGetBasicRendererBlockMap(None, None, None) != 0
