"""GPU: the RUN block map (ptSetBasicRendererBlockMap; include/pt_blockmap.h;
DESIGN.md §4 "Block map").

Under RUN an extend block traces one 64-position quarter of each of four
consecutive tiles instead of one tile's four quarters, tile groups own whole
runs, and extend is dispatched by an order over (run, quarter) units.  Which
block traces a position never changes a result: every slot, hit, pixel and
counter must equal the TILE map's and the CPU oracle's bit for bit.  A wrongly
built unit order skips or doubles a unit, which leaves stale hits behind: the
oracle comparison catches it.

C3 at sizes where the map can go wrong: 80x48 (5 x 3 tiles: runs cross tile
rows, the last run is short), 112x40 (partial tiles: positions outside the
image) and 64x16 (a single run).  Reset, Run(2), then 40 single rounds: the 16
training rounds of the length table, its first finalize and the re-sorts of
both orders at rounds 16 and 32 are inside.  The renderers run unfused rounds,
the launches RUN applies to."""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib
from test_gpu_parity import compare_state, scene_for

pytestmark = pytest.mark.gpu

AUTO, TILE, RUN = 0, 1, 2        # PT_BLOCK_MAP_*
LENGTH = 2                       # PT_RAY_ORDER_LENGTH
FLAGS = 3                        # ACCUMULATE | SAMPLE_JITTER
ROUNDS = 40
SIZES = [(80, 48), (112, 40), (64, 16)]


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def renderer(pt, dev, s, W, H, block_map, split=1, **kw):
    """A renderer on a device scene of its own (the length table belongs to
    the scene), with unfused single rounds."""
    ds = pt.DeviceScene(dev)
    ds.update(s)
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb, **kw)
    r.RenderFlags = FLAGS
    r.set_fused_rounds(0)
    r.set_round_batch(1)
    r.set_split(split)
    r.set_block_map(block_map)
    return r, sb, ds


def close(*renderers):
    for r, sb, ds in renderers:
        for x in (r, sb, ds):
            x.close()


def snapshot(dev, r, sb):
    dev.synchronize()
    return r.read_state(), sb.read(), r.stats(), r.FrameIndex


def assert_same(a, b, what=""):
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), f"slot state differs {what}"
    assert np.array_equal(bits(a[1]), bits(b[1])), f"accumulator differs {what}"
    assert a[2] == b[2] and a[3] == b[3], f"counters differ {what}"


_oracle = {}


def oracle_after(pt, W, H):
    """The oracle's (state, accumulator) after Reset + Run(2) and after the 40
    rounds that follow: computed once per size."""
    if (W, H) not in _oracle:
        o = oracle_lib.OracleRenderer(scene_for(pt, 3).packs(), W, H)
        o.RenderFlags = FLAGS
        o.reset()
        o.run(2)
        first = (o.state().copy(), o.accum().copy())
        for _ in range(ROUNDS):
            o.run(1)
        _oracle[(W, H)] = (first, (o.state().copy(), o.accum().copy()))
    return _oracle[(W, H)]


def assert_oracle(snap, want, W, H, rounds):
    compare_state(snap[0], want[0])
    assert np.array_equal(bits(snap[1]), bits(want[1])), "accumulator differs from the oracle"
    assert snap[2] == (W * H * rounds, int(want[1][..., 3].sum()))   # rays traced, paths completed


@pytest.mark.parametrize("K", [1, 2, 3, "changing"])
@pytest.mark.parametrize("W,H", SIZES, ids=["5x3-short-run", "partial-tiles", "one-run"])
def test_run_equals_tile_and_oracle(pt, dev, W, H, K):
    """The 40 rounds in one batch (RUN and TILE) and in several batches (RUN),
    in K tile groups or with K changing from batch to batch."""
    s = scene_for(pt, 3)
    k0 = 3 if K == "changing" else K
    one, many, tile = (renderer(pt, dev, s, W, H, m, split=k0) for m in (RUN, RUN, TILE))
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    for (r, _, _), m in ((one, RUN), (many, RUN), (tile, TILE)):
        assert r.block_map() == {"map": m, "used": m} and r.shade_info()["block_map"] == m
        assert r.ray_order()["used"] == LENGTH
        g = r.split()["groups"]
        assert g == min(k0, tiles)
        # group 0's tiles: runs 0, g, 2 g, ... under RUN, tiles 0, g, ... under TILE
        own = [t for t in range(tiles) if ((t // 4) if m == RUN else t) % g == 0]
        assert r.split()["timed_tiles"] == len(own)
        r.reset()
        r.run(2)
    first, last = oracle_after(pt, W, H)
    a = snapshot(dev, *one[:2])
    assert_same(a, snapshot(dev, *tile[:2]), "after Run(2)")
    assert_oracle(a, first, W, H, 2)
    one[0].run_rounds(ROUNDS)
    tile[0].run_rounds(ROUNDS)
    for n, k in ((7, 1), (10, 3), (1, 2), (16, 1), (6, 2)):   # 40 rounds; the finalize falls inside a batch
        if K == "changing":
            many[0].set_split(k)
        many[0].run_rounds(n)
    a, b, c = snapshot(dev, *one[:2]), snapshot(dev, *many[:2]), snapshot(dev, *tile[:2])
    assert_same(a, c, "RUN against TILE")
    assert_same(b, c, "RUN in batches against TILE")
    assert_oracle(a, last, W, H, 2 + ROUNDS)
    for x in (one, many, tile):
        t = x[2].length_table()
        assert t["trained"] and t["rounds"] == 2 + ROUNDS
    close(one, many, tile)


def test_active_tiles_fall_back_to_tile_and_return(pt, dev):
    """An active tile set in the middle of a run: RUN is off while it is in
    place (a masked list breaks runs) and returns when it is cleared.  Against
    a TILE renderer given the same calls, in three tile groups."""
    s = scene_for(pt, 3)
    W, H = 80, 48
    run, tile = renderer(pt, dev, s, W, H, RUN, split=3), renderer(pt, dev, s, W, H, TILE, split=3)
    mask = np.zeros((3, 5), np.uint8)
    mask[0, 1:4] = mask[1, 4] = mask[2, 0] = mask[2, 3:] = 1
    used = []
    for r, sb, _ in (run, tile):
        r.reset()
        r.run(2)
        r.run_rounds(9)
        r.set_active_tiles(mask)
        used.append(r.block_map()["used"])
        r.run_rounds(6)
        r.run(1)
        r.set_active_tiles(None)
        used.append(r.block_map()["used"])
        r.run_rounds(12)
    assert used == [TILE, RUN, TILE, TILE]
    assert_same(snapshot(dev, *run[:2]), snapshot(dev, *tile[:2]))
    close(run, tile)


def test_band_partition_with_path_streams(pt, dev):
    """Rank 1 of a two-rank band partition with two path streams: one band of
    5 tiles per stream, so a run holds tiles of both streams.  Every stream
    against the oracle's one-stream render of the band, and against TILE."""
    s = scene_for(pt, 3)
    W, H = 80, 48
    kw = dict(rank=1, nranks=2, streams=2)
    run, tile = renderer(pt, dev, s, W, H, RUN, split=2, **kw), renderer(pt, dev, s, W, H, TILE, split=2, **kw)
    assert run[0].slot_count == 2 * 5 * 256 and run[0].block_map()["used"] == RUN
    for r, _, _ in (run, tile):
        r.reset()
        r.run(2)
        r.run_rounds(20)
    dev.synchronize()
    owned = pt.owned_pixels(W, H, 1, 2)
    for k in range(2):
        o = oracle_lib.OracleRenderer(s.packs(), W, H, rank=1, nranks=2)
        o.RenderFlags = FLAGS
        o.FrameIndex = k << 24
        o.reset()
        o.run(2)
        for _ in range(20):
            o.run(1)
        got = run[0].read_state(k)
        assert np.array_equal(got.view(np.uint8), tile[0].read_state(k).view(np.uint8))
        compare_state(got[owned], o.state()[owned])
        acc = run[0].read_accumulator(k)
        assert np.array_equal(bits(acc), bits(tile[0].read_accumulator(k)))
        assert np.array_equal(bits(acc[owned]), bits(o.accum()[owned]))
        o.close()
    assert run[0].stats() == tile[0].stats()
    close(run, tile)


def test_render_frame_ends_at_the_same_round(pt, dev):
    """ptRenderFrame at 3 spp (batches, then guarded rounds): the same end
    round, samples and image under both maps."""
    s = scene_for(pt, 3)
    W, H = 80, 48
    run, tile = renderer(pt, dev, s, W, H, RUN, split=3), renderer(pt, dev, s, W, H, TILE, split=3)
    ends = [r.render_frame(3 * W * H) for r, _, _ in (run, tile)]
    assert ends[0] == ends[1] and ends[0][1] >= 3 * W * H
    assert_same(snapshot(dev, *run[:2]), snapshot(dev, *tile[:2]))
    close(run, tile)


def test_where_run_does_not_run(pt, dev):
    """C2 (several shapes and materials: no LENGTH order): RUN is refused with
    a message and AUTO reports TILE.  On C3, AUTO reports the map in use, and
    fused rounds, round batches and OCTANT order keep TILE."""
    L = pt._native.hip_lib()
    r, sb, ds = renderer(pt, dev, scene_for(pt, 2), 64, 32, AUTO)
    assert r.block_map() == {"map": AUTO, "used": TILE} and r.shade_info()["block_map"] == TILE
    with pytest.raises(pt.PathTracerError, match="RUN block map"):
        r.set_block_map(RUN)
    assert r.block_map() == {"map": AUTO, "used": TILE}
    assert L.ptSetBasicRendererBlockMap(r._h, 3) != 0
    close((r, sb, ds))
    r, sb, ds = renderer(pt, dev, scene_for(pt, 3), 64, 32, AUTO)
    assert r.block_map()["used"] in (TILE, RUN) and r.shade_info()["block_map"] == r.block_map()["used"]
    r.set_block_map(RUN)
    assert r.block_map()["used"] == RUN
    r.set_fused_rounds(2)
    assert r.block_map()["used"] == TILE
    r.set_fused_rounds(0)
    r.set_round_batch(4)
    assert r.block_map()["used"] == TILE
    r.set_round_batch(1)
    r.set_ray_order(1)
    assert r.block_map()["used"] == TILE
    r.reset()
    with pytest.raises(pt.PathTracerError, match="RUN block map"):   # RUN set, OCTANT asked for afterwards
        r.run(1)
    r.set_ray_order(0)
    r.run(2)
    assert r.block_map()["used"] == RUN
    close((r, sb, ds))
