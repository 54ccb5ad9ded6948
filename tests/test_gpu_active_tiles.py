"""GPU: active tile sets (ptSetBasicRendererActiveTiles).

Rounds under a mask launch the active tiles only.  A slot's round depends only
on its own previous round and the round's FrameIndex, so after the same calls
an active tile's slots and pixels must equal an unmasked renderer's and the
CPU oracle's bit for bit, in every scheduling mode, and an inactive tile must
keep every bit it had when the mask was set."""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib
from test_gpu_parity import compare_state, scene_for

pytestmark = pytest.mark.gpu

FLAGS = 3   # ACCUMULATE | SAMPLE_JITTER


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def checkerboard(W, H, phase=0):
    ty, tx = (H + 15) // 16, (W + 15) // 16
    return ((np.add.outer(np.arange(ty), np.arange(tx)) + phase) % 2 == 0).astype(np.uint8)


def pixels_of(mask, W, H):
    """The (H, W) boolean pixel mask of a tile mask."""
    return np.kron(mask, np.ones((16, 16), np.uint8))[:H, :W].astype(bool)


def valid_slots(mask, W, H):
    return int(pixels_of(mask, W, H).sum())


def renderer(pt, dev, ds, W, H, fused=None, batch=None, split=None):
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = FLAGS
    if fused is not None:
        r.set_fused_rounds(fused)
    if batch is not None:
        r.set_round_batch(batch)
    if split is not None:
        r.set_split(split)
    return r, sb


def schedule(r):
    """The masked part of every equality test: 8 rounds, FrameIndex + 1 each."""
    for _ in range(3):
        r.run(1)
    r.run_rounds(5)


_oracle = {}


def oracle(pt, config, W, H):
    """The CPU oracle after Reset, Run(2) and 8 Run(1): computed once per case."""
    key = (config, W, H)
    if key not in _oracle:
        o = oracle_lib.OracleRenderer(scene_for(pt, config).packs(), W, H)
        o.RenderFlags = FLAGS
        o.reset()
        o.run(2)
        for _ in range(8):
            o.run(1)
        _oracle[key] = (o.state(), o.accum())
        o.close()
    return _oracle[key]


def masked_against_unmasked(pt, dev, config, W, H, mask, **mode):
    s = scene_for(pt, config)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    (m, mb), (u, ub) = renderer(pt, dev, ds, W, H, **mode), renderer(pt, dev, ds, W, H, **mode)
    for r in (m, u):
        r.reset()
        r.run(2)
    dev.synchronize()
    snap_state, snap_accum = m.read_state(), mb.read()
    m.set_active_tiles(mask)
    tiles = mask.size
    assert m.active_tiles() == {"active": int(mask.sum()), "tiles": tiles}
    assert u.active_tiles() == {"active": tiles, "tiles": tiles}
    for r in (m, u):
        schedule(r)
    dev.synchronize()
    assert m.FrameIndex == u.FrameIndex
    ms, ma, us, ua = m.read_state(), mb.read(), u.read_state(), ub.read()
    os_, oa = oracle(pt, config, W, H)
    act = pixels_of(mask, W, H)
    assert act.any() and (~act).any()
    compare_state(ms[act], us[act])
    compare_state(ms[act], os_[act])
    assert np.array_equal(bits(ma[act]), bits(ua[act])) and np.array_equal(bits(ma[act]), bits(oa[act]))
    compare_state(ms[~act], snap_state[~act])
    assert np.array_equal(bits(ma[~act]), bits(snap_accum[~act]))
    assert (bits(ua[~act]) != bits(snap_accum[~act])).any()        # the rounds did change those pixels in U
    assert m.stats()[0] == 2 * W * H + 8 * valid_slots(mask, W, H)
    assert u.stats()[0] == 10 * W * H
    # cleared: the next rounds run everywhere again
    m.set_active_tiles(None)
    assert m.active_tiles()["active"] == tiles
    m.run_rounds(2)
    dev.synchronize()
    assert (bits(mb.read()[~act]) != bits(snap_accum[~act])).any()
    assert m.stats()[0] == 2 * W * H + 8 * valid_slots(mask, W, H) + 2 * W * H
    for x in (u, ub, m, mb, ds):
        x.close()


MODES = {
    "separate": dict(fused=0),
    "fused": dict(fused=2),
    "batch4": dict(batch=4),
    "split2": dict(fused=0, split=2),
    "split3": dict(fused=0, split=3),
}
# C1: 5 x 3 whole tiles; C3: 6 x 4 tiles whose bottom row is 6 pixels high
FRAMES = [(1, 80, 48), (3, 96, 54)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("config,W,H", FRAMES)
def test_masked_equals_unmasked_and_oracle(pt, dev, config, W, H, mode):
    mask = checkerboard(W, H)
    assert mask[-1].any() and mask[:, -1].any()                    # edge tiles among the active ones
    masked_against_unmasked(pt, dev, config, W, H, mask, **MODES[mode])


@pytest.mark.parametrize("config,W,H", FRAMES)
def test_single_active_tile_in_three_groups(pt, dev, config, W, H):
    """One active tile: two of the three tile groups launch nothing."""
    mask = np.zeros(((H + 15) // 16, (W + 15) // 16), np.uint8)
    mask[-1, -2] = 1
    masked_against_unmasked(pt, dev, config, W, H, mask, fused=0, split=3)


@pytest.mark.parametrize("config,W,H", [(2, 64, 48), (5, 80, 48)])
def test_class_lists_rest_under_a_mask(pt, dev, config, W, H):
    """Scenes with several material types in two tile groups shade through
    class lists; they are off while a mask is set, back on once it is cleared,
    and the masked tiles still equal the unmasked render (which uses them)."""
    s = scene_for(pt, config)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    r, sb = renderer(pt, dev, ds, W, H, fused=0, split=2)
    assert r.class_lists()
    r.set_active_tiles(checkerboard(W, H))
    assert not r.class_lists()
    r.set_active_tiles(None)
    assert r.class_lists()
    for x in (r, sb, ds):
        x.close()
    masked_against_unmasked(pt, dev, config, W, H, checkerboard(W, H, 1), fused=0, split=2)


def test_all_ones_and_all_zero_masks(pt, dev):
    config, W, H = 3, 96, 54
    s = scene_for(pt, config)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    grid = ((H + 15) // 16, (W + 15) // 16)
    (a, ab), (z, zb) = renderer(pt, dev, ds, W, H, fused=0, split=2), renderer(pt, dev, ds, W, H, fused=0, split=2)
    for r in (a, z):
        r.reset()
        r.run(2)
    dev.synchronize()
    snap_state, snap_accum, frame, rays = z.read_state(), zb.read(), z.FrameIndex, z.stats()[0]
    a.set_active_tiles(np.ones(grid, np.uint8))
    z.set_active_tiles(np.zeros(grid, np.uint8))
    assert z.active_tiles()["active"] == 0
    schedule(a)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    schedule(z)
    dev.synchronize()
    launches = sum(dev.kernel_stats(k)[0] for k in range(11))
    dev.set_profiling(False)
    # all ones: the bits of no mask (the oracle's)
    os_, oa = oracle(pt, config, W, H)
    compare_state(a.read_state(), os_)
    assert np.array_equal(bits(ab.read()), bits(oa)) and a.stats()[0] == 10 * W * H
    # all zero: nothing but FrameIndex
    assert launches == 0
    assert z.FrameIndex == frame + 8 == a.FrameIndex
    compare_state(z.read_state(), snap_state)
    assert np.array_equal(bits(zb.read()), bits(snap_accum)) and z.stats()[0] == rays
    for x in (z, zb, a, ab, ds):
        x.close()


def test_mask_schedule_is_deterministic(pt, dev):
    """Mask A, rounds, mask B overlapping A, rounds, cleared, rounds: the same
    bits from separate launches and from three tile groups; a Reset under a
    mask restarts every tile and keeps the mask."""
    config, W, H = 3, 96, 54
    s = scene_for(pt, config)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    A = checkerboard(W, H)
    B = np.zeros_like(A)
    B[1:, 2:] = 1
    assert (A & B).any() and (A & ~B & 1).any() and (B & ~A & 1).any()
    out = []
    for mode in (dict(fused=0), dict(fused=0, split=3), dict(batch=4)):
        r, sb = renderer(pt, dev, ds, W, H, **mode)
        r.set_active_tiles(A)
        r.reset()                                                  # raygen covers every tile
        assert r.active_tiles()["active"] == int(A.sum())
        dev.synchronize()
        assert not sb.read().any()
        r.run(2)
        r.run_rounds(4)
        r.set_active_tiles(B)
        r.run(1)
        r.run_rounds(5)
        r.set_active_tiles(None)
        r.run_rounds(3)
        dev.synchronize()
        rays = W * H * 3 + valid_slots(A, W, H) * 6 + valid_slots(B, W, H) * 6
        assert r.stats()[0] == rays
        out.append((r.read_state(), sb.read(), r.FrameIndex))
        r.close()
        sb.close()
    for state, accum, frame in out[1:]:
        compare_state(state, out[0][0])
        assert np.array_equal(bits(accum), bits(out[0][1])) and frame == out[0][2]
    # tiles in neither A nor B ran only the last three rounds
    idle = pixels_of((1 - A) & (1 - B), W, H)
    assert idle.any() and out[0][1][idle][:, 3].max() <= 3
    ds.close()


def test_refusals_launch_nothing(pt, dev):
    N = pt._native
    L = N.hip_lib()
    W, H = 80, 48
    s = scene_for(pt, 1)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    mask = np.ascontiguousarray(checkerboard(W, H))
    sbp, sbs, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    part = pt.BasicRenderer(dev, ds, sbp, rank=0, nranks=2)
    streams = pt.BasicRenderer(dev, ds, sbs, streams=2)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = FLAGS
    r.reset()
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)

    def refused(call):
        with pytest.raises(pt.PathTracerError):
            call()
        assert len(L.ptGetLastError()) > 0

    refused(lambda: part.set_active_tiles(mask))
    refused(lambda: streams.set_active_tiles(mask))
    p = mask.ctypes.data
    assert L.ptSetBasicRendererActiveTiles(dev.handle, r.handle, p, mask.size - 1) != 0      # a wrong tile count
    assert L.ptSetBasicRendererActiveTiles(dev.handle, r.handle, p, mask.size + 1) != 0
    assert L.ptSetBasicRendererActiveTiles(dev.handle, r.handle, None, mask.size) != 0       # NULL mask with a count
    assert L.ptSetBasicRendererActiveTiles(None, r.handle, p, mask.size) != 0
    assert L.ptSetBasicRendererActiveTiles(dev.handle, None, p, mask.size) != 0
    assert L.ptGetBasicRendererActiveTiles(None, None, None) != 0
    assert r.active_tiles() == {"active": 15, "tiles": 15}                                    # still no mask
    with pytest.raises(ValueError):
        r.set_active_tiles(np.ones((5, 3), np.uint8))
    r.set_active_tiles(mask)
    frame = r.FrameIndex
    refused(lambda: r.render_frame(4 * W * H, 100))
    assert r.FrameIndex == frame and r.active_tiles()["active"] == int(mask.sum())
    dev.synchronize()
    assert sum(dev.kernel_stats(k)[0] for k in range(11)) == 0     # nothing was launched
    dev.set_profiling(False)
    r.set_active_tiles(None)
    rounds, samples = r.render_frame(2 * W * H, 100)               # fine without the mask
    assert samples >= 2 * W * H
    for x in (r, streams, part, sb, sbs, sbp, ds):
        x.close()


def test_refine_tiles_after_reprojection(pt, dev):
    """Config 1 at 80x48: a frame of 48 rounds, a camera move, the history
    reprojected into half A.  refine_tiles with min_count: tiles whose pixels
    all carry at least min_count samples of history run min_rounds and stop
    (the noise rule is satisfied at threshold +inf: nothing is over); a tile with
    disoccluded pixels needs at least min_count / 2 > min_rounds rounds (a
    round adds at most one sample per half) and runs longer."""
    W, H = 80, 48
    MIN_ROUNDS, MIN_COUNT, STEP, MAX_ROUNDS = 4, 12.0, 4, 96
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    history = pt.FrameHistory(dev, W, H)
    sb0 = pt.SampleBuffer(dev, W, H)
    history.begin_frame(ds, 0, sb0)
    r0 = pt.BasicRenderer(dev, ds, sb0)
    r0.RenderFlags = FLAGS
    r0.reset()
    r0.run(2)
    r0.run_rounds(46)
    scene.move_camera(scene.find_camera(0), position=(0.5, -4.0, 1.0), rotation=(float(np.pi / 2), 0.0, 0.1))
    scene.pack()
    ds.update(scene)
    sa, sb = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    ra, rb = pt.BasicRenderer(dev, ds, sa), pt.BasicRenderer(dev, ds, sb)
    ra.FrameIndex = 1000
    rb.FrameIndex = 1000 + (1 << 24)
    for r in (ra, rb):
        r.RenderFlags = FLAGS
        r.reset()
    assert history.begin_frame(ds, 0, sa) is True
    before = sa.tile_statistics()
    settled = (before["empty"] == 0) & (before["min_count"] >= np.float32(MIN_COUNT))
    disoccluded = before["empty"] > 0
    print("history per tile: empty", before["empty"].tolist(), "min_count", before["min_count"].tolist())
    assert settled.any() and disoccluded.any()
    rounds, stats = pt.refine_tiles(ra, rb, float("inf"), min_rounds=MIN_ROUNDS, rounds_per_step=STEP,
                                    max_rounds=MAX_ROUNDS, min_count=MIN_COUNT)
    print("rounds per tile", rounds.tolist())
    assert rounds.shape == (3, 5) and stats.shape == (3, 5)
    assert (rounds[settled] == MIN_ROUNDS).all()
    assert (rounds[disoccluded] >= MIN_COUNT / 2).all() and (rounds[disoccluded] > MIN_ROUNDS).all()
    assert rounds.max() < MAX_ROUNDS                              # it converged: every tile met the rule
    assert (stats["min_count"][stats["filled"] > 0] >= MIN_COUNT).all() and (stats["pair"] > 0).all()
    assert stats.tobytes() == sa.tile_statistics(sb, float("inf")).tobytes()
    for r in (ra, rb):                                             # the mask is cleared on return
        assert r.active_tiles() == {"active": 15, "tiles": 15}
    assert ra.FrameIndex == 1000 + rounds.max() and rb.FrameIndex - ra.FrameIndex == 1 << 24
    with pytest.raises(ValueError):
        pt.refine_tiles(ra, rb, 0.1, rounds_per_step=0)
    for x in (rb, ra, sb, sa, r0, sb0, history, ds):
        x.close()
    scene.close()
