"""GPU: ray order LENGTH (ptSetBasicRendererRayOrder; DESIGN.md §4 "Length
classes").

A tile's new rays are placed by the traversal length predicted for their ray
key from a table the device scene learns on training rounds.  The order of a
tile's rays never changes a result, so every slot, pixel and counter must
equal the OCTANT order's and the CPU oracle's bit for bit -- through the
training rounds, the first round on trained classes and the rounds after it --
and the table itself must be the same on every run.  Frames are a few tiles
with ragged edges; the renderers run unfused rounds, the launches LENGTH
applies to."""
from __future__ import annotations

import numpy as np
import pytest

import fuzz_scenes
import oracle_lib
from test_gpu_mesh_extend import blob, chain_mesh, mesh_scene
from test_gpu_parity import compare_state, scene_for

pytestmark = pytest.mark.gpu

AUTO, OCTANT, LENGTH = 0, 1, 2   # PT_RAY_ORDER_*
FLAGS = 3                        # ACCUMULATE | SAMPLE_JITTER
TRAIN_FIRST = 16                 # the first LENGTH rounds after a clear train (rt_rounds.hip)


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def upload(pt, dev, s):
    ds = pt.DeviceScene(dev)
    ds.update(s)
    return ds


def renderer(pt, dev, ds, W, H, order, split=None, flags=FLAGS, termination=0.0):
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = flags
    r.PathTerminationProbability = termination
    r.set_fused_rounds(0)
    r.set_round_batch(1)
    r.set_ray_order(order)
    if split is not None:
        r.set_split(split)
    return r, sb


def oracle(s, W, H, flags=FLAGS, termination=0.0):
    o = oracle_lib.OracleRenderer(s.packs(), W, H)
    o.RenderFlags = flags
    o.PathTerminationProbability = termination
    return o


def snapshot(dev, r, sb):
    dev.synchronize()
    return r.read_state(), sb.read(), r.stats(), r.FrameIndex


def assert_same(a, b):
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), "slot state differs"
    assert np.array_equal(bits(a[1]), bits(b[1])), "accumulator differs"
    assert a[2] == b[2] and a[3] == b[3]


def assert_permutation(r):
    """Every tile's ray positions are a permutation of its 256 slots."""
    p = (r.ray_positions() >> 8).reshape(-1, 256)
    assert np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(256, dtype=np.uint16), p.shape))


@pytest.mark.parametrize("W,H", [(48, 40), (17, 9)], ids=["3x3-ragged", "one-column"])
def test_c3_length_equals_octant_and_oracle_every_round(pt, dev, W, H):
    """C3, Reset + Run(2) + 24 x Run(1): the table trains on the LENGTH rounds
    0..15, so training rounds, the first round on trained classes and the
    rounds after it are all inside.  After every call both orders equal each
    other and the oracle."""
    s = scene_for(pt, 3)
    dl, do = upload(pt, dev, s), upload(pt, dev, s)
    rl, sbl = renderer(pt, dev, dl, W, H, LENGTH)
    ro, sbo = renderer(pt, dev, do, W, H, OCTANT)
    assert rl.ray_order() == {"order": LENGTH, "used": LENGTH} and ro.ray_order() == {"order": OCTANT, "used": OCTANT}
    assert rl.shade_info()["ray_order"] == LENGTH and not rl.shade_info()["length_trained"]
    o = oracle(s, W, H)
    differ = False
    for x in (rl, ro, o):
        x.reset()
    for call, rounds in enumerate([2] + [1] * 24):
        for x in (rl, ro, o):
            x.run(rounds)
        a, b = snapshot(dev, rl, sbl), snapshot(dev, ro, sbo)
        assert_same(a, b)
        compare_state(a[0], o.state())
        assert np.array_equal(bits(a[1]), bits(o.accum())), f"accumulator differs from the oracle after call {call}"
        assert_permutation(rl)
        differ = differ or not np.array_equal(rl.ray_positions(), ro.ray_positions())
        t = dl.length_table()
        assert t["trained"] and t["rounds"] == 2 + call
    assert differ, "LENGTH never placed a ray differently from OCTANT"
    assert o.accum()[..., 3].sum() > 0
    t = dl.length_table()
    assert t["classes"].max() <= 6 and len(np.unique(t["classes"])) > 1
    assert rl.shade_info()["length_trained"]
    assert not do.length_table()["trained"] and do.length_table()["rounds"] == 0   # OCTANT never touches its table
    o.close()
    for x in (rl, sbl, ro, sbo, dl, do):
        x.close()


def test_table_and_positions_are_deterministic(pt, dev):
    """Two fresh device scenes and renderers: byte-identical class tables and
    ray positions.  A Reset and a cameras-only update keep the table; an update
    with a moved mesh clears it."""
    one = mesh_scene(pt, blob())
    moved = mesh_scene(pt, blob(), position=(-0.4, 0.2, 0.5), rotation=(0.1, 0.9, 0.2), scale=(0.9, 1.4, 1.1))
    W, H = 48, 40
    runs = []
    for _ in range(2):
        ds = upload(pt, dev, one)
        r, sb = renderer(pt, dev, ds, W, H, LENGTH)
        assert r.ray_order()["used"] == LENGTH
        r.reset()
        r.run(2)
        r.run_rounds(TRAIN_FIRST + 4)
        dev.synchronize()
        runs.append((ds, r, sb, ds.length_table(), r.ray_positions(), r.read_state()))
    (ds, r, sb, t0, p0, s0), (_, _, _, t1, p1, s1) = runs
    assert t0["trained"] and t1["trained"] and t0["rounds"] == t1["rounds"] == TRAIN_FIRST + 6
    assert np.array_equal(t0["classes"], t1["classes"]) and len(np.unique(t0["classes"])) > 1
    assert np.array_equal(p0, p1)
    assert np.array_equal(s0.view(np.uint8), s1.view(np.uint8))
    r.reset()
    kept = ds.length_table()
    assert kept["trained"] and np.array_equal(kept["classes"], t0["classes"])
    ds.update(one, pt.SCENE_DIRTY_CAMERAS)
    assert ds.length_table()["trained"]
    ds.update(moved)
    cleared = ds.length_table()
    assert not cleared["trained"] and cleared["rounds"] == 0 and np.all(cleared["classes"] == 3)
    # ... and the renderer goes on, training again, on the moved mesh
    r.FrameIndex = 0   # the oracle's seeds
    r.reset()
    r.run(2)
    r.run(1)
    o = oracle(moved, W, H)
    o.reset()
    o.run(2)
    o.run(1)
    dev.synchronize()
    compare_state(r.read_state(), o.state())
    assert np.array_equal(bits(sb.read()), bits(o.accum()))
    assert ds.length_table()["trained"] and ds.length_table()["rounds"] == 3
    o.close()
    for d_, r_, sb_, *_ in runs:
        for x in (r_, sb_, d_):
            x.close()
    for x in (one, moved):
        x.close()


def general_loop_scenes(pt):
    yield "C1", scene_for(pt, 1), 64, 64, dict(flags=FLAGS, termination=0.0), False
    s, st = fuzz_scenes.build(pt, 0)
    yield "fuzz-0", s, 72, 40, dict(flags=st["flags"], termination=st["termination"]), True
    yield "C5-spilled-stack", scene_for(pt, 5), 64, 32, dict(flags=FLAGS, termination=0.0), False
    c = mesh_scene(pt, chain_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.1), scale=(1.0, 1.0, 1.0))
    yield "one-mesh-spilled-stack", c, 48, 24, dict(flags=FLAGS, termination=0.0), True


def test_other_scenes_fall_back_to_octant(pt, dev):
    """Scenes LENGTH does not run on -- the general LaneStep loop (C1, a fuzz
    scene, C5 whose stack spills) and a one-mesh scene whose stack spills --
    report OCTANT when LENGTH is asked for, and equal the oracle."""
    for name, s, W, H, kw, own in general_loop_scenes(pt):
        ds = upload(pt, dev, s)
        if "spilled" in name:
            assert ds.stack_needed > 20, name
        r, sb = renderer(pt, dev, ds, W, H, LENGTH, **kw)
        assert r.ray_order() == {"order": LENGTH, "used": OCTANT}, name
        assert r.shade_info()["ray_order"] == OCTANT, name
        o = oracle(s, W, H, **kw)
        for x in (r, o):
            x.reset()
            x.run(2)
            x.run(1)
            x.run(1)
        dev.synchronize()
        compare_state(r.read_state(), o.state())
        assert np.array_equal(bits(sb.read()), bits(o.accum())), name
        assert not ds.length_table()["trained"], name
        o.close()
        for x in (r, sb, ds):
            x.close()
        if own:
            s.close()


def test_length_in_tile_groups(pt, dev):
    """Three tile groups forced on a frame two tiles wide (2 x 3 tiles, ragged
    bottom): the batch that holds the first training rounds is cut after them.
    Equal to the OCTANT renderer on one stream and to the oracle."""
    s = scene_for(pt, 3)
    W, H = 32, 40
    dl, do = upload(pt, dev, s), upload(pt, dev, s)
    rl, sbl = renderer(pt, dev, dl, W, H, LENGTH, split=3)
    ro, sbo = renderer(pt, dev, do, W, H, OCTANT, split=1)
    assert rl.split()["groups"] == 3
    o = oracle(s, W, H)
    for x in (rl, ro, o):
        x.reset()
        x.run(2)
    for k in (TRAIN_FIRST + 3, 5):
        rl.run_rounds(k)
        ro.run_rounds(k)
        for _ in range(k):
            o.run(1)
        a = snapshot(dev, rl, sbl)
        assert_same(a, snapshot(dev, ro, sbo))
        compare_state(a[0], o.state())
        assert np.array_equal(bits(a[1]), bits(o.accum()))
        assert_permutation(rl)
    t = dl.length_table()
    assert t["trained"] and t["rounds"] == 2 + TRAIN_FIRST + 3 + 5
    o.close()
    for x in (rl, sbl, ro, sbo, dl, do):
        x.close()


def test_length_across_state_write(pt, dev):
    """Save a LENGTH renderer's state in the middle of the training rounds,
    restore it into a new renderer of the same scene and go on: equal to the
    uninterrupted OCTANT render."""
    s = scene_for(pt, 3)
    W, H = 48, 40
    dl, do = upload(pt, dev, s), upload(pt, dev, s)
    a, sba = renderer(pt, dev, dl, W, H, LENGTH)
    a.reset()
    a.run(2)
    for _ in range(5):
        a.run(1)
    saved, acc, frame = a.read_state(), sba.read(), a.FrameIndex
    a.close()
    sba.close()
    b, sbb = renderer(pt, dev, dl, W, H, LENGTH)
    sbb.write(acc)
    b.FrameIndex = frame
    b.write_state(saved)
    assert_permutation(b)
    for _ in range(TRAIN_FIRST):
        b.run(1)
    c, sbc = renderer(pt, dev, do, W, H, OCTANT)
    c.reset()
    c.run(2)
    for _ in range(5 + TRAIN_FIRST):
        c.run(1)
    gb, gc = snapshot(dev, b, sbb), snapshot(dev, c, sbc)
    compare_state(gb[0], gc[0])
    assert np.array_equal(bits(gb[1]), bits(gc[1])) and gb[3] == gc[3]
    assert dl.length_table()["rounds"] == 2 + 5 + TRAIN_FIRST
    for x in (b, sbb, c, sbc, dl, do):
        x.close()


def test_auto_and_arguments(pt, dev):
    """AUTO resolves per scene; the calls reject bad arguments."""
    s = scene_for(pt, 3)
    ds = upload(pt, dev, s)
    r, sb = renderer(pt, dev, ds, 32, 16, AUTO)
    used = r.ray_order()
    assert used["order"] == AUTO and used["used"] in (OCTANT, LENGTH)
    assert r.shade_info()["ray_order"] == used["used"]
    L = pt._native.hip_lib()
    assert L.ptSetBasicRendererRayOrder(r._h, 3) != 0 and L.ptSetBasicRendererRayOrder(None, 0) != 0
    assert L.ptGetBasicRendererRayOrder(None, None, None) != 0
    assert L.ptReadSceneLengthTable(dev.handle, None, None, None, None) != 0
    assert L.ptReadBasicRendererRayPositions(dev.handle, r._h, None) != 0
    for x in (r, sb, ds):
        x.close()
