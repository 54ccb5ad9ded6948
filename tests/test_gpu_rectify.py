"""GPU: history validation.  The device kernel against
the host implementation and the numpy restatement bit for bit on every case
of tests/rectify_cases.py, out of place and in place; the argument errors; the
kernel counter; FrameHistory with validate from render to merge to further
rounds, and without it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rectify_cases as xc

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def hosts(pt):
    """{name: the host implementation's result}, computed once."""
    return {name: pt.rectify_host(c["hist"], c["cur"], c["guides"], xc.params_object(pt, c["params"]))
            for name, (c, _) in xc.all_cases().items()}


def upload(pt, dev, case):
    H, W = case["guides"].shape
    hist, cur, dst = (pt.SampleBuffer(dev, W, H) for _ in range(3))
    g = pt.DenoiseGuides(dev, W, H)
    hist.write(case["hist"])
    cur.write(case["cur"])
    g.write(case["guides"])
    return hist, cur, g, dst


@pytest.mark.parametrize("name", xc.names())
def test_device_matches_host(pt, dev, hosts, name):
    case, ref = xc.all_cases()[name]
    H, W = case["guides"].shape
    p = xc.params_object(pt, case["params"])
    hist, cur, g, dst = upload(pt, dev, case)
    dst.write(np.full((H, W, 4), 3.0, F))                         # every pixel must be rewritten
    first = hist.rectify(cur, g, p, out=dst).read()
    dst.write(np.full((H, W, 4), -5.0, F))
    second = hist.rectify(cur, g, p, out=dst).read()
    assert np.array_equal(bits(first), bits(second))
    same = xc.same_bits(first, hosts[name])
    assert same.all(), np.argwhere(~same)[:5]
    same = xc.same_bits(first, ref)                               # and so the numpy restatement
    assert same.all(), np.argwhere(~same)[:5]
    assert hist.read().tobytes() == case["hist"].tobytes()        # out of place: the inputs are not written
    assert hist.rectify(cur, g, p) is hist                        # in place
    assert np.array_equal(bits(hist.read()), bits(first))
    assert cur.read().tobytes() == case["cur"].tobytes()
    assert g.read().tobytes() == case["guides"].tobytes()
    for x in (dst, g, cur, hist):
        x.close()


def test_errors_leave_dst_untouched(pt, dev):
    N = pt._native
    L = N.hip_lib()
    case, _ = xc.all_cases()["16x16-r1"]
    hist, cur, g, dst = upload(pt, dev, case)
    small, small_guides = pt.SampleBuffer(dev, 16, 15), pt.DenoiseGuides(dev, 15, 16)
    marker = np.full((16, 16, 4), 5.0, F)
    dst.write(marker)
    small.write(marker[:15])
    P = pt.RectifyParameters

    def fails(call):
        with pytest.raises(pt.PathTracerError) as e:
            call()
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    fails(lambda: hist.rectify(cur, g, out=cur))                           # dst is current
    fails(lambda: cur.rectify(cur, g, out=dst))                            # history is current
    fails(lambda: small.rectify(cur, g, out=dst))                          # sizes differ
    fails(lambda: hist.rectify(small, g, out=dst))
    fails(lambda: hist.rectify(cur, small_guides, out=dst))
    fails(lambda: hist.rectify(cur, g, out=small))
    nan, inf = float("nan"), float("inf")
    for bad in (P(Radius=0), P(Radius=4), P(MinNeighbours=0), P(MinNeighbours=50), P(Sigma=-0.5), P(Sigma=inf),
                P(Sigma=nan), P(ClampedHistory=0.0), P(ClampedHistory=nan), P(NormalCosine=-1.0),
                P(NormalCosine=1.01), P(NormalCosine=nan)):
        fails(lambda: hist.rectify(cur, g, bad, out=dst))
    ok = P().as_struct()
    args = [dev.handle, hist.handle, cur.handle, g.handle, C.byref(ok), dst.handle]
    for i in range(len(args)):
        a = list(args)
        a[i] = None
        assert L.ptRectifyHistory(*a) != 0, i
    other = pt.Device(0)                                # a second pt_device: its objects belong to another device
    foreign, foreign_guides = pt.SampleBuffer(other, 16, 16), pt.DenoiseGuides(other, 16, 16)
    foreign.write(marker)
    foreign_guides.write(case["guides"])
    assert L.ptRectifyHistory(dev.handle, foreign.handle, cur.handle, g.handle, C.byref(ok), dst.handle) != 0
    assert len(L.ptGetLastError()) > 0                                     # history of another device
    fails(lambda: hist.rectify(foreign, g, out=dst))                       # current
    fails(lambda: hist.rectify(cur, foreign_guides, out=dst))              # guides
    fails(lambda: hist.rectify(cur, g, out=foreign))                       # dst
    assert L.ptRectifyHistory(other.handle, hist.handle, cur.handle, g.handle, C.byref(ok), dst.handle) != 0
    assert len(L.ptGetLastError()) > 0                                     # the device against all the rest
    assert np.array_equal(bits(foreign.read()), bits(marker))
    assert foreign_guides.read().tobytes() == case["guides"].tobytes()
    for x in (foreign_guides, foreign, other):
        x.close()
    dev.synchronize()
    assert np.array_equal(bits(dst.read()), bits(marker))                  # nothing was written
    assert np.array_equal(bits(small.read()), bits(marker[:15]))
    assert hist.read().tobytes() == case["hist"].tobytes()
    assert cur.read().tobytes() == case["cur"].tobytes()
    assert L.ptRectifyHistory(*args) == 0                                  # and the good call goes through
    assert not np.array_equal(bits(dst.read()), bits(marker))
    for x in (small_guides, small, dst, g, cur, hist):
        x.close()


def test_kernel_stats_count_one_launch_per_call(pt, dev):
    case, _ = xc.all_cases()["33x18-r2"]
    hist, cur, g, dst = upload(pt, dev, case)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    for radius in (1, 2, 3):
        hist.rectify(cur, g, pt.RectifyParameters(Radius=radius), out=dst)
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_REPROJECT)
    dev.set_profiling(False)
    assert n == 3 and ms > 0
    assert pt.KERNEL_REPROJECT == 10
    for x in (dst, g, cur, hist):
        x.close()


W, H = 64, 32
FLAGS = 3        # RENDER_FLAG_ACCUMULATE | RENDER_FLAG_SAMPLE_JITTER


def config1(pt):
    """Config 1 built through the scene API, so that the sphere's material is
    at hand: the same packed bytes as Scene.config(1)."""
    s = pt.Scene.create()
    m = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Sphere", BaseColor=(0.8, 0.3, 0.3))
    s.create_entity(pt.ENTITY_SPHERE, position=(0, 0, 1), material=m)
    cam = s.find_camera(0)
    s.move_camera(cam, position=(0, -4, 1), rotation=(np.pi / 2, 0, 0))
    s.set_camera_pinhole(cam, 90.0)
    s.pack()
    ref = pt.Scene.config(1)
    ref.pack()
    a, b = ref.arrays(), s.arrays()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    ref.close()
    return s, m


def renderer(pt, dev, ds, sb, frame):
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = FLAGS
    r.FrameIndex = frame
    r.reset()
    return r


def first_frame_then_edit(pt, dev, history):
    """16 rounds of config 1, then the sphere's colour changes: nothing moves,
    so every pixel keeps its history by geometry."""
    scene, material = config1(pt)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    sb0 = pt.SampleBuffer(dev, W, H)
    assert history.begin_frame(ds, 0, sb0) is False
    r0 = renderer(pt, dev, ds, sb0, 0)
    r0.run(16)
    accum0, guides0, cam0 = sb0.read(), history.guides.read(), history.camera.copy()
    scene.set_material_parameter(material, "BaseColor", (0.1, 0.2, 0.9))
    dirty = scene.pack()
    assert dirty != 0
    ds.update(scene, dirty)
    return scene, ds, sb0, r0, accum0, guides0, cam0


def test_end_to_end_with_validate(pt, dev):
    """Config 1 at 64x32: 16 rounds, a material edit, then reset, begin_frame,
    run(2), merge, run(2).  Sigma 0 makes every tested pixel's box the single
    point mu, and the sky and the plane give windows of 25 members, so the
    merge is known to change the history: a 16-round mean equals the mean of a
    window of 2-round pixels only by accident."""
    validate = pt.RectifyParameters(Sigma=0.0)
    default = pt.FrameHistory(dev, W, H, validate=True)                    # True: the default parameters
    assert vars(default.validate) == vars(pt.RectifyParameters())
    default.close()
    history = pt.FrameHistory(dev, W, H, validate=validate)
    with pytest.raises(ValueError):
        history.merge(None)                                               # before begin_frame
    scene, ds, sb0, r0, accum0, guides0, cam0 = first_frame_then_edit(pt, dev, history)
    history.merge(sb0)                                                     # nothing was carried: nothing happens
    assert np.array_equal(bits(sb0.read()), bits(accum0)) and history.held is None
    with pytest.raises(ValueError):
        history.merge(sb0)                                                 # twice in a frame

    sb1, sb2 = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    r1, r2 = renderer(pt, dev, ds, sb1, 100), renderer(pt, dev, ds, sb2, 100)
    assert history.begin_frame(ds, 0, sb1) is True
    assert not sb1.read().any()                                            # as Reset left it
    guides1, cam1 = history.guides.read(), history.camera.copy()
    reprojected = history.held.read()
    assert np.array_equal(bits(reprojected), bits(pt.reproject_host(accum0, guides0, cam0, guides1, cam1)))
    assert (reprojected[..., 3] > 0).mean() > 0.9                          # nothing moved

    r1.run(2)
    r2.run(2)
    fresh = sb2.read()
    assert np.array_equal(bits(sb1.read()), bits(fresh))                   # the same FrameIndex: the same samples
    with pytest.raises(ValueError):
        history.merge(sb2)                                                 # not begin_frame's buffer
    history.merge(sb1)
    with pytest.raises(ValueError):
        history.merge(sb1)
    rectified = pt.rectify_host(reprojected, fresh, guides1, validate)
    merged = sb1.read()
    assert np.array_equal(bits(history.held.read()), bits(rectified))
    assert np.array_equal(bits(merged), bits(fresh + rectified))           # one float32 add per component
    # A count is only ever cut, and then to ClampedHistory (16 rounds of history
    # against 8); some are, so merge() added a history that rectify changed.
    cut = rectified[..., 3] < reprojected[..., 3]
    assert cut.any()
    assert np.all(rectified[..., 3] <= reprojected[..., 3])
    assert np.all(rectified[..., 3][cut] == validate.ClampedHistory)
    assert np.array_equal(bits(sb0.read()), bits(accum0))                  # the old frame is not written

    r1.run(2)
    r2.run(2)
    after = sb1.read()
    k = (sb2.read()[..., 3] - fresh[..., 3]).astype(np.float64)
    assert np.array_equal(k, np.round(k)) and k.max() >= 1
    expect = merged[..., 3].astype(np.float64) + k
    assert np.all(np.abs(after[..., 3] - expect) <= (k + 1) * 2.0 ** -23 * expect)
    assert np.isfinite(after).all()
    for x in (r2, r1, r0, sb2, sb1, sb0, history, ds):
        x.close()
    assert history.held is None
    scene.close()


def test_without_validate_nothing_changes(pt, dev):
    """The same calls on a FrameHistory without validate: begin_frame
    reprojects into the frame's buffer, merge refuses, and reset,
    begin_frame, run(2), run(2) leave the bits of the order rows 8 and 9
    define, written here without a FrameHistory: reset, SampleBuffer.reproject
    into the buffer, run(2), run(2) at the same FrameIndex."""
    history = pt.FrameHistory(dev, W, H)
    scene, ds, sb0, r0, accum0, guides0, cam0 = first_frame_then_edit(pt, dev, history)
    prev_guides = pt.DenoiseGuides(dev, W, H)
    prev_guides.write(guides0)
    sb1, sb2 = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    r1, r2 = renderer(pt, dev, ds, sb1, 100), renderer(pt, dev, ds, sb2, 100)
    assert history.begin_frame(ds, 0, sb1) is True
    assert history.held is None and history.validate is None
    guides1, cam1 = history.guides.read(), history.camera.copy()
    host = pt.reproject_host(accum0, guides0, cam0, guides1, cam1)
    assert np.array_equal(bits(sb1.read()), bits(host))
    with pytest.raises(ValueError):
        history.merge(sb1)
    sb0.reproject(prev_guides, cam0, history.guides, cam1, out=sb2)
    for r in (r1, r2):
        r.run(2)
        r.run(2)
    after = sb1.read()
    assert np.array_equal(bits(after), bits(sb2.read()))
    assert np.all(after[..., 3] >= host[..., 3]) and (after[..., 3] > host[..., 3]).any()
    for x in (r2, r1, r0, sb2, sb1, sb0, prev_guides, history, ds):
        x.close()
    scene.close()
