"""GPU: temporal reprojection.  The device kernel
against the host implementation bit for bit on every case of
tests/reproject_cases.py, the argument errors, the kernel counter, and the
whole path render -> move the camera -> FrameHistory.begin_frame ->
accumulate on top."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import reproject_cases as rc

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


def params(pt):
    p = rc.PARAMS
    return pt.ReprojectParameters(p["normal_cosine"], p["depth_tolerance"], p["min_weight"], p["max_history"])


@pytest.fixture(scope="module")
def hosts(pt):
    """{name: the host implementation's result}, computed once."""
    return {name: pt.reproject_host(c["prev_accum"], c["prev_guides"], c["prev_cam"], c["guides"], c["cam"],
                                    params(pt)) for name, (c, _) in rc.all_cases().items()}


def upload(pt, dev, case):
    Hp, Wp = case["prev_guides"].shape
    H, W = case["guides"].shape
    prev, dst = pt.SampleBuffer(dev, Wp, Hp), pt.SampleBuffer(dev, W, H)
    pg, g = pt.DenoiseGuides(dev, Wp, Hp), pt.DenoiseGuides(dev, W, H)
    prev.write(case["prev_accum"])
    pg.write(case["prev_guides"])
    g.write(case["guides"])
    return prev, pg, g, dst


@pytest.mark.parametrize("name", rc.names())
def test_device_matches_host(pt, dev, hosts, name):
    case, ref = rc.all_cases()[name]
    H, W = case["guides"].shape
    prev, pg, g, dst = upload(pt, dev, case)
    dst.write(np.full((H, W, 4), 3.0, F))                         # every pixel must be rewritten
    first = prev.reproject(pg, case["prev_cam"], g, case["cam"], params(pt), out=dst).read()
    dst.write(np.full((H, W, 4), -5.0, F))
    second = prev.reproject(pg, case["prev_cam"], g, case["cam"], params(pt), out=dst).read()
    assert np.array_equal(bits(first), bits(second))
    same = rc.same_bits(first, hosts[name])
    assert same.all(), np.argwhere(~same)[:5]
    same = rc.same_bits(first, ref)                               # and so the numpy restatement
    assert same.all(), np.argwhere(~same)[:5]
    assert prev.read().tobytes() == case["prev_accum"].tobytes()  # the inputs are never written
    assert pg.read().tobytes() == case["prev_guides"].tobytes()
    assert g.read().tobytes() == case["guides"].tobytes()
    for x in (dst, g, pg, prev):
        x.close()


def test_errors_leave_dst_untouched(pt, dev):
    N = pt._native
    L = N.hip_lib()
    case, _ = rc.all_cases()["identity-16x16"]
    prev, pg, g, dst = upload(pt, dev, case)
    small, small_guides = pt.SampleBuffer(dev, 16, 15), pt.DenoiseGuides(dev, 15, 16)
    marker = np.full((16, 16, 4), 5.0, F)
    dst.write(marker)
    small.write(marker[:15])
    pc, c = case["prev_cam"], case["cam"]
    P = pt.ReprojectParameters

    def fails(call):
        with pytest.raises(pt.PathTracerError) as e:
            call()
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    fails(lambda: prev.reproject(pg, pc, g, c, out=prev))                  # prev is dst
    fails(lambda: prev.reproject(pg, pc, pg, c, out=dst))                  # prev_guides is guides
    fails(lambda: prev.reproject(small_guides, pc, g, c, out=dst))         # prev and prev_guides differ in size
    fails(lambda: small.reproject(pg, pc, g, c, out=dst))
    fails(lambda: prev.reproject(pg, pc, g, c, out=small))                 # dst and guides differ in size
    fails(lambda: prev.reproject(pg, pc, small_guides, c, out=dst))
    for bad in (P(NormalCosine=-1.0), P(NormalCosine=1.01), P(DepthTolerance=0.0), P(MinWeight=0.0),
                P(MinWeight=1.5), P(MaxHistory=0.0), P(MaxHistory=float("nan"))):
        fails(lambda: prev.reproject(pg, pc, g, c, bad, out=dst))
    ok = P().as_struct()
    cs = N.pt_packed_camera.from_buffer_copy(c.tobytes())
    args = [dev.handle, prev.handle, pg.handle, C.byref(cs), g.handle, C.byref(cs), C.byref(ok), dst.handle]
    for i in range(len(args)):
        a = list(args)
        a[i] = None
        assert L.ptReprojectSampleBuffer(*a) != 0, i
    assert np.array_equal(bits(dst.read()), bits(marker))                  # nothing was written
    assert np.array_equal(bits(small.read()), bits(marker[:15]))
    assert prev.read().tobytes() == case["prev_accum"].tobytes()
    assert L.ptReprojectSampleBuffer(*args) == 0                           # and the good call goes through
    assert not np.array_equal(bits(dst.read()), bits(marker))
    for x in (small_guides, small, dst, g, pg, prev):
        x.close()


def test_kernel_stats_count_one_launch_per_call(pt, dev):
    case, _ = rc.all_cases()["resize"]
    prev, pg, g, dst = upload(pt, dev, case)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    for _ in range(3):
        prev.reproject(pg, case["prev_cam"], g, case["cam"], out=dst)
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_REPROJECT)
    dev.set_profiling(False)
    assert n == 3 and ms > 0
    assert pt.KERNEL_REPROJECT == 10
    for x in (dst, g, pg, prev):
        x.close()


def test_end_to_end(pt, dev):
    """Config 1 at 64x32: 8 rounds; the camera moves through the scene API;
    FrameHistory.begin_frame reprojects into a fresh buffer, which equals
    reproject_host on the read-back inputs; a renderer with ACCUMULATE then
    adds 2 rounds on top.  Reset's raygen clears every pixel of its sample
    buffer (as the reference's restart does, basic_scatter.glsl:334; pinned
    at the end of this test), so the frame's order is reset(), begin_frame(),
    run(2): the reset comes before the reprojection, not after it.  Against
    the same reset(), run(2) on a zeroed buffer (same FrameIndex, so the same
    samples): after.w = reprojected.w + fresh.w.
    fresh.w is a small integer k, added to the buffer one sample at a time,
    so after.w went through at most k additions and the right-hand side
    through one: the two differ by at most (k + 1) roundings of 2^-23
    relative each."""
    W, H = 64, 32
    flags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    history = pt.FrameHistory(dev, W, H)
    sb0 = pt.SampleBuffer(dev, W, H)
    assert history.begin_frame(ds, 0, sb0) is False                       # nothing to carry yet
    r0 = pt.BasicRenderer(dev, ds, sb0)
    r0.RenderFlags = flags
    r0.reset()
    r0.run(8)
    accum0, guides0, cam0 = sb0.read(), history.guides.read(), history.camera.copy()
    assert (accum0[..., 3] > 0).mean() > 0.5

    scene.move_camera(scene.find_camera(0), position=(0.5, -4.0, 1.0), rotation=(float(np.pi / 2), 0.0, 0.1))
    scene.pack()
    ds.update(scene)
    sb1, sb2 = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    sb2.write(np.zeros((H, W, 4), F))
    renderers = []
    for sb in (sb1, sb2):
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = flags
        r.FrameIndex = 100
        r.reset()
        renderers.append(r)
    assert history.begin_frame(ds, 0, sb1) is True
    reprojected = sb1.read()
    guides1, cam1 = history.guides.read(), history.camera.copy()
    assert cam1.tobytes() == scene.arrays()["cameras"][0].tobytes() != cam0.tobytes()
    host = pt.reproject_host(accum0, guides0, cam0, guides1, cam1)
    assert np.array_equal(bits(reprojected), bits(host))
    have = reprojected[..., 3] > 0
    assert 0.25 < have.mean() < 0.95                                       # a history, and disocclusions
    assert np.array_equal(bits(sb0.read()), bits(accum0))                  # the old frame is not written
    stats = sb1.statistics()
    assert stats.empty == int((~have).sum())

    for r in renderers:
        r.run(2)
    assert renderers[0].FrameIndex == renderers[1].FrameIndex
    after, fresh = sb1.read(), sb2.read()
    k = fresh[..., 3].astype(np.float64)
    assert np.array_equal(k, np.round(k)) and k.max() >= 1
    expect = reprojected[..., 3].astype(np.float64) + k
    assert np.all(np.abs(after[..., 3] - expect) <= (k + 1) * 2.0 ** -23 * expect)
    assert np.all(after[..., 3] >= reprojected[..., 3])
    assert np.isfinite(after).all()
    renderers[0].reset()                                                   # why the reset comes first
    assert not sb1.read().any()
    for x in (*renderers, r0, sb2, sb1, sb0, history, ds):
        x.close()
    scene.close()
