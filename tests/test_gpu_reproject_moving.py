"""GPU: the moving-shape reprojection.  The device
kernel against the host implementation bit for bit on every case of
tests/reproject_moving_cases.py and, without a table or with a table of
unmoved shapes, against ptReprojectSampleBuffer on every case of
tests/reproject_cases.py; the position-coded history on the device result;
the argument errors; the kernel counter; and the whole path render -> move a
shape -> FrameHistory(follow_shapes=True).begin_frame -> accumulate on top."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import reproject_cases as rc
import reproject_moving_cases as mc

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(pt, p=mc.PARAMS):
    return pt.ReprojectParameters(p["normal_cosine"], p["depth_tolerance"], p["min_weight"], p["max_history"])


def upload(pt, dev, case):
    Hp, Wp = case["prev_guides"].shape
    H, W = case["guides"].shape
    prev, dst = pt.SampleBuffer(dev, Wp, Hp), pt.SampleBuffer(dev, W, H)
    pg, g = pt.DenoiseGuides(dev, Wp, Hp), pt.DenoiseGuides(dev, W, H)
    prev.write(case["prev_accum"])
    pg.write(case["prev_guides"])
    g.write(case["guides"])
    return prev, pg, g, dst


def on_device(pt, dev, case, motion, p):
    prev, pg, g, dst = upload(pt, dev, case)
    out = prev.reproject(pg, case["prev_cam"], g, case["cam"], p, out=dst, motion=motion).read()
    for x in (dst, g, pg, prev):
        x.close()
    return out


@pytest.mark.parametrize("name", mc.names())
def test_device_matches_host(pt, dev, name):
    case, ref, _ = mc.all_cases()[name]
    H, W = case["guides"].shape
    host = pt.reproject_host(case["prev_accum"], case["prev_guides"], case["prev_cam"], case["guides"], case["cam"],
                             params(pt), motion=case["motion"])
    prev, pg, g, dst = upload(pt, dev, case)
    dst.write(np.full((H, W, 4), 3.0, F))                         # every pixel must be rewritten
    first = prev.reproject(pg, case["prev_cam"], g, case["cam"], params(pt), out=dst, motion=case["motion"]).read()
    dst.write(np.full((H, W, 4), -5.0, F))
    second = prev.reproject(pg, case["prev_cam"], g, case["cam"], params(pt), out=dst, motion=case["motion"]).read()
    assert np.array_equal(bits(first), bits(second))              # two calls, the same bits
    same = rc.same_bits(first, host)
    assert same.all(), np.argwhere(~same)[:5]
    same = rc.same_bits(first, ref)                               # and so the numpy restatement
    assert same.all(), np.argwhere(~same)[:5]
    assert prev.read().tobytes() == case["prev_accum"].tobytes()  # the inputs are never written
    assert pg.read().tobytes() == case["prev_guides"].tobytes()
    assert g.read().tobytes() == case["guides"].tobytes()
    for x in (dst, g, pg, prev):
        x.close()


@pytest.mark.parametrize("name", rc.names() + ["scene-96x54", "scene-17x16"])
def test_no_table_and_unmoved_tables_give_row_8(pt, dev, name):
    """ptReprojectSampleBufferMoving with NULL, 0 and with a table of unmoved
    shapes: ptReprojectSampleBuffer's bits, on row 8's cases and on two of the
    scene's (whose shapes then count as unmoved)."""
    case = (rc.all_cases() if name in rc.all_cases() else mc.all_cases())[name][0]
    N = pt._native
    L = N.hip_lib()
    p = params(pt, rc.PARAMS)
    prev, pg, g, dst = upload(pt, dev, case)
    row8 = prev.reproject(pg, case["prev_cam"], g, case["cam"], p, out=dst).read()
    shapes = case["guides"]["shape"]
    count = int(shapes[shapes != NONE].max()) + 1 if (shapes != NONE).any() else 1
    packed = np.zeros(count, pt.SHAPE_DTYPE)
    packed["Transform"]["To"][:] = packed["Transform"]["From"][:] = np.eye(4, dtype=F).reshape(-1)
    table = pt.shape_motion(packed, packed)
    dst.write(np.full(row8.shape, 3.0, F))
    out = prev.reproject(pg, case["prev_cam"], g, case["cam"], p, out=dst, motion=table).read()
    assert np.array_equal(bits(out), bits(row8))
    dst.write(np.full(row8.shape, 3.0, F))
    pc = N.pt_packed_camera.from_buffer_copy(case["prev_cam"].tobytes())
    c = N.pt_packed_camera.from_buffer_copy(case["cam"].tobytes())
    ps = p.as_struct()
    assert L.ptReprojectSampleBufferMoving(dev.handle, prev.handle, pg.handle, C.byref(pc), g.handle, C.byref(c), None,
                                           0, C.byref(ps), dst.handle) == 0
    assert np.array_equal(bits(dst.read()), bits(row8))
    for x in (dst, g, pg, prev):
        x.close()


def test_position_coded_history_follows_the_surface(pt, dev):
    """tests/test_reproject_moving.py's check on the device's result."""
    mc.position_coded_check(lambda case, motion: on_device(pt, dev, case, motion, params(pt, mc.DEFAULTS)))


def test_errors_leave_dst_untouched(pt, dev):
    N = pt._native
    L = N.hip_lib()
    case, _, _ = mc.all_cases()["scene-17x16"]
    prev, pg, g, dst = upload(pt, dev, case)
    small, small_guides = pt.SampleBuffer(dev, 17, 15), pt.DenoiseGuides(dev, 15, 16)
    marker = np.full((16, 17, 4), 5.0, F)
    dst.write(marker)
    small.write(marker[:15])
    pc, c, m = case["prev_cam"], case["cam"], case["motion"]
    P = pt.ReprojectParameters
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)

    def fails(call):
        with pytest.raises(pt.PathTracerError) as e:
            call()
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    fails(lambda: prev.reproject(pg, pc, g, c, out=prev, motion=m))                  # prev is dst
    fails(lambda: prev.reproject(pg, pc, pg, c, out=dst, motion=m))                  # prev_guides is guides
    fails(lambda: prev.reproject(small_guides, pc, g, c, out=dst, motion=m))         # prev and prev_guides differ in size
    fails(lambda: small.reproject(pg, pc, g, c, out=dst, motion=m))
    fails(lambda: prev.reproject(pg, pc, g, c, out=small, motion=m))                 # dst and guides differ in size
    fails(lambda: prev.reproject(pg, pc, small_guides, c, out=dst, motion=m))
    for bad in (P(NormalCosine=-1.0), P(NormalCosine=1.01), P(DepthTolerance=0.0), P(MinWeight=0.0),
                P(MinWeight=1.5), P(MaxHistory=0.0), P(MaxHistory=float("nan"))):
        fails(lambda: prev.reproject(pg, pc, g, c, bad, out=dst, motion=m))
    ok = P().as_struct()
    cs = N.pt_packed_camera.from_buffer_copy(c.tobytes())
    args = [dev.handle, prev.handle, pg.handle, C.byref(cs), g.handle, C.byref(cs), m.ctypes.data, len(m),
            C.byref(ok), dst.handle]
    for i in range(len(args)):
        if i == 7:
            continue
        a = list(args)
        a[i] = None                                                        # i == 6: a count without a table
        assert L.ptReprojectSampleBufferMoving(*a) != 0, i
    a = list(args)
    a[6], a[7], a[9] = None, 0, None                                       # no table: row 8's own checks
    assert L.ptReprojectSampleBufferMoving(*a) != 0
    dev.synchronize()
    assert dev.kernel_stats(pt.KERNEL_REPROJECT)[0] == 0                   # nothing was launched
    assert np.array_equal(bits(dst.read()), bits(marker))                  # nothing was written
    assert np.array_equal(bits(small.read()), bits(marker[:15]))
    assert prev.read().tobytes() == case["prev_accum"].tobytes()
    assert L.ptReprojectSampleBufferMoving(*args) == 0                     # and the good call goes through
    dev.synchronize()
    assert dev.kernel_stats(pt.KERNEL_REPROJECT)[0] == 1
    dev.set_profiling(False)
    assert not np.array_equal(bits(dst.read()), bits(marker))
    for x in (small_guides, small, dst, g, pg, prev):
        x.close()


def test_kernel_stats_count_one_launch_per_call(pt, dev):
    """With a table, with none, and with tables of growing length (the device's buffer is reallocated)."""
    case, _, _ = mc.all_cases()["scene-64x40-50x37"]
    prev, pg, g, dst = upload(pt, dev, case)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    big = np.concatenate([case["motion"]] * 50)
    tables = (case["motion"], None, case["motion"][:2], big, case["motion"])
    outs = [prev.reproject(pg, case["prev_cam"], g, case["cam"], params(pt), out=dst, motion=m).read() for m in tables]
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_REPROJECT)
    dev.set_profiling(False)
    assert n == len(tables) and ms > 0
    assert np.array_equal(bits(outs[0]), bits(outs[3])) and np.array_equal(bits(outs[0]), bits(outs[4]))
    assert np.array_equal(bits(outs[0]), bits(mc.all_cases()["scene-64x40-50x37"][1]))
    assert np.array_equal(bits(outs[2]), bits(mc.all_cases()["table-cut"][1]))
    for x in (dst, g, pg, prev):
        x.close()


def test_end_to_end(pt, dev):
    """The test scene at 64x36: 8 rounds; the sphere moves through the scene
    API; FrameHistory(follow_shapes=True).begin_frame reprojects into a fresh
    buffer, which equals reproject_host with the table of the two packs on the
    read-back inputs; a renderer with ACCUMULATE then adds 2 rounds on top.
    As in tests/test_gpu_reproject.py: the frame's order is reset(),
    begin_frame(), run(2); against the same reset(), run(2) on a zeroed buffer,
    after.w = reprojected.w + fresh.w to within (k + 1) roundings of 2^-23
    relative.  The sphere's pixels carry history (w > 2): at least the 75 %
    of them that the position-coded test requires to have all four taps valid
    at the same move, and more of them than the default history
    (follow_shapes=False) leaves any."""
    W, H = 64, 36
    flags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    scene, sphere, cube = mc.build_scene(pt)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    shapes0 = scene.arrays()["shapes"].copy()
    assert ds.shapes.tobytes() == shapes0.tobytes()
    history, plain = pt.FrameHistory(dev, W, H, follow_shapes=True), pt.FrameHistory(dev, W, H)
    assert plain.follow_shapes is False
    sb0 = pt.SampleBuffer(dev, W, H)
    assert history.begin_frame(ds, 0, sb0) is False and plain.begin_frame(ds, 0, sb0) is False
    r0 = pt.BasicRenderer(dev, ds, sb0)
    r0.RenderFlags = flags
    r0.reset()
    r0.run(8)
    accum0, guides0, cam0 = sb0.read(), history.guides.read(), history.camera.copy()

    scene.set_transform(sphere, position=mc.SPHERE[1])
    scene.pack()
    ds.update(scene)
    shapes1 = scene.arrays()["shapes"].copy()
    assert ds.shapes.tobytes() == shapes1.tobytes() != shapes0.tobytes()
    sb1, sb2, sb3 = (pt.SampleBuffer(dev, W, H) for _ in range(3))
    sb2.write(np.zeros((H, W, 4), F))
    renderers = []
    for sb in (sb1, sb2):
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = flags
        r.FrameIndex = 100
        r.reset()
        renderers.append(r)
    assert history.begin_frame(ds, 0, sb1) is True and plain.begin_frame(ds, 0, sb3) is True
    reprojected, unfollowed = sb1.read(), sb3.read()
    guides1, cam1 = history.guides.read(), history.camera.copy()
    table = pt.shape_motion(shapes0, shapes1)
    s = scene.shape_index(sphere)
    assert [int(f) for f in table["Flags"]] == [1 if i == s else 0 for i in range(len(table))]
    host = pt.reproject_host(accum0, guides0, cam0, guides1, cam1, motion=table)
    assert np.array_equal(bits(reprojected), bits(host))
    assert np.array_equal(bits(unfollowed), bits(pt.reproject_host(accum0, guides0, cam0, guides1, cam1)))
    assert np.array_equal(bits(sb0.read()), bits(accum0))                  # the old frame is not written

    for r in renderers:
        r.run(2)
    after, fresh = sb1.read(), sb2.read()
    k = fresh[..., 3].astype(np.float64)
    assert np.array_equal(k, np.round(k)) and k.max() >= 1
    expect = reprojected[..., 3].astype(np.float64) + k
    assert np.all(np.abs(after[..., 3] - expect) <= (k + 1) * 2.0 ** -23 * expect)
    assert np.isfinite(after).all()
    on_sphere = guides1["shape"] == s
    carried = (after[..., 3] > 2) & on_sphere
    print(f"sphere pixels {int(on_sphere.sum())}: with history {int(carried.sum())} (follow_shapes), "
          f"{int(((unfollowed[..., 3] > 0) & on_sphere).sum())} (default)")
    assert on_sphere.sum() > 50 and carried.sum() >= 0.75 * on_sphere.sum()
    assert carried.sum() > ((unfollowed[..., 3] > 0) & on_sphere).sum()
    for x in (*renderers, r0, sb3, sb2, sb1, sb0, plain, history, ds):
        x.close()
    scene.close()
