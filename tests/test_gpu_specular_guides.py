"""GPU: the guides that follow mirrors and smooth glass.
guides_kernel's SPECULAR instantiation against the restated chain
(tests/specular_guides_restatement.py) bit for bit in every field, on the
benchmark scenes with a glass sphere, a crafted scene and a scene whose
traversal stack spills; zero bounces against the plain kernel; the consumers
(filter, reprojection, FrameHistory) on the new records; the argument
errors."""
from __future__ import annotations

import numpy as np
import pytest

import specular_guides_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
MESH_INSTANCE = 0          # PT_SHAPE_TYPE_MESH_INSTANCE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def render(pt, dev, ds, camera, W, H, bounces):
    guides = pt.DenoiseGuides(dev, W, H)
    guides.render(ds, camera, specular_bounces=bounces)
    got = guides.read()
    guides.close()
    return got


def assert_same_records(got, ref):
    """The four views of test_gpu_denoise.check_guides."""
    assert np.array_equal(got["shape"], ref["shape"]), ("shape", np.argwhere(got["shape"] != ref["shape"])[:5])
    for f in ("normal", "time", "albedo"):
        bad = np.argwhere(bits(got[f]) != bits(ref[f]))
        assert bad.size == 0, (f, bad[:5])


def check(pt, dev, key, scene, camera, W, H, bounces):
    """The device's records of `scene` equal the restated ones; (records, trace, stack need)."""
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    got = render(pt, dev, ds, camera, W, H, bounces)
    stack = ds.stack_needed
    ds.close()
    ref, trace = sc.reference(key, scene, camera, W, H, bounces)
    assert_same_records(got, ref)
    return ref, trace, stack


@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_c2_matches_restatement(pt, dev, bounces):
    scene = pt.Scene.config(2)
    ref, trace, _ = check(pt, dev, "c2", scene, 0, 64, 64, bounces)
    scene.close()
    assert (trace["bounces"] > 0).sum() >= 100                            # the glass sphere
    assert trace["bounces"].max() == min(bounces, 2)                      # in and out


@pytest.mark.parametrize("camera", [0, 1], ids=["thin-lens", "360"])
def test_c5_matches_restatement(pt, dev, camera):
    """Rays the sphere refracted go on through the room's mesh instance,
    which encloses the scene: the lane's own ray is what TlasStep restores
    when it leaves the BLAS.  (The records cannot show that a ray passed
    through a BLAS; test_crafted_scene_matches_restatement has chains that
    end inside one.)"""
    scene = pt.Scene.config(5)
    assert (scene.arrays()["shapes"]["Type"] == MESH_INSTANCE).any()
    ref, trace, _ = check(pt, dev, "c5", scene, camera, 64, 32, 8)
    scene.close()
    followed = trace["bounces"] > 0
    assert followed.sum() >= 10
    assert (followed & (ref["shape"] != NONE)).sum() >= 10               # chains that end on a surface


def test_crafted_scene_matches_restatement(pt, dev, tmp_path):
    """Facing mirrors, a glass slab, a per-texel roughness, a chain that
    starts on a mesh (tests/test_specular_guides.py checks that the scene
    shows each of them)."""
    scene, idx = sc.crafted(pt, tmp_path)
    ref, trace, _ = check(pt, dev, "crafted", scene, 0, 64, 32, 8)
    scene.close()
    assert (ref["shape"] >> 16 == idx["mesh_mirror"] + 1).sum() >= 10
    assert trace["bounces"].max() >= 3


def test_spilled_stack_after_a_bounce(pt, dev, tmp_path):
    scene, spheres = sc.mirrored_chain(pt, tmp_path)
    ref, trace, stack = check(pt, dev, "chain", scene, 0, 64, 32, 8)
    scene.close()
    assert stack > 20
    hit = ref["shape"] != NONE
    tag, shape = ref["shape"] >> 16, ref["shape"] & 0xFFFF
    on_other_sphere = hit & (tag > 0) & np.isin(shape, spheres) & (shape + 1 != tag)
    assert on_other_sphere.any()
    assert (trace["bounces"] > 0).sum() >= 20


def test_zero_bounces_are_the_plain_kernel(pt, dev):
    """ptRenderDenoiseGuidesSpecular(0) against ptRenderDenoiseGuides; at 8
    bounces only the pixels whose primary hit is followed change (191 of
    them by the restatement: the glass sphere)."""
    W = H = 64
    L = pt._native.hip_lib()
    scene = pt.Scene.config(2)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    plain = render(pt, dev, ds, 0, W, H, 0)
    guides = pt.DenoiseGuides(dev, W, H)
    guides.write(np.zeros((H, W), pt.DENOISE_GUIDE_DTYPE))
    assert L.ptRenderDenoiseGuidesSpecular(dev.handle, ds.handle, guides.handle, 0, 0) == 0
    assert guides.read().tobytes() == plain.tobytes()
    guides.close()
    deep = render(pt, dev, ds, 0, W, H, 8)
    ds.close()
    _, trace = sc.reference("c2", scene, 0, W, H, 8)
    scene.close()
    followed = trace["bounces"] > 0
    assert deep[~followed].tobytes() == plain[~followed].tobytes()
    differ = (deep.view(np.uint8).reshape(H, W, -1) != plain.view(np.uint8).reshape(H, W, -1)).any(-1)
    assert differ.sum() >= 40 and not differ[~followed].any()
    # a scene without a metal or translucent material: nothing to follow at any cap
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    assert render(pt, dev, ds, 0, W, H, 8).tobytes() == render(pt, dev, ds, 0, W, H, 0).tobytes()
    ds.close()
    scene.close()


def test_a_second_render_gives_the_same_bits(pt, dev):
    scene = pt.Scene.config(5)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    first = render(pt, dev, ds, 1, 64, 32, 8)
    second = pt.DenoiseGuides(dev, 64, 32)
    stale = np.zeros((32, 64), pt.DENOISE_GUIDE_DTYPE)
    stale["time"], stale["shape"] = 7.0, 7
    second.write(stale)                                                   # every record is rewritten
    second.render(ds, 1, specular_bounces=8)
    assert second.read().tobytes() == first.tobytes()
    for x in (second, ds):
        x.close()
    scene.close()


def test_consumers_take_the_records(pt, dev):
    """C2 at 64x32, 8 rounds.  The filter and the reprojection read the new
    records as they read any: the device equals the host on the same guides.
    Then FrameHistory(follow_shapes=True, specular_bounces=8) across an
    object move: a tagged pixel's shape word lies beyond the motion table, so
    it carries no history."""
    W, H = 64, 32
    flags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    scene = pt.Scene.config(2)
    pebble = scene.create_entity(pt.ENTITY_SPHERE, position=(-1.0, -2.0, 0.3), scale=(0.3, 0.3, 0.3))
    scene.pack()
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    history = pt.FrameHistory(dev, W, H, follow_shapes=True, specular_bounces=8)
    sb0 = pt.SampleBuffer(dev, W, H)
    assert history.begin_frame(ds, 0, sb0) is False
    r0 = pt.BasicRenderer(dev, ds, sb0)
    r0.RenderFlags = flags
    r0.reset()
    r0.run(8)
    accum0, guides0, cam0 = sb0.read(), history.guides.read(), history.camera.copy()
    shapes0 = scene.arrays()["shapes"].copy()
    tagged0 = (guides0["shape"] != NONE) & (guides0["shape"] >> 16 != 0)
    assert tagged0.sum() >= 40
    assert_same_records(guides0, sc.reference("c2-pebble", scene, 0, W, H, 8)[0])

    filtered = sb0.denoise(history.guides)
    assert np.array_equal(bits(filtered.read()), bits(pt.denoise_host(accum0, guides0)))
    filtered.close()

    # a small camera move, the entities where they were: row 8 with the two specular guide sets
    scene.move_camera(scene.find_camera(0), position=(0.3, -10.0, 3.1), rotation=(float(np.pi / 2), 0.0, 0.02))
    scene.pack()
    ds.update(scene)
    moved = pt.DenoiseGuides(dev, W, H)
    moved.render(ds, 0, specular_bounces=8)
    cam1 = ds.cameras[0].copy()
    out = sb0.reproject(history.guides, cam0, moved, cam1)
    host = pt.reproject_host(accum0, guides0, cam0, moved.read(), cam1)
    assert np.array_equal(bits(out.read()), bits(host))
    assert (host[..., 3] > 0).mean() > 0.25
    for x in (out, moved):
        x.close()

    # the camera back, the pebble moved: row 9 through FrameHistory
    scene.move_camera(scene.find_camera(0), position=(0.0, -10.0, 3.0), rotation=(float(np.pi / 2), 0.0, 0.0))
    scene.set_transform(pebble, position=(-0.8, -2.0, 0.3), scale=(0.3, 0.3, 0.3))
    scene.pack()
    ds.update(scene)
    table = pt.shape_motion(shapes0, scene.arrays()["shapes"])
    assert int(table["Flags"][scene.shape_index(pebble)]) == 1
    sb1 = pt.SampleBuffer(dev, W, H)
    sb1.write(np.zeros((H, W, 4), F))
    assert history.begin_frame(ds, 0, sb1) is True
    carried, guides1 = sb1.read(), history.guides.read()
    assert np.array_equal(bits(carried), bits(pt.reproject_host(accum0, guides0, cam0, guides1, history.camera,
                                                               motion=table)))
    tagged1 = (guides1["shape"] != NONE) & (guides1["shape"] >> 16 != 0)
    assert tagged1.sum() >= 40 and not carried[tagged1].any()
    assert (carried[~tagged1][:, 3] > 0).mean() > 0.5                    # the rest kept theirs
    for x in (r0, sb1, sb0, history, ds):
        x.close()
    scene.close()


def test_bad_arguments_launch_nothing(pt, dev):
    N = pt._native
    L = N.hip_lib()
    W, H = 32, 16
    scene = pt.Scene.config(2)
    ds, unpacked = pt.DeviceScene(dev), pt.DeviceScene(dev)
    ds.update(scene)
    guides = pt.DenoiseGuides(dev, W, H)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    guides.render(ds, 0, specular_bounces=N.GUIDE_MAX_BOUNCES)
    dev.synchronize()
    before = dev.kernel_stats(pt.KERNEL_GUIDES)
    assert before[0] == 1
    written = guides.read()
    calls = [(dev.handle, ds.handle, guides.handle, 0, N.GUIDE_MAX_BOUNCES + 1),           # too many bounces
             (None, ds.handle, guides.handle, 0, 1), (dev.handle, None, guides.handle, 0, 1),
             (dev.handle, ds.handle, None, 0, 1),                                            # NULL handles
             (dev.handle, unpacked.handle, guides.handle, 0, 1),                             # a scene without packs
             (dev.handle, ds.handle, guides.handle, len(scene.arrays()["cameras"]), 1)]      # camera out of range
    other = pt.Device(1) if pt.device_count() > 1 else None
    if other is not None:                                                                    # a scene of another device
        far = pt.DeviceScene(other)
        far.update(scene)
        calls.append((dev.handle, far.handle, guides.handle, 0, 1))
    for args in calls:
        assert L.ptRenderDenoiseGuidesSpecular(*args) != 0, args
        assert len(L.ptGetLastError()) > 0
    with pytest.raises(pt.PathTracerError):
        guides.render(ds, 0, specular_bounces=N.GUIDE_MAX_BOUNCES + 1)
    dev.synchronize()
    assert dev.kernel_stats(pt.KERNEL_GUIDES)[0] == before[0]
    dev.set_profiling(False)
    assert guides.read().tobytes() == written.tobytes()
    if other is not None:
        far.close()
        other.close()
    for x in (guides, unpacked, ds):
        x.close()
    scene.close()
