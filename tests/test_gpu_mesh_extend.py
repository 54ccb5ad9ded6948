"""GPU: the mesh-only extend loop of one-mesh scenes (traverse.hpp MeshStep).

A scene that is one mesh instance under a leaf TLAS root is traced by a loop
without the two-level machinery (dscene::single_mesh, classified at upload).
A ray's traversal performs the same operations in the same order, so every
hit, slot, pixel and counter must equal the CPU oracle's and the general
loop's (ptSetSceneExtendForm forces it) bit for bit.  Frames are smaller than
8 tiles with partial tiles; the renderers run unfused rounds, the launches
that take the new kernel."""
from __future__ import annotations

import numpy as np
import pytest

import fuzz_scenes
import oracle_lib
from test_gpu_parity import compare_hits, compare_state

pytestmark = pytest.mark.gpu

AUTO, GENERAL, MESH = 0, 1, 2   # PT_EXTEND_FORM_*
FLAGS = 3                       # ACCUMULATE | SAMPLE_JITTER
FAR = 1048576.0


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mesh_scene(pt, mesh_arrays, position=(0.3, 0.4, 0.2), rotation=(0.4, 0.3, 0.7), scale=(1.3, 0.8, 1.7),
               instances=1, sphere=False, only_sphere=False):
    """One camera and: `instances` instances of one mesh (the first at the
    given transform), a sphere beside them, or a sphere alone."""
    s = pt.Scene.empty()
    m = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Clay", BaseColor=(0.8, 0.6, 0.4))
    if not only_sphere:
        mesh = s.create_mesh(*mesh_arrays, name="Mesh")
        for i in range(instances):
            e = s.create_entity(pt.ENTITY_MESH_INSTANCE, position=tuple(p + 2.2 * i for p in position),
                                rotation=rotation, scale=scale, material=m)
            s.set_mesh(e, mesh)
    if sphere or only_sphere:
        s.create_entity(pt.ENTITY_SPHERE, position=(-1.9, 0.3, 0.1), scale=(0.7, 0.7, 0.7), material=m)
    s.set_root(skybox_brightness=1.2)
    cam = s.create_entity(pt.ENTITY_CAMERA, position=(0.0, -6.0, 1.0), rotation=(1.45, 0.0, 0.0))
    s.set_camera_pinhole(cam, fov_degrees=55.0)
    s.pack()
    return s


def blob(seed=3):
    return fuzz_scenes.blob_mesh(np.random.default_rng(seed), 8, 12, 0.15)   # 168 faces


def chain_mesh(links=56):
    """Triangles each twice the size and distance of the last (all within the
    fast division's coordinate range): the BVH is a chain about half as deep
    as the mesh has faces, and a ray fired along it sets aside a far child at
    every level."""
    pos, idx = [], []
    for i in range(links):
        c, r = 3.0 * 2.0 ** (i - 18), 0.5 * 2.0 ** (i - 18)
        pos += [(c, -r, 1.0 - r), (c, r, 1.0 - r), (c, 0.0, 1.0 + r)]
        idx.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(pos, np.float32), np.array(idx, np.uint32)


def upload(pt, dev, s, form=AUTO, stack_format=0, ds=None):
    ds = ds if ds is not None else pt.DeviceScene(dev)
    ds.set_extend_form(form)
    ds.set_stack_format(stack_format)
    ds.update(s)
    return ds


def gpu_render(pt, dev, ds, W, H, schedule, split=None, mask=None):
    """Reset + the schedule on unfused rounds: (state, accumulator, (rays, samples))."""
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = FLAGS
    r.set_fused_rounds(0)
    r.set_round_batch(1)
    if split is not None:
        r.set_split(split)
    r.reset()
    r.run(schedule[0])
    if mask is not None:
        r.set_active_tiles(mask)
    for rounds in schedule[1:]:
        if rounds == 1:
            r.run(1)
        else:
            r.run_rounds(rounds)
    dev.synchronize()
    out = (r.read_state(), sb.read(), r.stats(), r.FrameIndex)
    r.close()
    sb.close()
    return out


def assert_same_render(a, b):
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), "slot state differs"
    assert np.array_equal(bits(a[1]), bits(b[1])), "accumulator differs"
    assert a[2] == b[2] and a[3] == b[3]


def oracle_render(s, W, H, rounds):
    o = oracle_lib.OracleRenderer(s.packs(), W, H)
    o.RenderFlags = FLAGS
    o.reset()
    o.run(2)
    for _ in range(rounds):
        o.run(1)
    out = (o.state(), o.accum(), o.counters())
    o.close()
    return out


def special_rays(s, n, seed):
    """Rays around the scene, every wave a mix of ordinary rays and: axis-
    aligned directions (zero velocity components), origin components that are
    zero, tiny (below 2^-50) or huge (above 2^40), and Duration limits
    shorter than the first hit."""
    rng = np.random.default_rng(seed)
    box = s.arrays()["shape_nodes"][0]
    lo, hi = box["Minimum"].astype(np.float64) - 1.0, box["Maximum"].astype(np.float64) + 1.0
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    centre = 0.5 * (lo + hi)
    d = (centre + rng.normal(0.0, 0.6, size=(n, 3))) - o          # towards the mesh, roughly
    k = np.arange(n)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, -0.6, 0.8]], float)
    ax = k % 4 == 1                                               # a quarter of every wave
    d[ax] = axes[(k[ax] // 4) % len(axes)]
    for a in range(3):                                            # ... fired at the mesh along their axis
        sel = ax & (np.abs(d[:, a]) == 1.0)
        o[sel] = (centre + rng.normal(0.0, 0.4, size=(int(sel.sum()), 3))).astype(np.float32)
        o[sel, a] = np.where(d[sel, a] > 0, lo[a], hi[a]).astype(np.float32)
    odd = k % 8 == 2
    o[odd, (k[odd] // 8) % 3] = np.array([0.0, 1e-30, -1e-20, 3e12], np.float32)[(k[odd] // 24) % 4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    vel = oracle_lib.pack_unit_vectors(d.astype(np.float32))
    dur = np.full(n, FAR, np.float32)
    short = k % 8 == 5
    dur[short] = rng.uniform(0.01, 1.5, size=int(short.sum())).astype(np.float32)
    return o, vel, dur


def test_one_mesh_render_bit_exact(pt, dev):
    """Reset, Run(2) and 12 rounds of one transformed mesh instance: the
    mesh-only form against the oracle and against the general form."""
    s = mesh_scene(pt, blob())
    W, H = 48, 32
    dm = upload(pt, dev, s)
    dg = upload(pt, dev, s, form=GENERAL)
    assert dm.extend_form == MESH and dg.extend_form == GENERAL
    m = gpu_render(pt, dev, dm, W, H, [2] + [1] * 12)
    g = gpu_render(pt, dev, dg, W, H, [2] + [1] * 12)
    os_, oa, oc = oracle_render(s, W, H, 12)
    assert_same_render(m, g)
    compare_state(m[0], os_)
    assert oa[..., 3].sum() > 0 and (os_["hit"]["shape_material"] != 0xFFFFFFFF).any()
    assert np.array_equal(bits(m[1]), bits(oa))
    assert m[2] == oc
    for x in (dm, dg, s):
        x.close()


@pytest.mark.parametrize("rotation,position", [((0.4, 0.3, 0.7), (0.3, 0.4, 0.2)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))],
                         ids=["rotated", "axis-aligned"])
def test_trace_rays_special_cases(pt, dev, rotation, position):
    """ptTraceRays (the per-ray Duration source).  The unrotated, untranslated
    instance keeps the zero velocity components and the out-of-range origin
    components in the mesh's space, where the lanes then take the IEEE
    division beside the fast-division lanes of their wave."""
    s = mesh_scene(pt, blob(), position=position, rotation=rotation)
    o, v, d = special_rays(s, 4096, seed=17)
    ref = oracle_lib.trace_rays(s.packs(), o, v, d)
    hit = ref["shape_material"] != 0xFFFFFFFF
    k = np.arange(len(v))
    assert hit[k % 4 == 1].any() and hit[k % 8 == 2].any() and hit[k % 4 == 0].any()
    assert (~hit[k % 8 == 5]).any()
    dm = upload(pt, dev, s)
    dg = upload(pt, dev, s, form=GENERAL)
    assert dm.extend_form == MESH and dg.extend_form == GENERAL
    gm, gg = dm.trace_rays(o, v, d), dg.trace_rays(o, v, d)
    assert np.array_equal(gm.view(np.uint8), gg.view(np.uint8))
    compare_hits(gm, ref)
    for x in (dm, dg, s):
        x.close()


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["stack16", "stack32-packed", "stack32-node-index"])
def test_stack_formats_and_spill(pt, dev, fmt):
    """Every stack entry format in the mesh-only loop, on the blob and on a
    chain mesh more than 20 levels deep, whose entries beyond the 20 in LDS
    take the spill rows."""
    s = mesh_scene(pt, blob())
    o, v, d = special_rays(s, 2048, seed=23)
    dm = upload(pt, dev, s, stack_format=fmt)
    assert dm.extend_form == MESH
    compare_hits(dm.trace_rays(o, v, d), oracle_lib.trace_rays(s.packs(), o, v, d))
    dm.close()
    s.close()

    c = mesh_scene(pt, chain_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.1), scale=(1.0, 1.0, 1.0))
    rng = np.random.default_rng(5)
    n = 2048
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = rng.uniform(-40.0, -2.0, n)
    o[:, 1:] = rng.normal(0.0, 0.3, (n, 2)) + [0.0, 1.0]
    dirs = np.zeros((n, 3))
    dirs[:, 0] = 1.0
    dirs[:, 1:] = rng.normal(0.0, 0.02, (n, 2))
    dirs[n // 2:] = rng.normal(size=(n - n // 2, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    v = oracle_lib.pack_unit_vectors(dirs.astype(np.float32))
    d = np.full(n, FAR * 4096.0, np.float32)
    dm = upload(pt, dev, c, stack_format=fmt)
    dg = upload(pt, dev, c, form=GENERAL, stack_format=fmt)
    assert dm.extend_form == MESH and dm.stack_needed > 20
    gm = dm.trace_rays(o, v, d)
    assert np.array_equal(gm.view(np.uint8), dg.trace_rays(o, v, d).view(np.uint8))
    ref = oracle_lib.trace_rays(c.packs(), o, v, d)
    assert (ref["shape_material"] != 0xFFFFFFFF).sum() > n // 8
    compare_hits(gm, ref)
    for x in (dm, dg, c):
        x.close()


@pytest.mark.parametrize("kind", ["two-instances", "mesh-and-sphere", "one-sphere"])
def test_other_scenes_stay_general(pt, dev, kind):
    s = mesh_scene(pt, blob(), instances=2 if kind == "two-instances" else 1, sphere=kind == "mesh-and-sphere",
                   only_sphere=kind == "one-sphere")
    W, H = 40, 24
    da = upload(pt, dev, s)
    assert da.extend_form == GENERAL
    a = gpu_render(pt, dev, da, W, H, [2] + [1] * 4)
    os_, oa, oc = oracle_render(s, W, H, 4)
    compare_state(a[0], os_)
    assert np.array_equal(bits(a[1]), bits(oa)) and a[2] == oc
    o, v, d = special_rays(s, 1024, seed=29)
    compare_hits(da.trace_rays(o, v, d), oracle_lib.trace_rays(s.packs(), o, v, d))
    da.close()
    s.close()


def test_form_follows_scene_updates(pt, dev):
    """An editor's sequence on one device scene: one mesh, the mesh beside a
    sphere, the mesh alone again.  The form follows each upload (the kernel
    arguments of the mesh-only loop are rewritten with it) and every stage
    matches the oracle."""
    one = mesh_scene(pt, blob())
    two = mesh_scene(pt, blob(), sphere=True)
    moved = mesh_scene(pt, blob(5), position=(-0.4, 0.2, 0.5), rotation=(0.1, 0.9, 0.2), scale=(0.9, 1.4, 1.1))
    ds = pt.DeviceScene(dev)
    W, H = 40, 24
    for s, form in ((one, MESH), (two, GENERAL), (moved, MESH), (one, MESH)):
        ds.update(s)
        assert ds.extend_form == form
        g = gpu_render(pt, dev, ds, W, H, [2, 1, 1])
        os_, oa, oc = oracle_render(s, W, H, 2)
        compare_state(g[0], os_)
        assert np.array_equal(bits(g[1]), bits(oa)) and g[2] == oc
    # the switch takes effect at the next upload, whatever that upload touches
    ds.set_extend_form(GENERAL)
    assert ds.extend_form == MESH
    ds.update(one, pt.SCENE_DIRTY_CAMERAS)
    assert ds.extend_form == GENERAL
    ds.set_extend_form(AUTO)
    ds.update(one, pt.SCENE_DIRTY_CAMERAS)
    assert ds.extend_form == MESH
    L = pt._native.hip_lib()
    assert L.ptSetSceneExtendForm(ds.handle, 2) != 0 and L.ptSetSceneExtendForm(None, 0) != 0
    assert L.ptGetSceneExtendForm(ds.handle, None) != 0
    for x in (ds, one, two, moved):
        x.close()


def test_frame_schedules_match_general_form(pt, dev):
    """Tile groups forced on the small frame, an active-tile mask, and a
    ptRenderFrame whose target falls inside the guarded rounds: the same
    renderer in both forms."""
    s = mesh_scene(pt, blob())
    W, H = 48, 32
    dm = upload(pt, dev, s)
    dg = upload(pt, dev, s, form=GENERAL)
    assert dm.extend_form == MESH and dg.extend_form == GENERAL
    plain = gpu_render(pt, dev, dm, W, H, [2, 6])
    assert_same_render(gpu_render(pt, dev, dm, W, H, [2, 6], split=3), gpu_render(pt, dev, dg, W, H, [2, 6], split=3))
    assert_same_render(gpu_render(pt, dev, dm, W, H, [2, 6], split=3), plain)
    mask = np.array([[1, 0, 1], [0, 1, 1]], np.uint8)
    assert_same_render(gpu_render(pt, dev, dm, W, H, [2, 1, 4], mask=mask), gpu_render(pt, dev, dg, W, H, [2, 1, 4], mask=mask))
    out = []
    for ds in (dm, dg):
        sb = pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = FLAGS
        r.set_fused_rounds(0)
        r.set_round_batch(1)
        rounds, samples = r.render_frame(5 * W * H)
        dev.synchronize()
        out.append((r.read_state(), sb.read(), (rounds, samples) + r.stats(), r.FrameIndex))
        r.close()
        sb.close()
    assert_same_render(out[0], out[1])
    assert out[0][2][1] >= 5 * W * H and out[0][2][0] > 2
    for x in (dm, dg, s):
        x.close()
