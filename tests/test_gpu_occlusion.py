"""GPU: the any-hit occlusion query (ptOccludedRays).

The any-hit traversal is Trace() stopped at its first accepted intersection,
a prefix of the closest-hit traversal of the same ray, so a ray's bit must
equal "ptTraceRays hits" and "the oracle's Trace() hits" exactly: on every
extend form and stack format, with a spilled stack, with durations on either
side of and exactly at the closest hit, and for every batch size around the
wave and block boundaries."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fuzz_scenes
import oracle_lib
from rays import random_rays
from test_gpu_mesh_extend import AUTO, GENERAL, MESH, chain_mesh, mesh_scene, upload

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CASES = ["c1", "c2", "c3", "c5", "fuzz1", "fuzz2", "fuzz3", "fuzz4"]
_batches = {}


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def batch(pt, case):
    """(scene, rays, the oracle's hit mask) of a case, built once and left unchanged."""
    if case not in _batches:
        s = pt.Scene.config(int(case[1:])) if case[0] == "c" else fuzz_scenes.build(pt, int(case[4:]))[0]
        o, v, d = random_rays(s.arrays(), 4096, 7)
        ref = oracle_lib.trace_rays(s.packs(), o, v, d)["shape_material"] != NONE
        _batches[case] = (s, (o, v, d), ref)
    return _batches[case]


def hits(ds, o, v, d):
    return ds.trace_rays(o, v, d)["shape_material"] != NONE


@pytest.mark.parametrize("case", CASES)
def test_mask_equals_the_closest_hit_query(pt, dev, case):
    """4096 random rays per scene, both extend forms, the three stack formats:
    the mask equals ptTraceRays' hits and the oracle's.  Between 10 % and 90 %
    of each batch is occluded (the oracle: C1 46.9 %, C2 50.8 %, C3 15.3 %, C5
    49.7 %, fuzz 1-4 44.7-46.0 %), so no constant mask passes."""
    s, (o, v, d), ref = batch(pt, case)
    share = ref.mean()
    print(f"{case}: {100 * share:.1f} % of the batch occluded (oracle)")
    assert 0.10 <= share <= 0.90
    ds = pt.DeviceScene(dev)
    forms = set()
    for form in (AUTO, GENERAL):
        for fmt in (0, 1, 2):
            upload(pt, dev, s, form=form, stack_format=fmt, ds=ds)
            forms.add(ds.extend_form)
            got = ds.occluded(o, v, d)
            assert got.dtype == bool and got.shape == ref.shape
            assert np.array_equal(got, hits(ds, o, v, d)), (case, form, fmt)
            assert np.array_equal(got, ref), (case, form, fmt)
    assert GENERAL in forms
    print(f"{case}: extend forms run {sorted(forms)}")
    ds.close()


def chain_rays(n=2048):
    """Rays along the chain (each sets a far child aside at every level) and across it."""
    rng = np.random.default_rng(5)
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = rng.uniform(-40.0, -2.0, n)
    o[:, 1:] = rng.normal(0.0, 0.3, (n, 2)) + [0.0, 1.0]
    dirs = np.zeros((n, 3))
    dirs[:, 0] = 1.0
    dirs[:, 1:] = rng.normal(0.0, 0.02, (n, 2))
    dirs[n // 2:] = rng.normal(size=(n - n // 2, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    v = oracle_lib.pack_unit_vectors(dirs.astype(np.float32))
    return o, v, np.full(n, 1048576.0 * 4096.0, np.float32)


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["stack16", "stack32-packed", "stack32-node-index"])
def test_spilled_stack(pt, dev, fmt):
    """A chain mesh more than 20 levels deep: entries beyond the 20 in LDS
    take the per-ray spill rows, in the mesh-only and in the general loop."""
    c = mesh_scene(pt, chain_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.1), scale=(1.0, 1.0, 1.0))
    o, v, d = chain_rays()
    ref = oracle_lib.trace_rays(c.packs(), o, v, d)["shape_material"] != NONE
    assert 0.10 <= ref.mean() <= 0.90 and ref[:1024].any() and ref[1024:].any()
    dm = upload(pt, dev, c, stack_format=fmt)
    dg = upload(pt, dev, c, form=GENERAL, stack_format=fmt)
    assert dm.extend_form == MESH and dg.extend_form == GENERAL and dm.stack_needed > 20
    for ds in (dm, dg):
        got = ds.occluded(o, v, d)
        assert np.array_equal(got, hits(ds, o, v, d))
        assert np.array_equal(got, ref)
    steps_any, steps_all = dg.occluded_stats(o, v, d)[1], dg.trace_rays_stats(o, v, d)[1]
    assert np.all(steps_any <= steps_all) and np.array_equal(steps_any[~ref], steps_all[~ref])
    for x in (dm, dg, c):
        x.close()


def test_duration_boundary(pt, dev):
    """The rays of a C2 batch that hit, with each ray's duration set to its
    closest-hit time, one ulp below and one ulp above: whether a hit at
    exactly the duration counts is each shape's own rule (a plane, sphere or
    face at t == duration is accepted, a cube is not), and the any-hit loop
    restates none of them.  The oracle has 12.1 %, 0 % and 76.8 % occluded."""
    s = pt.Scene.config(2)
    o, v, d = random_rays(s.arrays(), 2048, 11)
    first = oracle_lib.trace_rays(s.packs(), o, v, d)
    h = first["shape_material"] != NONE
    o, v, t = o[h], v[h], first["time"][h].astype(np.float32)
    assert len(t) > 512
    ds = pt.DeviceScene(dev)
    shares = []
    for form in (AUTO, GENERAL):
        upload(pt, dev, s, form=form, ds=ds)
        for dur in (t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))):
            ref = oracle_lib.trace_rays(s.packs(), o, v, dur)["shape_material"] != NONE
            got = ds.occluded(o, v, dur)
            assert np.array_equal(got, hits(ds, o, v, dur))
            assert np.array_equal(got, ref)
            shares.append(ref.mean())
    print("occluded at t, t - ulp, t + ulp:", ["%.1f %%" % (100 * x) for x in shares[:3]])
    assert 0.0 < shares[0] < 1.0 and shares[1] < shares[0] < shares[2] < 1.0
    ds.close()
    s.close()


def raw_mask(pt, dev, ds, n, o, v, d, words):
    N = pt._native
    return N.hip_lib().ptOccludedRays(dev.handle, ds.handle, n, N.fptr(o), N.u32ptr(v), N.fptr(d),
                                      words.ctypes.data_as(C.POINTER(C.c_uint64)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4133])
def test_sizes_and_tail_bits(pt, dev, n):
    """The caller pre-fills the words with ones: every word is written, the
    last word's bits at and above n are 0, and the words beyond are untouched."""
    s, (o, v, d), ref = batch(pt, "c2")
    k = np.arange(n) % len(v)
    o, v, d, ref = np.ascontiguousarray(o[k]), np.ascontiguousarray(v[k]), np.ascontiguousarray(d[k]), ref[k]
    ds = upload(pt, dev, s)
    count = (n + 63) // 64
    words = np.full(count + 2, 0xFFFFFFFFFFFFFFFF, np.uint64)
    assert raw_mask(pt, dev, ds, n, o, v, d, words) == 0
    assert np.all(words[count:] == 0xFFFFFFFFFFFFFFFF)
    got = np.unpackbits(words[:count].view(np.uint8), bitorder="little")
    assert np.array_equal(got[:n].astype(bool), ref)
    assert not got[n:].any()
    assert np.array_equal(ds.occluded(o, v, d), ref)
    ds.close()


def test_empty_batch_empty_scene_and_a_lone_sphere(pt, dev):
    s, (o, v, d), ref = batch(pt, "c1")
    ds = upload(pt, dev, s)
    words = np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)
    assert raw_mask(pt, dev, ds, 0, o, v, d, words) == 0
    assert pt._native.hip_lib().ptOccludedRays(dev.handle, ds.handle, 0, None, None, None, None) == 0
    assert np.all(words == 0xFFFFFFFFFFFFFFFF)
    assert ds.occluded(o[:0], v[:0], d[:0]).shape == (0,)
    counters, steps = ds.occluded_stats(o[:0], v[:0], d[:0])
    assert counters["rays"] == 0 and steps.shape == (0,)
    ds.close()

    e = pt.Scene.empty()
    cam = e.create_entity(pt.ENTITY_CAMERA, position=(0.0, -6.0, 1.0), rotation=(1.45, 0.0, 0.0))
    e.set_camera_pinhole(cam, fov_degrees=55.0)
    e.pack()
    de = upload(pt, dev, e)
    assert not de.occluded(o[:300], v[:300], d[:300]).any()
    assert not hits(de, o[:300], v[:300], d[:300]).any()
    de.close()
    e.close()

    ball = mesh_scene(pt, None, only_sphere=True)
    bo, bv, bd = random_rays(ball.arrays(), 1000, 3)
    bref = oracle_lib.trace_rays(ball.packs(), bo, bv, bd)["shape_material"] != NONE
    assert 0.02 < bref.mean() < 0.98
    for form in (AUTO, GENERAL):
        db = upload(pt, dev, ball, form=form)
        assert db.extend_form == GENERAL
        assert np.array_equal(db.occluded(bo, bv, bd), bref)
        db.close()
    ball.close()


@pytest.mark.parametrize("case", CASES)
def test_any_hit_takes_a_prefix_of_the_steps(pt, dev, case):
    """ptOccludedRaysStats against ptTraceRaysStats: per ray the any-hit steps
    are at most the closest-hit steps and equal where nothing occludes; the
    counters agree on the rays.  The ratio of the step sums over the occluded
    rays is printed (a measurement)."""
    s, (o, v, d), ref = batch(pt, case)
    ds = upload(pt, dev, s)
    ca, sa = ds.occluded_stats(o, v, d)
    cc, sc = ds.trace_rays_stats(o, v, d)
    assert ca["rays"] == cc["rays"] == len(v)
    assert np.all(sa <= sc)
    assert np.array_equal(sa[~ref], sc[~ref])
    assert int(sa.sum()) == ca["lane_steps"] and int(sc.sum()) == cc["lane_steps"]
    assert sa[ref].sum() <= sc[ref].sum()
    print(f"{case}: any-hit / closest-hit steps over the occluded rays {sa[ref].sum() / sc[ref].sum():.3f}, "
          f"over the batch {sa.sum() / sc.sum():.3f}")
    ds.close()
