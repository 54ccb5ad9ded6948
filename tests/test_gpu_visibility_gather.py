"""GPU: visibility gathered at caller-given points (ptGatherVisibility;
DESIGN.md §6 row 15).

The kernel runs one lane per (point, sample) over ptOccludedRays' any-hit
traversal, takes a point's mask from the wave's ballot and its bent vector
from cross-lane rounds.  Its records must equal, every field as integers, the
host twin's reduction (ptsGatherVisibilityReduce) of the bits that ptTraceRays
and the oracle's Trace() give on the restated rays: on every extend form and
stack format, with a spilled stack, at every segment, wave and block
boundary, in one launch or several.

The points of every test are hit points of rays.random_rays(arrays, 4096, 7)
through the oracle (gather_restatement.config_points); Seed 3, FirstIndex 0
unless the test is about them."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gather_restatement as gr
import oracle_lib
from test_gpu_mesh_extend import AUTO, GENERAL, MESH, chain_mesh, mesh_scene, upload
from test_gpu_occlusion import chain_rays

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
INF = float("inf")
SEED = 3
K_EXTEND = 1
_refs = {}


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def same_records(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def hits(ds, o, v, d):
    return ds.trace_rays(o, v, d)["shape_material"] != NONE


def mask_bits(rec, samples):
    """(n, samples) bools from the records' masks."""
    return ((rec["OccludedMask"][:, None] >> np.arange(samples, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def reference(pt, scene, key, P, Nr, samples, radius, first=0):
    """(rays, the oracle's bits, the expected records), computed once per key and left unchanged."""
    key = (key, len(P), samples, radius, first)
    if key not in _refs:
        o, v, d = gr.rays(P, Nr, samples, radius, SEED, 1e-3, first)
        occ = oracle_lib.trace_rays(scene.packs(), o, v, d)["shape_material"] != NONE
        _refs[key] = ((o, v, d), occ, pt.gather_visibility_reduce_host(samples, v, occ))
    return _refs[key]


def raw_gather(pt, dev, ds, P, Nr, params, out, n=None, max_lanes=None):
    N = pt._native
    n = len(Nr if P is None else P) if n is None else n
    pp = None if P is None else N.fptr(P)
    pn = None if Nr is None else N.fptr(Nr)
    po = None if out is None else out.ctypes.data
    ps = None if params is None else C.byref(params)
    if max_lanes is None:
        return N.hip_lib().ptGatherVisibility(dev.handle, ds.handle, n, pp, pn, ps, po)
    return N.hip_lib().ptGatherVisibilityChunked(dev.handle, ds.handle, n, pp, pn, ps, max_lanes, po)


def sentinel(pt, n):
    return np.full(n * 32, 0xA5, np.uint8).view(pt.VISIBILITY_RECORD_DTYPE)


# --- bit-exact parity -------------------------------------------------------------------

@pytest.mark.parametrize("radius", [INF, 0.5], ids=["sky", "r0.5"])
@pytest.mark.parametrize("samples", [16, 64])
@pytest.mark.parametrize("config", [2, 3, 5])
def test_records_equal_the_host_twin(pt, dev, config, samples, radius):
    """Both extend forms, the three stack formats.  The inputs can fail: from
    the oracle alone, between 10 % and 90 % of the rays are occluded and at
    least 20 % of the points have 0 < u < S (measured on the CPU: C2 60.6 % /
    58-63 % at radius inf and 12.3 % / 23-26 % at 0.5; C3 27.6-27.8 % / 54-57 %
    and 14.4-14.5 % / 36-45 %; C5 13.1-13.3 % / 30-42 % at radius inf).  C5 at
    radius 0.5 has 2.0 % occluded: no share is asserted for it, parity stays
    exact."""
    scene, P, Nr = gr.config_points(pt, config)
    (o, v, d), occ, expect = reference(pt, scene, config, P, Nr, samples, radius)
    share = occ.mean()
    u = expect["Unoccluded"]
    partial = np.mean((u > 0) & (u < samples))
    print(f"C{config} S={samples} radius={radius}: {len(P)} points, {100 * share:.1f} % of the rays occluded, "
          f"{100 * partial:.1f} % of the points with 0 < u < S (oracle)")
    if (config, radius) != (5, 0.5):
        assert 0.10 <= share <= 0.90
        assert partial >= 0.20
    ds = pt.DeviceScene(dev)
    forms = set()
    for form in (AUTO, GENERAL):
        for fmt in (0, 1, 2):
            upload(pt, dev, scene, form=form, stack_format=fmt, ds=ds)
            forms.add(ds.extend_form)
            got = ds.gather_visibility(P, Nr, samples, radius, SEED)
            assert got.dtype == pt.VISIBILITY_RECORD_DTYPE
            assert same_records(got, expect), (config, form, fmt)
            assert same_records(got, pt.gather_visibility_reduce_host(samples, v, hits(ds, o, v, d))), (config, form, fmt)
            assert np.array_equal(mask_bits(got, samples).reshape(-1), ds.occluded(o, v, d)), (config, form, fmt)
    assert GENERAL in forms
    ds.close()


# --- segment, wave and block boundaries ---------------------------------------------------

BOUNDARIES = ([(1, n) for n in (1, 63, 64, 65, 257)] + [(s, 37) for s in (2, 4, 8, 32)]
              + [(16, n) for n in (1, 3, 4, 5, 16, 17)] + [(64, n) for n in (1, 2, 4, 5)])


@pytest.mark.parametrize("samples,n", BOUNDARIES)
def test_segment_wave_and_block_boundaries(pt, dev, samples, n):
    """The output is pre-filled with a sentinel and has two extra records:
    records 0..n-1 are written whole (Reserved 0, no mask bit at or above S),
    the extra ones stay."""
    scene, P, Nr = gr.config_points(pt, 2)
    P, Nr = np.ascontiguousarray(P[100:100 + n]), np.ascontiguousarray(Nr[100:100 + n])
    _, occ, expect = reference(pt, scene, "c2-boundary", P, Nr, samples, INF)
    ds = upload(pt, dev, scene)
    out = sentinel(pt, n + 2)
    keep = out.copy()
    p = pt.VisibilityGatherParameters(samples, INF, SEED).as_struct()
    assert raw_gather(pt, dev, ds, P, Nr, p, out) == 0
    assert same_records(out[n:], keep[n:])
    assert same_records(out[:n], expect)
    assert np.all(out["Reserved"][:n] == 0) and np.all(out["Samples"][:n] == samples)
    if samples < 64:
        assert np.all(out["OccludedMask"][:n] >> np.uint64(samples) == 0)
    assert np.array_equal(mask_bits(out[:n], samples).reshape(-1), occ)
    ds.close()


# --- a spilled stack ----------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["stack16", "stack32-packed", "stack32-node-index"])
def test_spilled_stack(pt, dev, fmt):
    """The chain mesh more than 20 levels deep, points where chain_rays() hit
    it: the mesh-only and the general loop, in one launch and in launches of
    1024 lanes (the spill rows are as wide as a launch)."""
    c = mesh_scene(pt, chain_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.1), scale=(1.0, 1.0, 1.0))
    P, Nr = gr.hit_points(c, *chain_rays())
    assert len(P) > 200
    (o, v, d), occ, expect = reference(pt, c, "chain", P, Nr, 16, INF)
    print(f"chain: {len(P)} points, {100 * occ.mean():.1f} % of the rays occluded (oracle)")
    assert occ.any() and not occ.all()
    dm = upload(pt, dev, c, stack_format=fmt)
    dg = upload(pt, dev, c, form=GENERAL, stack_format=fmt)
    assert dm.extend_form == MESH and dg.extend_form == GENERAL and dm.stack_needed > 20
    p = pt.VisibilityGatherParameters(16, INF, SEED).as_struct()
    for ds in (dm, dg):
        got = ds.gather_visibility(P, Nr, 16, INF, SEED)
        assert same_records(got, expect)
        assert same_records(got, pt.gather_visibility_reduce_host(16, v, hits(ds, o, v, d)))
        out = sentinel(pt, len(P))
        assert raw_gather(pt, dev, ds, P, Nr, p, out, max_lanes=1024) == 0
        assert same_records(out, expect)
    for x in (dm, dg, c):
        x.close()


# --- nesting, partition independence, chunked launches -------------------------------------

def test_nesting_and_partition_independence(pt, dev):
    scene, P, Nr = gr.config_points(pt, 2)
    P, Nr = np.ascontiguousarray(P[:2079]), np.ascontiguousarray(Nr[:2079])
    ds = upload(pt, dev, scene)
    full = ds.gather_visibility(P, Nr, 64, 0.5, SEED)
    assert same_records(full, reference(pt, scene, "c2-nesting", P, Nr, 64, 0.5)[2])
    assert 0 < (full["Unoccluded"] < 64).mean() < 1
    for S in (16, 4, 1):
        small = ds.gather_visibility(P, Nr, S, 0.5, SEED)
        assert np.array_equal(small["OccludedMask"], full["OccludedMask"] & np.uint64((1 << S) - 1)), S
        assert np.all(small["Samples"] == S)
    a = ds.gather_visibility(P[:1000], Nr[:1000], 64, 0.5, SEED, first_index=0)
    b = ds.gather_visibility(P[1000:], Nr[1000:], 64, 0.5, SEED, first_index=1000)
    assert same_records(np.concatenate([a, b]), full)
    assert not same_records(ds.gather_visibility(P[1000:], Nr[1000:], 64, 0.5, SEED), full[1000:])   # FirstIndex matters
    ds.close()


@pytest.mark.parametrize("samples,max_lanes,launches", [(16, 4096, 9), (64, 64, 300), (1, 64, 33)])
def test_chunked_launches(pt, dev, samples, max_lanes, launches):
    """The test probe lowers the lanes per launch: the same records from
    several launches, each counted under PT_KERNEL_EXTEND."""
    scene, P, Nr = gr.config_points(pt, 2)
    n = {16: 2079, 64: 300, 1: 2079}[samples]
    P, Nr = np.ascontiguousarray(P[:n]), np.ascontiguousarray(Nr[:n])
    expect = reference(pt, scene, "c2-chunks", P, Nr, samples, INF)[2]
    ds = upload(pt, dev, scene)
    p = pt.VisibilityGatherParameters(samples, INF, SEED).as_struct()
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    out = sentinel(pt, n + 2)
    keep = out.copy()
    assert raw_gather(pt, dev, ds, P, Nr, p, out, max_lanes=max_lanes) == 0
    count, _ = dev.kernel_stats(K_EXTEND)
    assert count == launches == -(-n // (max_lanes // samples))
    dev.reset_kernel_stats()
    whole = ds.gather_visibility(P, Nr, samples, INF, SEED)
    assert dev.kernel_stats(K_EXTEND)[0] == 1
    dev.set_profiling(False)
    assert same_records(out[:n], expect) and same_records(out[n:], keep[n:])
    assert same_records(whole, expect)
    ds.close()


# --- an empty scene, an empty batch, invalid arguments --------------------------------------

def test_empty_scene_gives_the_full_tree_sum(pt, dev):
    scene, P, Nr = gr.config_points(pt, 3)
    e = pt.Scene.empty()
    cam = e.create_entity(pt.ENTITY_CAMERA, position=(0.0, -6.0, 1.0), rotation=(1.45, 0.0, 0.0))
    e.set_camera_pinhole(cam, fov_degrees=55.0)
    e.pack()
    de = upload(pt, dev, e)
    for S in (1, 16, 64):
        o, v, d = gr.rays(P, Nr, S, INF, SEED)
        expect = pt.gather_visibility_reduce_host(S, v, np.zeros(len(v), bool))
        got = de.gather_visibility(P, Nr, S, INF, SEED)
        assert same_records(got, expect)
        assert np.all(got["Unoccluded"] == S) and np.all(got["OccludedMask"] == 0)
    assert np.all(np.einsum("ij,ij->i", got["Bent"], Nr) > 0.3 * 64)
    de.close()
    e.close()


def test_empty_batch_writes_nothing(pt, dev):
    scene, P, Nr = gr.config_points(pt, 2)
    ds = upload(pt, dev, scene)
    out = sentinel(pt, 2)
    keep = out.copy()
    p = pt.VisibilityGatherParameters(16, INF, SEED).as_struct()
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    assert raw_gather(pt, dev, ds, P, Nr, p, out, n=0) == 0
    assert raw_gather(pt, dev, ds, None, None, p, None, n=0) == 0
    assert dev.kernel_stats(K_EXTEND)[0] == 0
    dev.set_profiling(False)
    assert same_records(out, keep)
    assert ds.gather_visibility(P[:0], Nr[:0]).shape == (0,)
    ds.close()


def test_invalid_arguments_fail_and_launch_nothing(pt, dev):
    N = pt._native
    scene, P, Nr = gr.config_points(pt, 2)
    P, Nr = np.ascontiguousarray(P[:8]), np.ascontiguousarray(Nr[:8])
    ds = upload(pt, dev, scene)
    bare = pt.DeviceScene(dev)           # never updated: no packs
    out = sentinel(pt, 8)
    keep = out.copy()
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)

    def params(samples=16, radius=1.0, offset=1e-3, first=0):
        return N.pt_visibility_gather_parameters(samples, radius, SEED, offset, first)

    for bad in (dict(samples=0), dict(samples=3), dict(samples=24), dict(samples=65), dict(samples=128),
                dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(offset=-1e-3),
                dict(offset=INF), dict(offset=float("nan")), dict(first=0xFFFFFFF9)):
        assert raw_gather(pt, dev, ds, P, Nr, params(**bad), out) != 0, bad
        assert b"ptGatherVisibility" in N.hip_lib().ptGetLastError()
    ok = params()
    assert raw_gather(pt, dev, ds, P, Nr, params(first=0xFFFFFFF8), sentinel(pt, 8)) == 0   # FirstIndex + n == 2^32
    launched = dev.kernel_stats(K_EXTEND)[0]
    assert launched == 1
    assert raw_gather(pt, dev, ds, None, Nr, ok, out) != 0 and raw_gather(pt, dev, ds, P, None, ok, out) != 0
    assert raw_gather(pt, dev, ds, P, Nr, None, out) != 0 and raw_gather(pt, dev, ds, P, Nr, ok, None) != 0
    L = N.hip_lib()
    assert L.ptGatherVisibility(None, ds.handle, 8, N.fptr(P), N.fptr(Nr), C.byref(ok), out.ctypes.data) != 0
    assert L.ptGatherVisibility(dev.handle, None, 8, N.fptr(P), N.fptr(Nr), C.byref(ok), out.ctypes.data) != 0
    assert raw_gather(pt, dev, bare, P, Nr, ok, out) != 0
    assert b"packs" in L.ptGetLastError()
    for lanes in (0, 63, (1 << 22) + 1):
        assert raw_gather(pt, dev, ds, P, Nr, ok, out, max_lanes=lanes) != 0, lanes
    assert raw_gather(pt, dev, ds, P, Nr, ok, out, n=(1 << 26) + 1) != 0
    if pt.device_count() > 1:
        other = pt.Device(1)
        assert L.ptGatherVisibility(other.handle, ds.handle, 8, N.fptr(P), N.fptr(Nr), C.byref(ok), out.ctypes.data) != 0
        assert b"another device" in L.ptGetLastError()
        other.close()
    assert dev.kernel_stats(K_EXTEND)[0] == launched
    dev.set_profiling(False)
    assert same_records(out, keep)
    with pytest.raises(pt.PathTracerError):
        ds.gather_visibility(P, Nr, samples=12)
    with pytest.raises(ValueError):
        ds.gather_visibility(P, Nr[:3])
    bare.close()
    ds.close()
