"""CPU: visibility gathered at caller-given points on the
host: include/pt_visibility.h compiled into libptscene.so
(ptsGatherVisibilityRays, ptsGatherVisibilityReduce, ptsVisibilitySkip)
against the numpy restatement bit for bit and against row 14's restatement,
the definition's two properties through the oracle's ray query, the lobe's
statistics, the argument checks of every new entry point and the
surface-point helper."""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np
import pytest

import gather_restatement as gr
import oracle_lib
import visibility_restatement as vr

NONE = 0xFFFFFFFF
INF = float("inf")
HIP_SYMBOLS = ("ptGatherVisibility", "ptGatherVisibilityChunked")
SCENE_SYMBOLS = ("ptsGatherVisibilityRays", "ptsGatherVisibilityReduce", "ptsVisibilitySkip")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_records(a, b):
    """Every field of two record arrays as integers."""
    return a.dtype.itemsize == b.dtype.itemsize == 32 and np.array_equal(
        np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def oracle_occluded(scene, o, v, d):
    return oracle_lib.trace_rays(scene.packs(), o, v, d)["shape_material"] != NONE


# --- exports and signatures -----------------------------------------------------------

def test_libraries_export_the_entry_points(pt):
    N = pt._native
    for name in HIP_SYMBOLS:
        assert hasattr(N.hip_lib(), name) and name in N.HIP_API, name
    for name in SCENE_SYMBOLS:
        assert hasattr(N.scene_lib(), name) and name in N.SCENE_API, name


def test_structs_and_python_surface(pt):
    N = pt._native
    assert C.sizeof(N.pt_visibility_gather_parameters) == 20
    assert [f[0] for f in N.pt_visibility_gather_parameters._fields_] == ["Samples", "Radius", "Seed", "Offset",
                                                                          "FirstIndex"]
    assert N.VISIBILITY_RECORD_DTYPE == gr.RECORD_DTYPE and N.VISIBILITY_RECORD_DTYPE.itemsize == 32
    assert [N.VISIBILITY_RECORD_DTYPE.fields[k][1] for k in ("Bent", "Unoccluded", "OccludedMask", "Samples",
                                                              "Reserved")] == [0, 12, 16, 24, 28]
    p = pt.VisibilityGatherParameters()
    assert (p.Samples, p.Radius, p.Seed, p.Offset, p.FirstIndex) == (16, INF, 0, 1e-3, 0)
    q = pt.VisibilityGatherParameters(Samples=4, Radius=0.5, Seed=9, Offset=0.25, FirstIndex=7).as_struct()
    assert (q.Samples, q.Radius, q.Seed, q.Offset, q.FirstIndex) == (4, 0.5, 9, 0.25, 7)
    with pytest.raises(ValueError):
        pt.VisibilityGatherParameters(FirstIndex=1 << 32).as_struct()
    sig = inspect.signature(pt.DeviceScene.gather_visibility)
    assert list(sig.parameters)[1:8] == ["points", "normals", "samples", "radius", "seed", "offset", "first_index"]
    assert [sig.parameters[k].default for k in ("samples", "radius", "seed", "offset", "first_index")] == [16, INF, 0, 1e-3, 0]
    import path_tracer_amd.integrator as integrator
    for name in ("VisibilityGatherParameters", "gather_visibility_rays_host", "gather_visibility_reduce_host",
                 "shape_surface_points"):
        assert name in pt.__all__ and getattr(integrator, name) is getattr(pt, name), name


# --- argument checks -------------------------------------------------------------------

def test_device_entry_points_reject_null_arguments(pt):
    L = pt._native.hip_lib()
    out = np.full(2, 0x5A, np.uint8).repeat(32).view(pt.VISIBILITY_RECORD_DTYPE)
    keep = out.copy()
    p = pt._native.pt_visibility_gather_parameters(16, 1.0, 0, 1e-3, 0)
    x = np.zeros(3, np.float32)
    fp = pt._native.fptr(x)
    assert L.ptGatherVisibility(None, None, 1, fp, fp, C.byref(p), out.ctypes.data) != 0
    assert b"null" in L.ptGetLastError()
    assert L.ptGatherVisibility(None, None, 0, None, None, C.byref(p), None) != 0
    assert L.ptGatherVisibilityChunked(None, None, 1, fp, fp, C.byref(p), 64, out.ctypes.data) != 0
    assert b"null" in L.ptGetLastError()
    assert same_records(out, keep)


def test_host_rays_argument_checks(pt):
    N = pt._native
    L = N.scene_lib()
    P = np.zeros((2, 3), np.float32)
    Nr = np.tile(np.array([0, 0, 1], np.float32), (2, 1))
    o, v, d = np.full((128, 3), 5.0, np.float32), np.full(128, 5, np.uint32), np.full(128, 5.0, np.float32)

    def call(samples=4, radius=1.0, offset=1e-3, first=0, n=2, points=P, out=o):
        p = N.pt_visibility_gather_parameters(samples, radius, 0, offset, first)
        return L.ptsGatherVisibilityRays(C.byref(p), n, None if points is None else N.fptr(points), N.fptr(Nr),
                                         None if out is None else N.fptr(out), N.u32ptr(v), N.fptr(d))

    for samples in (0, 3, 5, 48, 65, 128):
        assert call(samples=samples) != 0, samples
    for radius in (0.0, -1.0, float("nan")):
        assert call(radius=radius) != 0, radius
    for offset in (-1e-3, INF, -INF, float("nan")):
        assert call(offset=offset) != 0, offset
    assert call(first=0xFFFFFFFF) != 0                      # FirstIndex + 2 > 2^32
    assert call(n=(1 << 26) + 1) != 0
    assert call(points=None) != 0 and call(out=None) != 0
    assert L.ptsGatherVisibilityRays(None, 2, N.fptr(P), N.fptr(Nr), N.fptr(o), N.u32ptr(v), N.fptr(d)) != 0
    assert np.all(o == 5.0) and np.all(v == 5) and np.all(d == 5.0)
    assert call(first=0xFFFFFFFE) == 0                      # FirstIndex + 2 == 2^32
    assert call(samples=64, radius=INF, offset=0.0) == 0 and not np.any(v == 5) and np.all(d == 1048576.0)
    p = N.pt_visibility_gather_parameters(4, 1.0, 0, 1e-3, 0)
    assert L.ptsGatherVisibilityRays(C.byref(p), 0, None, None, None, None, None) == 0
    with pytest.raises(pt.PathTracerError):
        pt.gather_visibility_rays_host(P, Nr, pt.VisibilityGatherParameters(Samples=3))
    with pytest.raises(ValueError):
        pt.gather_visibility_rays_host(P, Nr[:1])


def test_host_reduce_argument_checks(pt):
    N = pt._native
    L = N.scene_lib()
    v = np.zeros(128, np.uint32)
    w = np.zeros(2, np.uint64)
    wp = w.ctypes.data_as(C.POINTER(C.c_uint64))
    out = np.full(2, 0x5A, np.uint8).repeat(32).view(pt.VISIBILITY_RECORD_DTYPE)
    keep = out.copy()
    for samples in (0, 3, 65, 128):
        assert L.ptsGatherVisibilityReduce(samples, 2, N.u32ptr(v), wp, out.ctypes.data) != 0, samples
    assert L.ptsGatherVisibilityReduce(4, 2, None, wp, out.ctypes.data) != 0
    assert L.ptsGatherVisibilityReduce(4, 2, N.u32ptr(v), None, out.ctypes.data) != 0
    assert L.ptsGatherVisibilityReduce(4, 2, N.u32ptr(v), wp, None) != 0
    assert L.ptsGatherVisibilityReduce(4, (1 << 26) + 1, N.u32ptr(v), wp, out.ctypes.data) != 0
    assert same_records(out, keep)
    assert L.ptsGatherVisibilityReduce(4, 0, None, None, None) == 0
    assert L.ptsGatherVisibilityReduce(64, 2, N.u32ptr(v), wp, out.ctypes.data) == 0 and not same_records(out, keep)
    with pytest.raises(ValueError):
        pt.gather_visibility_reduce_host(4, v[:6], np.zeros(6, bool))
    with pytest.raises(ValueError):
        pt.gather_visibility_reduce_host(4, v[:8], np.zeros(7, bool))


# --- the LCG skip ----------------------------------------------------------------------

def test_skip_equals_sequential_stepping(pt):
    L = pt._native.scene_lib()
    for s0 in (0, 1, 0x9E3779B9, 0xFFFFFFFF):
        state = s0
        for steps in range(127):
            assert L.ptsVisibilitySkip(s0, steps) == state, (s0, steps)
            state = gr.lcg(state, 1)
    for steps in (65537, 1000003):
        assert L.ptsVisibilitySkip(12345, steps) == gr.lcg(12345, steps), steps
    # two steps of 2^31 are 2^32 steps, the generator's full period
    half = L.ptsVisibilitySkip(777, 1 << 31)
    assert half != 777 and L.ptsVisibilitySkip(half, 1 << 31) == 777
    assert L.ptsVisibilitySkip(L.ptsVisibilitySkip(777, 0xFFFFFFFF), 1) == 777


# --- the rays against the restatements --------------------------------------------------

@pytest.mark.parametrize("config", [1, 2, 3])
def test_header_on_the_host_equals_the_restatement(pt, config):
    """ptsGatherVisibilityRays makes sample k directly (the skip); the
    restatement steps every stream sequentially.  Origins, packed words and
    durations, bit for bit, on the surface points of a config."""
    scene, P, Nr = gr.config_points(pt, config)
    assert len(P) > 500
    for samples, seed, first in ((1, 3, 0), (4, 3, 65530), (64, 11, 0)):
        for offset, radius in ((0.0, INF), (1e-3, 0.5), (0.05, INF)):
            p = pt.VisibilityGatherParameters(samples, radius, seed, offset, first)
            o, v, d = pt.gather_visibility_rays_host(P, Nr, p)
            ro, rv, rd = gr.rays(P, Nr, samples, radius, seed, offset, first)
            assert o.shape == (len(P) * samples, 3)
            assert np.array_equal(bits(o), bits(ro)), (config, samples, offset)
            assert np.array_equal(v, rv), (config, samples, offset)
            assert np.array_equal(bits(d), bits(rd)) and d[0] == (0.5 if radius == 0.5 else 1048576.0)


@pytest.mark.parametrize("config", [1, 2, 3])
def test_rays_equal_row_14s_restatement(pt, config):
    """An independent reading: row 14's sample_rays for pixel (j & 0xFFFF,
    j >> 16) with the primary ray arriving along -N at time 0 gives the same
    rays at Offset 1e-3.  It forms P + 0 * V, which turns a -0 component of P
    into +0: such points are left out."""
    scene, P, Nr = gr.config_points(pt, config)
    keep = ~np.any((P == 0) & np.signbit(P), axis=1)
    assert keep.sum() > 500
    first, seed, S = 65000, 3, 16
    j = first + np.arange(len(P))
    o, v, _ = pt.gather_visibility_rays_host(P, Nr, pt.VisibilityGatherParameters(S, INF, seed, 1e-3, first))
    so, sv = vr.sample_rays(j & 0xFFFF, j >> 16, seed, S, P, -Nr, np.zeros(len(P), np.float32), Nr)
    assert np.array_equal(bits(o).reshape(-1, S, 3)[keep], bits(so)[keep])
    assert np.array_equal(v.reshape(-1, S)[keep], sv[keep])


# --- the reduction ---------------------------------------------------------------------

@pytest.mark.parametrize("samples", [1, 2, 4, 8, 16, 32, 64])
def test_reduce_equals_the_numpy_tree(pt, samples):
    rng = np.random.default_rng(samples)
    n = 301
    dirs = rng.normal(size=(n * samples, 3)).astype(np.float32)
    packed = oracle_lib.pack_unit_vectors(dirs / np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32))
    for name, occ in (("random", rng.random(n * samples) < 0.5), ("sparse", rng.random(n * samples) < 0.05),
                      ("all", np.ones(n * samples, bool)), ("none", np.zeros(n * samples, bool))):
        got = pt.gather_visibility_reduce_host(samples, packed, occ)
        ref = gr.reduce(samples, packed, occ)
        assert same_records(got, ref), (samples, name)
        assert np.all(got["Reserved"] == 0) and np.all(got["Samples"] == samples)
        assert np.all(got["OccludedMask"] >> np.uint64(samples - 1) <= 1)
        assert np.array_equal(got["Unoccluded"], samples - occ.reshape(n, samples).sum(axis=1))
    assert np.all(pt.gather_visibility_reduce_host(samples, packed, np.ones(n * samples, bool))["Bent"] == 0.0)


# --- the definition's two properties ----------------------------------------------------

def test_nesting_and_partition_independence(pt):
    scene, P, Nr = gr.config_points(pt, 2)
    P, Nr = P[:2079], Nr[:2079]
    full = pt.VisibilityGatherParameters(64, 0.5, 3, 1e-3, 0)
    o, v, d = pt.gather_visibility_rays_host(P, Nr, full)
    occ = oracle_occluded(scene, o, v, d)
    rec = pt.gather_visibility_reduce_host(64, v, occ)
    assert 0.02 < occ.mean() < 0.98
    for S in (16, 4, 1):
        so, sv, sd = pt.gather_visibility_rays_host(P, Nr, pt.VisibilityGatherParameters(S, 0.5, 3, 1e-3, 0))
        assert np.array_equal(bits(so), bits(o.reshape(-1, 64, 3)[:, :S].reshape(-1, 3)))
        assert np.array_equal(sv, v.reshape(-1, 64)[:, :S].reshape(-1))
        small = pt.gather_visibility_reduce_host(S, sv, oracle_occluded(scene, so, sv, sd))
        assert np.array_equal(small["OccludedMask"], rec["OccludedMask"] & np.uint64((1 << S) - 1))
    parts = []
    for a, b in ((0, 1000), (1000, 2079)):
        po, pv, pd = pt.gather_visibility_rays_host(P[a:b], Nr[a:b], pt.VisibilityGatherParameters(64, 0.5, 3, 1e-3, a))
        assert np.array_equal(bits(po), bits(o[a * 64:b * 64])) and np.array_equal(pv, v[a * 64:b * 64])
        parts.append(pt.gather_visibility_reduce_host(64, pv, oracle_occluded(scene, po, pv, pd)))
    assert same_records(np.concatenate(parts), rec)


# --- lobe statistics ------------------------------------------------------------------

def test_cosine_lobe_mean(pt):
    """Nothing occludes in an empty scene, so Bent is the sum of all 64
    directions.  The cosine lobe's mean cosine is 2/3 with variance 1/18: over
    65 536 rays the standard error is 0.0009, and 0.005 is five of them."""
    e = pt.Scene.empty()
    e.pack()
    rng = np.random.default_rng(15)
    Nr = rng.normal(size=(1024, 3))
    Nr = (Nr / np.linalg.norm(Nr, axis=1, keepdims=True)).astype(np.float32)
    P = rng.uniform(-3, 3, (1024, 3)).astype(np.float32)
    o, v, d = pt.gather_visibility_rays_host(P, Nr, pt.VisibilityGatherParameters(64, INF, 1))
    occ = oracle_occluded(e, o, v, d)
    assert not occ.any()
    rec = pt.gather_visibility_reduce_host(64, v, occ)
    assert np.all(rec["Unoccluded"] == 64.0) and np.all(rec["OccludedMask"] == 0)
    mean = float(np.mean(np.einsum("ij,ij->i", rec["Bent"].astype(np.float64), Nr.astype(np.float64)) / 64.0))
    print(f"mean cosine {mean:.5f}")
    assert abs(mean - 2.0 / 3.0) < 0.005
    e.close()


# --- the surface-point helper -----------------------------------------------------------

def test_surface_points_of_a_transformed_quad(pt):
    s = pt.Scene.empty()
    m = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Clay", BaseColor=(0.8, 0.8, 0.8))
    pos = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    mesh = s.create_mesh(pos, np.array([(0, 1, 2), (0, 2, 3)], np.uint32), nrm, name="Quad")
    angle, scale, at = 0.5, np.array([2.0, 3.0, 1.5]), np.array([0.25, -0.5, 1.0])
    e = s.create_entity(pt.ENTITY_MESH_INSTANCE, position=tuple(at), rotation=(angle, 0.0, 0.0), scale=tuple(scale),
                        material=m)
    s.set_mesh(e, mesh)
    s.pack()
    shape = s.arrays()["shapes"][0]
    P, Nr, index = pt.shape_surface_points(s, 0)
    assert P.dtype == Nr.dtype == np.float32 and index.dtype == np.uint32
    assert len(P) == 4 and len(np.unique(index)) == 4
    # the packed matrix itself, applied by hand (column-major, column 3 the translation) ...
    M = shape["Transform"]["To"].astype(np.float64).reshape(4, 4).T
    expect = pos.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    order = np.lexsort(expect.T)
    assert np.abs(P[np.lexsort(P.astype(np.float64).T)] - expect[order]).max() < 1e-6
    # ... and the analytic placement: scale, a rotation about one axis, translation
    assert np.abs(np.linalg.norm(P - at.astype(np.float32), axis=1) - np.hypot(2.0, 3.0)).max() < 1e-5
    n0 = M[:3, :3] @ np.array([0.0, 0.0, 1.0])     # a plane's normal under a rotation and an in-plane scale
    n0 /= np.linalg.norm(n0)
    assert np.abs(Nr - n0).max() < 1e-6
    assert abs(abs(n0 @ np.array([0.0, 0.0, 1.0])) - np.cos(angle)) < 1e-6
    with pytest.raises(ValueError):
        pt.shape_surface_points(s, 1)
    s.close()
    scene, _, _ = gr.config_points(pt, 2)
    with pytest.raises(ValueError):
        pt.shape_surface_points(scene, 0)          # a cube, not a mesh


def test_surface_points_of_the_room_mesh(pt):
    scene, _, _ = gr.config_points(pt, 3)
    a = scene.arrays()
    assert int(a["shapes"][0]["Type"]) == 0
    P, Nr, index = pt.shape_surface_points(a, 0)
    ranges, stack = [], [int(a["shapes"][0]["MeshRootNodeIndex"])]
    while stack:
        node = a["mesh_nodes"][stack.pop()]
        if node["FaceEndIndex"] > 0:
            ranges.append((int(node["FaceBeginOrNodeIndex"]), int(node["FaceEndIndex"])))
        else:
            stack += [int(node["FaceBeginOrNodeIndex"]), int(node["FaceBeginOrNodeIndex"]) + 1]
    lo, hi = min(r[0] for r in ranges), max(r[1] for r in ranges)
    assert sum(e - b for b, e in ranges) == hi - lo          # the leaves tile one face range
    f = a["mesh_faces"][lo:hi]
    distinct = np.unique(np.concatenate([f["VertexIndex0"], f["VertexIndex1"], f["VertexIndex2"]]))
    assert len(P) == len(distinct) > 1000 and np.array_equal(np.sort(index), distinct)
    assert np.abs(np.linalg.norm(Nr.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    root = a["shape_nodes"][0]
    assert np.all(P >= root["Minimum"]) and np.all(P <= root["Maximum"])
    scene_again = pt.shape_surface_points(scene, 0)
    assert np.array_equal(scene_again[0], P) and np.array_equal(scene_again[2], index)
