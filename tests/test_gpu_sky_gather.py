"""GPU: sky light gathered at caller-given points (ptGatherSkyLight; DESIGN.md
§6 row 16).

The kernel runs one lane per (point, sample) over ptOccludedRays' any-hit
traversal, looks the sky up along the open rays, multiplies by the nine
spherical harmonics and sums the 27 products by cross-lane rounds.  Its
records must equal, every field as integers, the host twin's reduction
(ptsSkyGatherReduce) of the oracle's any-hit bits and the numpy restatement's
contributions on the restated rays: on both lobes, every extend form and stack
format, with a spilled stack, at every segment, wave and block boundary, in
one launch or several.

The points of every test are hit points of rays.random_rays(arrays, 4096, 7)
through the oracle (gather_restatement.config_points); Seed 3, FirstIndex 0
unless the test is about them.  A ray's direction, L0 and contribution depend
on neither Samples nor Radius, so the restated rays and contributions are made
once per (scene, lobe) at 64 samples and sliced: the first S of a point's 64
are its rays at Samples = S (test_restated_rays_nest checks that of the
restatement itself).

M = 256 points: the smallest multiple of 64 from 256 up at which, on the CPU
and from the oracle and restatement alone, every (config, lobe, S, radius)
below has 10-90 % of its rays occluded and at least 20 % of its points with
0 < u < S (measured: C2 cosine 61.8-62.1 % / 52.7-59.4 % at radius inf and
13.6-14.1 % / 30.5-35.5 % at 0.5; C2 sphere 78.3 % / 76.2-94.1 % and
33.7-33.9 % / 98-100 %; C3 cosine 26.6-26.9 % / 52.7-55.9 % and 13.7-14.0 % /
34.0-45.3 %; C3 sphere 32.6 % / 93.4-99.6 % and 19.5-19.6 % / 68.8-90.6 %),
so no share condition is dropped."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gather_restatement as gr
import oracle_lib
import path_restatement as pr
import sky_gather_restatement as sr
from test_gpu_mesh_extend import AUTO, GENERAL, MESH, chain_mesh, mesh_scene, upload
from test_gpu_occlusion import chain_rays

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
INF = float("inf")
SEED = 3
K_EXTEND = 1
M = 256
COSINE, SPHERE = 0, 1
LOBES = pytest.mark.parametrize("lobe", [COSINE, SPHERE], ids=["cosine", "sphere"])
_sets = {}
_worlds = {}


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def same_records(a, b):
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize == 128 and np.array_equal(
        np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def mask_bits(rec, samples):
    """(n, samples) bools from the records' masks."""
    return ((rec["OccludedMask"][:, None] >> np.arange(samples, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


class RaySet:
    """The restated rays of n points at 64 samples for one scene and lobe, the
    oracle's bits per radius and the restated contributions, each computed
    once and left unchanged."""

    def __init__(self, scene, P, Nr, lobe, first=0):
        self.scene, self.n, self.lobe = scene, len(P), lobe
        self.o, self.v, _, self.l0 = sr.rays(P, Nr, 64, INF, SEED, 1e-3, first, lobe)
        if id(scene) not in _worlds:
            _worlds[id(scene)] = (scene, pr.World(scene))
        self.contrib = sr.Contributions(_worlds[id(scene)][1], self.v, self.l0)
        self.occ = {}

    def occluded(self, radius):
        if radius not in self.occ:
            d = np.full(len(self.v), gr.duration(radius), np.float32)
            self.occ[radius] = oracle_lib.trace_rays(self.scene.packs(), self.o, self.v, d)["shape_material"] != NONE
        return self.occ[radius]

    def expect(self, pt, samples, radius, n=None):
        """(packed words, the oracle's bits, contributions, expected records) of
        the first n points at `samples` samples."""
        n = self.n if n is None else n
        pick = (np.arange(n)[:, None] * 64 + np.arange(samples)[None, :]).reshape(-1)
        occ = self.occluded(radius)[pick]
        c = self.contrib.of(np.isin(np.arange(len(self.v)), pick[~occ]))[pick]
        v = self.v[pick]
        return v, occ, c, pt.sky_gather_reduce_host(samples, v, occ, c)


def ray_set(key, scene, P, Nr, lobe, first=0):
    key = (key, len(P), lobe, first)
    if key not in _sets:
        _sets[key] = RaySet(scene, P, Nr, lobe, first)
    return _sets[key]


def config_set(pt, config, lobe):
    scene, P, Nr = gr.config_points(pt, config)
    P, Nr = np.ascontiguousarray(P[:M]), np.ascontiguousarray(Nr[:M])
    return scene, P, Nr, ray_set(config, scene, P, Nr, lobe)


def gather(ds, P, Nr, samples, radius, lobe, **kw):
    return ds.gather_sky_light(P, Nr if lobe == COSINE else None, samples, radius, SEED, lobe=lobe, **kw)


def raw_gather(pt, dev, ds, P, Nr, params, out, n=None, max_lanes=None):
    N = pt._native
    n = len(Nr if P is None else P) if n is None else n
    pp = None if P is None else N.fptr(P)
    pn = None if Nr is None else N.fptr(Nr)
    po = None if out is None else out.ctypes.data
    ps = None if params is None else C.byref(params)
    if max_lanes is None:
        return N.hip_lib().ptGatherSkyLight(dev.handle, ds.handle, n, pp, pn, ps, po)
    return N.hip_lib().ptGatherSkyLightChunked(dev.handle, ds.handle, n, pp, pn, ps, max_lanes, po)


def sentinel(pt, n):
    return np.full(n * 128, 0xA5, np.uint8).view(pt.SKY_RECORD_DTYPE)


# --- the restatement's own nesting (CPU work, here because the GPU tests lean on it) ------

@LOBES
def test_restated_rays_nest(pt, lobe):
    scene, P, Nr, rs = config_set(pt, 2, lobe)
    for S in (16, 4, 1):
        o, v, d, l0 = sr.rays(P, Nr, S, 0.5, SEED, 1e-3, 0, lobe)
        pick = (np.arange(M)[:, None] * 64 + np.arange(S)[None, :]).reshape(-1)
        assert np.array_equal(o.view(np.uint32), rs.o[pick].view(np.uint32)) and np.array_equal(v, rs.v[pick])
        assert np.array_equal(l0.view(np.uint32), rs.l0[pick].view(np.uint32)) and np.all(d == 0.5)


# --- bit-exact parity -------------------------------------------------------------------

@LOBES
@pytest.mark.parametrize("radius", [INF, 0.5], ids=["sky", "r0.5"])
@pytest.mark.parametrize("samples", [16, 64])
@pytest.mark.parametrize("config", [2, 3])
def test_records_equal_the_restatement(pt, dev, config, samples, radius, lobe):
    """C2: textured sky, analytic shapes, the general loop.  C3: constant sky
    (the sky_flat path), the mesh-only loop and, forced, the general one.  The
    three stack formats each.  The inputs can fail: the conditions on them are
    asserted from the oracle and the restatement alone, before the device is
    asked."""
    scene, P, Nr, rs = config_set(pt, config, lobe)
    v, occ, c, expect = rs.expect(pt, samples, radius)
    share = occ.mean()
    u = expect["Unoccluded"]
    partial = np.mean((u > 0) & (u < samples))
    distinct = len(np.unique(c[~occ][:, 1]))
    print(f"C{config} S={samples} radius={radius} lobe={lobe}: {M} points, {100 * share:.1f} % of the rays occluded, "
          f"{100 * partial:.1f} % of the points with 0 < u < S, {distinct} distinct C.y among the open rays")
    assert 0.10 <= share <= 0.90
    assert partial >= 0.20
    if config == 2:
        assert distinct >= 16
    assert np.any(expect["SH"] != 0)
    ds = pt.DeviceScene(dev)
    forms = set()
    for form in (AUTO, GENERAL):
        for fmt in (0, 1, 2):
            upload(pt, dev, scene, form=form, stack_format=fmt, ds=ds)
            forms.add(ds.extend_form)
            got = gather(ds, P, Nr, samples, radius, lobe)
            assert got.dtype == pt.SKY_RECORD_DTYPE
            assert same_records(got, expect), (config, form, fmt)
    assert GENERAL in forms and (config != 3 or MESH in forms)
    ds.close()


@pytest.mark.parametrize("samples", [16, 64])
@pytest.mark.parametrize("config", [2, 3])
def test_cosine_mask_and_count_are_row_15s(pt, dev, config, samples):
    scene, P, Nr = gr.config_points(pt, config)
    ds = upload(pt, dev, scene)
    for radius in (INF, 0.5):
        sky = ds.gather_sky_light(P, Nr, samples, radius, SEED, 1e-3, 5)
        vis = ds.gather_visibility(P, Nr, samples, radius, SEED, 1e-3, 5)
        assert np.array_equal(sky["OccludedMask"], vis["OccludedMask"])
        assert np.array_equal(sky["Unoccluded"].view(np.uint32), vis["Unoccluded"].view(np.uint32))
        assert np.array_equal(sky["Samples"], vis["Samples"])
        assert 0 < (sky["Unoccluded"] < samples).mean() < 1
    ds.close()


# --- segment, wave and block boundaries ---------------------------------------------------

LANES = (1, 63, 64, 65, 255, 256, 257, 513)
BOUNDARIES = ([(S, L // S) for S in (1, 2, 16, 64) for L in LANES if L % S == 0]
              + [(2, 33), (2, 129), (4, 37), (8, 37), (32, 9), (16, 5), (16, 17), (16, 33), (64, 2), (64, 5), (64, 9)])


@pytest.mark.parametrize("samples,n", BOUNDARIES)
def test_segment_wave_and_block_boundaries(pt, dev, samples, n):
    """The output is pre-filled with a sentinel and has two extra records:
    records 0..n-1 are written whole (Reserved 0, no mask bit at or above S),
    the extra ones stay.  Both lobes."""
    scene, P, Nr = gr.config_points(pt, 2)
    top = max(m for s, m in BOUNDARIES if s == samples)
    Pt, Nt = np.ascontiguousarray(P[100:100 + top]), np.ascontiguousarray(Nr[100:100 + top])
    ds = upload(pt, dev, scene)
    for lobe in (COSINE, SPHERE):
        _, occ, _, expect = ray_set("c2-boundary", scene, Pt, Nt, lobe).expect(pt, samples, INF, n)
        out = sentinel(pt, n + 2)
        keep = out.copy()
        p = pt.SkyGatherParameters(samples, INF, SEED, Lobe=lobe).as_struct()
        assert raw_gather(pt, dev, ds, Pt[:n], Nt[:n] if lobe == COSINE else None, p, out) == 0
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
    if "chain" not in _sets:
        c = mesh_scene(pt, chain_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.1), scale=(1.0, 1.0, 1.0))
        _sets["chain"] = (c,) + gr.hit_points(c, *chain_rays())
    c, P, Nr = _sets["chain"]
    assert len(P) > 200
    dm = upload(pt, dev, c, stack_format=fmt)
    dg = upload(pt, dev, c, form=GENERAL, stack_format=fmt)
    assert dm.extend_form == MESH and dg.extend_form == GENERAL and dm.stack_needed > 20
    for lobe in (COSINE, SPHERE):
        _, occ, _, expect = ray_set("chain", c, P, Nr, lobe).expect(pt, 16, INF)
        print(f"chain lobe={lobe}: {len(P)} points, {100 * occ.mean():.1f} % of the rays occluded (oracle)")
        assert occ.any() and not occ.all()
        p = pt.SkyGatherParameters(16, INF, SEED, Lobe=lobe).as_struct()
        for ds in (dm, dg):
            assert same_records(gather(ds, P, Nr, 16, INF, lobe), expect)
            out = sentinel(pt, len(P))
            assert raw_gather(pt, dev, ds, P, Nr if lobe == COSINE else None, p, out, max_lanes=1024) == 0
            assert same_records(out, expect)
    dm.close()
    dg.close()


# --- nesting, partition independence, chunked launches -------------------------------------

@LOBES
def test_nesting_and_partition_independence(pt, dev, lobe):
    scene, P, Nr, rs = config_set(pt, 2, lobe)
    ds = upload(pt, dev, scene)
    full = gather(ds, P, Nr, 64, 0.5, lobe)
    assert same_records(full, rs.expect(pt, 64, 0.5)[3])
    assert np.any(full["Unoccluded"] < 64) and np.any(full["Unoccluded"] > 0)
    for S in (16, 4, 1):
        small = gather(ds, P, Nr, S, 0.5, lobe)
        assert np.array_equal(small["OccludedMask"], full["OccludedMask"] & np.uint64((1 << S) - 1)), S
        assert same_records(small, rs.expect(pt, S, 0.5)[3]), S
    a = gather(ds, P[:100], Nr[:100], 64, 0.5, lobe, first_index=0)
    b = gather(ds, P[100:], Nr[100:], 64, 0.5, lobe, first_index=100)
    assert same_records(np.concatenate([a, b]), full)
    assert not same_records(gather(ds, P[100:], Nr[100:], 64, 0.5, lobe), full[100:])   # FirstIndex matters
    ds.close()


@pytest.mark.parametrize("samples,max_lanes,launches,lobe", [(16, 4096, 9, COSINE), (1, 64, 33, SPHERE)])
def test_chunked_launches(pt, dev, samples, max_lanes, launches, lobe):
    """The test probe lowers the lanes per launch: the same records from
    several launches, each counted under PT_KERNEL_EXTEND."""
    scene, P, Nr = gr.config_points(pt, 2)
    n = 2079
    P, Nr = np.ascontiguousarray(P[:n]), np.ascontiguousarray(Nr[:n])
    expect = ray_set("c2-chunks", scene, P, Nr, lobe).expect(pt, samples, INF)[3]
    ds = upload(pt, dev, scene)
    p = pt.SkyGatherParameters(samples, INF, SEED, Lobe=lobe).as_struct()
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    out = sentinel(pt, n + 2)
    keep = out.copy()
    assert raw_gather(pt, dev, ds, P, Nr if lobe == COSINE else None, p, out, max_lanes=max_lanes) == 0
    count, _ = dev.kernel_stats(K_EXTEND)
    assert count == launches == -(-n // (max_lanes // samples))
    dev.reset_kernel_stats()
    whole = gather(ds, P, Nr, samples, INF, lobe)
    assert dev.kernel_stats(K_EXTEND)[0] == 1
    dev.set_profiling(False)
    assert same_records(out[:n], expect) and same_records(out[n:], keep[n:])
    assert same_records(whole, expect)
    ds.close()


# --- an empty scene ------------------------------------------------------------------------

def empty_scene(pt):
    if "empty" not in _sets:
        e = pt.Scene.empty()
        e.set_root(skybox_brightness=1.2)
        cam = e.create_entity(pt.ENTITY_CAMERA, position=(0.0, -6.0, 1.0), rotation=(1.45, 0.0, 0.0))
        e.set_camera_pinhole(cam, fov_degrees=55.0)
        e.pack()
        _sets["empty"] = e
    return _sets["empty"]


@LOBES
def test_empty_scene_gives_the_full_tree_sum(pt, dev, lobe):
    """Nothing occludes: u = S and SH is the whole tree of the restated
    contributions.  The sky is untextured, so a ray's contribution is the
    observer at its own four wavelengths times one constant: SH[0] at S = 64
    is the tree of 64 such values, which differ from point to point (a test of
    the tree and the L0 stream, not a constant)."""
    _, P, Nr = gr.config_points(pt, 3)
    P, Nr = np.ascontiguousarray(P[:M]), np.ascontiguousarray(Nr[:M])
    e = empty_scene(pt)
    assert int(e.arrays()["globals"][0]["SkyboxTextureIndex"]) == NONE
    rs = ray_set("empty", e, P, Nr, lobe)
    de = upload(pt, dev, e)
    for S in (1, 16, 64):
        v, occ, c, expect = rs.expect(pt, S, INF)
        assert not occ.any()
        got = gather(de, P, Nr, S, INF, lobe)
        assert same_records(got, expect)
        assert np.all(got["Unoccluded"] == S) and np.all(got["OccludedMask"] == 0)
    assert len(np.unique(got["SH"][:, 0, 1])) > M // 2 and np.all(got["SH"][:, 0, :] > 0)
    assert same_records(expect, sr.reduce(64, v, occ, c))
    de.close()


def test_normalisation_against_the_integrator(pt, dev):
    """Constant sky, empty scene: every camera ray leaves the scene, so a
    pixel's accumulator is the sum of its paths' escape contributions, and
    sum / count estimates E[C] over a uniform L0; SH[0] / (Y0 S) of a sphere-lobe
    point is the mean of S such contributions.  The two means, over 64 x 64
    pixels at 16 rounds and over 4 096 points at 64 samples, must agree within
    five standard errors of their difference, each standard error from its own
    sample's standard deviation; the integrator's side is the reference."""
    e = empty_scene(pt)
    de = upload(pt, dev, e)
    sb = pt.SampleBuffer(dev, 64, 64)
    r = pt.BasicRenderer(dev, de, sb)
    r.RenderFlags = 3
    r.reset()
    r.run(16)
    dev.synchronize()
    acc = sb.read().reshape(-1, 4).astype(np.float64)
    r.close()
    sb.close()
    assert np.all(acc[:, 3] > 0)
    pixel = acc[:, :3] / acc[:, 3:4]
    rng = np.random.default_rng(16)
    P = rng.uniform(-3, 3, (4096, 3)).astype(np.float32)
    rec = de.gather_sky_light(P, None, 64, INF, 1000, first_index=1 << 20, lobe="sphere")
    assert np.all(rec["Unoccluded"] == 64)
    point = rec["SH"][:, 0, :].astype(np.float64) / (0.28209479 * 64.0)
    for ch in range(3):
        a, b = pixel[:, ch], point[:, ch]
        se = np.hypot(a.std(ddof=1) / np.sqrt(len(a)), b.std(ddof=1) / np.sqrt(len(b)))
        print(f"channel {ch}: integrator {a.mean():.6f}, gathered {b.mean():.6f}, difference "
              f"{(b.mean() - a.mean()) / se:+.2f} standard errors of {se:.2e}")
        assert se > 0 and abs(b.mean() - a.mean()) <= 5.0 * se
    de.close()


# --- an empty batch, invalid arguments -------------------------------------------------------

def test_empty_batch_writes_nothing(pt, dev):
    scene, P, Nr = gr.config_points(pt, 2)
    ds = upload(pt, dev, scene)
    out = sentinel(pt, 2)
    keep = out.copy()
    p = pt.SkyGatherParameters(16, INF, SEED).as_struct()
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    assert raw_gather(pt, dev, ds, P, Nr, p, out, n=0) == 0
    assert raw_gather(pt, dev, ds, None, None, p, None, n=0) == 0
    assert dev.kernel_stats(K_EXTEND)[0] == 0
    dev.set_profiling(False)
    assert same_records(out, keep)
    assert ds.gather_sky_light(P[:0], Nr[:0]).shape == (0,)
    assert ds.gather_sky_light(P[:0], lobe="sphere").shape == (0,)
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

    def params(samples=16, radius=1.0, offset=1e-3, first=0, lobe=COSINE):
        return N.pt_sky_gather_parameters(samples, radius, SEED, offset, first, lobe)

    for bad in (dict(samples=0), dict(samples=3), dict(samples=24), dict(samples=65), dict(samples=128),
                dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(offset=-1e-3),
                dict(offset=INF), dict(offset=float("nan")), dict(first=0xFFFFFFF9), dict(lobe=2),
                dict(lobe=0xFFFFFFFF)):
        assert raw_gather(pt, dev, ds, P, Nr, params(**bad), out) != 0, bad
        assert b"ptGatherSkyLight" in N.hip_lib().ptGetLastError()
    ok = params()
    assert raw_gather(pt, dev, ds, P, Nr, params(first=0xFFFFFFF8), sentinel(pt, 8)) == 0   # FirstIndex + n == 2^32
    assert raw_gather(pt, dev, ds, P, None, params(lobe=SPHERE), sentinel(pt, 8)) == 0      # no normals, sphere
    launched = dev.kernel_stats(K_EXTEND)[0]
    assert launched == 2
    assert raw_gather(pt, dev, ds, P, None, ok, out) != 0                                   # no normals, cosine
    assert b"null" in N.hip_lib().ptGetLastError()
    assert raw_gather(pt, dev, ds, None, Nr, ok, out) != 0
    assert raw_gather(pt, dev, ds, P, Nr, None, out) != 0 and raw_gather(pt, dev, ds, P, Nr, ok, None) != 0
    assert raw_gather(pt, dev, ds, None, None, params(lobe=SPHERE), out, n=8) != 0
    L = N.hip_lib()
    assert L.ptGatherSkyLight(None, ds.handle, 8, N.fptr(P), N.fptr(Nr), C.byref(ok), out.ctypes.data) != 0
    assert L.ptGatherSkyLight(dev.handle, None, 8, N.fptr(P), N.fptr(Nr), C.byref(ok), out.ctypes.data) != 0
    assert raw_gather(pt, dev, bare, P, Nr, ok, out) != 0
    assert b"packs" in L.ptGetLastError()
    for lanes in (0, 63, (1 << 22) + 1):
        assert raw_gather(pt, dev, ds, P, Nr, ok, out, max_lanes=lanes) != 0, lanes
    assert raw_gather(pt, dev, ds, P, Nr, ok, out, n=(1 << 26) + 1) != 0
    if pt.device_count() > 1:
        other = pt.Device(1)
        assert L.ptGatherSkyLight(other.handle, ds.handle, 8, N.fptr(P), N.fptr(Nr), C.byref(ok), out.ctypes.data) != 0
        assert b"another device" in L.ptGetLastError()
        other.close()
    assert dev.kernel_stats(K_EXTEND)[0] == launched
    dev.set_profiling(False)
    assert same_records(out, keep)
    with pytest.raises(pt.PathTracerError):
        ds.gather_sky_light(P, Nr, samples=12)
    with pytest.raises(pt.PathTracerError):
        ds.gather_sky_light(P, Nr, lobe=2)
    with pytest.raises(ValueError):
        ds.gather_sky_light(P, Nr[:3])
    with pytest.raises(ValueError):
        ds.gather_sky_light(P)               # the cosine lobe needs normals
    bare.close()
    ds.close()
