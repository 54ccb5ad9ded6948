"""CPU: sky light gathered at caller-given points on the
host: include/pt_visibility.h compiled into libptscene.so (ptsSkyGatherRays,
ptsSkyGatherReduce, ptsSkyGatherBasis) against the numpy restatement bit for
bit and against row 15's rays, the L0 stream, the record layout, the argument
checks of every new entry point, and the float64 helpers against analytic
results."""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np
import pytest

import gather_restatement as gr
import kat
import oracle_lib
import sky_gather_restatement as sr

INF = float("inf")
COSINE, SPHERE = 0, 1
HIP_SYMBOLS = ("ptGatherSkyLight", "ptGatherSkyLightChunked")
SCENE_SYMBOLS = ("ptsSkyGatherRays", "ptsSkyGatherReduce", "ptsSkyGatherBasis")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_records(a, b):
    """Every field of two record arrays as integers."""
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize == 128 and np.array_equal(
        np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def sentinel(n):
    return np.full(n * 128, 0x5A, np.uint8).view(sr.RECORD_DTYPE)


# --- exports, layout and the Python surface ----------------------------------------------

def test_libraries_export_the_entry_points(pt):
    N = pt._native
    for name in HIP_SYMBOLS:
        assert hasattr(N.hip_lib(), name) and name in N.HIP_API, name
    for name in SCENE_SYMBOLS:
        assert hasattr(N.scene_lib(), name) and name in N.SCENE_API, name


def test_structs_and_python_surface(pt):
    N = pt._native
    import path_tracer_amd.layout as layout
    assert C.sizeof(N.pt_sky_gather_parameters) == 24
    assert [f[0] for f in N.pt_sky_gather_parameters._fields_] == ["Samples", "Radius", "Seed", "Offset", "FirstIndex",
                                                                   "Lobe"]
    assert [getattr(N.pt_sky_gather_parameters, f).offset for f, _ in N.pt_sky_gather_parameters._fields_] == [
        0, 4, 8, 12, 16, 20]
    D = layout.SKY_RECORD_DTYPE
    assert pt.SKY_RECORD_DTYPE is D and D == sr.RECORD_DTYPE and D.itemsize == 128
    assert [D.fields[k][1] for k in ("SH", "Unoccluded", "OccludedMask", "Samples", "Reserved")] == [0, 108, 112, 120, 124]
    assert D.fields["SH"][0].shape == (9, 3) and D.fields["OccludedMask"][1] % 8 == 0
    assert (pt.SKY_GATHER_COSINE, pt.SKY_GATHER_SPHERE) == (0, 1)
    p = pt.SkyGatherParameters()
    assert (p.Samples, p.Radius, p.Seed, p.Offset, p.FirstIndex, p.Lobe) == (16, INF, 0, 1e-3, 0, 0)
    q = pt.SkyGatherParameters(Samples=4, Radius=0.5, Seed=9, Offset=0.25, FirstIndex=7, Lobe="sphere").as_struct()
    assert (q.Samples, q.Radius, q.Seed, q.Offset, q.FirstIndex, q.Lobe) == (4, 0.5, 9, 0.25, 7, 1)
    assert pt.SkyGatherParameters(Lobe=1).Lobe == 1 and pt.SkyGatherParameters(Lobe="cosine").Lobe == 0
    with pytest.raises(ValueError):
        pt.SkyGatherParameters(Lobe="hemisphere")
    with pytest.raises(ValueError):
        pt.SkyGatherParameters(FirstIndex=1 << 32).as_struct()
    sig = inspect.signature(pt.DeviceScene.gather_sky_light)
    assert list(sig.parameters)[1:] == ["points", "normals", "samples", "radius", "seed", "offset", "first_index",
                                        "lobe", "params"]
    assert [sig.parameters[k].default for k in ("normals", "samples", "radius", "seed", "offset", "first_index",
                                                "lobe", "params")] == [None, 16, INF, 0, 1e-3, 0, "cosine", None]
    import path_tracer_amd.integrator as integrator
    for name in ("SkyGatherParameters", "sky_gather_rays_host", "sky_gather_reduce_host", "sh9_basis",
                 "sky_irradiance", "sky_radiance_sh", "sh9_irradiance"):
        assert name in pt.__all__ and getattr(integrator, name) is getattr(pt, name), name


# --- argument checks -------------------------------------------------------------------

def test_device_entry_points_reject_null_arguments(pt):
    L = pt._native.hip_lib()
    out = sentinel(2)
    keep = out.copy()
    p = pt._native.pt_sky_gather_parameters(16, 1.0, 0, 1e-3, 0, SPHERE)
    x = np.zeros(3, np.float32)
    fp = pt._native.fptr(x)
    assert L.ptGatherSkyLight(None, None, 1, fp, fp, C.byref(p), out.ctypes.data) != 0
    assert b"null" in L.ptGetLastError()
    assert L.ptGatherSkyLight(None, None, 0, None, None, C.byref(p), None) != 0
    assert L.ptGatherSkyLightChunked(None, None, 1, fp, fp, C.byref(p), 64, out.ctypes.data) != 0
    assert b"null" in L.ptGetLastError()
    assert same_records(out, keep)


def test_host_rays_argument_checks(pt):
    N = pt._native
    L = N.scene_lib()
    P = np.zeros((2, 3), np.float32)
    Nr = np.tile(np.array([0, 0, 1], np.float32), (2, 1))
    o, v = np.full((128, 3), 5.0, np.float32), np.full(128, 5, np.uint32)
    d, l0 = np.full(128, 5.0, np.float32), np.full(128, 5.0, np.float32)

    def call(samples=4, radius=1.0, offset=1e-3, first=0, lobe=COSINE, n=2, points=P, normals=Nr, lam=l0):
        p = N.pt_sky_gather_parameters(samples, radius, 0, offset, first, lobe)
        return L.ptsSkyGatherRays(C.byref(p), n, None if points is None else N.fptr(points),
                                  None if normals is None else N.fptr(normals), N.fptr(o), N.u32ptr(v), N.fptr(d),
                                  None if lam is None else N.fptr(lam))

    for samples in (0, 3, 5, 48, 65, 128):
        assert call(samples=samples) != 0, samples
    for radius in (0.0, -1.0, float("nan")):
        assert call(radius=radius) != 0, radius
    for offset in (-1e-3, INF, -INF, float("nan")):
        assert call(offset=offset) != 0, offset
    for lobe in (2, 3, 0xFFFFFFFF):
        assert call(lobe=lobe) != 0, lobe
    assert call(first=0xFFFFFFFF) != 0                      # FirstIndex + 2 > 2^32
    assert call(n=(1 << 26) + 1) != 0
    assert call(points=None) != 0 and call(lam=None) != 0
    assert call(normals=None) != 0                          # the cosine lobe reads them
    assert L.ptsSkyGatherRays(None, 2, N.fptr(P), N.fptr(Nr), N.fptr(o), N.u32ptr(v), N.fptr(d), N.fptr(l0)) != 0
    assert np.all(o == 5.0) and np.all(v == 5) and np.all(d == 5.0) and np.all(l0 == 5.0)
    assert call(first=0xFFFFFFFE) == 0                      # FirstIndex + 2 == 2^32
    assert call(samples=64, radius=INF, offset=0.0, lobe=SPHERE, normals=None) == 0
    assert not np.any(v == 5) and np.all(d == 1048576.0) and np.all((l0 >= 0) & (l0 <= 1))
    p = N.pt_sky_gather_parameters(4, 1.0, 0, 1e-3, 0, COSINE)
    assert L.ptsSkyGatherRays(C.byref(p), 0, None, None, None, None, None, None) == 0
    with pytest.raises(pt.PathTracerError):
        pt.sky_gather_rays_host(P, Nr, pt.SkyGatherParameters(Samples=3))
    with pytest.raises(pt.PathTracerError):
        pt.sky_gather_rays_host(P, Nr, pt.SkyGatherParameters(Lobe=2))
    with pytest.raises(ValueError):
        pt.sky_gather_rays_host(P, Nr[:1])
    with pytest.raises(ValueError):
        pt.sky_gather_rays_host(P, None)


def test_host_reduce_argument_checks(pt):
    N = pt._native
    L = N.scene_lib()
    v = np.zeros(128, np.uint32)
    c = np.ones((128, 3), np.float32)
    w = np.zeros(2, np.uint64)
    wp = w.ctypes.data_as(C.POINTER(C.c_uint64))
    out = sentinel(2)
    keep = out.copy()
    for samples in (0, 3, 65, 128):
        assert L.ptsSkyGatherReduce(samples, 2, N.u32ptr(v), wp, N.fptr(c), out.ctypes.data) != 0, samples
    assert L.ptsSkyGatherReduce(4, 2, None, wp, N.fptr(c), out.ctypes.data) != 0
    assert L.ptsSkyGatherReduce(4, 2, N.u32ptr(v), None, N.fptr(c), out.ctypes.data) != 0
    assert L.ptsSkyGatherReduce(4, 2, N.u32ptr(v), wp, None, out.ctypes.data) != 0
    assert L.ptsSkyGatherReduce(4, 2, N.u32ptr(v), wp, N.fptr(c), None) != 0
    assert L.ptsSkyGatherReduce(4, (1 << 26) + 1, N.u32ptr(v), wp, N.fptr(c), out.ctypes.data) != 0
    assert L.ptsSkyGatherBasis(2, None, N.fptr(c)) != 0 and L.ptsSkyGatherBasis(2, N.u32ptr(v), None) != 0
    assert same_records(out, keep)
    assert L.ptsSkyGatherReduce(4, 0, None, None, None, None) == 0 and L.ptsSkyGatherBasis(0, None, None) == 0
    assert L.ptsSkyGatherReduce(64, 2, N.u32ptr(v), wp, N.fptr(c), out.ctypes.data) == 0
    assert not same_records(out, keep)
    with pytest.raises(ValueError):
        pt.sky_gather_reduce_host(4, v[:6], np.zeros(6, bool), c[:6])
    with pytest.raises(ValueError):
        pt.sky_gather_reduce_host(4, v[:8], np.zeros(7, bool), c[:8])
    with pytest.raises(ValueError):
        pt.sky_gather_reduce_host(4, v[:8], np.zeros(8, bool), c[:7])


# --- the rays and L0 ---------------------------------------------------------------------

@pytest.mark.parametrize("lobe", [COSINE, SPHERE], ids=["cosine", "sphere"])
@pytest.mark.parametrize("config", [1, 2, 3])
def test_header_on_the_host_equals_the_restatement(pt, config, lobe):
    """ptsSkyGatherRays makes sample k and its L0 directly (the skip); the
    restatement steps every stream sequentially.  Origins, packed words,
    durations and L0, bit for bit, on the surface points of a config."""
    scene, P, Nr = gr.config_points(pt, config)
    assert len(P) > 500
    for samples, seed, first in ((1, 3, 0), (4, 3, 65530), (64, 11, 0)):
        for offset, radius in ((0.0, INF), (1e-3, 0.5)):
            p = pt.SkyGatherParameters(samples, radius, seed, offset, first, lobe)
            o, v, d, l0 = pt.sky_gather_rays_host(P, Nr if lobe == COSINE else None, p)
            ro, rv, rd, rl = sr.rays(P, Nr, samples, radius, seed, offset, first, lobe)
            assert o.shape == (len(P) * samples, 3) and l0.shape == (len(P) * samples,)
            assert np.array_equal(bits(o), bits(ro)), (config, samples, offset)
            assert np.array_equal(v, rv), (config, samples, offset)
            assert np.array_equal(bits(d), bits(rd)) and d[0] == (0.5 if radius == 0.5 else 1048576.0)
            assert np.array_equal(bits(l0), bits(rl)), (config, samples)
    # the sphere lobe does not read the normals
    if lobe == SPHERE:
        a = pt.sky_gather_rays_host(P, None, p)
        b = pt.sky_gather_rays_host(P, -Nr, p)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("config", [1, 2, 3])
def test_cosine_rays_are_row_15s_as_bytes(pt, config):
    scene, P, Nr = gr.config_points(pt, config)
    for samples, radius, seed, offset, first in ((1, INF, 3, 1e-3, 0), (16, 0.5, 3, 0.0, 65530), (64, INF, 11, 0.05, 7)):
        o, v, d, _ = pt.sky_gather_rays_host(P, Nr, pt.SkyGatherParameters(samples, radius, seed, offset, first, COSINE))
        go, gv, gd = pt.gather_visibility_rays_host(P, Nr, pt.VisibilityGatherParameters(samples, radius, seed, offset,
                                                                                         first))
        assert o.tobytes() == go.tobytes() and v.tobytes() == gv.tobytes() and d.tobytes() == gd.tobytes()


def test_lambda0_is_draw_128_plus_k_of_a_single_stepped_stream(pt):
    """Point i's stream starts at seed(FirstIndex + i, Seed); its draw number
    t (from 0) is the output after t + 1 single steps.  L0 of sample k is draw
    128 + k whatever S and the lobe are: past the 128 direction draws of S = 64."""
    P = np.zeros((5, 3), np.float32)
    Nr = np.tile(np.array([0, 0, 1], np.float32), (5, 1))
    first, seed = 65534, 9
    s0 = gr.seeds(5, seed, first)
    for S in (1, 16, 64):
        for lobe in (COSINE, SPHERE):
            l0 = pt.sky_gather_rays_host(P, Nr, pt.SkyGatherParameters(S, INF, seed, 1e-3, first, lobe))[3].reshape(5, S)
            for i in range(5):
                state = gr.lcg(int(s0[i]), 128)
                for k in range(S):
                    state = gr.lcg(state, 1)
                    w = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
                    w = (w >> 22) ^ w
                    assert bits(l0[i, k]) == bits(np.float32(w) * np.float32(2.0 ** -32)), (S, lobe, i, k)
    # nesting: the first S' samples of S = 64 are the samples of S'
    full = pt.sky_gather_rays_host(P, Nr, pt.SkyGatherParameters(64, INF, seed, 1e-3, first, SPHERE))
    for S in (16, 4, 1):
        small = pt.sky_gather_rays_host(P, Nr, pt.SkyGatherParameters(S, INF, seed, 1e-3, first, SPHERE))
        assert np.array_equal(bits(small[0]), bits(full[0].reshape(5, 64, 3)[:, :S].reshape(-1, 3)))
        assert np.array_equal(small[1], full[1].reshape(5, 64)[:, :S].reshape(-1))
        assert np.array_equal(bits(small[3]), bits(full[3].reshape(5, 64)[:, :S].reshape(-1)))
    # partition independence
    part = pt.sky_gather_rays_host(P[2:], Nr[2:], pt.SkyGatherParameters(64, INF, seed, 1e-3, first + 2, SPHERE))
    assert all(np.array_equal(a.view(np.uint32), b[2 * 64:].view(np.uint32)) for a, b in zip(part, full))


# --- the basis and the reduction ----------------------------------------------------------

def unit_words(rng, n):
    """Packed unit vectors: the six axes, then random directions."""
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    dirs = rng.normal(size=(n - 6, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    return oracle_lib.pack_unit_vectors(np.concatenate([axes, dirs]))


def test_basis_equals_the_restatement(pt):
    N = pt._native
    words = unit_words(np.random.default_rng(16), 4096)
    out = np.zeros((4096, 9), np.float32)
    assert N.scene_lib().ptsSkyGatherBasis(4096, N.u32ptr(words), N.fptr(out)) == 0
    V = kat.unpack_unit_vector(words).astype(np.float32)
    assert np.array_equal(np.abs(V[:6]).argmax(axis=1), [0, 0, 1, 1, 2, 2]) and np.all(np.abs(V[:6]).max(axis=1) == 1.0)
    assert np.array_equal(bits(out), bits(sr.basis(V)))
    # the float64 helper has the same harmonics (float32 rounding of five operations at most)
    assert np.abs(pt.sh9_basis(V.astype(np.float64)) - out).max() < 1e-6


@pytest.mark.parametrize("samples", [1, 2, 4, 8, 16, 32, 64])
def test_reduce_equals_the_numpy_tree(pt, samples):
    rng = np.random.default_rng(samples)
    n = 301
    packed = unit_words(rng, n * samples)
    # contributions over ten decades, a few of them negative or zero
    c = (10.0 ** rng.uniform(-5, 5, (n * samples, 3))).astype(np.float32)
    c[rng.random(n * samples) < 0.05] *= np.float32(-1.0)
    c[rng.random(n * samples) < 0.05] = 0.0
    for name, occ in (("random", rng.random(n * samples) < 0.5), ("sparse", rng.random(n * samples) < 0.05),
                      ("all", np.ones(n * samples, bool)), ("none", np.zeros(n * samples, bool))):
        got = pt.sky_gather_reduce_host(samples, packed, occ, c)
        ref = sr.reduce(samples, packed, occ, c)
        assert got.dtype == pt.SKY_RECORD_DTYPE
        assert same_records(got, ref), (samples, name)
        assert np.all(got["Reserved"] == 0) and np.all(got["Samples"] == samples)
        assert np.all(got["OccludedMask"] >> np.uint64(samples - 1) <= 1)
        assert np.array_equal(got["Unoccluded"], samples - occ.reshape(n, samples).sum(axis=1))
    assert np.all(pt.sky_gather_reduce_host(samples, packed, np.ones(n * samples, bool), c)["SH"] == 0.0)
    if samples == 1:
        # S = 1: the record is the ray's products themselves
        one = pt.sky_gather_reduce_host(1, packed, np.zeros(n, bool), c)
        Y = sr.basis(kat.unpack_unit_vector(packed).astype(np.float32))
        assert np.array_equal(bits(one["SH"]), bits(c[:, None, :] * Y[:, :, None]))


# --- the float64 helpers against analytic results ------------------------------------------

def quadrature():
    """64 Gauss-Legendre nodes in z = cos(theta) times 128 equal steps in phi:
    exact for every polynomial in (x, y, z) of degree <= 127 (degree <= 127 in
    z; trigonometric degree <= 127 in phi).  The integrands below are
    polynomials of degree <= 4, so the only error is float64 rounding: a sum
    of 8 192 terms, each formed from nodes, weights and factors good to a few
    ulp, is off by at most 8192 * 2^-53 * integral(|f|) ~ 1e-12 * integral(|f|),
    and in practice by ~1e-15."""
    z, wz = np.polynomial.legendre.leggauss(64)
    phi = (np.arange(128) + 0.5) * (2.0 * np.pi / 128)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    d = np.stack([r * np.cos(pp), r * np.sin(pp), zz], axis=-1).reshape(-1, 3)
    w = np.repeat(wz, 128) * (2.0 * np.pi / 128)
    return d, w


def test_sh9_basis_is_orthonormal(pt):
    d, w = quadrature()
    assert abs(w.sum() - 4.0 * np.pi) < 1e-12
    Y = pt.sh9_basis(d)
    assert Y.shape == (len(d), 9)
    gram = np.einsum("n,ni,nj->ij", w, Y, Y)
    # integral(|Y_i Y_j|) <= 1 (Cauchy-Schwarz), so the rounding bound of quadrature() is 1e-12
    assert np.abs(gram - np.eye(9)).max() < 1e-12


def test_sh9_irradiance_of_a_linear_sky(pt):
    """Radiance a + b w_z per channel, projected by the quadrature (exact for
    its degree-3 integrands up to rounding), convolved with the clamped cosine:
    E(n) = pi a + (2 pi / 3) b n_z.  The issue's bound is 1e-6 relative; what
    is left is quadrature rounding, ~1e-12 at the worst (quadrature())."""
    d, w = quadrature()
    a, b = np.array([0.7, 1.3, 0.2]), np.array([0.4, -0.5, 0.15])
    L = a[None, :] + b[None, :] * d[:, 2:3]
    coeffs = np.einsum("n,ni,nc->ic", w, pt.sh9_basis(d), L)
    rng = np.random.default_rng(9)
    n = rng.normal(size=(100, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    E = pt.sh9_irradiance(coeffs, n)
    expect = np.pi * a[None, :] + (2.0 * np.pi / 3.0) * b[None, :] * n[:, 2:3]
    assert E.shape == (100, 3)
    assert np.abs(E / expect - 1.0).max() < 1e-6
    # one coefficient set per normal gives the same
    assert np.abs(pt.sh9_irradiance(np.broadcast_to(coeffs, (100, 9, 3)), n) - E).max() < 1e-12


def test_record_readers(pt):
    """sky_irradiance and sky_radiance_sh on hand-made records: a sphere-lobe
    record of an unoccluded constant sky L has SH[0] = S L Y0, whose radiance
    coefficient (4 pi / S) SH[0] = L sqrt(4 pi) convolves to E = pi L; a
    cosine-lobe record of the same sky has SH[0] = S (L) Y0 too and
    sky_irradiance gives pi L directly."""
    L = np.array([0.5, 1.0, 2.0])
    rec = np.zeros(3, pt.SKY_RECORD_DTYPE)
    for i, S in enumerate((1, 16, 64)):
        rec["Samples"][i] = S
        rec["SH"][i, 0] = S * L * 0.28209479
    assert np.abs(pt.sky_irradiance(rec) / (np.pi * L) - 1.0).max() < 1e-6
    coeffs = pt.sky_radiance_sh(rec)
    assert coeffs.shape == (3, 9, 3)
    assert np.abs(coeffs[:, 0] / (L * np.sqrt(4.0 * np.pi)) - 1.0).max() < 1e-6
    up = np.tile(np.array([0.0, 0.0, 1.0]), (3, 1))
    assert np.abs(pt.sh9_irradiance(coeffs, up) / (np.pi * L) - 1.0).max() < 1e-6
