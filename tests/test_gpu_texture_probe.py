"""GPU: the device's SampleTexture against the oracle's at chosen UVs.

The device sampler (pt_device.hpp) differs in structure from the oracle's: the
atlas is stored in 4x2-texel blocks (AtlasIndex, filled by atlas_tile_kernel)
when W % 4 == 0 and H % 2 == 0 and row-major otherwise, and the lean shade
kernel wraps texel coordinates with two selects (Texel<true>) where the oracle
takes a remainder.  Rendered hits never put a UV exactly on a texel border or
reach fract(UV) == 1.0f (x - floor(x) of a tiny negative x); ptSampleTextures
samples at caller-given UVs, oracle_sample_textures is its host counterpart.

Raw packs with tiny atlases of seeded random texel bits (negatives and
denormals included, so a wrong texel cannot match by chance): 8x4 and 12x6 in
two layers (tiled), 6x3 (row-major); nearest and bilinear textures placed on
the whole layer, on an interior rectangle and on rectangles touching each
atlas edge; a second scene per atlas adds a placement outside [0, 1], which
only the remainder wrap may serve.  Every result must equal the oracle's bit
for bit with either wrap, and the two wraps must agree wherever the two-select
one is allowed.  No case is left out.

Non-finite UVs (+-inf, NaN) are a recorded set, not asserted.  Reading the
code, both sides stay inside the atlas: fract(inf) and fract(NaN) are NaN, so
U and V are NaN; the device's saturating convert turns (int)floor(NaN) into
texel index 0, the host's x86 convert into INT_MIN, whose remainder by W
(wrapped into [0, W)) is again a valid index, though in general another texel.
Such UVs reach the sampler from a file: a half-float vt above 65504 in an OBJ
becomes inf.  The counts are printed and go into the report.  Measured
(profiles/numerics_probe/README.md): the nearest-filtered samples differ on
the 12x6 and 6x3 atlases (180 of 360, 90 of 180) and agree on 8x4, where
INT_MIN mod W is 0 as for every power-of-two atlas; bilinear samples are NaN
on both sides.  Clamping half UVs to the finite range at import would close
the route; it is recommended, not built.
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import numerics_cases as nc
import oracle_lib
from path_tracer_amd import _native as N

pytestmark = pytest.mark.gpu

NEAREST = 1   # PT_TEXTURE_FLAG_FILTER_NEAREST


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


class AtlasPacks:
    """pt_scene_packs holding only globals, texture records and an atlas."""

    def __init__(self, W, H, layers, placements, seed):
        rng = np.random.default_rng(seed)
        bits = rng.integers(0, 2 ** 32, (layers, H, W, 4), dtype=np.uint32)
        exponent = rng.integers(1, 188, bits.shape, dtype=np.uint32)        # finite: up to 2^60, no overflow in a blend
        exponent[rng.random(bits.shape) < 0.125] = 0                        # denormals
        self.atlas = np.ascontiguousarray(((bits & 0x807FFFFF) | (exponent << 23)).view(np.float32))
        records = []
        for layer in range(layers):
            for flags in (NEAREST, 0):
                for mn, mx in placements:
                    records.append((mn, mx, layer, 0, flags, 0))
        self.textures = np.array(records, dtype=N.TEXTURE_DTYPE)
        self.globals = np.zeros(1, dtype=N.GLOBALS_DTYPE)
        self.globals[0]["SkyboxTextureIndex"] = 0xFFFFFFFF
        p = N.pt_scene_packs()
        p.globals = self.globals.ctypes.data
        p.textures = self.textures.ctypes.data
        p.texture_count = len(self.textures)
        p.atlas = self.atlas.ctypes.data
        p.atlas_width, p.atlas_height, p.atlas_layer_count = W, H, layers
        self._p = p
        self.W, self.H = W, H

    def packs(self):
        return self._p


def unit_placements(W, H):
    """The whole layer, an interior rectangle, and one rectangle on each atlas edge (texel-aligned)."""
    f = np.float32
    return [((0, 0), (1, 1)),
            ((f(1) / f(W), f(1) / f(H)), (f(W - 2) / f(W), f(H - 1) / f(H))),
            ((0, f(1) / f(H)), (f(3) / f(W), f(H - 1) / f(H))),                 # left edge
            ((f(W - 3) / f(W), f(1) / f(H)), (1, f(H - 1) / f(H))),             # right edge
            ((f(1) / f(W), 0), (f(W - 1) / f(W), f(2) / f(H))),                 # top edge
            ((f(1) / f(W), f(H - 2) / f(H)), (f(W - 1) / f(W), 1))]             # bottom edge


OUTSIDE = ((-0.25, -0.5), (1.5, 1.75))      # a placement beyond the unit square: the remainder wrap only


def axis_values(n):
    """UV coordinates along an axis of n texels."""
    k = np.arange(0, n + 1, dtype=np.float64)
    v = [nc.u2f(nc.around(k / n, 1)),                                   # every border k/n +- 1 ulp (0 and 1 among them)
         ((k[:-1] + 0.5) / n).astype(np.float32),                       # texel centres
         np.float32([0.0, 1.0, -(2.0 ** -30), -0.25, -1.5, -3.999, -1.0, 0.999999, 1e6, 2.0 ** 24 + 1, 2.0 ** 24 + 2,
                     2.5, 1.0 / 3.0])]
    v = np.concatenate(v)
    return v[np.isfinite(v)]


def uv_grid(W, H):
    u, v = axis_values(W), axis_values(H)
    g = np.array(list(itertools.product(u.tolist(), v.tolist())), dtype=np.float32)
    assert np.any(g[:, 0] - np.floor(g[:, 0]) == np.float32(1.0))       # fract(UV) == 1.0f is reached
    return g


def samples(packs):
    """Every texture of the scene at every UV of the grid."""
    g = uv_grid(packs.W, packs.H)
    t = np.repeat(np.arange(len(packs.textures), dtype=np.uint32), len(g))
    return t, np.tile(g, (len(packs.textures), 1))


def assert_same_bits(what, t, uv, got, want):
    bad = np.any(got.view(np.uint32) != want.view(np.uint32), axis=1)
    rows = [f"texture {int(t[i])} uv ({uv[i, 0]!r}, {uv[i, 1]!r}) got {got[i].view(np.uint32)} want {want[i].view(np.uint32)}"
            for i in np.flatnonzero(bad)[:5]]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} samples differ; first: " + "; ".join(rows)


ATLASES = [(8, 4, 2), (12, 6, 2), (6, 3, 1)]


@pytest.mark.parametrize("W,H,layers", ATLASES)
def test_sampler_equals_oracle(pt, dev, W, H, layers):
    """Unit placements: both wraps against the oracle, and against each other."""
    packs = AtlasPacks(W, H, layers, unit_placements(W, H), seed=100 + W)
    ds = pt.DeviceScene(dev)
    ds.update(packs)
    t, uv = samples(packs)
    want = oracle_lib.sample_textures(packs.packs(), t, uv)
    assert len(np.unique(want.view(np.uint32), axis=0)) > W * H        # the texels are told apart
    remainder = ds.sample_textures(t, uv, wrap=0)
    selects = ds.sample_textures(t, uv, wrap=1)
    assert_same_bits(f"{W}x{H} remainder wrap", t, uv, remainder, want)
    assert_same_bits(f"{W}x{H} two-select wrap", t, uv, selects, want)
    assert_same_bits(f"{W}x{H} two-select against remainder", t, uv, selects, remainder)
    ds.close()


@pytest.mark.parametrize("W,H,layers", ATLASES)
def test_placement_outside_unit_square(pt, dev, W, H, layers):
    """A scene with a placement beyond [0, 1]: PT_SHADE_TEXWRAP refuses the
    two-select wrap and writes nothing; the remainder wrap equals the oracle
    for every texture."""
    packs = AtlasPacks(W, H, layers, unit_placements(W, H) + [OUTSIDE], seed=200 + W)
    ds = pt.DeviceScene(dev)
    ds.update(packs)
    t, uv = samples(packs)
    assert_same_bits(f"{W}x{H} outside placement", t, uv, ds.sample_textures(t, uv, wrap=0),
                     oracle_lib.sample_textures(packs.packs(), t, uv))
    out = np.full((4, 4), 7.0, dtype=np.float32)
    L = N.hip_lib()
    rc = L.ptSampleTextures(dev.handle, ds.handle, 4, N.u32ptr(t[:4].copy()), N.fptr(uv[:4].copy()), 1, N.fptr(out))
    assert rc != 0 and b"two-select" in L.ptGetLastError() and np.all(out == 7.0)
    ds.close()


def test_argument_errors_write_nothing(pt, dev):
    packs = AtlasPacks(8, 4, 1, unit_placements(8, 4), seed=5)
    ds = pt.DeviceScene(dev)
    L = N.hip_lib()
    t = np.zeros(2, dtype=np.uint32)
    uv = np.zeros((2, 2), dtype=np.float32)
    out = np.full((2, 4), 7.0, dtype=np.float32)
    assert L.ptSampleTextures(dev.handle, ds.handle, 2, N.u32ptr(t), N.fptr(uv), 0, N.fptr(out)) != 0   # no packs yet
    ds.update(packs)
    assert L.ptSampleTextures(dev.handle, ds.handle, 2, None, N.fptr(uv), 0, N.fptr(out)) != 0
    assert L.ptSampleTextures(dev.handle, ds.handle, 2, N.u32ptr(t), None, 0, N.fptr(out)) != 0
    assert L.ptSampleTextures(dev.handle, ds.handle, 2, N.u32ptr(t), N.fptr(uv), 0, None) != 0
    assert L.ptSampleTextures(dev.handle, ds.handle, 2, N.u32ptr(t), N.fptr(uv), 2, N.fptr(out)) != 0
    t[1] = len(packs.textures)
    assert L.ptSampleTextures(dev.handle, ds.handle, 2, N.u32ptr(t), N.fptr(uv), 0, N.fptr(out)) != 0
    assert b"texture index" in L.ptGetLastError()
    assert np.all(out == 7.0)
    assert L.ptSampleTextures(dev.handle, ds.handle, 0, None, None, 0, None) == 0
    with pytest.raises(ValueError):
        oracle_lib.sample_textures(packs.packs(), t, uv)
    ds.close()


@pytest.mark.parametrize("W,H,layers", ATLASES)
def test_non_finite_uvs_are_recorded(pt, dev, W, H, layers, record_property):
    """+-inf and NaN UVs: compared and counted, not asserted (module docstring).
    A bilinear texture blends with NaN weights on both sides; a nearest one
    reads texel 0 on the device and the remainder of INT_MIN on the host."""
    packs = AtlasPacks(W, H, layers, unit_placements(W, H), seed=100 + W)
    ds = pt.DeviceScene(dev)
    ds.update(packs)
    bad_values = np.float32([np.inf, -np.inf, np.nan, 0.25])
    g = np.array([p for p in itertools.product(bad_values.tolist(), repeat=2) if not np.all(np.isfinite(p))],
                 dtype=np.float32)
    t = np.repeat(np.arange(len(packs.textures), dtype=np.uint32), len(g))
    uv = np.tile(g, (len(packs.textures), 1))
    want = oracle_lib.sample_textures(packs.packs(), t, uv)
    for wrap in (0, 1):
        got = ds.sample_textures(t, uv, wrap=wrap)
        differ = int(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1).sum())
        nan = int(np.isnan(got).any(axis=1).sum())
        print(f"[recorded] {W}x{H} non-finite UVs, wrap {wrap}: {differ} of {len(t)} differ from the host; "
              f"{nan} device results hold a NaN")
        record_property(f"non_finite_uv_differ_wrap{wrap}", f"{differ}/{len(t)}")
    ds.close()
