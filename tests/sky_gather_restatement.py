"""A numpy float32 restatement of the sky light gathered at caller-given
points, written from the definition apart from
include/pt_visibility.h and csrc/hip/occlusion.hip (test infrastructure only;
tests/test_sky_gather.py, tests/test_gpu_sky_gather.py):

  rays           the n S rays of n points and each ray's L0, point-major:
                 every point's stream is stepped sequentially (no skip-ahead),
                 two draws per sample for the directions, then on to draw 128,
                 then one draw per sample for L0.
  basis          the nine real spherical harmonics at float32 unit vectors.
  contributions  C_k of chosen rays: tests/path_restatement.py's
                 World.sky_spectrum, parametric and observer at the ray's four
                 wavelengths, the sky's brightness, the sum over the
                 wavelengths left to right and the division by 4.
  reduce         the records from one bit and one contribution per ray: the
                 27 products, then "reshape, add adjacent pairs".

Numerics: DESIGN.md §2's convention in numpy float32 (nothing fused, sums
left to right, IEEE sqrt and division, the convention's functions)."""
from __future__ import annotations

import numpy as np

import gather_restatement as gr
import kat
import path_restatement as pr

f32 = np.float32
u32 = np.uint32
COSINE, SPHERE = 0, 1
Y0 = f32(0.28209479)
RECORD_DTYPE = np.dtype([("SH", "<f4", (9, 3)), ("Unoccluded", "<f4"), ("OccludedMask", "<u8"), ("Samples", "<f4"),
                         ("Reserved", "<u4", (1,))])


def rays(points, normals, samples, radius=np.inf, seed=0, offset=1e-3, first_index=0, lobe=COSINE):
    """origins (n S, 3), packed velocities (n S,), durations (n S,), L0 (n S,):
    ray i S + k is sample k of point i."""
    P = np.asarray(points, f32).reshape(-1, 3)
    n, S, off = len(P), int(samples), f32(offset)
    one = f32(1.0)
    state = gr.seeds(n, seed, first_index)
    if lobe == COSINE:
        # The cosine lobe is row 15's by definition: its restatement's rays.
        origins, packed, durations = gr.rays(P, normals, S, radius, seed, offset, first_index)
        for _ in range(2 * S):
            gr._random01(state)
    else:
        origins, packed = np.zeros((n, S, 3), f32), np.zeros((n, S), u32)
        with np.errstate(all="ignore"):
            for k in range(S):
                z = f32(2.0) * gr._random01(state) - one
                r = np.sqrt(one - z * z)
                phi = gr.TAU * gr._random01(state)
                w = np.stack([r * gr._fp("cos", phi), r * gr._fp("sin", phi), z], axis=1).astype(f32)
                origins[:, k] = P + (off * w).astype(f32)
                packed[:, k] = kat.pack_unit_vector(w)
        origins, packed = origins.reshape(-1, 3), packed.reshape(-1)
        durations = np.full(n * S, gr.duration(radius), f32)
    for _ in range(128 - 2 * S):
        gr._random01(state)
    l0 = np.zeros((n, S), f32)
    for k in range(S):
        l0[:, k] = gr._random01(state)
    return origins, packed, durations, l0.reshape(-1)


def basis(V):
    """(m, 9) float32 at unit vectors (m, 3) float32."""
    V = np.asarray(V, f32)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    c1, c2 = f32(0.48860251), f32(1.09254843)
    return np.stack([np.full(len(V), Y0, f32), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z),
                     f32(0.31539157) * (f32(3.0) * (z * z) - f32(1.0)), c2 * (x * z),
                     f32(0.54627422) * (x * x - y * y)], axis=1).astype(f32)


def lambdas(l0):
    """PathLambda: the four wavelengths of a normalised first wavelength."""
    l0 = f32(l0)
    lo, hi = pr.LAMBDA_MIN, pr.LAMBDA_MAX
    return [pr._mix(lo, hi, l0)] + [pr._mix(lo, hi, pr._fract(l0 + f32(q))) for q in (0.25, 0.50, 0.75)]


def contribution(world, v, l0):
    """What a camera ray leaving the scene along v adds to its pixel: the
    escape branch of Scatter for a fresh path (throughput 1, cluster PDF 4)."""
    lam = lambdas(l0)
    sp = world.sky_spectrum([f32(v[0]), f32(v[1]), f32(v[2])])
    em = [sp[3] * pr.parametric(sp[:3], l) * world.sky_brightness for l in lam]
    obs = [pr.observer(l) for l in lam]
    return [(((obs[0][i] * em[0] + obs[1][i] * em[1]) + obs[2][i] * em[2]) + obs[3][i] * em[3]) / f32(4.0)
            for i in range(3)]


class Contributions:
    """The contributions of a fixed ray set, computed on demand and kept: a
    ray's C_k depends on neither Radius nor Samples."""

    def __init__(self, world, packed, l0):
        self.world, self.l0 = world, np.asarray(l0, f32)
        self.V = kat.unpack_unit_vector(np.asarray(packed, u32)).astype(f32)
        self.C = np.zeros((len(self.l0), 3), f32)
        self.done = np.zeros(len(self.l0), bool)

    def of(self, want):
        """(len, 3) float32, valid where `want` (bools) is set, zero elsewhere."""
        want = np.asarray(want, bool)
        for r in np.flatnonzero(want & ~self.done):
            self.C[r] = contribution(self.world, self.V[r], self.l0[r])
        self.done |= want
        return np.where(want[:, None], self.C, f32(0.0)).astype(f32)


def reduce(samples, packed, occluded, contributions):
    """The records of n points from their n S packed velocities, one bool per
    ray and one XYZ contribution per ray (an occluded ray's counts as zero)."""
    S = int(samples)
    occ = np.asarray(occluded, bool).reshape(-1, S)
    n = len(occ)
    Y = basis(kat.unpack_unit_vector(np.asarray(packed, u32)).astype(f32)).reshape(n, S, 9)
    C = np.where(occ[:, :, None], f32(0.0), np.asarray(contributions, f32).reshape(n, S, 3)).astype(f32)
    b = (C[:, :, None, :] * Y[:, :, :, None]).astype(f32)          # (n, S, 9, 3)
    while b.shape[1] > 1:
        b = (b[:, 0::2] + b[:, 1::2]).astype(f32)
    out = np.zeros(n, RECORD_DTYPE)
    out["SH"] = b[:, 0]
    out["OccludedMask"] = (occ.astype(np.uint64) << np.arange(S, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    out["Unoccluded"] = (S - occ.sum(axis=1)).astype(f32)
    out["Samples"] = f32(S)
    return out
