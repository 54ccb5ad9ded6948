"""A numpy float32 restatement of the visibility gathered at caller-given
points, written from the definition apart from
include/pt_visibility.h and csrc/hip/occlusion.hip (test infrastructure only;
tests/test_visibility_gather.py, tests/test_gpu_visibility_gather.py):

  rays     the n S rays of n points, point-major: every point's stream is
           stepped sequentially, two draws per sample (no skip-ahead).
  reduce   the records from one bit per ray: reshape, then add adjacent pairs
           until one vector is left.
  lcg      the stream's generator stepped one step at a time.

Numerics: DESIGN.md §2's convention in numpy float32 (nothing fused, sums
left to right, IEEE sqrt and division, the convention's sin and cos)."""
from __future__ import annotations

import numpy as np

import kat
import oracle_lib

f32 = np.float32
u32 = np.uint32
M32 = 0xFFFFFFFF
HIT_TIME_LIMIT = f32(1048576.0)
TAU = f32(6.28318530717958647692)
RECORD_DTYPE = np.dtype([("Bent", "<f4", (3,)), ("Unoccluded", "<f4"), ("OccludedMask", "<u8"), ("Samples", "<f4"),
                         ("Reserved", "<u4")])


def lcg(state: int, steps: int) -> int:
    """`state` after `steps` single steps of x -> 747796405 x + 2891336453 mod 2^32."""
    for _ in range(steps):
        state = (state * 747796405 + 2891336453) & M32
    return state


def duration(radius):
    r = f32(radius)
    return r if r < HIT_TIME_LIMIT else HIT_TIME_LIMIT


def _random01(state):
    """Random0To1 over an array of uint32 states, each advanced one step in place."""
    state *= u32(747796405)
    state += u32(2891336453)
    s = state
    w = ((s >> ((s >> u32(28)) + u32(4))) ^ s) * u32(277803737)
    return ((w >> u32(22)) ^ w).astype(f32) * f32(2.0 ** -32)


def _fp(name, a):
    return oracle_lib.fp_eval(name, np.ascontiguousarray(a, f32).view(u32)).view(f32)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)


def seeds(n, seed, first_index):
    j = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    x, y = j & np.uint64(0xFFFF), j >> np.uint64(16)
    return ((y * np.uint64(65537) + x + np.uint64((int(seed) & M32) * 277803737)) & np.uint64(M32)).astype(u32)


def rays(points, normals, samples, radius=np.inf, seed=0, offset=1e-3, first_index=0):
    """origins (n S, 3), packed velocities (n S,), durations (n S,): ray i S + k
    is sample k of point i."""
    P = np.asarray(points, f32).reshape(-1, 3)
    N = np.asarray(normals, f32).reshape(-1, 3)
    n, S, off = len(P), int(samples), f32(offset)
    one, zero = f32(1.0), f32(0.0)
    with np.errstate(all="ignore"):
        state = seeds(n, seed, first_index)
        A = np.where((np.abs(N[:, 0]) < f32(0.9))[:, None], np.array([1, 0, 0], f32), np.array([0, 1, 0], f32)).astype(f32)
        X = _cross(A, N)
        X = (X * (one / np.sqrt(_dot(X, X)))[:, None]).astype(f32)
        Y = _cross(X, N)
        origins, packed = np.zeros((n, S, 3), f32), np.zeros((n, S), u32)
        for k in range(S):
            z = f32(2.0) * _random01(state) - one
            r = np.sqrt(one - z * z)
            phi = TAU * _random01(state)
            d = np.stack([r * _fp("cos", phi) + zero, r * _fp("sin", phi) + zero, z + one], axis=1).astype(f32)
            lsq = _dot(d, d)
            l = np.where((lsq < f32(1e-12))[:, None], np.array([0, 0, 1], f32), d / np.sqrt(lsq)[:, None]).astype(f32)
            w = ((l[:, 0:1] * X + l[:, 1:2] * Y) + l[:, 2:3] * N).astype(f32)
            origins[:, k] = P + (off * w).astype(f32)
            packed[:, k] = kat.pack_unit_vector(w)
    return origins.reshape(-1, 3), packed.reshape(-1), np.full(n * S, duration(radius), f32)


def hit_points(scene, o, v, d):
    """Surface points of a scene: the closest hits of a ray batch through the
    oracle, P = o + t V in float32, N the unpacked hit normal turned to the
    side the ray came from."""
    hits = oracle_lib.trace_rays(scene.packs(), o, v, d)
    h = hits["shape_material"] != M32
    V = kat.unpack_unit_vector(v[h]).astype(f32)
    P = (o[h] + hits["time"][h].astype(f32)[:, None] * V).astype(f32)
    N = kat.unpack_unit_vector(hits["packed_normal"][h]).astype(f32)
    N = np.where((_dot(N, V) > 0)[:, None], -N, N).astype(f32)
    return np.ascontiguousarray(P), np.ascontiguousarray(N)


_config_points = {}


def config_points(pt, config):
    """(scene, P, N): the hit points of rays.random_rays(arrays, 4096, 7) on
    benchmark config `config`, built once per process and left unchanged."""
    if config not in _config_points:
        from rays import random_rays
        scene = pt.Scene.config(config)
        _config_points[config] = (scene,) + hit_points(scene, *random_rays(scene.arrays(), 4096, 7))
    return _config_points[config]


def reduce(samples, packed, occluded):
    """The records of n points from their n S packed velocities and one bool per ray."""
    S = int(samples)
    occ = np.asarray(occluded, bool).reshape(-1, S)
    n = len(occ)
    b = kat.unpack_unit_vector(np.asarray(packed, u32)).astype(f32).reshape(n, S, 3)
    b = np.where(occ[:, :, None], f32(0.0), b).astype(f32)
    while b.shape[1] > 1:
        b = (b[:, 0::2] + b[:, 1::2]).astype(f32)
    out = np.zeros(n, RECORD_DTYPE)
    out["Bent"] = b[:, 0]
    out["OccludedMask"] = (occ.astype(np.uint64) << np.arange(S, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    out["Unoccluded"] = (S - occ.sum(axis=1)).astype(f32)
    out["Samples"] = f32(S)
    return out
