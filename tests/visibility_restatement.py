"""A numpy float32 restatement of the ambient-occlusion / sky-visibility image
(DESIGN.md §6 row 14), written from the definition apart from
include/pt_visibility.h and csrc/hip/occlusion.hip (test infrastructure only;
tests/test_occlusion.py, tests/test_gpu_ambient_occlusion.py):

  pixel_rays   one pixel's sample rays from the integrator's restated pieces
               (path_restatement.Rng, random_direction, coordinate_frame), a
               scalar loop: the reading of the definition.
  sample_rays  the same over arrays of pixels (a vectorised PCG, the oracle's
               batch sin / cos), which the tests hold against pixel_rays and
               then use for whole images.
  primary      the pixels' central camera rays (denoise_restatement.central_ray)
               and their closest hits through the oracle's ray query.
  ray_set      the rays of every hit pixel of a frame; image() turns the
               records of any ray query over them into the expected image.

Numerics: DESIGN.md §2's convention in numpy float32 (nothing fused, sums
left to right, IEEE sqrt and division, the convention's sin and cos)."""
from __future__ import annotations

import functools

import numpy as np

import denoise_restatement as dr
import kat
import oracle_lib
import path_restatement as pr

f32 = np.float32
NONE = 0xFFFFFFFF
OFFSET = f32(1e-3)
MAX_SAMPLES = 64


def duration(radius):
    """A radius at or beyond HIT_TIME_LIMIT (inf included) is HIT_TIME_LIMIT."""
    r = f32(radius)
    return r if r < pr.HIT_TIME_LIMIT else pr.HIT_TIME_LIMIT


def pixel_rays(x, y, seed, samples, O, V, t, Nq):
    """One pixel: origins (samples, 3) float32 and packed velocities (samples,)."""
    O, V, Nq = ([f32(c) for c in a] for a in (O, V, Nq))
    t = f32(t)
    with np.errstate(all="ignore"):
        N = [-c for c in Nq] if pr._dot(Nq, V) > 0 else list(Nq)
        X, Y = pr.coordinate_frame(N)
        g = pr.Rng(x, y, seed)
        pos = [O[i] + t * V[i] for i in range(3)]
        origins, packed = np.zeros((samples, 3), f32), np.zeros(samples, np.uint32)
        for k in range(samples):
            d = pr.random_direction(g)
            l = pr._safe_normalize([d[0] + f32(0.0), d[1] + f32(0.0), d[2] + f32(1.0)])
            w = [(l[0] * X[i] + l[1] * Y[i]) + l[2] * N[i] for i in range(3)]
            origins[k] = [pos[i] + OFFSET * w[i] for i in range(3)]
            packed[k] = kat.pack_unit_vector(np.array([w], f32))[0]
    return origins, packed


def _pcg01(state):
    """Random0To1 over an array of states, advanced in place."""
    state *= np.uint32(747796405)
    state += np.uint32(2891336453)
    s = state
    w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return ((w >> np.uint32(22)) ^ w).astype(f32) * f32(2.0 ** -32)


def _fp(name, a):
    return oracle_lib.fp_eval(name, np.ascontiguousarray(a, f32).view(np.uint32)).view(f32)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)


def sample_rays(xs, ys, seed, samples, O, V, t, Nq):
    """P pixels at once: origins (P, samples, 3) and packed velocities (P, samples)."""
    xs, ys = np.asarray(xs, np.uint64), np.asarray(ys, np.uint64)
    O, V, Nq = (np.asarray(a, f32).reshape(-1, 3) for a in (O, V, Nq))
    t = np.asarray(t, f32).reshape(-1)
    P = len(xs)
    one, zero = f32(1.0), f32(0.0)
    with np.errstate(all="ignore"):
        state = ((ys * 65537 + xs + (int(seed) & NONE) * 277803737) & NONE).astype(np.uint32)
        N = np.where((_dot(Nq, V) > 0)[:, None], -Nq, Nq).astype(f32)
        A = np.where((np.abs(N[:, 0]) < f32(0.9))[:, None], np.array([1, 0, 0], f32), np.array([0, 1, 0], f32))
        X = _cross(A.astype(f32), N)
        X = (X * (one / np.sqrt(_dot(X, X)))[:, None]).astype(f32)
        Y = _cross(X, N)
        pos = (O + t[:, None] * V).astype(f32)
        origins, packed = np.zeros((P, samples, 3), f32), np.zeros((P, samples), np.uint32)
        for k in range(samples):
            z = f32(2.0) * _pcg01(state) - one
            r = np.sqrt(one - z * z)
            phi = pr.TAU * _pcg01(state)
            d = np.stack([r * _fp("cos", phi) + zero, r * _fp("sin", phi) + zero, z + one], axis=1).astype(f32)
            lsq = _dot(d, d)
            l = np.where((lsq < f32(1e-12))[:, None], np.array([0, 0, 1], f32), d / np.sqrt(lsq)[:, None]).astype(f32)
            w = ((l[:, 0:1] * X + l[:, 1:2] * Y) + l[:, 2:3] * N).astype(f32)
            origins[:, k] = pos + OFFSET * w
            packed[:, k] = kat.pack_unit_vector(w)
    return origins, packed


def primary(scene, camera, W, H):
    """The frame's central rays and their closest hits: origins (W H, 3),
    packed velocities and oracle hit records, pixels in row-major order; None
    for a camera of unknown model."""
    cam = scene.arrays()["cameras"][camera]
    rays = [dr.central_ray(cam, x, y, W, H) for y in range(H) for x in range(W)]
    if rays[0] is None:
        return None
    O = np.array([r[0] for r in rays], f32)
    PV = np.array([r[1] for r in rays], np.uint32)
    hits = oracle_lib.trace_rays(scene.packs(), O, PV, np.full(len(PV), pr.HIT_TIME_LIMIT, f32))
    return O, PV, hits


def ray_set(scene, camera, W, H, samples, radius, seed):
    """The sample rays of every hit pixel: a dict with `pixels` (indices y W + x
    of the hit pixels, ascending), `normals` (their facing-independent guide
    normals), `origins` (P samples, 3), `packed`, `durations` (P samples,),
    pixel-major, and the frame's `shape`."""
    assert 1 <= samples <= MAX_SAMPLES
    out = {"shape": (H, W), "samples": samples, "pixels": np.zeros(0, np.int64), "normals": np.zeros((0, 3), f32), "view": np.zeros((0, 3), f32),
           "origins": np.zeros((0, 3), f32), "packed": np.zeros(0, np.uint32), "durations": np.zeros(0, f32)}
    p = primary(scene, camera, W, H)
    if p is None:
        return out
    O, PV, hits = p
    pix = np.flatnonzero(hits["shape_material"] != NONE)
    V = kat.unpack_unit_vector(PV[pix])
    Nq = kat.unpack_unit_vector(hits["packed_normal"][pix])
    o, v = sample_rays(pix % W, pix // W, seed, samples, O[pix], V, hits["time"][pix], Nq)
    out.update(pixels=pix, normals=Nq, view=V, origins=o.reshape(-1, 3), packed=v.reshape(-1),
               durations=np.full(len(pix) * samples, duration(radius), f32))
    return out


def image(rays, records):
    """The expected image (H, W, 4) from the hit records of any closest-hit
    query over rays["origins"], ["packed"], ["durations"]: u = the misses."""
    H, W = rays["shape"]
    S = rays["samples"]
    out = np.full((H * W, 4), f32(S), f32)
    u = (records["shape_material"] == NONE).reshape(-1, S).sum(axis=1).astype(f32)
    out[rays["pixels"], :3] = u[:, None]
    return out.reshape(H, W, 4)


@functools.lru_cache(maxsize=None)
def _config_scene(config):
    import path_tracer_amd as pt
    return pt.Scene.config(config)


def prefix(rays, samples, radius):
    """The ray set of fewer samples and another radius: a pixel's stream is
    sequential, so its first `samples` rays are the rays of that count."""
    S0, P = rays["samples"], len(rays["pixels"])
    assert 1 <= samples <= S0
    out = dict(rays)
    out.update(samples=samples, origins=np.ascontiguousarray(rays["origins"].reshape(P, S0, 3)[:, :samples]).reshape(-1, 3),
               packed=np.ascontiguousarray(rays["packed"].reshape(P, S0)[:, :samples]).reshape(-1),
               durations=np.full(P * samples, duration(radius), f32))
    return out


@functools.lru_cache(maxsize=None)
def _config_rays(config, W, H, seed):
    return ray_set(_config_scene(config), 0, W, H, 16, np.inf, seed)


@functools.lru_cache(maxsize=None)
def config_case(config, W, H, samples, radius, seed):
    """(scene, rays, the oracle's image) of benchmark config `config` at up to
    16 samples, computed once per process and shared (callers leave all three
    unchanged)."""
    scene = _config_scene(config)
    rays = prefix(_config_rays(config, W, H, seed), samples, radius)
    records = oracle_lib.trace_rays(scene.packs(), rays["origins"], rays["packed"], rays["durations"])
    return scene, rays, image(rays, records)
