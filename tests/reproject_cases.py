"""Inputs shared by the reprojection tests (tests/test_reproject.py on the
CPU, tests/test_gpu_reproject.py on the device).

Coherent cases: real guide images of one small scene seen by two cameras
(denoise_restatement.guides on the CPU oracle's ray query) and a random
history in the previous view.

  pinhole-pan   config 1 (a sphere on a plane under the sky), 64x32: the
                camera moves sideways and pans, so the sphere uncovers ground
                and a strip of the new view was never seen
  thin-lens     config 5, camera 0, 64x32: the same kind of move
  360-rotation  config 5, camera 1, 64x32: a rotation about the vertical (the
                panorama covers it: only the seam column loses taps, there
                being no wrap-around) with a step aside, which uncovers
                what the spheres hid
  resize        config 1, 64x32 -> 37x21 with the pan

Adversarial cases perturb coherent ones, one perturbation per previous pixel
in a 12-pixel pattern: the shape id flipped, the time nudged to just inside
and just outside DepthTolerance, the normal tilted to just inside and just
outside NormalCosine, the history made empty, NaN or infinite.  Bases: the
identity camera change at 16x16 and at 1x1, and a pan from 29x33 to 37x21.
look-away turns the previous camera round, so every point lies behind it.

all_cases() computes the restatement once per case and asserts the coverage
the tests rely on: every coherent case gives at least 25 % of the pixels a
history and leaves at least 5 % without one; every tap rule (frame, history,
shape, normal, depth) turns down, somewhere, a tap of a located pixel that
the four other rules accept (an out-of-frame tap is judged on the nearest
pixel of the image); some pixel lies behind the previous camera; some pixel
has valid taps whose weights sum to less than MinWeight."""
from __future__ import annotations

import functools
import sys

import numpy as np

import denoise_restatement as dr
import reproject_restatement as rr

F = np.float32
NONE = 0xFFFFFFFF
PARAMS = dict(rr.DEFAULTS)
HALF_PI = float(np.pi / 2)


def history(W, H, seed):
    """A random accumulator: XYZ means in [0.1, 2) times counts in 1..200
    (so MaxHistory = 64 caps some), with a few empty pixels."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 200, size=(H, W)).astype(F)
    a = np.zeros((H, W, 4), F)
    a[..., :3] = rng.uniform(0.1, 2.0, size=(H, W, 3)).astype(F) * n[..., None]
    a[..., 3] = n
    a[rng.uniform(size=(H, W)) < 0.02] = 0
    return a


def _two_views(pt, config, camera, prev_size, size, prev_pose, pose, seed):
    """prev_pose, pose: (position, rotation) of the camera entity."""
    scene = pt.Scene.config(config)
    ent = scene.find_camera(camera)
    scene.move_camera(ent, position=prev_pose[0], rotation=prev_pose[1])
    scene.pack()
    prev_cam = scene.arrays()["cameras"][camera].copy()
    prev_guides = dr.guides(scene, camera, *prev_size)
    scene.move_camera(ent, position=pose[0], rotation=pose[1])
    scene.pack()
    cam = scene.arrays()["cameras"][camera].copy()
    guides = dr.guides(scene, camera, *size)
    scene.close()
    return dict(prev_accum=history(*prev_size, seed), prev_guides=prev_guides, prev_cam=prev_cam, guides=guides,
                cam=cam)


C1_PREV = ((0.0, -4.0, 1.0), (HALF_PI, 0.0, 0.0))
C1_PAN = ((0.5, -4.0, 1.0), (HALF_PI, 0.0, 0.1))


@functools.lru_cache(maxsize=None)
def _coherent():
    pt = sys.modules["path_tracer_amd"]       # loaded by tests/conftest.py
    return {
        "pinhole-pan": _two_views(pt, 1, 0, (64, 32), (64, 32), C1_PREV, C1_PAN, 1),
        "thin-lens": _two_views(pt, 5, 0, (64, 32), (64, 32), ((0.0, -2.5, 1.2), (HALF_PI - 0.05, 0.0, 0.0)),
                                ((0.3, -2.5, 1.2), (HALF_PI - 0.05, 0.0, 0.1)), 2),
        "360-rotation": _two_views(pt, 5, 1, (64, 32), (64, 32), ((0.0, 0.5, 1.6), (HALF_PI, 0.0, 0.0)),
                                   ((0.2, 0.6, 1.6), (HALF_PI, 0.0, 0.6)), 3),
        "resize": _two_views(pt, 1, 0, (64, 32), (37, 21), C1_PREV, C1_PAN, 4),
    }


def _tilt(n, angle):
    """Unit normals n (.., 3) turned by `angle` about an axis at right angles."""
    n = n.astype(np.float64)
    a = np.where(np.abs(n[..., :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(n, a)
    t /= np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-30)
    return (np.cos(angle) * n + np.sin(angle) * t).astype(F)


def perturb(case):
    """One perturbation per previous pixel, chosen by (x + 5 y) mod 12."""
    c = dict(case)
    g, a = case["prev_guides"].copy(), case["prev_accum"].copy()
    H, W = g.shape
    ys, xs = np.mgrid[0:H, 0:W]
    k = (xs + 5 * ys) % 12
    hit = g["shape"] != NONE
    tol, cosine = PARAMS["depth_tolerance"], PARAMS["normal_cosine"]
    g["shape"][(k == 3) & hit] += 1                                   # another shape
    g["shape"][(k == 3) & ~hit] = 0                                   # the sky becomes a shape
    g["time"][k == 4] *= F(1.0 + 0.9 * tol)                           # just inside DepthTolerance
    g["time"][k == 5] *= F(1.0 + 1.1 * tol)                           # just outside
    angle = float(np.arccos(cosine))
    g["normal"][k == 6] = _tilt(g["normal"][k == 6], 0.98 * angle)    # just inside NormalCosine
    g["normal"][k == 7] = _tilt(g["normal"][k == 7], 1.02 * angle)    # just outside
    a[k == 8] = 0                                                     # empty
    a[k == 9, 1] = np.nan
    a[k == 10, 0] = np.inf
    a[(k == 11) & (xs % 2 == 0), 3] = -np.inf
    c["prev_guides"], c["prev_accum"] = g, a
    return c


@functools.lru_cache(maxsize=None)
def _adversarial():
    pt = sys.modules["path_tracer_amd"]       # loaded by tests/conftest.py
    out = {}
    for name, size in (("identity-16x16", (16, 16)), ("identity-1x1", (1, 1))):
        out[name] = _two_views(pt, 1, 0, size, size, C1_PREV, C1_PREV, 10 + size[0])
    out["identity-16x16-perturbed"] = perturb(out["identity-16x16"])
    nan = dict(out["identity-1x1"])
    nan["prev_accum"] = np.full((1, 1, 4), np.nan, F)
    out["identity-1x1-nan"] = nan
    out["pan-29x33-to-37x21-perturbed"] = perturb(_two_views(pt, 1, 0, (29, 33), (37, 21), C1_PREV, C1_PAN, 20))
    out["pinhole-pan-perturbed"] = perturb(_coherent()["pinhole-pan"])
    out["look-away"] = _two_views(pt, 1, 0, (64, 32), (64, 32), ((0.0, -4.0, 1.0), (HALF_PI, 0.0, float(np.pi))),
                                  C1_PREV, 21)
    return out


def restate(case, detail=False, **params):
    p = dict(PARAMS, **params)
    return rr.reproject(case["prev_accum"], case["prev_guides"], case["prev_cam"], case["guides"], case["cam"],
                        detail=detail, **p)


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (case, the restatement's result)}, coverage asserted."""
    out, rejected = {}, {r: 0 for r in rr.RULES}
    behind = short = 0
    for kind, cases in (("coherent", _coherent()), ("adversarial", _adversarial())):
        for name, case in cases.items():
            ref, d = restate(case, detail=True)
            out[name] = (case, ref)
            have = ref[..., 3] > 0
            if kind == "coherent":
                assert have.mean() >= 0.25, (name, have.mean())
                assert (~have).mean() >= 0.05, (name, (~have).mean())
            for r in rr.RULES:
                others = np.ones_like(d[r])
                for o in rr.RULES:
                    if o != r:
                        others &= d[o]
                rejected[r] += int((d["located"][None] & ~d[r] & others).sum())
            behind += int(d["behind"].sum())
            short += int((d["located"] & (d["wsum"] > 0) & (d["wsum"] < F(PARAMS["min_weight"]))).sum())
    assert all(rejected.values()), rejected
    assert behind > 0 and short > 0, (behind, short)
    return out


def names():
    return ["pinhole-pan", "thin-lens", "360-rotation", "resize", "identity-16x16", "identity-16x16-perturbed",
            "identity-1x1", "identity-1x1-nan", "pan-29x33-to-37x21-perturbed",
            "pinhole-pan-perturbed", "look-away"]


def same_bits(a, b):
    """Elementwise: equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
