"""Inputs shared by the moving-shape reprojection tests
(tests/test_reproject_moving.py on the CPU, tests/test_gpu_reproject_moving.py
on the device).

The test scene: a white diffuse plane, a red diffuse sphere at (-0.8, 0, 1)
that moves to (-0.5, 0.2, 1), a blue diffuse cube at (1.5, 0.5, 0.7), scale
0.7, whose rotation goes from (0, 0, 0) to (0, 0, 0.3), and an unmoved camera
at (0, -5, 1.5), rotation (1.45, 0, 0).  Guide images come from
denoise_restatement.guides on the CPU oracle's ray query, the motion table
from the restatement, the history from reproject_cases.history.

  scene-96x54        the test scene, pinhole
  scene-64x40-50x37  previous 64x40, current 50x37
  scene-360          the camera made a 360 one, 96x48 (the shapes are small in a panorama)
  scene-thin-lens    a thin lens, 48x27
  scene-17x16        one tile and a column
  scene-1x1          one pixel
  table-*            scene-64x40-50x37 with a synthetic table: its last
                     record cut off (the cube's index == count, the sphere's
                     == count - 1), an empty table, every flag combination,
                     a Normal that sends the normal to zero, NaN and infinite
                     entries

all_cases() computes the restatement once per case and asserts what the tests
rely on: moved pixels with and without a history, static pixels, pixels
without a record."""
from __future__ import annotations

import functools
import sys

import numpy as np

import denoise_restatement as dr
import reproject_cases as rc
import reproject_moving_restatement as rm
import reproject_restatement as rr

F = np.float32
NONE = 0xFFFFFFFF
PARAMS = dict(rc.PARAMS)
SPHERE = ((-0.8, 0.0, 1.0), (-0.5, 0.2, 1.0))
CUBE_ROTATION = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.3))
CAMERA = ((0.0, -5.0, 1.5), (1.45, 0.0, 0.0))


def build_scene(pt, camera="pinhole"):
    """(scene, sphere entity, cube entity), before the move, packed."""
    s = pt.Scene.empty()
    cam = s.create_entity(pt.ENTITY_CAMERA, position=CAMERA[0], rotation=CAMERA[1])
    if camera == "360":
        s.set_camera_360(cam)
    elif camera == "thin-lens":
        s.set_camera_thin_lens(cam, aperture_mm=0.0, focus=5.0)
    white = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "White", BaseColor=(0.9, 0.9, 0.9))
    red = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Red", BaseColor=(0.8, 0.1, 0.1))
    blue = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Blue", BaseColor=(0.1, 0.2, 0.8))
    s.create_entity(pt.ENTITY_PLANE, material=white)
    sphere = s.create_entity(pt.ENTITY_SPHERE, position=SPHERE[0], material=red)
    cube = s.create_entity(pt.ENTITY_CUBE, position=(1.5, 0.5, 0.7), rotation=CUBE_ROTATION[0], scale=(0.7, 0.7, 0.7),
                           material=blue)
    s.pack()
    return s, sphere, cube


def move(scene, sphere, cube):
    scene.set_transform(sphere, position=SPHERE[1])
    scene.set_transform(cube, position=(1.5, 0.5, 0.7), rotation=CUBE_ROTATION[1], scale=(0.7, 0.7, 0.7))
    scene.pack()


def two_frames(pt, prev_size, size, seed, camera="pinhole"):
    scene, sphere, cube = build_scene(pt, camera)
    case = dict(prev_cam=scene.arrays()["cameras"][0].copy(), prev_shapes=scene.arrays()["shapes"].copy(),
                prev_guides=dr.guides(scene, 0, *prev_size), prev_accum=rc.history(*prev_size, seed))
    move(scene, sphere, cube)
    case.update(cam=scene.arrays()["cameras"][0].copy(), shapes=scene.arrays()["shapes"].copy(),
                guides=dr.guides(scene, 0, *size), sphere=scene.shape_index(sphere), cube=scene.shape_index(cube))
    scene.close()
    case["motion"] = rm.shape_motion(case["prev_shapes"], case["shapes"])
    return case


def _with_table(case, motion):
    c = dict(case)
    c["motion"] = motion
    return c


@functools.lru_cache(maxsize=None)
def _cases():
    pt = sys.modules["path_tracer_amd"]       # loaded by tests/conftest.py
    out = {
        "scene-96x54": two_frames(pt, (96, 54), (96, 54), 31),
        "scene-64x40-50x37": two_frames(pt, (64, 40), (50, 37), 32),
        "scene-360": two_frames(pt, (96, 48), (96, 48), 33, "360"),
        "scene-thin-lens": two_frames(pt, (48, 27), (48, 27), 34, "thin-lens"),
        "scene-17x16": two_frames(pt, (17, 16), (17, 16), 35),
        "scene-1x1": two_frames(pt, (1, 1), (1, 1), 36),
    }
    base = out["scene-64x40-50x37"]
    table = base["motion"]
    assert len(table) == 3 and max(base["sphere"], base["cube"]) == 2
    out["table-cut"] = _with_table(base, table[:2].copy())             # s == count - 1 and s == count both occur
    out["table-empty"] = _with_table(base, table[:0].copy())
    flagged = table.copy()
    flagged["Flags"] = [rm.MOVED | rm.NO_HISTORY, rm.MOVED | 4, 8]      # no history; moved; row 8's path
    flagged["Point"][0] = table["Point"][1]
    out["table-flagged"] = _with_table(base, flagged)
    zero = table.copy()
    zero["Normal"][base["sphere"]] = 0
    zero["Normal"][base["cube"]][6:] = 0                               # its sides' normals survive, its top's goes to zero
    out["table-zero-normal"] = _with_table(base, zero)
    bad = table.copy()
    bad["Point"][base["sphere"]][3] = np.nan
    bad["Normal"][base["cube"]][4] = np.inf
    out["table-nan-inf"] = _with_table(base, bad)
    bad2 = table.copy()
    bad2["Normal"][base["sphere"]][:] = np.nan
    bad2["Point"][base["cube"]][5] = -np.inf
    bad2["Flags"][0] = rm.MOVED                                          # the unmoved plane through the moved path: identity
    out["table-nan-inf-2"] = _with_table(base, bad2)
    return out


def names():
    return ["scene-96x54", "scene-64x40-50x37", "scene-360", "scene-thin-lens", "scene-17x16", "scene-1x1",
            "table-cut", "table-empty", "table-flagged", "table-zero-normal", "table-nan-inf", "table-nan-inf-2"]


def restate(case, detail=False, motion="own", **params):
    p = dict(PARAMS, **params)
    m = case["motion"] if isinstance(motion, str) else motion
    return rm.reproject_moving(case["prev_accum"], case["prev_guides"], case["prev_cam"], case["guides"], case["cam"],
                               m, detail=detail, **p)


# --- the position-coded history -----------------------------------------------------

OFFSET = 4.0        # keeps the coded unit-primitive coordinates positive


def object_points(cam, guides, shapes):
    """(H, W, 3) float64: each hit pixel's primary hit in its shape's own
    space, From[s] (O + V t); NaN on misses."""
    H, W = guides.shape
    O, V = rr.rays(cam, W, H)
    t = guides["time"].astype(np.float64)
    P = np.stack([float(O[k]) + V[..., k].astype(np.float64) * t for k in range(3)], axis=-1)
    hit = guides["shape"] != NONE
    idx = np.where(hit, guides["shape"], 0).astype(np.int64)
    m = shapes["Transform"]["From"][idx].astype(np.float64).reshape(H, W, 4, 4)      # [column][row]
    obj = np.einsum("hwcr,hwc->hwr", m[:, :, :3, :3], P) + m[:, :, 3, :3]
    obj[~hit] = np.nan
    return obj


def position_coded(case):
    """The case with a previous accumulator that holds, per hit pixel, its
    object-space point + OFFSET with w = 1 (misses: OFFSET)."""
    c = dict(case)
    obj = object_points(case["prev_cam"], case["prev_guides"], case["prev_shapes"])
    a = np.ones(obj.shape[:2] + (4,), F)
    a[..., :3] = np.where(np.isnan(obj), 0.0, obj) + OFFSET
    c["prev_accum"] = a
    return c


def position_errors(coded, out, **params):
    """Per shape name, (error, bound, pixels, share): over the shape's current
    pixels whose four taps are all valid (the restatement's verdict; `share`
    of the shape's pixels), the distance between the reprojected mean and the
    pixel's own object point, and the largest distance between two of the
    four taps' object points.  Pixels where `out` has no history: error inf.
    params: the parameters `out` was made with (default: PARAMS)."""
    _, d = restate(coded, detail=True, **params)
    own = object_points(coded["cam"], coded["guides"], coded["shapes"])
    prev = coded["prev_accum"][..., :3].astype(np.float64) - OFFSET
    four = d["valid"].all(axis=0)
    res = {}
    for name in ("sphere", "cube"):
        of_shape = coded["guides"]["shape"] == coded[name]
        ys, xs = np.nonzero(four & of_shape)
        taps = np.stack([prev[d["y0"][ys, xs] + (i >> 1), d["x0"][ys, xs] + (i & 1)] for i in range(4)], axis=1)
        bound = np.linalg.norm(taps[:, :, None] - taps[:, None], axis=-1).max(axis=(1, 2))
        o = out[ys, xs].astype(np.float64)
        with np.errstate(all="ignore"):
            mean = o[:, :3] / o[:, 3:4] - OFFSET
        err = np.where(o[:, 3] > 0, np.linalg.norm(mean - own[ys, xs], axis=-1), np.inf)
        res[name] = (err, bound, (ys, xs), len(ys) / max(int(of_shape.sum()), 1))
    return res


DEFAULTS = dict(normal_cosine=0.9, depth_tolerance=0.05, min_weight=0.25, max_history=64.0)   # ReprojectParameters()


def position_coded_check(reproject):
    """`reproject(case, motion)` -> (H, W, 4), with the default parameters.
    The test scene at 96x54 with a position-coded history; over the moved
    shapes' pixels whose four taps are all valid (at least 45 % of the cube's
    and 75 % of the sphere's):

      with the table    every pixel's error is within the largest distance
                        between two of its taps' object points (cube), twice
                        that (sphere);
      without (control) more than half of those pixels, the two shapes taken
                        together, have a history whose error is beyond that
                        bound (a pixel left without a history is not counted
                        as beyond it)."""
    case, _, _ = all_cases()["scene-96x54"]
    coded = position_coded(case)
    with_table = position_errors(coded, reproject(coded, coded["motion"]), **DEFAULTS)
    without = position_errors(coded, reproject(coded, None), **DEFAULTS)
    beyond = pixels = 0
    for name, factor, share in (("cube", 1.0, 0.45), ("sphere", 2.0, 0.75)):
        err, bound, _, have = with_table[name]
        ctl = without[name][0]
        wrong = np.isfinite(ctl) & (ctl > factor * bound)
        print(f"{name}: four valid taps on {have:.3f} of its pixels ({len(err)}); with the table max error "
              f"{err.max():.5f}, largest bound {factor * bound.max():.5f}; without: median error "
              f"{np.median(ctl[np.isfinite(ctl)]):.4f}, beyond the bound {wrong.mean():.3f}, "
              f"no history {(~np.isfinite(ctl)).mean():.3f}")
        assert have >= share, (name, have)
        assert np.all(err <= factor * bound), (name, int((err > factor * bound).sum()))
        beyond += int(wrong.sum())
        pixels += len(ctl)
    print(f"without the table: {beyond} of {pixels} pixels beyond their bound")
    assert beyond > 0.5 * pixels


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: (case, the restatement's result, its detail)}, coverage asserted."""
    out = {}
    for name, case in _cases().items():
        ref, d = restate(case, detail=True)
        out[name] = (case, ref, d)
    have = lambda n: out[n][1][..., 3] > 0
    for n in ("scene-96x54", "scene-64x40-50x37", "scene-360", "scene-thin-lens"):
        d = out[n][2]
        assert (d["moved"] & have(n)).sum() >= 20 and (d["moved"] & ~have(n)).sum() >= 1, n
        assert (d["static"] & have(n)).sum() >= 20 and not d["none"].any(), n
    assert out["scene-17x16"][2]["moved"].any()
    d = out["table-cut"][2]
    assert d["none"].any() and d["moved"].any() and (d["moved"] & have("table-cut")).any()
    assert out["table-empty"][2]["none"].sum() == (out["table-empty"][0]["guides"]["shape"] != NONE).sum() > 0
    d = out["table-flagged"][2]
    assert d["none"].any() and d["moved"].any() and d["static"].any()
    d = out["table-zero-normal"][2]
    sphere = out["table-zero-normal"][0]["guides"]["shape"] == out["table-zero-normal"][0]["sphere"]
    assert sphere.sum() > 20 and not (sphere & have("table-zero-normal")).any()
    assert (d["moved"] & have("table-zero-normal")).any()
    return out
