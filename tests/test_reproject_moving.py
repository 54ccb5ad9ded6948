"""Moving-shape reprojection on the CPU: ptsShapeMotion
and ptsReprojectMoving against the numpy restatement
(tests/reproject_moving_restatement.py) bit for bit, equality with row 8
wherever nothing moved, the position-coded history that shows the history
follows the surface, a real frame of the oracle, and the argument checks."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_lib
import reproject_cases as rc
import reproject_moving_cases as mc
import reproject_moving_restatement as rm

F = np.float32
NONE = 0xFFFFFFFF


def params(pt, **kw):
    p = dict(mc.PARAMS, **kw)
    return pt.ReprojectParameters(p["normal_cosine"], p["depth_tolerance"], p["min_weight"], p["max_history"])


def host(pt, case, motion="own", **kw):
    m = case["motion"] if isinstance(motion, str) else motion
    return pt.reproject_host(case["prev_accum"], case["prev_guides"], case["prev_cam"], case["guides"], case["cam"],
                             params(pt, **kw), motion=m)


# --- the motion table ---------------------------------------------------------------

def packed_shapes(pt, edits=()):
    """The packed shapes of a small scene: a plane, a sphere, a cube and a
    sphere inside a rotated, non-uniformly scaled container.  edits: (entity
    name, transform keywords) applied before packing."""
    s = pt.Scene.empty()
    s.create_entity(pt.ENTITY_CAMERA, position=(0, -5, 1.5))
    m = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "M", BaseColor=(0.5, 0.5, 0.5))
    box = s.create_entity(pt.ENTITY_CONTAINER, position=(0.3, 1.0, 0.2), rotation=(0.2, -0.4, 1.1), scale=(1.5, 0.5, 2.0))
    ents = dict(plane=s.create_entity(pt.ENTITY_PLANE, material=m),
                sphere=s.create_entity(pt.ENTITY_SPHERE, position=(-0.8, 0.0, 1.0), material=m),
                cube=s.create_entity(pt.ENTITY_CUBE, position=(1.5, 0.5, 0.7), scale=(0.7, 0.7, 0.7), material=m),
                inner=s.create_entity(pt.ENTITY_SPHERE, parent=box, position=(0.1, 0.2, 0.3), material=m), box=box)
    for name, kw in edits:
        s.set_transform(ents[name], **kw)
    s.pack()
    shapes = s.arrays()["shapes"].copy()
    index = {k: s.shape_index(e) for k, e in ents.items() if k != "box"}
    s.close()
    return shapes, index


MOVES = {
    "translation": [("sphere", dict(position=(-0.5, 0.2, 1.0)))],
    "rotation": [("cube", dict(position=(1.5, 0.5, 0.7), rotation=(0.0, 0.0, 0.3), scale=(0.7, 0.7, 0.7)))],
    "non-uniform-scale": [("cube", dict(position=(1.5, 0.5, 0.7), rotation=(0.4, 0.1, -0.3), scale=(0.7, 1.3, 0.2)))],
    "inside-a-container": [("inner", dict(position=(0.4, -0.2, 0.3), rotation=(0.5, 0.0, 0.2), scale=(1.0, 2.0, 0.5)))],
    "the-container": [("box", dict(position=(0.3, 1.2, 0.2), rotation=(0.2, -0.3, 1.1), scale=(1.5, 0.6, 2.0)))],
}


@pytest.mark.parametrize("name", list(MOVES))
def test_shape_motion_matches_restatement(pt, name):
    prev, index = packed_shapes(pt)
    cur, _ = packed_shapes(pt, MOVES[name])
    out = pt.shape_motion(prev, cur)
    ref = rm.shape_motion(prev, cur)
    assert out.dtype == pt.SHAPE_MOTION_DTYPE and out.tobytes() == ref.tobytes()
    target = "inner" if name == "the-container" else MOVES[name][0][0]
    for k, i in index.items():
        assert int(out["Flags"][i]) == (pt.SHAPE_MOTION_MOVED if k == target else 0), k
    # What the matrices mean, in float64: Point takes the current world point of an
    # object point to its previous world point, Normal is Point's inverse transpose.
    i = index[target]
    to_p = prev["Transform"]["To"][i].astype(np.float64).reshape(4, 4).T
    to_c = cur["Transform"]["To"][i].astype(np.float64).reshape(4, 4).T
    point = np.vstack([out["Point"][i].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
    q = np.array([0.3, -0.6, 0.5, 1.0])
    assert np.allclose(point @ (to_c @ q), to_p @ q, atol=1e-4)
    assert np.allclose(out["Normal"][i].astype(np.float64).reshape(3, 3), np.linalg.inv(point[:3, :3]).T, atol=1e-4)


def test_shape_motion_of_equal_transforms_is_the_exact_identity(pt):
    prev, _ = packed_shapes(pt)
    cur, _ = packed_shapes(pt)
    cur["MaterialIndex"] += 1                                # not part of the comparison
    out = pt.shape_motion(prev, cur)
    assert out.tobytes() == rm.shape_motion(prev, cur).tobytes()
    assert not out["Flags"].any()
    eye4, eye3 = np.eye(4, dtype=F)[:3].reshape(-1), np.eye(3, dtype=F).reshape(-1)
    for m in out:
        assert m["Point"].tobytes() == eye4.tobytes() and m["Normal"].tobytes() == eye3.tobytes()


def test_shape_motion_without_a_history(pt):
    prev, index = packed_shapes(pt)
    moved, _ = packed_shapes(pt, MOVES["translation"])
    cur = moved.copy()
    cur["Type"][index["cube"]] = 2                           # a cube became a sphere
    cur["MeshRootNodeIndex"][index["plane"]] += 1
    cur["Transform"]["To"][index["inner"]][5] = np.nan
    out = pt.shape_motion(prev[:4], np.concatenate([cur, cur[:2]]))     # count growth: indices 4.. are new
    ref = rm.shape_motion(prev[:4], np.concatenate([cur, cur[:2]]))
    assert out.tobytes() == ref.tobytes()
    expect = {index["cube"]: 2, index["plane"]: 2, index["inner"]: 2, index["sphere"]: 1}
    for i in range(len(out)):
        want = 2 if i >= 4 else expect[i]
        assert int(out["Flags"][i]) == want, i
        if want == 2:
            assert not out["Point"][i].any() and not out["Normal"][i].any()
    for where, field in (("prev", "From"), ("cur", "To"), ("cur", "From")):       # a non-finite value on either side
        a, b = prev.copy(), moved.copy()
        (a if where == "prev" else b)["Transform"][field][index["sphere"]][12] = np.inf
        out = pt.shape_motion(a, b)
        assert int(out["Flags"][index["sphere"]]) == 2 and out.tobytes() == rm.shape_motion(a, b).tobytes()
    both = prev.copy()
    both["Transform"]["To"][0][0] = np.nan                   # bytewise equal, but not finite
    assert int(pt.shape_motion(both, both)["Flags"][0]) == 2
    assert len(pt.shape_motion(prev, prev[:0])) == 0 and int(pt.shape_motion(prev[:0], prev)["Flags"].min()) == 2


# --- the reprojection ---------------------------------------------------------------

def test_case_list_is_complete():
    assert sorted(mc.names()) == sorted(mc.all_cases())          # all_cases() asserts the coverage conditions


@pytest.mark.parametrize("name", mc.names())
def test_host_matches_restatement(pt, name):
    case, ref, _ = mc.all_cases()[name]
    before = {k: np.array(v, copy=True) for k, v in case.items()}
    out = host(pt, case)
    same = rc.same_bits(out, ref)
    assert same.all(), np.argwhere(~same)[:5]
    for k, v in case.items():
        assert np.asarray(v).tobytes() == before[k].tobytes(), k
    assert case["motion"].tobytes() == pt.shape_motion(case["prev_shapes"], case["shapes"]).tobytes() \
        or name.startswith("table-")


def test_other_parameters_match_restatement(pt):
    case, _, _ = mc.all_cases()["scene-64x40-50x37"]
    for kw in (dict(normal_cosine=0.5, depth_tolerance=0.2, min_weight=0.01, max_history=float("inf")),
               dict(normal_cosine=1.0, depth_tolerance=1e-4, min_weight=1.0, max_history=0.5)):
        same = rc.same_bits(host(pt, case, **kw), mc.restate(case, **kw))
        assert same.all(), (kw, np.argwhere(~same)[:5])


@pytest.mark.parametrize("name", rc.names())
def test_unmoved_tables_give_row_8(pt, name):
    """Every case of tests/reproject_cases.py: motion=None and a table of
    unmoved shapes (as ptsShapeMotion makes it of two equal packs) both give
    reproject_host's bits; so does the restatement."""
    case, ref = rc.all_cases()[name]
    p = pt.ReprojectParameters(*(rc.PARAMS[k] for k in ("normal_cosine", "depth_tolerance", "min_weight",
                                                          "max_history")))
    args = (case["prev_accum"], case["prev_guides"], case["prev_cam"], case["guides"], case["cam"], p)
    row8 = pt.reproject_host(*args)
    shapes = case["guides"]["shape"]
    count = int(shapes[shapes != NONE].max()) + 2 if (shapes != NONE).any() else 1   # the perturbed ids included
    packed = np.zeros(count, pt.SHAPE_DTYPE)
    packed["Transform"]["To"][:] = packed["Transform"]["From"][:] = np.eye(4, dtype=F).reshape(-1)
    table = pt.shape_motion(packed, packed)
    assert not table["Flags"].any()
    for motion in (None, table):
        out = pt.reproject_host(*args, motion=motion)
        assert np.array_equal(out.view(np.uint32), row8.view(np.uint32))
    assert rc.same_bits(mc.rm.reproject_moving(*args[:5], table, **rc.PARAMS), ref).all()


def test_position_coded_history_follows_the_surface(pt):
    """The previous accumulator holds each pixel's object-space hit point.
    With the table a moved pixel gets back its own point, to within the extent
    of its four taps (planar faces: both lie in the taps' quad; the sphere:
    twice that, for the sagitta of the hull).  Without it, row 8 returns a
    point about 0.3 object units away on more than half of these pixels
    (reproject_moving_cases.position_coded_check).  Fails without the table."""
    assert vars(pt.ReprojectParameters()) == dict(NormalCosine=0.9, DepthTolerance=0.05, MinWeight=0.25, MaxHistory=64.0)
    mc.position_coded_check(lambda c, m: host(pt, c, motion=m, **mc.DEFAULTS))


def oracle_frame(pt, scene, W, H, rounds, frame_index):
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.FrameIndex = frame_index
    o.reset()
    o.run(2)
    for _ in range(rounds - 2):
        o.run(1)
    a = o.accum()
    o.close()
    return a


def test_real_frame_history_helps_on_moved_pixels(pt):
    """The test scene at 64x36 on the CPU oracle: 32 rounds before the move;
    after it 2 fresh rounds and a 512-round reference.  Over the moved shapes'
    pixels, the error of history + 2 rounds over the error of the 2 rounds
    alone.  Measured: 0.4597 with the table, 0.6523 without; the bound
    asserted after the comparison is halfway between 0.4597 and 1: 0.7299."""
    import denoise_restatement as dr
    W, H = 64, 36
    scene, sphere, cube = mc.build_scene(pt)
    prev = oracle_frame(pt, scene, W, H, 32, 0)
    prev_cam, prev_shapes = scene.arrays()["cameras"][0].copy(), scene.arrays()["shapes"].copy()
    prev_guides = dr.guides(scene, 0, W, H)
    mc.move(scene, sphere, cube)
    cam, shapes = scene.arrays()["cameras"][0].copy(), scene.arrays()["shapes"].copy()
    guides = dr.guides(scene, 0, W, H)
    fresh = oracle_frame(pt, scene, W, H, 2, 1 << 24)
    reference = oracle_frame(pt, scene, W, H, 512, 2 << 24)
    moved = np.isin(guides["shape"], [scene.shape_index(sphere), scene.shape_index(cube)])
    scene.close()
    assert moved.sum() > 100

    def mean(acc):
        with np.errstate(all="ignore"):
            return np.where(acc[..., 3:4] > 0, acc[..., :3] / acc[..., 3:4], 0).astype(np.float64)

    ref = mean(reference)[moved]
    alone = np.linalg.norm(mean(fresh)[moved] - ref)
    ratio = {}
    for key, motion in (("with", pt.shape_motion(prev_shapes, shapes)), ("without", None)):
        carried = pt.reproject_host(prev, prev_guides, prev_cam, guides, cam, motion=motion)
        ratio[key] = np.linalg.norm(mean(carried + fresh)[moved] - ref) / alone
    print(f"moved pixels ({int(moved.sum())}): error ratio with the table {ratio['with']:.4f}, without {ratio['without']:.4f}")
    assert ratio["with"] < ratio["without"]
    assert ratio["with"] < 0.7299


# --- arguments ----------------------------------------------------------------------

def test_argument_errors_leave_out_untouched(pt):
    N = pt._native
    L = N.scene_lib()
    case, _, _ = mc.all_cases()["scene-17x16"]
    a, pg, g, m = case["prev_accum"], case["prev_guides"], case["guides"].copy(), case["motion"].copy()
    pc = N.pt_packed_camera.from_buffer_copy(case["prev_cam"].tobytes())
    c = N.pt_packed_camera.from_buffer_copy(case["cam"].tobytes())
    out = np.full((16, 17, 4), 7.0, F)
    ok = N.pt_reproject_parameters(0.9, 0.02, 0.25, 64.0)

    def call(**kw):
        d = dict(wp=17, hp=16, a=N.fptr(a), pg=pg.ctypes.data, pc=C.byref(pc), w=17, h=16, g=g.ctypes.data,
                 c=C.byref(c), m=m.ctypes.data, n=len(m), p=C.byref(ok), out=N.fptr(out))
        d.update(kw)
        return L.ptsReprojectMoving(d["wp"], d["hp"], d["a"], d["pg"], d["pc"], d["w"], d["h"], d["g"], d["c"],
                                    d["m"], d["n"], d["p"], d["out"])

    bad = [dict(a=None), dict(pg=None), dict(pc=None), dict(g=None), dict(c=None), dict(p=None), dict(wp=0),
           dict(hp=0), dict(w=0), dict(h=0), dict(g=pg.ctypes.data), dict(m=None),
           dict(p=C.byref(N.pt_reproject_parameters(0.9, 0.0, 0.25, 64.0))),
           dict(m=None, n=0, a=None), dict(m=None, n=0, w=0)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert np.all(out == 7.0)
    assert call(out=None) != 0
    assert call(m=None, n=0) == 0 and not np.all(out == 7.0)                 # no table: row 8
    assert out.tobytes() == pt.reproject_host(a, pg, case["prev_cam"], g, case["cam"], params(pt)).tobytes()
    assert call() == 0 and call(n=0) == 0
    assert L.ptsShapeMotion(None, 1, m.ctypes.data, 0, None) != 0 and L.ptsShapeMotion(None, 0, None, 1, None) != 0
    assert L.ptsShapeMotion(None, 0, None, 0, None) == 0
    with pytest.raises(pt.PathTracerError):
        host(pt, case, min_weight=0.0)
    assert pt.SHAPE_MOTION_DTYPE.itemsize == 96 and pt.SHAPE_MOTION_DTYPE.fields["Flags"][1] == 84
    assert pt.SHAPE_DTYPE.itemsize == 144 and (pt.SHAPE_MOTION_MOVED, pt.SHAPE_MOTION_NO_HISTORY) == (1, 2)
