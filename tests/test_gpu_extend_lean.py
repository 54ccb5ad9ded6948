"""GPU: the lean extend loop (DESIGN.md §4 "Lean extend"): the face test with
the fast reciprocal, the folded miss flag and 32-bit record offsets, and the
mesh-only step's joined update on wave masks with its wave-uniform skips.

None of it may change a result: every ray keeps its sequence of nodes, faces
and arithmetic results, so slots, pixels and hit records are held to the CPU
oracle bit for bit:

  * C3 at 80x48 and 64x16 over 42 rounds (Reset, Run(2), 40 rounds: through the
    length table's training rounds and its first finalize), in LENGTH order
    with the RUN block map and in OCTANT order with the TILE map;
  * C2 (the general loop: several shapes) at 64x64 over 8 rounds;
  * a hand-made mesh of 16 triangles through the ray-query entry point, with
    coordinates beyond the exact fast division's range (the loops' IEEE
    variant), in the mesh-only and the general loop and on every stack format:
    zero-area faces, a needle, |Det| on either side of PT_EPSILON, |Det| at and
    around 2^126 and strictly between 2^126 and 2^127 (beyond the fast
    reciprocal's bound: the IEEE division block), a
    denormal |Det|, rays along edges and through vertices (U = 0, W = 0,
    U + W = 1 exactly) and rays whose duration is exactly the hit time;
  * the any-hit query on the same mesh and rays against the oracle's hit mask.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib
from test_gpu_block_map import FLAGS, LENGTH, RUN, TILE, assert_oracle, close, oracle_after, renderer, snapshot
from test_gpu_mesh_extend import AUTO, GENERAL, MESH, mesh_scene, upload
from test_gpu_parity import compare_hits, compare_state, render_pair, scene_for

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = 0xFFFFFFFF
OCTANT = 1                       # PT_RAY_ORDER_OCTANT
EPS = f32(1e-9)                  # PT_EPSILON


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("order,block_map", [(LENGTH, RUN), (OCTANT, TILE)], ids=["length-run", "octant-tile"])
@pytest.mark.parametrize("W,H", [(80, 48), (64, 16)], ids=["80x48", "64x16"])
def test_c3_42_rounds_equal_the_oracle(pt, dev, W, H, order, block_map):
    r = renderer(pt, dev, scene_for(pt, 3), W, H, block_map, split=3)
    if order == OCTANT:
        r[0].set_ray_order(OCTANT)
    r[0].reset()
    r[0].run(2)
    first, last = oracle_after(pt, W, H)
    assert r[0].ray_order()["used"] == order and r[0].block_map()["used"] == block_map
    assert_oracle(snapshot(dev, *r[:2]), first, W, H, 2)
    r[0].run_rounds(40)
    assert_oracle(snapshot(dev, *r[:2]), last, W, H, 42)
    if order == LENGTH:
        assert r[2].length_table()["trained"]
    close(r)


def test_c2_general_loop_8_rounds_equal_the_oracle(pt, dev):
    gs, os_, ga, oa = render_pair(pt, dev, 2, 64, 64, [2, 1, 1, 1, 1, 1, 1])
    compare_state(gs, os_)
    assert np.array_equal(ga.view(np.uint32), oa.view(np.uint32))


# --- the hand-made mesh -------------------------------------------------------------
#
# Object space is world space (identity instance transform) and the test rays
# run along +z from z = 0, so for a face {P0, P0 + (a, 0, 0), P0 + (0, b, 0)}
# the arithmetic of the face test is exact where the test needs it:
# Det = -a b, U = x - P0.x over a, W = y - P0.y over b, T = P0.z.

A15 = f32(2.0 ** -15)
B_EPS = f32(EPS * f32(2.0 ** 15))            # a b = PT_EPSILON exactly (a power-of-two scaling)
BIG = f32(2.0 ** 63)


def below(x):
    return np.nextafter(f32(x), f32(0))


def above(x):
    return np.nextafter(f32(x), f32(np.inf))


def right_face(x0, y0, z, a, b):
    return [(x0, y0, z), (f32(x0) + f32(a), y0, z), (x0, f32(y0) + f32(b), z)]


FACES = [
    right_face(0.0, 0.0, 1.0, 1.0, 1.0),                                  # 0 the unit triangle: edges and vertices
    [(3.0, 0.0, 1.0), (4.0, 0.0, 1.0), (5.0, 0.0, 1.0)],                  # 1 zero area: collinear
    [(3.0, 0.5, 1.0), (3.0, 0.5, 1.0), (3.0, 0.5, 1.0)],                  # 2 zero area: one point
    right_face(6.0, 0.0, 1.0, 1e-6, 1.0),                                 # 3 a needle
    right_face(8.0, 0.0, 1.0, A15, B_EPS),                                # 4 |Det| == PT_EPSILON: tested
    right_face(9.0, 0.0, 1.0, A15, below(B_EPS)),                         # 5 just below: rejected
    right_face(10.0, 0.0, 1.0, A15, above(B_EPS)),                        # 6 just above
    right_face(12.0, 0.0, 1.0, A15, f32(2.0 ** -120)),                    # 7 denormal |Det| (2^-135)
    # Huge faces from x = 16, 32, 64, 128 on, each in front of the last: the closest at x = 20, 40, 100, 200
    # is 8, 9, 10, 11.  The fast reciprocal is proven below 2^126 only, so 8, 10 and 11 need the division.
    right_face(16.0, -BIG / 4, 2.0, BIG, BIG),                            # 8 |Det| == 2^126: the division block
    right_face(32.0, -BIG / 4, 1.75, BIG, below(BIG)),                    # 9 just below 2^126: the fast reciprocal
    right_face(64.0, -BIG / 4, 1.5, BIG, f32(2.0) * BIG),                 # 10 |Det| == 2^127
    right_face(128.0, -BIG / 4, 1.25, BIG, f32(1.5) * BIG),               # 11 |Det| == 1.5 * 2^126: inside (2^126, 2^127)
    [(3.2, 2.1, 0.9), (3.9, 2.3, 0.5), (3.4, 2.9, 0.7)],                  # 12-15 ordinary, tilted faces
    [(5.1, 2.2, 0.5), (5.8, 2.1, 0.9), (5.5, 2.9, 0.6)],
    [(6.6, 2.1, 0.7), (7.4, 2.3, 0.6), (6.9, 2.8, 0.9)],
    [(1.5, 2.2, 0.8), (2.4, 2.1, 0.6), (2.0, 2.9, 0.5)],
]


def lean_mesh():
    pos = np.array([p for face in FACES for p in face], np.float32)
    idx = np.arange(3 * len(FACES), dtype=np.uint32).reshape(-1, 3)
    return pos, idx


def axial(points, dur):
    """Rays from (x, y, 0) along +z."""
    o = np.array([(x, y, 0.0) for x, y in points], np.float32)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(o), 1))
    return o, oracle_lib.pack_unit_vectors(d), np.full(len(o), dur, np.float32)


def lean_rays():
    """{name: (origins, packed velocities, durations)}; `all` is their
    concatenation with 1500 random rays (an odd count over several blocks, the
    special rays spread among ordinary ones in every wave)."""
    h, q = f32(0.5), f32(0.25)
    one_m, one_p = below(1.0), above(1.0)
    groups = {
        # U = 0, W = 0, U + W = 1, the three vertices, and the floats next to each bound
        "edges": axial([(0.0, h), (h, 0.0), (h, h), (q, 0.75), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0),
                        (-1e-45, h), (h, -1e-45), (h, above(above(h))), (one_p, 0.0), (0.0, one_p), (one_m, 0.0),
                        (below(h), h), (-0.0, h), (h, -0.0), (h, above(h))], 1048576.0),
        "edges_at_duration": axial([(0.0, h), (h, 0.0), (h, h), (q, q)], 1.0),        # T == duration: accepted
        "edges_short": axial([(0.0, h), (h, 0.0), (h, h), (q, q)], below(1.0)),      # T one ulp beyond
        "eps": axial([(f32(8.0) + A15 / 4, B_EPS / 4)], 1048576.0),
        "eps_below": axial([(f32(9.0) + A15 / 4, B_EPS / 4)], 1048576.0),
        "eps_above": axial([(f32(10.0) + A15 / 4, B_EPS / 4)], 1048576.0),
        "denormal": axial([(f32(12.0) + A15 / 4, f32(2.0 ** -122))], 1048576.0),
        "zero_area": axial([(3.5, 0.0), (4.0, 0.0), (3.0, 0.5)], 1048576.0),
        "needle": axial([(f32(6.0) + f32(2.5e-7), 0.25), (6.0, 0.5), (f32(6.0) + f32(1e-6), 0.0)], 1048576.0),
        "huge": axial([(20.0, 5.0), (40.0, 30.0), (100.0, 20.0), (200.0, 9.0), (1000.0, -7.0)], 1048576.0),
        "huge_at_duration": axial([(20.0, 5.0), (24.0, -3.0)], 2.0),
        "huge_short": axial([(20.0, 5.0), (24.0, -3.0)], below(2.0)),
    }
    rng = np.random.default_rng(11)
    n = 1500
    o = np.column_stack([rng.uniform(-1, 9, n), rng.uniform(-0.5, 3.5, n), rng.uniform(-1, 0.4, n)]).astype(np.float32)
    target = np.column_stack([rng.uniform(-0.5, 24.0, n), rng.uniform(-0.2, 3.2, n), rng.uniform(0.5, 1.0, n)])
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dur = np.where(rng.random(n) < 0.25, rng.uniform(0.3, 2.5, n), 1048576.0).astype(np.float32)
    groups["random"] = (o, oracle_lib.pack_unit_vectors(d.astype(np.float32)), dur)
    parts = list(groups.values())
    order = np.random.default_rng(12).permutation(sum(len(p[0]) for p in parts))
    allr = tuple(np.ascontiguousarray(np.concatenate([p[i] for p in parts])[order]) for i in range(3))
    return groups, allr


_lean = {}


def lean_case(pt):
    """(scene, {group: (rays, the oracle's hits)}, all rays, the oracle's hits of all rays):
    built once, left unchanged."""
    if not _lean:
        s = mesh_scene(pt, lean_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0))
        groups, allr = lean_rays()
        groups = {name: (rays, oracle_lib.trace_rays(s.packs(), *rays)) for name, rays in groups.items()}
        _lean["case"] = (s, groups, allr, oracle_lib.trace_rays(s.packs(), *allr))
    return _lean["case"]


def test_the_mesh_is_what_it_claims(pt):
    """The oracle alone: each special face and ray does what its name says, so
    the comparisons below compare something.  (Needs the package, not a device.)"""
    s, groups, allr, ref = lean_case(pt)
    assert len(FACES) == 16
    t = lambda name: groups[name][1]
    hit = lambda h: h["shape_material"] != NONE
    e = t("edges")
    assert np.all(hit(e)[:7]) and np.all(e["time"][:7] == 1.0)                # the bounds belong to the face
    assert not hit(e)[7:12].any()                                             # one ulp outside
    assert np.all(hit(e)[12:]) and np.all(e["time"][12:] == 1.0)              # one ulp inside, -0, a sum that rounds to 1
    assert np.all(hit(t("edges_at_duration"))) and np.all(t("edges_at_duration")["time"] == 1.0)
    assert not hit(t("edges_short")).any()
    assert t("eps")["time"][0] == 1.0 and t("eps_above")["time"][0] == 1.0 and hit(t("eps"))[0] and hit(t("eps_above"))[0]
    assert not hit(t("eps_below"))[0] and not hit(t("denormal"))[0]
    assert not hit(t("zero_area")).any()
    assert np.all(hit(t("needle"))) and np.all(t("needle")["time"] == 1.0)
    assert np.all(hit(t("huge"))) and np.allclose(t("huge")["time"], [2.0, 1.75, 1.5, 1.25, 1.25], rtol=1e-6, atol=0)
    assert t("huge")["time"][0] == 2.0
    assert np.all(hit(t("huge_at_duration"))) and np.all(t("huge_at_duration")["time"] == 2.0)
    assert not hit(t("huge_short")).any()
    share = (ref["shape_material"] != NONE).mean()
    assert 0.10 <= share <= 0.95 and len(allr[0]) % 64 != 0 and len(allr[0]) > 1024


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["stack16", "stack32-packed", "stack32-node-index"])
@pytest.mark.parametrize("form", [AUTO, GENERAL], ids=["mesh-loop", "general-loop"])
def test_hand_made_mesh_hit_records(pt, dev, form, fmt):
    s, groups, allr, ref = lean_case(pt)
    ds = upload(pt, dev, s, form=form, stack_format=fmt)
    assert ds.extend_form == (MESH if form == AUTO else GENERAL)
    compare_hits(ds.trace_rays(*allr), ref)
    for rays, want in groups.values():      # each group alone: the special lanes are their wave's only ones
        compare_hits(ds.trace_rays(*rays), want)
    ds.close()


@pytest.mark.parametrize("form", [AUTO, GENERAL], ids=["mesh-loop", "general-loop"])
def test_hand_made_mesh_any_hit(pt, dev, form):
    s, groups, allr, ref = lean_case(pt)
    ds = upload(pt, dev, s, form=form)
    assert np.array_equal(ds.occluded(*allr), ref["shape_material"] != NONE)
    ds.close()
