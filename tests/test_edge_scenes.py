"""The edge-case catalogue (tests/edge_scenes.py) on the CPU: the oracle
against the two restatements written apart from it, and the catalogue against
its own claims.

  * every TIES and DEGENERATE ray set: the oracle's whole trace record against
    tests/trace_restatement.py, bit for bit.  An exact tie is where the visit
    order shows: a mesh face, a plane and a sphere reject on T > Hit.Time (the
    later visit wins), a cube on T >= Hit.Time (the earlier one), a child box
    entered exactly at the hit time is pruned, and TimeA > TimeB sends equal
    children to A first (scene.glsl.inc:304-520).
  * every MATERIALS scene: slots and accumulator after Reset, Run(2) and four
    Run(1) against tests/path_restatement.py.
  * "it is what it claims", from the oracle alone: the tie scenes hold rays
    with two candidates at a bit-equal time, the degenerate sets reach the
    pole tangent, the cancelled normal, both tangent branches and fract() = 0
    and 1, the shells fill the four active-shape entries, and no scene stores
    more than a quarter of its pixels non-finite.

The sphere pole: TangentX = normalize(cross(P, (-P.y, P.x, 0))) is
normalize(0) there, a NaN vector, which PackUnitVector packs as 0x80018001
(each snorm16 clamps a NaN to -1).  tests/kat.py's pack_snorm2x16 used
np.clip, which hands the NaN on to the integer cast (0x00000000);
test_pole_tangent_packs_as_the_convention_says fails on that version.
"""
from __future__ import annotations

import numpy as np
import pytest

import edge_scenes as es
import kat
import oracle_lib
import path_restatement as pr
import trace_restatement as tr
from test_path_restatement import check as check_path
from test_trace_restatement import check as check_trace

NONE = 0xFFFFFFFF
CUBE = 3                      # PT_SHAPE_TYPE_CUBE
SCHEDULE = [2, 1, 1, 1, 1]    # Reset, Run(2), four Run(1)
W, H = 16, 12
NONFINITE_CAP = 0.25


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def record_differs(a, b):
    """Per ray: another shape / material word, normal, tangent or UV."""
    out = a["shape_material"] != b["shape_material"]
    for f in ("packed_normal", "packed_tangent", "u", "v"):
        out |= bits(a[f]) != bits(b[f])
    return out


# --- the pole ----------------------------------------------------------------------

def test_pole_tangent_packs_as_the_convention_says(pt):
    """One unit sphere, rays down the axis (north, south, 1e-30 off axis): the
    oracle and the restatement both pack the 0/0 tangent as 0x80018001."""
    s = pt.Scene.empty()
    s.create_entity(pt.ENTITY_SPHERE)
    s.create_entity(pt.ENTITY_CAMERA, position=(0.0, 0.0, 3.0))
    s.pack()
    o = np.array([(0, 0, 3), (0, 0, -3), (0, 1e-30, 3)], np.float32)
    d = np.array([(0, 0, -1), (0, 0, 1), (0, 0, -1)], np.float32)
    vel = oracle_lib.pack_unit_vectors(d)
    dur = np.full(3, es.FAR, np.float32)
    rec = oracle_lib.trace_rays(s.packs(), o, vel, dur)
    assert rec["packed_tangent"].tolist() == [es.POLE_TANGENT] * 3
    times, sm, pn, ptg, uv = tr.trace_records(s.arrays(), o, kat.unpack_unit_vector(vel), dur)
    assert ptg.tolist() == [es.POLE_TANGENT] * 3
    assert kat.pack_snorm2x16(np.array([[np.nan, 0.5], [2.0, np.nan]], np.float32)).tolist() == [0x40008001, 0x80017FFF]
    assert check_trace(s.arrays(), s.packs(), o, vel, dur) == 3
    s.close()


# --- ties --------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(es.TIES))
def test_tie_rays_match_independent_restatement(pt, name):
    case = es.TIES[name]
    s = case.build(pt)
    o, v, d = es.tie_rays(s, case)
    assert len(v) % 2 == 1 and len(v) % 64 != 0 and 1500 < len(v) < 2600
    assert check_trace(s.arrays(), s.packs(), o, v, d) > 150
    s.close()


@pytest.mark.parametrize("name", sorted(es.TIES))
def test_tie_scenes_are_what_they_claim(pt, name):
    """At least 50 rays have two candidates at a bit-equal time: with the
    winner moved away, the ray hits something else at the same time bits.  In
    the scene that mixes the cube's rule with the others', a cube and a
    non-cube each win somewhere.  The Duration copies: a ray limited to
    exactly its hit time keeps a sphere hit (T > Hit.Time rejects) and loses a
    cube hit (T >= Hit.Time); one float shorter loses every such hit."""
    case = es.TIES[name]
    s = case.build(pt)
    o, v, d = es.tie_rays(s, case)
    n = len(v) // 3
    full = oracle_lib.trace_rays(s.packs(), o, v, d)
    far, exact, shorter = full[:n], full[n:2 * n], full[2 * n:]
    hit = far["shape_material"] != NONE
    tied = np.zeros(n, bool)
    for k in range(case.candidates):
        sk = case.build(pt, away=k)
        rk = oracle_lib.trace_rays(sk.packs(), o[:n], v[:n], d[:n])
        tied |= hit & (rk["shape_material"] != NONE) & (bits(rk["time"]) == bits(far["time"])) & record_differs(rk, far)
        sk.close()
    assert tied.sum() >= 50, int(tied.sum())
    types = s.arrays()["shapes"]["Type"]
    winner_is_cube = types[far["shape_material"][hit] >> 16] == CUBE
    cube = np.zeros(n, bool)
    cube[hit] = winner_is_cube
    if case.mixed:
        assert (tied & cube).sum() >= 5 and (tied & hit & ~cube).sum() >= 5, ((tied & cube).sum(), (tied & ~cube).sum())
    # Duration exactly the hit time, and one float less
    kept = (exact["shape_material"] == far["shape_material"]) & (bits(exact["time"]) == bits(far["time"]))
    assert not (kept & hit & cube).any()
    if name == "three-spheres":
        assert (kept & hit).sum() >= 50
    short_hit = shorter["shape_material"] != NONE
    assert not (short_hit & hit & (shorter["time"] >= far["time"])).any()
    assert (hit & ~short_hit).sum() >= 50
    s.close()


# --- degenerate hit attributes -----------------------------------------------------

@pytest.mark.parametrize("name", sorted(es.DEGENERATE))
def test_degenerate_rays_match_independent_restatement(pt, name):
    case = es.DEGENERATE[name]
    s = case.build(pt)
    o, v, d = case.rays(s)
    assert len(v) % 2 == 1 and len(v) > 64
    assert check_trace(s.arrays(), s.packs(), o, v, d) > 50
    s.close()


def traced(pt, name):
    case = es.DEGENERATE[name]
    s = case.build(pt)
    o, v, d = case.rays(s)
    rec = oracle_lib.trace_rays(s.packs(), o, v, d)
    s.close()
    return o, v, rec


def test_degenerate_sets_are_what_they_claim(pt):
    # poles: the NaN tangent, on both poles, from outside and inside, -0 velocities included
    o, v, rec = traced(pt, "sphere-poles")
    pole = rec["packed_tangent"] == es.POLE_TANGENT
    assert pole.sum() >= 20 and (pole & (rec["v"] == 1.0)).any() and (pole & (rec["v"] == 0.0)).any()
    near = (rec["shape_material"] != NONE) & ~pole & ((rec["v"] > 0.999) | (rec["v"] < 0.001))
    assert near.sum() >= 5          # next to a pole: a tangent from a tiny cross product
    # cube: corners (both UV coordinates 0 or 1; the rays in two face planes at once miss), edges (one),
    # the face's inside
    o, v, rec = traced(pt, "cube-edges")
    hit = rec["shape_material"] != NONE
    end_u, end_v = np.isin(rec["u"], (0.0, 1.0)), np.isin(rec["v"], (0.0, 1.0))
    assert (hit & end_u & end_v).sum() >= 8 and (hit & (end_u ^ end_v)).sum() >= 16 and (hit & ~end_u & ~end_v).sum() >= 16
    assert (~hit).sum() >= 16       # just outside the edges
    # mesh normals: the cancelled sum answers +Z (SafeNormalize), its neighbours -Z or +Z by a hair;
    # both branches of ComputeTangentVector on the sweeps
    o, v, rec = traced(pt, "mesh-normals")
    hit = rec["shape_material"] != NONE
    up = kat.pack_unit_vector(np.float32([[0, 0, 1]]))[0]
    down = kat.pack_unit_vector(np.float32([[0, 0, -1]]))[0]
    face0 = hit & (o[:, 0] <= 1.0) & (o[:, 0] >= 0.0) & (o[:, 1] >= 0.0) & (o[:, 1] <= 1.0)
    cancelled = face0 & (o[:, 0] == 0.5) & (o[:, 1] < 0.5)
    assert cancelled.sum() >= 4 and (rec["packed_normal"][cancelled] == up).all()
    assert (rec["packed_normal"][face0] == down).any()
    for k in (2, 3, 4):
        face = hit & (np.abs(o[:, 2]) == 2.0) & (o[:, 0] >= 2.0 * k) & (o[:, 0] <= 2.0 * k + 1.0)   # the axial rays
        n = kat.unpack_unit_vector(rec["packed_normal"][face])
        t = kat.unpack_unit_vector(rec["packed_tangent"][face])
        x_branch = np.abs(t[:, 0]) < 1e-3        # cross((1,0,0), N) has no x; cross((0,1,0), N) has no y
        y_branch = np.abs(t[:, 1]) < 1e-3
        assert (np.abs(n[:, 0]) >= 0.9)[y_branch & ~x_branch].all()
        if k == 2:      # cross((0,1,0), (1,0,0)) = (0,0,-1)
            assert y_branch.all() and (np.abs(t[:, 2]) > 0.999).all() and face.sum() >= 4
        else:
            assert (x_branch & ~y_branch).sum() >= 10 and (y_branch & ~x_branch).sum() >= 10
    # plane: fract() gives 0 at whole numbers and rounds to 1 just below them
    o, v, rec = traced(pt, "plane-coordinates")
    hit = rec["shape_material"] != NONE
    assert (hit & (rec["u"] == 0.0)).sum() >= 20 and (hit & (rec["u"] == 1.0)).sum() >= 20
    assert (hit & (np.abs(o[:, 0]) >= 1e6)).sum() >= 20 and (hit & (o[:, 0] < 0)).sum() >= 20


# --- material parameter edges ------------------------------------------------------

MATERIAL_CASES = [(name, flags) for name in sorted(es.MATERIALS) for flags in es.MATERIALS[name].flags]


@pytest.mark.parametrize("name,flags", MATERIAL_CASES)
def test_material_scene_matches_independent_restatement(pt, name, flags):
    """Every slot field and the accumulator, and the restatement took the
    branches the scene is named for."""
    case = es.MATERIALS[name]
    s = case.build(pt)
    w, h = es.frame_size(case, W, H)
    with np.errstate(all="ignore"):
        oa = check_path(s, w, h, SCHEDULE, flags, case.ptp, openpbr=case.openpbr)
    for branch in case.branches:
        assert pr.STATS[branch] >= 1, (branch, sorted(pr.STATS.items()))
    assert np.mean(~np.isfinite(oa).all(-1)) <= NONFINITE_CAP
    s.close()


def oracle_rounds(s, case, w, h, flags):
    """The oracle's state after every Run of the schedule, and its accumulator."""
    o = oracle_lib.OracleRenderer(s.packs(), w, h)
    o.set_openpbr(case.openpbr)
    o.RenderFlags = flags
    o.PathTerminationProbability = case.ptp
    o.reset()
    states = []
    for r in SCHEDULE + [1, 1, 1]:
        o.run(r)
        states.append(o.state())
    acc = o.accum()
    o.close()
    return states, acc


def active_entries(st):
    return np.stack([st["active01"] & 0xFFFF, st["active01"] >> 16, st["active23"] & 0xFFFF, st["active23"] >> 16], -1)


@pytest.mark.parametrize("name", sorted(es.MATERIALS))
def test_material_scenes_are_what_they_claim(pt, name):
    """From the oracle alone, at the device tests' 32x24 over 8 rounds: at
    most a quarter of the accumulator is non-finite; the shells hold slots
    with all four active entries set, the overlapping lenses slots whose
    entry 0 is empty while another is held; the lit pole's centre slot
    carries the NaN tangent; roulette at probability 1 completes a path per
    slot and round."""
    case = es.MATERIALS[name]
    s = case.build(pt)
    w, h = es.frame_size(case, 32, 24)
    states, acc = oracle_rounds(s, case, w, h, case.flags[0])
    assert np.mean(~np.isfinite(acc).all(-1)) <= NONFINITE_CAP
    assert acc[..., 3].sum() > 0
    # nothing non-finite is stored (such paths end inside their round), so the
    # device tests' raw-bit comparison meets no NaN payloads
    for st in states:
        assert all(np.isfinite(st[f]).all() for f in ("origin", "lambda0", "throughput", "probability", "sample"))
    entries = [active_entries(st) for st in states]
    if name == "shells":
        assert sum(int((a != 0xFFFF).all(-1).sum()) for a in entries) >= 100
    if name == "overlap":
        assert sum(int(((a[..., 0] == 0xFFFF) & (a[..., 1:] != 0xFFFF).any(-1)).sum()) for a in entries) >= 10
    if name == "lit-pole":
        o = oracle_lib.OracleRenderer(s.packs(), w, h)
        o.RenderFlags = case.flags[0]
        o.reset()
        o.run(1)
        first = o.state()["hit"]
        o.close()
        assert first["packed_tangent"][h // 2, w // 2] == es.POLE_TANGENT
        assert (first["packed_tangent"] == es.POLE_TANGENT).sum() == 1
    if name == "termination-one":
        hits = sum(int((st["hit"]["shape_material"] != NONE).sum()) for st in states[:-1])
        assert hits > 0 and acc[..., 3].sum() >= w * h * (len(states) - 1)
    s.close()
