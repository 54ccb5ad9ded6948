"""GPU: the exact fast slab division at the edges of its proven domain.

Every box test of every traversal takes its six quotients (Min - O) / V from
FastQuot (pt_device.hpp), an FMA-corrected reciprocal with no guard of its
own, whenever two gates hold: the scene's (rt_scene.hip FastDivBoxes, once per
upload: every box coordinate 0 or in [2^-50, 2^40]) and the ray's
(pt_device.hpp FastDivRay, per ray and traversal level in SetLevelRay: every
origin component in that set, every velocity component in [2^-59, 2^27]).
Bit parity with the oracle rests on the quotients being IEEE's inside those
gates and on the gates refusing everything else.

* ptEvalSlabTest runs SetLevelRay and IntersectBoxPair as the traversal calls
  them over the case sets of slab_cases.py (1.8 M rays and boxes: the domain's
  bulk, its edges, near-cancelling origins, operands outside it, reaches that
  tie) against a numpy IEEE restatement of the test, bit for bit, and the
  ray's flag against the domain as DESIGN.md §2 states it.
* Scenes put the gates' boundaries into whole traversals (ptTraceRays,
  ptOccludedRays and short renders against the oracle): mesh-space velocities
  on both sides of 2^27 within a wave, box coordinates at 0, 2^-50 and 2^40 and
  one ulp outside, and one device scene updated across the scene gate.  Each
  asserts the branch it ran (DeviceScene.fast_division).

The ray gate's lower velocity bound is left to the probe: a mesh-space
velocity near 2^-59 needs an instance scale so large that the reference's
|Det| < 1e-9 test rejects every face, so no box decision made there can reach
a hit record.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle_lib
import slab_cases as sc
import slab_scenes as ss
from test_gpu_mesh_extend import AUTO, GENERAL, MESH, bits, gpu_render, oracle_render, upload
from test_gpu_parity import compare_hits, compare_state

pytestmark = pytest.mark.gpu

W, H = 32, 24


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


# --- the probe ---------------------------------------------------------------------

def report(name, gate, ok, ref, got_bits, c):
    bad = np.flatnonzero(~ok)
    print(f"{name} gate {gate}: {len(bad)} of {len(ok)} entry times differ")
    for i in bad[:5]:
        print(f"  case {i}: o {c['o'][i]} v {c['v'][i]} reach {c['reach'][i]} box {c['lo'][i]} {c['hi'][i]}"
              f" -> {sc.from_bits(got_bits[i:i + 1])[0]!r} ({int(got_bits[i]):08x}), IEEE {ref[i]!r}"
              f" ({int(sc.bits(ref[i:i + 1])[0]):08x})")
    return len(bad)


@pytest.mark.parametrize("name", sc.CLASSES)
def test_slab_probe_matches_ieee(dev, name):
    """The ray's flag equals the domain's statement under scene gate 1 and is
    0 under gate 0, and the entry time equals the IEEE reference bit for bit.
    Two exceptions, both stated by the convention: two zeros of either sign
    are equal (a zero numerator may give the other zero, and every consumer of
    the value compares), and two NaNs are equal.

    Every case is compared under gate 0.  Gate 1 is the upload's promise that
    the boxes lie in the coordinate range, so under gate 1 the entry times are
    compared for every case whose box keeps that promise or whose ray is
    refused anyway; the flag is compared for all."""
    c = sc.cases(name)
    ref, flag, box = sc.expected(name)
    args = (c["o"], c["v"], c["reach"], c["lo"], c["hi"])

    e0, x0 = dev.eval_slab_test(*args, scene_gate=0)
    e1, x1 = dev.eval_slab_test(*args, scene_gate=1)
    wrong_flag = np.flatnonzero((x1 != 0) != flag)
    print(f"{name}: {len(ref)} cases, flag 1 expected for {int(flag.sum())}, got {int((x1 != 0).sum())};"
          f" {len(wrong_flag)} flags differ; boxes in range {int(box.sum())}")
    for i in wrong_flag[:5]:
        print(f"  case {i}: o {c['o'][i]} v {c['v'][i]} flag {int(x1[i])}, expected {int(flag[i])}")
    ok0 = sc.same_entry(e0, ref)
    ok1 = sc.same_entry(e1, ref)
    held = box | ~flag
    n0 = report(name, 0, ok0, ref, e0, c)
    n1 = report(name, 1, ok1 | ~held, ref, e1, c)
    print(f"{name}: under gate 1 compared {int(held.sum())}, fast path {int((held & flag).sum())}")

    assert not x0.any(), "flag set under scene gate 0"
    assert set(np.unique(x1).tolist()) <= {0, 1}
    assert len(wrong_flag) == 0
    assert n0 == 0 and n1 == 0
    if name in sc.IN_DOMAIN:
        assert (held & flag).sum() >= len(ref) // 4     # the fast path itself was compared


def test_slab_probe_arguments(pt, dev):
    N = pt._native
    L = N.hip_lib()
    f3, f1 = np.ones((4, 3), np.float32), np.ones(4, np.float32)
    out = np.zeros(4, np.uint32)
    good = [N.fptr(f3), N.fptr(f3), N.fptr(f1), N.fptr(f3), N.fptr(f3)]
    assert L.ptEvalSlabTest(dev.handle, 4, *good, 1, N.u32ptr(out), N.u32ptr(out)) == 0
    assert L.ptEvalSlabTest(None, 4, *good, 1, N.u32ptr(out), N.u32ptr(out)) != 0
    assert L.ptEvalSlabTest(dev.handle, 4, *good, 2, N.u32ptr(out), N.u32ptr(out)) != 0
    for k in range(5):
        bad = list(good)
        bad[k] = None
        assert L.ptEvalSlabTest(dev.handle, 4, *bad, 1, N.u32ptr(out), N.u32ptr(out)) != 0
    assert L.ptEvalSlabTest(dev.handle, 4, *good, 1, None, N.u32ptr(out)) != 0
    assert L.ptEvalSlabTest(dev.handle, 4, *good, 1, N.u32ptr(out), None) != 0
    assert L.ptEvalSlabTest(dev.handle, 0, None, None, None, None, None, 0, None, None) == 0
    # a point-sized box at the ray's point 2: entry 2, in the domain
    o, v = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    p = np.full((1, 3), 2.0, np.float32)
    e, x = dev.eval_slab_test(o, v, [4.0], p, p)
    assert sc.from_bits(e)[0] == 2.0 and x[0] == 1
    with pytest.raises(ValueError):
        dev.eval_slab_test(o, v, [4.0, 4.0], p, p)
    ds = pt.DeviceScene(dev)
    assert ds.fast_division is False            # no packs yet
    assert L.ptSceneFastDivision(None, None) != 0 and L.ptSceneFastDivision(ds.handle, None) != 0
    ds.close()


# --- scenes ------------------------------------------------------------------------------

def check_hits(ds, scene, rays, min_hit_share):
    o, v, d = rays
    ref = oracle_lib.trace_rays(scene.packs(), o, v, d)
    hit = ref["shape_material"] != 0xFFFFFFFF
    assert hit.mean() >= min_hit_share, hit.mean()
    compare_hits(ds.trace_rays(o, v, d), ref)
    assert np.array_equal(ds.occluded(o, v, d), hit)


def check_render(pt, dev, ds, scene, rounds):
    g = gpu_render(pt, dev, ds, W, H, [2] + [1] * rounds)
    os_, oa, oc = oracle_render(scene, W, H, rounds)
    compare_state(g[0], os_)
    assert oa[..., 3].sum() > 0
    assert np.array_equal(bits(g[1]), bits(oa)) and g[2] == oc


@pytest.fixture(scope="module")
def straddle(pt):
    """(scene, rays, shares) of the one- and the two-instance scene, made once."""
    out = {}
    for instances in (1, 2):
        s = ss.straddle_scene(pt, instances)
        rays = ss.special_rays(s, 4096, seed=17)
        out[instances] = (s, rays, ss.straddle_shares(s, rays))
    yield out
    for s, _, _ in out.values():
        s.close()


@pytest.mark.parametrize("kind", ["mesh-only", "general", "two-instances"])
def test_velocity_straddles_the_ray_gate_inside_a_blas(pt, dev, straddle, kind):
    """Mesh-space velocity components on both sides of 2^27 within every wave
    (the blob times 2^27 under an instance scale of 2^-27 (1.3, 0.8, 1.7)), in
    the mesh-only loop, the general loop and a two-instance scene.  From the
    packed From matrix: 83 % of the 4 096 rays pass the ray gate in mesh space
    (required: 10-90 %), 14 % have a velocity component on either side of 2^27,
    70 % (43 % with two instances) hit.  The scene gate is on, so the lanes of
    a wave split between FastQuot and division at the BLAS level."""
    scene, rays, (exact, both, hit) = straddle[2 if kind == "two-instances" else 1]
    print(f"{kind}: mesh-space rays inside the ray gate {exact:.3f}, velocity on both sides of 2^27 {both:.3f}, hits {hit:.3f}")
    assert 0.10 <= exact <= 0.90 and both >= 0.05 and hit >= 0.25
    assert ss.box_gate(scene)
    ds = upload(pt, dev, scene, form=GENERAL if kind == "general" else AUTO)
    assert ds.fast_division is True
    assert ds.extend_form == (MESH if kind == "mesh-only" else GENERAL)
    check_hits(ds, scene, rays, 0.25)
    check_render(pt, dev, ds, scene, 4)
    ds.close()


@pytest.mark.parametrize("name,value,gate", ss.GATE_CASES, ids=[c[0] for c in ss.GATE_CASES])
def test_scene_gate_at_its_bounds(pt, dev, name, value, gate):
    """One vertex coordinate of the (cleaned) blob at 0, 2^-50 and 2^40, where
    the scene gate stays on, and at 2^-60 and one ulp outside either bound,
    where it goes off and every box test of the scene divides.  Hits (closest
    and any) and a short render equal the oracle's bit for bit on both
    branches."""
    scene = ss.edited_blob_scene(pt, value)
    clean = ss.edited_blob_scene(pt)
    rays = ss.special_rays(clean, 4096, seed=17)
    assert ss.box_gate(scene) == gate
    for form, want in ((AUTO, MESH), (GENERAL, GENERAL)):
        ds = upload(pt, dev, scene, form=form)
        assert ds.fast_division is gate and ds.extend_form == want
        check_hits(ds, scene, rays, 0.25)
        if form == AUTO:
            check_render(pt, dev, ds, scene, 2)
        ds.close()
    for x in (scene, clean):
        x.close()


@pytest.mark.parametrize("links,gate", [(56, True), (59, False)])
def test_chain_past_the_coordinate_range(pt, dev, links, gate):
    """The chain mesh of test_gpu_mesh_extend.py (56 links, the largest
    coordinate 3 * 2^37) and the same chain lengthened to 59 links (3 * 2^40,
    beyond the range: the scene gate goes off), each more than 20 levels deep."""
    scene = ss.long_chain_scene(pt, links)
    assert ss.box_gate(scene) == gate
    ds = upload(pt, dev, scene)
    assert ds.fast_division is gate and ds.extend_form == MESH and ds.stack_needed > 20
    check_hits(ds, scene, ss.chain_rays(), 0.125)
    check_render(pt, dev, ds, scene, 2)
    ds.close()
    scene.close()


def test_gate_follows_scene_updates(pt, dev):
    """One device scene updated with a scene inside the coordinate range, one
    outside it and the first again: the flag and the hits follow each upload."""
    on, off = ss.edited_blob_scene(pt), ss.edited_blob_scene(pt, ss.below(2.0 ** -50))
    far = ss.long_chain_scene(pt, 59)
    rays = ss.special_rays(on, 2048, seed=31)
    ds = pt.DeviceScene(dev)
    for scene, gate, r, share in ((on, True, rays, 0.25), (off, False, rays, 0.25), (on, True, rays, 0.25),
                                  (far, False, ss.chain_rays(), 0.125), (on, True, rays, 0.25)):
        ds.update(scene)
        assert ds.fast_division is gate
        check_hits(ds, scene, r, share)
        check_render(pt, dev, ds, scene, 1)
    # an upload that touches nothing but the cameras still re-states the gate
    ds.update(off)
    assert ds.fast_division is False
    ds.update(off, pt.SCENE_DIRTY_CAMERAS)
    assert ds.fast_division is False
    for x in (ds, on, off, far):
        x.close()
