"""GPU: the edge-case catalogue (tests/edge_scenes.py) on the device against
the CPU oracle, bit for bit.

The device restates traversal and shading apart from the oracle
(traverse.hpp, shade.hpp, bsdf.hpp, path.hpp) and walks differently: the
mesh-only loop with its joined update on wave masks, the LDS node cache's BVH
relayout, three stack formats, the lean face test.  On untied rays the order
of visits cannot show; here it does.  tests/test_edge_scenes.py holds the
oracle itself to the independent restatements on the same inputs.

  * ptTraceRays on every TIES and DEGENERATE ray set, in extend form AUTO
    (the one-mesh scenes must report the mesh loop) and GENERAL, stack formats
    0, 1 and 2, both hit-record forms; ptOccludedRays against the oracle's
    hit mask.
  * RenderPreview at 72x40 on the tie scenes: image, AOVs and pick.
  * renders of the tie scenes and of every MATERIALS scene at 32x24, schedule
    [2, 1, 1, 1, 1, 1], fused modes 0 and 2, the OpenPBR scenes with OpenPBR
    on; the scenes of several material types once more in three tile groups
    through the class lists.
"""
from __future__ import annotations

import numpy as np
import pytest

import edge_scenes as es
import oracle_lib
from test_gpu_parity import compare_hits, compare_state

pytestmark = pytest.mark.gpu

AUTO, GENERAL, MESH = 0, 1, 2   # PT_EXTEND_FORM_*
NONE = 0xFFFFFFFF
W, H = 32, 24
SCHEDULE = [2, 1, 1, 1, 1, 1]


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_cache = {}


def ray_case(pt, name):
    """(scene, rays, the oracle's records): built and traced once per name."""
    if name not in _cache:
        if name in es.TIES:
            s = es.TIES[name].build(pt)
            rays = es.tie_rays(s, es.TIES[name])
        else:
            s = es.DEGENERATE[name].build(pt)
            rays = es.DEGENERATE[name].rays(s)
        _cache[name] = (s, rays, oracle_lib.trace_rays(s.packs(), *rays))
    return _cache[name]


def one_mesh(scene):
    return scene.arrays()["shapes"]["Type"].tolist() == [0]


@pytest.mark.parametrize("name", sorted(es.TIES) + sorted(es.DEGENERATE))
def test_trace_rays_bit_exact(pt, dev, name):
    s, (o, v, d), ref = ray_case(pt, name)
    assert one_mesh(s) == (name in ("double-mesh", "mesh-normals"))
    for form in (AUTO, GENERAL):
        for fmt in (0, 1, 2):
            for record in (0, 1):
                ds = pt.DeviceScene(dev)
                ds.set_extend_form(form)
                ds.set_stack_format(fmt)
                ds.set_hit_record_form(record)
                ds.update(s)
                assert ds.extend_form == (MESH if form == AUTO and one_mesh(s) else GENERAL)
                try:
                    compare_hits(ds.trace_rays(o, v, d), ref)
                except AssertionError as e:
                    raise AssertionError(f"extend form {form}, stack format {fmt}, hit record {record}: {e}") from None
                ds.close()


@pytest.mark.parametrize("name", sorted(es.TIES) + sorted(es.DEGENERATE))
def test_occluded_equals_oracle_hit_mask(pt, dev, name):
    """The any-hit query stops at the first hit inside Duration: a cube
    exactly at Duration is no hit (T >= Hit.Time), a face, plane or sphere
    there is one unless its box was entered at exactly that time."""
    s, (o, v, d), ref = ray_case(pt, name)
    want = ref["shape_material"] != NONE
    for form in (AUTO, GENERAL):
        ds = pt.DeviceScene(dev)
        ds.set_extend_form(form)
        ds.update(s)
        got = ds.occluded(o, v, d)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"extend form {form}: {bad.size} rays differ, first {bad[:8].tolist()}"
        ds.close()


@pytest.mark.parametrize("name", sorted(es.TIES))
def test_preview_bit_exact(pt, dev, name):
    s, _, _ = ray_case(pt, name)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    cam = s.arrays()["cameras"][0]["Transform"]["To"]
    ctx = pt.PreviewRenderContext(dev, ds)
    for mode in range(7):
        p = pt.PreviewParameters(cam, RenderMode=mode, RenderSizeX=72, RenderSizeY=40, Brightness=1.5,
                                 SelectedShapeIndex=0, MouseX=36, MouseY=24)
        ctx.render(p)
        img, aov, q = ctx.image(), ctx.aovs(), ctx.query()
        ref_img, ref_aov, ref_q = oracle_lib.preview(s.packs(), p)
        same = (bits(img) == bits(ref_img)) | (np.isnan(img) & np.isnan(ref_img))
        assert same.all(), (mode, np.argwhere(~same)[:5].tolist())
        assert np.array_equal(aov.view(np.uint8), ref_aov.view(np.uint8)), mode
        assert q == ref_q, mode
    ctx.close()
    ds.close()


def render_both(pt, dev, s, w, h, flags=3, ptp=0.0, openpbr=False, fused=None, groups=None):
    """Reset + SCHEDULE on the device and in the oracle: (device state, oracle
    state, device accumulator, oracle accumulator).  groups: the Run(1)
    rounds as one run of consecutive rounds in that many tile groups, shaded
    through the class lists (asserted; the shade instantiation with OpenPBR
    has no class-list form, so those scenes keep the tile-local shade in
    their groups, asserted too)."""
    ds = pt.DeviceScene(dev)
    ds.update(s)
    sb = pt.SampleBuffer(dev, w, h)
    r = pt.BasicRenderer(dev, ds, sb)
    o = oracle_lib.OracleRenderer(s.packs(), w, h)
    r.set_openpbr(openpbr)
    o.set_openpbr(openpbr)
    if fused is not None:
        r.set_fused_rounds(fused)
    if groups is not None:
        r.set_fused_rounds(0)
        r.set_split(groups)
        assert r.split()["groups"] == groups and r.class_lists() == (not openpbr)
    for x in (r, o):
        x.RenderFlags = flags
        x.PathTerminationProbability = ptp
        x.reset()
    for rounds in SCHEDULE:
        o.run(rounds)
    if groups is None:
        for rounds in SCHEDULE:
            r.run(rounds)
    else:
        r.run(SCHEDULE[0])
        r.run_rounds(len(SCHEDULE) - 1)
    dev.synchronize()
    out = (r.read_state(), o.state(), sb.read(), o.accum())
    o.close()
    for x in (r, sb, ds):
        x.close()
    return out


def check_render(out):
    gs, os_, ga, oa = out
    compare_state(gs, os_)
    bad = np.argwhere(bits(ga) != bits(oa))
    assert bad.size == 0, f"accumulator differs at {bad[:4].tolist()}"
    assert oa[..., 3].sum() > 0


@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name", sorted(es.TIES))
def test_tie_scene_render_bit_exact(pt, dev, name, fused):
    s, _, _ = ray_case(pt, name)
    check_render(render_both(pt, dev, s, W, H, fused=fused))


MATERIAL_CASES = [(name, flags) for name in sorted(es.MATERIALS) for flags in es.MATERIALS[name].flags]


@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name,flags", MATERIAL_CASES)
def test_material_scene_render_bit_exact(pt, dev, name, flags, fused):
    case = es.MATERIALS[name]
    s = case.build(pt)
    w, h = es.frame_size(case, W, H)
    check_render(render_both(pt, dev, s, w, h, flags=flags, ptp=case.ptp, openpbr=case.openpbr, fused=fused))
    s.close()


# one material type: no class lists to take
SINGLE_TYPE = ("double-mesh", "black-sky")


@pytest.mark.parametrize("name", [n for n in sorted(es.TIES) + sorted(es.MATERIALS) if n not in SINGLE_TYPE])
def test_render_in_tile_groups_through_class_lists(pt, dev, name):
    if name in es.TIES:
        s, case = ray_case(pt, name)[0], None
        args = dict(w=W, h=H)
    else:
        case = es.MATERIALS[name]
        s = case.build(pt)
        w, h = es.frame_size(case, W, H)
        args = dict(w=w, h=h, flags=case.flags[0], ptp=case.ptp, openpbr=case.openpbr)
    assert len(es.material_types(s)) > 1
    check_render(render_both(pt, dev, s, groups=3, **args))
    if case is not None:
        s.close()


def test_single_type_scenes_are_single_type(pt):
    for name in SINGLE_TYPE:
        s = (es.TIES[name] if name in es.TIES else es.MATERIALS[name]).build(pt)
        assert len(es.material_types(s)) == 1
        s.close()
