"""The restated guides through mirrors and smooth glass (DESIGN.md §6 row 13;
tests/specular_guides_restatement.py) held against what can be known without
a device: the primary-hit guides at zero bounces, the analytic image of a
planar mirror, a parallel slab's unchanged direction, total internal
reflection, and the bounce cap.  The GPU suite holds the kernel against this
restatement bit for bit (tests/test_gpu_specular_guides.py)."""
from __future__ import annotations

import numpy as np
import pytest

import denoise_restatement as dr
import kat
import specular_guides_cases as sc
import specular_guides_restatement as sg

F = np.float32
NONE = 0xFFFFFFFF
# The packed unit vector's quantisation (kat.pack_unit_vector): the two
# octahedral coordinates are rounded to multiples of 1 / 32767, so each moves
# by at most 1 / 65534.  The vector they decode to before normalisation,
# (px, py, 1 - |px| - |py|), then moves by at most
# sqrt(e^2 + e^2 + (2 e)^2) = sqrt(6) / 65534, and its length is at least
# 1 / sqrt(3) (its L1 norm is 1), so the direction turns by at most
PACK_ANGLE = np.sqrt(6.0) / 65534.0 * np.sqrt(3.0)        # 6.5e-5 rad


def primary_rays(scene, W, H):
    cam = scene.arrays()["cameras"][0]
    rays = [dr.central_ray(cam, x, y, W, H) for y in range(H) for x in range(W)]
    O = np.array([r[0] for r in rays], np.float64).reshape(H, W, 3)
    V = kat.unpack_unit_vector(np.array([r[1] for r in rays], np.uint32)).astype(np.float64).reshape(H, W, 3)
    return O, V


@pytest.mark.parametrize("config,camera,W,H", [(2, 0, 32, 32), (5, 0, 32, 16), (5, 1, 32, 16)],
                         ids=["c2", "c5-thin-lens", "c5-360"])
def test_zero_bounces_are_the_primary_guides(pt, config, camera, W, H):
    scene = pt.Scene.config(config)
    assert sg.guides(scene, camera, W, H, 0).tobytes() == dr.guides(scene, camera, W, H).tobytes()
    scene.close()


def test_planar_mirror_shows_the_image_at_its_distance(pt):
    """A sphere behind the camera seen in a planar mirror: time is the
    distance to the sphere's mirror image along the primary ray.

    Tolerance.  The mirror's normal and tangent are axis vectors, which the
    packed form holds exactly, so W is V's mirror image up to float rounding.
    (1) The second ray starts 1e-3 along W past the mirror, so the summed
    time is short of the distance by 1e-3 (W's length is 1 within 1e-6).
    (2) The second ray's direction is W after its packed round trip, off by
    at most PACK_ANGLE; over a second segment of length L the hit moves
    sideways by L * PACK_ANGLE, which changes the hit time by that times
    tan(i), i the angle of incidence on the sphere, to first order; the
    second-order term L^2 PACK_ANGLE^2 / (2 r cos^3 i) is below 2e-6 for
    cos i >= 0.5, the pixels compared.  (3) Float rounding: two times below 16
    and their sum, each within an ulp(16) = 1.9e-6, and the oracle's own
    intersection arithmetic of the same order.  So
    |time - (distance - 1e-3)| <= 1.1 L PACK_ANGLE tan(i) + 2e-5."""
    W = H = 32
    scene, mirror, ball = sc.planar_mirror(pt)
    g = sg.guides(scene, 0, W, H, 1)
    O, V = primary_rays(scene, W, H)
    scene.close()
    shown = (g["shape"] != NONE) & ((g["shape"] & 0xFFFF) == ball)
    assert shown.sum() >= 60
    assert np.all(g["shape"][shown] >> 16 == mirror + 1)
    centre = np.array(sc.SPHERE_CENTRE)
    image = np.array([centre[0], 2.0 * sc.MIRROR_Y - centre[1], centre[2]])
    oc = O - image
    bq = (oc * V).sum(-1)
    disc = bq * bq - ((oc * oc).sum(-1) - sc.SPHERE_RADIUS ** 2)
    compared = 0
    for y, x in np.argwhere(shown):
        assert disc[y, x] > 0
        d = -bq[y, x] - np.sqrt(disc[y, x])
        n = (O[y, x] + d * V[y, x] - image) / sc.SPHERE_RADIUS
        cos_i = -(n * V[y, x]).sum()
        if cos_i < 0.5:
            continue
        L = d - sc.MIRROR_Y / V[y, x, 1]
        tol = 1.1 * L * PACK_ANGLE * np.sqrt(1.0 - cos_i ** 2) / cos_i + 2e-5
        assert abs(float(g["time"][y, x]) - (d - 1e-3)) <= tol, (x, y, g["time"][y, x], d, tol)
        compared += 1
    assert compared >= 40


def test_glass_slab_keeps_the_direction(pt):
    """Two parallel faces: the ray leaves as it entered.

    Tolerance.  The faces' normals and tangents are axis vectors, exact in the
    packed form.  The direction inside the glass is off by at most PACK_ANGLE
    after its round trip; the second refraction turns an error d inside into
    at most (eta cos(ti) / cos(to)) d in the plane of incidence and eta d
    across it, ti and to the angles inside and outside, and
    eta cos(ti) / cos(to) >= eta cos(ti) >= eta sqrt(1 - 1 / eta^2) > 1 is the
    larger; the exit direction then takes a round trip of its own.  Float
    rounding of the two refractions is a few 1e-7."""
    W = H = 32
    scene, slab, wall = sc.glass_slab(pt)
    trace = {}
    g = sg.guides(scene, 0, W, H, 8, trace)
    _, V = primary_rays(scene, W, H)
    scene.close()
    assert np.all(trace["refracted"] == 2) and np.all(trace["reflected"] == 0)
    assert np.all(g["shape"] == ((slab + 1) << 16 | wall))
    out = kat.unpack_unit_vector(trace["packed_velocity"].reshape(-1)).astype(np.float64).reshape(H, W, 3)
    cos_o = V[..., 1]                                        # the faces' normal is the y axis
    cos_i = np.sqrt(1.0 - (1.0 - cos_o ** 2) / sc.SLAB_IOR ** 2)
    bound = (sc.SLAB_IOR * cos_i / cos_o + 1.0) * PACK_ANGLE + 1e-6
    angle = np.linalg.norm(np.cross(out, V), axis=-1)
    assert np.all(angle <= bound), (angle.max(), bound.min())
    assert angle.max() > 0                                   # quantised, not copied
    # The 0.6 of glass is crossed closer to the normal than the straight ray would cross it: the
    # summed time is the straight ray's less 0.6 (1 / cos(to) - 1 / cos(ti)) < 0.6 / cos(to), and less
    # the two restart offsets.
    straight = (8.0 - 0.2) / cos_o
    assert np.all(g["time"] < straight + 1e-4) and np.all(g["time"] > straight - 0.6 / cos_o - 2e-3 - 1e-4)


def test_total_internal_reflection_takes_the_mirror_branch(pt):
    """Inside glass of index 1.5 the critical angle has sin = 1 / 1.5."""
    n, tx = [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]
    for sin_i, refracts in ((0.60, True), (0.66, True), (0.67, False), (0.95, False)):
        v = [sin_i, 0.0, np.sqrt(1.0 - sin_i ** 2)]           # leaving: along the normal
        w, refracted = sg.direction([True], [F(1.5)], [n], [tx], [v])
        assert bool(refracted[0]) == refracts
        if refracts:
            assert abs(w[0, 0] - 1.5 * sin_i) < 1e-6 and w[0, 2] > 0
        else:
            assert np.allclose(w[0], [v[0], 0.0, -v[2]], atol=1e-7)
    # a camera at the centre of a glass cube: the face met is the axis of V's largest
    # component, whose size is the cosine of incidence
    W, H = 32, 16
    scene, box = sc.glass_box(pt)
    trace = {}
    g = sg.guides(scene, 0, W, H, 1, trace)
    _, V = primary_rays(scene, W, H)
    scene.close()
    cos_i = np.abs(V).max(-1)
    critical = np.sqrt(1.0 - 1.0 / sc.SLAB_IOR ** 2)
    beyond, within = cos_i < critical - 1e-3, cos_i > critical + 1e-3
    assert beyond.sum() > 20 and within.sum() > 20
    assert np.all(trace["reflected"][beyond] == 1) and np.all(trace["refracted"][beyond] == 0)
    assert np.all(trace["refracted"][within] == 1) and np.all(trace["reflected"][within] == 0)
    assert np.all(g["shape"][beyond] == ((box + 1) << 16 | box))      # the cap ends the chain on the cube
    assert np.all(g["shape"][within] == NONE)                         # out into the sky: no tag on a miss


def test_cap_ends_the_chain_on_a_mirror(pt):
    W = H = 8
    scene, mirrors = sc.facing_mirrors(pt)
    previous = np.zeros((H, W), F)
    for cap in range(1, sg.MAX_BOUNCES + 1):
        trace = {}
        g = sg.guides(scene, 0, W, H, cap, trace)
        assert np.all(trace["bounces"] == cap)
        # the first mirror hit is mirrors[0]; they alternate, and hit cap + 1 is recorded
        assert np.all(g["shape"] == ((mirrors[0] + 1) << 16 | mirrors[cap % 2]))
        assert np.all(g["time"] > previous + 6.9)             # one more crossing of the 7 between the faces
        previous = g["time"].copy()
    scene.close()


def test_every_material_type_and_a_textured_roughness(pt, tmp_path):
    """The crafted scene of the GPU test shows each feature it is there for."""
    scene, idx = sc.crafted(pt, tmp_path)
    g, trace = sc.reference("crafted", scene, 0, 64, 32, 8)
    scene.close()
    hit = g["shape"] != NONE
    tag, shape = g["shape"] >> 16, g["shape"] & 0xFFFF
    for name in ("mirror_a", "mirror_b", "slab", "spotty", "mesh_mirror"):
        assert (hit & (tag == idx[name] + 1)).sum() >= 10, name          # chains start on each of them
    spotty = hit & (shape == idx["spotty"])
    assert (spotty & (tag == 0)).sum() >= 5                              # rough texels: seen as a surface
    assert (hit & (tag == idx["spotty"] + 1)).sum() >= 5                 # smooth texels: followed
    assert (hit & (tag == idx["slab"] + 1) & (shape == idx["wall"])).sum() >= 20
    assert (hit & (tag > 0) & (shape == idx["ball"])).any()              # the sphere between the mirrors, reflected
    assert (hit & (tag > 0) & (shape > idx["mesh_mirror"])).any()        # a bounced ray ends inside the model's BLAS
    assert trace["bounces"].max() >= 3 and trace["refracted"].sum() > 0 and trace["reflected"].sum() > 0
