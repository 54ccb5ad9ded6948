"""Scenes shared by the specular-guide tests (tests/test_specular_guides.py on
the CPU, tests/test_gpu_specular_guides.py on the device), and the restated
guides of a scene, computed once per process and left unchanged."""
from __future__ import annotations

import ctypes as C

import numpy as np

import specular_guides_restatement as sg

F = np.float32
HALF_PI = 1.5707963267948966
_REFERENCES = {}


def reference(key, scene, camera, W, H, bounces):
    """(records, trace) of sg.guides, cached under `key` (which names the scene)."""
    k = (key, camera, W, H, bounces)
    if k not in _REFERENCES:
        trace = {}
        g = sg.guides(scene, camera, W, H, bounces, trace)
        for a in (g, *trace.values()):
            a.setflags(write=False)
        _REFERENCES[k] = (g, trace)
    return _REFERENCES[k]


def _camera(pt, s, position=(0.0, 0.0, 0.0), fov=60.0, panorama=False):
    """At `position`, looking along +y."""
    cam = s.create_entity(pt.ENTITY_CAMERA, position=position, rotation=(HALF_PI, 0.0, 0.0))
    if panorama:
        s.set_camera_360(cam)
    else:
        s.set_camera_pinhole(cam, fov_degrees=fov)
    return cam


def mirror_material(pt, s, name="Mirror"):
    return s.create_material(pt.MATERIAL_BASIC_METAL, name, BaseColor=(0.9, 0.9, 0.95), SpecularColor=(1.0, 1.0, 1.0),
                             Roughness=0.0)


def glass_material(pt, s, ior, name="Glass"):
    return s.create_material(pt.MATERIAL_BASIC_TRANSLUCENT, name, IOR=ior, AbbeNumber=40.0, Roughness=0.0,
                             TransmissionColor=(0.9, 0.95, 1.0), TransmissionDepth=10.0)


# The planar mirror: its face towards the camera is the plane y = MIRROR_Y, and
# the sphere sits behind the camera.
MIRROR_Y = 3.5
SPHERE_CENTRE = (0.5, -3.0, 0.3)
SPHERE_RADIUS = 1.5


def planar_mirror(pt):
    """(scene, mirror's shape index, sphere's shape index)."""
    s = pt.Scene.empty()
    red = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Red", BaseColor=(0.8, 0.2, 0.2))
    m = s.create_entity(pt.ENTITY_CUBE, position=(0.0, MIRROR_Y + 0.5, 0.0), scale=(3.0, 0.5, 3.0),
                        material=mirror_material(pt, s))
    b = s.create_entity(pt.ENTITY_SPHERE, position=SPHERE_CENTRE, scale=(SPHERE_RADIUS,) * 3, material=red)
    _camera(pt, s)
    s.pack()
    return s, s.shape_index(m), s.shape_index(b)


SLAB_IOR = 1.5


def glass_slab(pt):
    """(scene, slab's shape index, wall's shape index): a slab with faces
    y = 2.7 and y = 3.3 in front of a diffuse wall."""
    s = pt.Scene.empty()
    grey = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Grey", BaseColor=(0.6, 0.6, 0.6))
    g = s.create_entity(pt.ENTITY_CUBE, position=(0.0, 3.0, 0.0), scale=(4.0, 0.3, 4.0),
                        material=glass_material(pt, s, SLAB_IOR))
    w = s.create_entity(pt.ENTITY_CUBE, position=(0.0, 8.0, 0.0), scale=(12.0, 0.2, 12.0), material=grey)
    _camera(pt, s)
    s.pack()
    return s, s.shape_index(g), s.shape_index(w)


def glass_box(pt):
    """(scene, box's shape index): a 360 camera at the centre of an
    axis-aligned glass cube, so every primary hit meets a face from inside."""
    s = pt.Scene.empty()
    g = s.create_entity(pt.ENTITY_CUBE, position=(0.0, 0.0, 0.0), scale=(2.0, 2.0, 2.0),
                        material=glass_material(pt, s, SLAB_IOR))
    _camera(pt, s, panorama=True)
    s.pack()
    return s, s.shape_index(g)


def facing_mirrors(pt):
    """(scene, the two mirrors' shape indices): faces y = 3.5 and y = -3.5
    around the camera, 16 x 16 each.  A ray of the 10-degree camera leaves
    the axis by at most tan(5 deg) sqrt(2) = 0.124 per unit of y, and nine
    segments cover 3.5 + 8 * 7 = 59.5 of y: 7.4 < 8, so every pixel is still
    between the mirrors after 8 bounces."""
    s = pt.Scene.empty()
    mat = mirror_material(pt, s)
    a = s.create_entity(pt.ENTITY_CUBE, position=(0.0, 4.0, 0.0), scale=(8.0, 0.5, 8.0), material=mat)
    b = s.create_entity(pt.ENTITY_CUBE, position=(0.0, -4.0, 0.0), scale=(8.0, 0.5, 8.0), material=mat)
    _camera(pt, s, fov=10.0)
    s.pack()
    return s, (s.shape_index(a), s.shape_index(b))


def crafted(pt, tmp_path):
    """(scene, names -> shape index) seen by a 360 camera at the origin: two
    facing mirror cubes (+y, -y) with a diffuse sphere between them; a glass
    slab in front of a checkered diffuse wall (+x); a metal sphere whose
    RoughnessTexture has texels on both sides of 1e-3 (-x); a mirror mesh
    instance overhead (+z), so a chain starts on a BLAS hit; the imported
    model's own instances, which bounced rays pass through; a checkered floor."""
    from test_ingestion import write_model
    N = pt._native
    s = pt.Scene.empty()
    checker = s.create_checker_texture("Checker", pt.TEXTURE_REFLECTANCE_WITH_ALPHA,
                                       (0.9, 0.9, 0.9, 1.0), (0.2, 0.3, 0.7, 1.0))
    rough = np.zeros((2, 2, 4), F)
    rough[..., 0] = [[0.0, 0.5], [5e-4, 2e-3]]
    rough[..., 3] = 1.0
    rough_tex = s.create_texture("Rough", pt.TEXTURE_RAW, rough, nearest=True)
    floor = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Floor", BaseColor=(0.8, 0.7, 0.6))
    s.set_material_parameter(floor, "BaseTexture", checker)
    wall = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Wall", BaseColor=(0.9, 0.8, 0.5))
    s.set_material_parameter(wall, "BaseTexture", checker)
    green = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Green", BaseColor=(0.2, 0.7, 0.3))
    mirror = mirror_material(pt, s)
    spotty = s.create_material(pt.MATERIAL_BASIC_METAL, "Spotty", BaseColor=(0.7, 0.4, 0.4),
                               SpecularColor=(0.9, 0.9, 0.9), Roughness=1.0)
    s.set_material_parameter(spotty, "RoughnessTexture", rough_tex)
    e = {}
    e["floor"] = s.create_entity(pt.ENTITY_PLANE, position=(0.0, 0.0, -2.0), material=floor)
    e["mirror_a"] = s.create_entity(pt.ENTITY_CUBE, position=(0.0, 4.0, 0.0), scale=(2.0, 0.2, 1.5), material=mirror)
    e["mirror_b"] = s.create_entity(pt.ENTITY_CUBE, position=(0.0, -4.0, 0.0), scale=(2.0, 0.2, 1.5), material=mirror)
    e["ball"] = s.create_entity(pt.ENTITY_SPHERE, position=(0.8, 2.0, 0.3), scale=(0.5, 0.5, 0.5), material=green)
    e["slab"] = s.create_entity(pt.ENTITY_CUBE, position=(3.0, 0.0, 0.0), scale=(0.2, 1.5, 1.5),
                                material=glass_material(pt, s, SLAB_IOR))
    e["wall"] = s.create_entity(pt.ENTITY_CUBE, position=(6.0, 0.0, 0.0), scale=(0.2, 3.0, 3.0), material=wall)
    e["spotty"] = s.create_entity(pt.ENTITY_SPHERE, position=(-3.0, 0.0, 0.0), scale=(1.2, 1.2, 1.2), material=spotty)
    prefab = s.load_model_as_prefab(write_model(tmp_path))
    material, position = C.c_void_p(), np.zeros(3, F)
    quad = N.scene_lib().ptsPrefabMesh(prefab, 0, C.byref(material), N.fptr(position))   # "Bottom": a 2 x 2 quad
    e["mesh_mirror"] = s.create_entity(pt.ENTITY_MESH_INSTANCE, position=(0.0, 0.0, 3.0), scale=(1.5, 1.5, 1.5),
                                       material=mirror)
    s.set_mesh(e["mesh_mirror"], quad)
    model = s.instantiate_prefab(prefab)
    s.set_transform(model, position=(1.5, -2.0, -1.0), scale=(0.5, 0.5, 0.5))
    _camera(pt, s, panorama=True)
    s.pack()
    return s, {k: s.shape_index(v) for k, v in e.items()}


def mirrored_chain(pt, tmp_path):
    """test_gpu_denoise.test_guides_with_spilled_stack's scene -- 24 doubling
    spheres, a chain-shaped TLAS deeper than the guide kernel's 20 LDS stack
    entries, and the imported model -- with every second sphere a mirror and
    the camera between sphere 3 (diffuse, behind it) and sphere 4 (a mirror).
    (scene, the spheres' shape indices)."""
    from test_ingestion import write_model
    s = pt.Scene.create()
    mirror = mirror_material(pt, s)
    spheres = []
    for i in range(24):
        spheres.append(s.create_entity(pt.ENTITY_SPHERE, position=(3.0 * 2.0 ** i, 0.0, 1.0), scale=(0.5 * 2.0 ** i,) * 3,
                                       material=mirror if i % 2 == 0 else None))
    s.instantiate_prefab(s.load_model_as_prefab(write_model(tmp_path)))
    s.pack()
    cam = s.find_camera(0)
    s.set_camera_360(cam)
    s.move_camera(cam, position=(32.0, 0.0, 1.0))
    s.pack()
    return s, [s.shape_index(e) for e in spheres]
