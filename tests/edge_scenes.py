"""Edge-case scenes and ray sets: exact hit ties, degenerate hit attributes and
material parameters at the ends of their ranges (tests/test_edge_scenes.py on
the CPU, tests/test_gpu_edge_scenes.py on the device).

What the configs, the fuzz scenes (tests/fuzz_scenes.py) and the hand-made
meshes never hold: two surfaces at a bit-equal hit time, a hit whose tangent
or normal is 0/0, and a Scatter whose material makes an infinity or a NaN for
a few instructions.  Everything is built through the host scene API from
fixed numbers; only the oblique filler rays come from a (fixed) seed.

Three families, each a dict of name -> case:

TIES         tie scenes; `build(pt, away=None)` makes the scene, `away=k`
             the same scene with tie candidate k moved out of every ray's
             reach (shape and material indices unchanged), which is how
             tests/test_edge_scenes.py shows that a second candidate sat at
             the same time.  Every coordinate is a multiple of 1/8, every tie
             ray axial, so the candidates' hit times are exact and equal.
DEGENERATE   scenes whose rays reach a sphere's poles, a cube's edges,
             corners and faces (from outside, inside and within the face
             plane), mesh faces whose interpolated normal cancels or passes
             |Normal.x| = 0.9, and plane hits whose fract() is 0 or rounds to 1.
MATERIALS    one small scene per parameter edge inside Scatter (a plane, one
             or two spheres, a pinhole camera), the OpenPBR twins, and a
             sphere lit from straight above without jitter.
"""
from __future__ import annotations

import collections

import numpy as np

import oracle_lib

FAR = 1048576.0
FAR_AWAY = 1000.0            # where `away=k` puts a tie candidate
POLE_TANGENT = 0x80018001    # PackUnitVector(normalize(0)): both snorm16 clamp a NaN to -1

Tie = collections.namedtuple("Tie", "build candidates one_mesh mixed x_range")
Degenerate = collections.namedtuple("Degenerate", "build rays")
Material = collections.namedtuple("Material", "build openpbr flags ptp size branches")


# --- meshes ------------------------------------------------------------------------

def grid_mesh(cells=6, step=0.25, copy=0, shift=0.0):
    """A flat grid of cells x cells quads in z = 0, centred, two triangles a
    quad ((a, b, c), (b, d, c): the shared edge is the anti-diagonal).
    copy 1 is the same surface with other UVs and tilted normals."""
    n = cells + 1
    c = ((np.arange(n) - cells / 2) * step).astype(np.float32)
    X, Y = np.meshgrid(c, c, indexing="xy")
    pos = np.stack([X.reshape(-1) + shift, Y.reshape(-1) + shift, np.zeros(n * n) + shift], -1).astype(np.float32)
    I, J = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    uv = np.stack([I.reshape(-1) / cells, J.reshape(-1) / cells], -1)
    nrm = np.tile([0.0, 0.0, 1.0], (n * n, 1))
    if copy:
        uv = 1.0 - 0.5 * uv
        nrm = np.tile([0.6, 0.0, 0.8], (n * n, 1))
    idx = []
    for j in range(cells):
        for i in range(cells):
            a, b = j * n + i, j * n + i + 1
            c_, d = a + n, b + n
            idx += [(a, b, c_), (b, d, c_)]
    return pos, np.array(idx, np.uint32), nrm.astype(np.float32), uv.astype(np.float32)


def double_grid_mesh(away=None):
    """Every face of the grid twice: the copy has its own vertices (other UVs
    and normals, so a record shows which copy won) and its faces run in
    reverse order."""
    p0, i0, n0, u0 = grid_mesh(copy=0, shift=FAR_AWAY if away == 0 else 0.0)
    p1, i1, n1, u1 = grid_mesh(copy=1, shift=FAR_AWAY if away == 1 else 0.0)
    return (np.concatenate([p0, p1]), np.concatenate([i0, i1[::-1] + len(p0)]),
            np.concatenate([n0, n1]), np.concatenate([u0, u1]))


# --- tie scenes --------------------------------------------------------------------

def _camera(s, pt, position=(0.4, -5.0, 2.5), rotation=(1.1, 0.0, 0.05), fov=60.0):
    cam = s.create_entity(pt.ENTITY_CAMERA, position=position, rotation=rotation)
    s.set_camera_pinhole(cam, fov_degrees=fov, aperture_mm=0.0)


def _tie_materials(s, pt):
    return [s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Clay", BaseColor=(0.8, 0.6, 0.4)),
            s.create_material(pt.MATERIAL_BASIC_METAL, "Steel", BaseColor=(0.7, 0.7, 0.8), SpecularColor=(0.9, 0.9, 0.9),
                              Roughness=0.3),
            s.create_material(pt.MATERIAL_BASIC_TRANSLUCENT, "Glass", IOR=1.5, AbbeNumber=40.0, Roughness=0.0),
            s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Chalk", BaseColor=(0.3, 0.5, 0.8))]


def _place(away, k, position=(0.0, 0.0, 0.0)):
    return (FAR_AWAY, FAR_AWAY, FAR_AWAY) if away == k else position


def tie_double_mesh(pt, away=None):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    e = s.create_entity(pt.ENTITY_MESH_INSTANCE, material=m[0])
    s.set_mesh(e, s.create_mesh(*double_grid_mesh(away), name="DoubleGrid"))
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt)
    s.pack()
    return s


def tie_twin_instances(pt, away=None):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    mesh = s.create_mesh(*grid_mesh(), name="Grid")
    for k in range(2):
        e = s.create_entity(pt.ENTITY_MESH_INSTANCE, position=_place(away, k), material=m[k])
        s.set_mesh(e, mesh)
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt)
    s.pack()
    return s


def tie_three_spheres(pt, away=None):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    for k in range(3):
        s.create_entity(pt.ENTITY_SPHERE, position=_place(away, k), material=m[(k + 2) % 3])   # glass, clay, steel
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt)
    s.pack()
    return s


def tie_two_cubes(pt, away=None):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    for k in range(2):
        s.create_entity(pt.ENTITY_CUBE, position=_place(away, k), material=m[k])
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt)
    s.pack()
    return s


def tie_cubes_sharing_face(pt, away=None):
    """[-1, 1]^3 and [1, 3] x [-1, 1]^2: the face x = 1 belongs to both, as the
    exit of one and the entry of the other."""
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    s.create_entity(pt.ENTITY_CUBE, position=_place(away, 0), material=m[0])
    s.create_entity(pt.ENTITY_CUBE, position=_place(away, 1, (2.0, 0.0, 0.0)), material=m[2])
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt, position=(1.4, -6.0, 2.5))
    s.pack()
    return s


def tie_plane_cube_mesh(pt, away=None):
    """z = 0 three times: a plane, the top of a cube and a grid mesh.  The cube
    keeps the earlier visit, the other two the later one.  Beside them a
    second cube whose top is a second instance of the grid, at z = 1."""
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    s.create_entity(pt.ENTITY_PLANE, position=_place(away, 0), material=m[0])
    s.create_entity(pt.ENTITY_CUBE, position=_place(away, 1, (0.0, 0.0, -0.5)), scale=(0.5, 0.5, 0.5), material=m[1])
    grid = s.create_mesh(*grid_mesh(), name="Grid")
    e = s.create_entity(pt.ENTITY_MESH_INSTANCE, position=_place(away, 2), material=m[3])
    s.set_mesh(e, grid)
    # and z = 1 twice, clear of the plane (a plane set aside on the stack is
    # not tested against its box again, so it wins every tie it takes part in)
    s.create_entity(pt.ENTITY_CUBE, position=_place(away, 3, (2.0, 0.0, 0.5)), scale=(0.5, 0.5, 0.5), material=m[1])
    e = s.create_entity(pt.ENTITY_MESH_INSTANCE, position=_place(away, 4, (2.0, 0.0, 1.0)), material=m[3])
    s.set_mesh(e, grid)
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt, position=(1.4, -6.0, 2.5))
    s.pack()
    return s


TIES = {
    "double-mesh": Tie(tie_double_mesh, 2, True, False, (-1.0, 1.0)),
    "twin-instances": Tie(tie_twin_instances, 2, False, False, (-1.0, 1.0)),
    "three-spheres": Tie(tie_three_spheres, 3, False, False, (-1.0, 1.0)),
    "two-cubes": Tie(tie_two_cubes, 2, False, False, (-1.0, 1.0)),
    "cubes-sharing-face": Tie(tie_cubes_sharing_face, 2, False, False, (-1.0, 3.0)),
    "plane-cube-mesh": Tie(tie_plane_cube_mesh, 5, False, True, (-1.0, 3.0)),
}


# --- rays --------------------------------------------------------------------------

AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)


def _axial(points, axis, sign, start):
    """Rays along sign * axis from `start` on that axis through (u, v) points
    of the other two coordinates."""
    other = [a for a in range(3) if a != axis]
    o = np.zeros((len(points), 3), np.float32)
    o[:, other[0]], o[:, other[1]], o[:, axis] = points[:, 0], points[:, 1], start
    d = np.tile(AXES[axis] * sign, (len(points), 1)).astype(np.float32)
    return o, d


def _lattice(us, vs):
    U, V = np.meshgrid(np.asarray(us, np.float32), np.asarray(vs, np.float32), indexing="ij")
    return np.stack([U.reshape(-1), V.reshape(-1)], -1)


def filler_rays(n, lo, hi, seed):
    """Oblique rays from a sphere around the box [lo, hi] towards points in it."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    centre, radius = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo) + 2.0
    u = rng.normal(size=(n, 3))
    o = centre + radius * u / np.linalg.norm(u, axis=1, keepdims=True)
    d = rng.uniform(lo, hi, size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def _pad(o, d, lo, hi, seed):
    """Filler until the count is odd and no multiple of 64 (a ragged last wave)."""
    extra = 61
    while (len(o) + extra) % 2 == 0 or (3 * (len(o) + extra)) % 64 == 0:
        extra += 1
    fo, fd = filler_rays(extra, lo, hi, seed)
    return np.concatenate([o, fo]), np.concatenate([d, fd])


def tie_rays(scene, case, seed=1):
    """(origins, packed velocities, durations) for a tie scene: axial rays on
    the lattice lines, vertices and shared edges of the grid (1/8 steps:
    vertices, edge midpoints, cell centres on the shared diagonal, points
    beside the mesh; a ray in a box's boundary plane misses that box, 0/0 in
    its slab test, so most of these test the boxes and miss the faces), the
    same lattice moved by 1/16 (cell interiors, a third of them on the shared
    diagonal), from above, from behind and from inside the solids, and oblique
    filler; then every ray three times -- unlimited, with Duration
    exactly the hit time, and one float shorter."""
    x0, x1 = case.x_range
    xs = np.linspace(x0, x1, 17)
    ys = np.arange(-2, 3) * 0.125
    coarse = np.arange(-2, 3) * 0.5
    o, d = [], []
    for start, sign in ((3.0, -1.0), (-3.0, 1.0)):                  # along z, from above and from behind
        a, b = _axial(_lattice(xs, ys), 2, sign, start)
        o.append(a); d.append(b)
        a, b = _axial(_lattice(np.linspace(x0, x1, 9) + 0.0625, ys + 0.0625), 2, sign, start)   # cell interiors
        o.append(a); d.append(b)
    for start in (-0.5, 0.5):                                       # along z, from inside the solids
        for sign in (-1.0, 1.0):
            a, b = _axial(_lattice(np.linspace(x0, x1, 9)[:-1] + 0.125, np.arange(-2, 2) * 0.25 + 0.125), 2, sign, start)
            o.append(a); d.append(b)
    for axis in (0, 1):                                             # along x and y: from outside, then from inside
        for start, sign in ((-4.0, 1.0), (4.0, -1.0), (0.0, 1.0), (0.0, -1.0), (2.0, -1.0)):
            pts = _lattice(coarse, coarse) if axis == 0 else _lattice(np.linspace(x0, x1, 5), coarse)
            if axis == 0 and abs(start) < 4.0:
                pts = _lattice(np.arange(-3, 4) * 0.25, np.arange(-3, 4) * 0.25)
            if start == 2.0 and (axis == 1 or x1 < 2.0):
                continue
            a, b = _axial(pts, axis, sign, start)
            o.append(a); d.append(b)
    o, d = np.concatenate(o), np.concatenate(d)
    # A ray lying in a plane shape's own surface has the hit time -0 / 0: a NaN
    # that is accepted (neither T < 0 nor T > Hit.Time) and whose sign bit is
    # the hardware's.  No tie, and nothing GLSL defines: left out.
    rec = oracle_lib.trace_rays(scene.packs(), o, oracle_lib.pack_unit_vectors(d), np.full(len(o), FAR, np.float32))
    keep = ~np.isnan(rec["time"])
    o, d = _pad(o[keep], d[keep], (x0, -1.0, -1.0), (x1, 1.0, 1.0), seed)
    vel = oracle_lib.pack_unit_vectors(d)
    far = np.full(len(vel), FAR, np.float32)
    rec = oracle_lib.trace_rays(scene.packs(), o, vel, far)
    hit = rec["shape_material"] != 0xFFFFFFFF
    exact = np.where(hit, rec["time"], far).astype(np.float32)
    shorter = np.where(hit, np.nextafter(exact, np.float32(0.0)), far).astype(np.float32)
    return np.tile(o, (3, 1)), np.tile(vel, 3), np.concatenate([far, exact, shorter])


# --- degenerate hit attributes -----------------------------------------------------

def _z_word(sx, sy):
    """The packed velocity whose unpacking is (sx 0, sy 0, -1): the octahedral
    fold keeps the sign of a -1 / +1 corner coordinate on a zero."""
    return ((0x7FFF if sx > 0 else 0x8001) | ((0x7FFF if sy > 0 else 0x8001) << 16))


def degenerate_spheres(pt):
    """A unit sphere at the origin, one moved and scaled along its axes, one
    rotated and scaled (its poles are reached to within the octahedral
    packing of the ray direction)."""
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    s.create_entity(pt.ENTITY_SPHERE, material=m[0])
    s.create_entity(pt.ENTITY_SPHERE, position=(-4.0, 0.5, 0.25), scale=(1.25, 0.75, 1.5), material=m[1])
    s.create_entity(pt.ENTITY_SPHERE, position=(4.0, 0.0, 0.0), rotation=(0.4, 0.3, 0.7), scale=(1.3, 0.8, 1.7), material=m[3])
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt, position=(0.0, -8.0, 2.0), rotation=(1.35, 0.0, 0.0))
    s.pack()
    return s


def sphere_rays(scene):
    o, d, words = [], [], []
    for x, y in ((0.0, 0.0), (1e-20, 0.0), (0.0, 1e-30), (1e-30, -1e-20), (-0.0, 0.0), (1e-4, 0.0), (0.0, -1e-3)):
        for z, dz in ((3.0, -1.0), (-3.0, 1.0), (0.0, 1.0), (0.0, -1.0), (0.5, 1.0)):      # outside, centre, inside
            o.append((x, y, z)); d.append((0.0, 0.0, dz))
    for x, y in ((-4.0, 0.5), (-4.0, 0.5000001), (-3.9999998, 0.5)):                       # the scaled sphere's axis
        for z, dz in ((5.0, -1.0), (-5.0, 1.0), (0.25, 1.0)):
            o.append((x, y, z)); d.append((0.0, 0.0, dz))
    to = scene.arrays()["shapes"][2]["Transform"]["To"].astype(np.float64).reshape(4, 4).T   # column-major
    for z, dz in ((3.0, -1.0), (-3.0, 1.0), (0.0, 1.0)):                                   # the rotated sphere's axis
        p = to @ np.array([0.0, 0.0, z, 1.0])
        v = to @ np.array([0.0, 0.0, dz, 0.0])
        o.append(tuple(p[:3])); d.append(tuple(v[:3] / np.linalg.norm(v[:3])))
    o, d = np.array(o, np.float32), np.array(d, np.float32)
    o, d = _pad(o, d, (-5.5, -1.0, -1.5), (5.5, 1.0, 1.5), 2)
    vel = oracle_lib.pack_unit_vectors(d)
    # the same poles with -0 velocity components (they reach the TLAS slab tests)
    wo = np.array([(0.0, 0.0, 3.0), (1e-30, 0.0, 3.0), (-4.0, 0.5, 5.0)] * 3, np.float32)
    wv = np.repeat(np.array([_z_word(-1, 1), _z_word(1, -1), _z_word(-1, -1)], np.uint32), 3)
    o, vel = np.concatenate([o, wo]), np.concatenate([vel, wv])
    if len(vel) % 2 == 0:
        o, vel = o[:-1], vel[:-1]
    return o, vel, np.full(len(vel), FAR, np.float32)


def degenerate_cubes(pt):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    s.create_entity(pt.ENTITY_CUBE, material=m[0])
    s.create_entity(pt.ENTITY_CUBE, position=(5.0, 0.5, 0.0), scale=(0.5, 1.0, 2.0), material=m[1])
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt, position=(2.0, -9.0, 3.0), rotation=(1.3, 0.0, 0.0))
    s.pack()
    return s


def cube_rays(scene):
    """Per cube, in its own coordinates: axial rays at face centres, edges,
    corners, just inside and just outside them, rays lying in a face plane
    (0/0 in one slab), from outside and from the centre; diagonal rays into all
    eight corners; -z rays with -0 components."""
    up = np.nextafter(np.float32(1.0), np.float32(2.0))
    dn = np.nextafter(np.float32(1.0), np.float32(0.0))
    vals = [0.0, 0.25, 1.0, -1.0, float(dn), float(up), -float(dn)]
    pts = _lattice(vals, vals)
    lo_, ld = [], []
    for axis in range(3):
        for start, sign in ((3.0, -1.0), (-3.0, 1.0), (0.0, 1.0), (1.0, -1.0), (1.0, 1.0)):
            a, b = _axial(pts, axis, sign, start)
            lo_.append(a); ld.append(b)
    corners = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    lo_.append(3.0 * corners); ld.append(-corners / np.sqrt(np.float32(3.0)))
    lo_.append(np.zeros((8, 3), np.float32)); ld.append(corners / np.sqrt(np.float32(3.0)))
    lo_, ld = np.concatenate(lo_), np.concatenate(ld)
    o, d = [lo_], [ld]
    o.append(lo_ * np.float32([0.5, 1.0, 2.0]) + np.float32([5.0, 0.5, 0.0])); d.append(ld)   # axial stay axial
    o, d = np.concatenate(o), np.concatenate(d)
    n = np.linalg.norm(d, axis=1, keepdims=True)
    o, d = _pad(o, (d / n).astype(np.float32), (-1.5, -1.5, -2.0), (6.0, 1.5, 2.0), 3)
    vel = oracle_lib.pack_unit_vectors(d)
    wo = np.array([(x, y, 3.0) for x in (0.0, 1.0, -1.0) for y in (0.25, 1.0)], np.float32)
    wv = np.tile(np.array([_z_word(-1, 1), _z_word(1, -1), _z_word(-1, -1)], np.uint32), 2)
    o, vel = np.concatenate([o, np.tile(wo, (1, 1))]), np.concatenate([vel, wv])
    if len(vel) % 2 == 0:
        o, vel = o[:-1], vel[:-1]
    return o, vel, np.full(len(vel), FAR, np.float32)


def normals_mesh():
    """Five triangles in z = 0, side by side (triangle k spans x in [2k, 2k + 1],
    y in [0, 1]), that differ in their vertex normals:
      0  (0,0,1), (0,0,-1), (0,0,1): the sum cancels exactly where the second
         coordinate is 1/2, and SafeNormalize answers +Z;
      1  three normals 120 degrees apart in the xy plane: they cancel (to the
         precision of their packing) at the centroid;
      2  (1,0,0) everywhere: ComputeTangentVector's other branch;
      3  x from 0.85 to 0.95 across the face: |Normal.x| passes 0.9;
      4  the same, negative x."""
    def unit(v):
        v = np.asarray(v, float)
        return v / np.linalg.norm(v)
    s3 = np.sqrt(3.0) / 2
    normals = [[(0, 0, 1), (0, 0, -1), (0, 0, 1)],
               [(1, 0, 0), (-0.5, s3, 0), (-0.5, -s3, 0)],
               [(1, 0, 0)] * 3,
               [unit((0.85, 0.2, np.sqrt(1 - 0.85 ** 2 - 0.04))), unit((0.95, 0.2, np.sqrt(1 - 0.95 ** 2 - 0.04))),
                unit((0.9, 0.2, np.sqrt(1 - 0.81 - 0.04)))],
               [unit((-0.85, 0.0, np.sqrt(1 - 0.85 ** 2))), unit((-0.95, 0.0, np.sqrt(1 - 0.95 ** 2))),
                unit((-0.9, 0.0, np.sqrt(1 - 0.81)))]]
    pos, nrm, uv, idx = [], [], [], []
    for k, n3 in enumerate(normals):
        pos += [(2.0 * k, 0.0, 0.0), (2.0 * k + 1.0, 0.0, 0.0), (2.0 * k, 1.0, 0.0)]
        nrm += n3
        uv += [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
    return np.array(pos, np.float32), np.array(idx, np.uint32), np.array(nrm, np.float32), np.array(uv, np.float32)


def degenerate_normals(pt):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    e = s.create_entity(pt.ENTITY_MESH_INSTANCE, material=m[0])
    s.set_mesh(e, s.create_mesh(*normals_mesh(), name="Normals"))
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt, position=(4.5, 0.5, 8.0), rotation=(0.0, 0.0, 0.0))
    s.pack()
    return s


def normals_rays(scene):
    o = []
    for y in (0.0, 0.125, 0.25, 0.5):                       # face 0: u = 1/2 and its neighbours
        for x in (0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(1))),
                  0.4375, 0.25, 0.75, 0.50001, 0.4999995, 0.5000005):   # |sum| = |1 - 2 x| against SafeNormalize's 1e-6
            o.append((x, y, 2.0))
    third = np.float32(1.0) / np.float32(3.0)
    for dx in (-1e-3, -1e-5, -1e-7, 0.0, 1e-7, 1e-5, 1e-3):  # face 1: around the centroid
        for dy in (-1e-5, 0.0, 1e-5):
            o.append((2.0 + float(third) + dx, float(third) + dy, 2.0))
    for x, y in ((4.25, 0.25), (4.0, 0.0), (5.0, 0.0), (4.0, 1.0), (4.5, 0.5)):   # face 2, vertices and the long edge
        o.append((x, y, 2.0))
    for k in (3, 4):                                          # faces 3, 4: a sweep of the interpolated normal
        for t in np.linspace(0.0, 1.0, 101):
            o.append((2.0 * k + 0.9 * t, 0.05, 2.0))
        for t in np.linspace(0.0, 0.9, 31):
            o.append((2.0 * k + 0.02, t, 2.0))
    o = np.array(o, np.float32)
    d = np.tile(np.float32([0.0, 0.0, -1.0]), (len(o), 1))
    ob = o.copy(); ob[:, 2] = -2.0                            # and from behind
    o, d = np.concatenate([o, ob]), np.concatenate([d, -d])
    o, d = _pad(o, d, (0.0, 0.0, -0.1), (9.0, 1.0, 0.1), 4)
    return o, oracle_lib.pack_unit_vectors(d), np.full(len(o), FAR, np.float32)


def degenerate_plane(pt):
    s = pt.Scene.empty()
    m = _tie_materials(s, pt)
    s.create_entity(pt.ENTITY_PLANE, material=m[0])
    s.set_root(skybox_brightness=1.2)
    _camera(s, pt)
    s.pack()
    return s


def plane_rays(scene):
    """Plane hits whose coordinates are negative, huge or whole numbers:
    fract() is 0, or 1 - 2^-24 and smaller differences round it to 1."""
    vals = [0.0, -0.0, 1.0, -1.0, 5.0, -3.0, 0.25, -0.25, -1e-9, -1e-30, 1e-30, 0.99999994, -0.99999994, 16777216.0,
            -16777216.0, 8388607.5, -8388607.5, 3.0e6 + 0.25, 1.0e9, -1.0e9, 2.5e8]
    pts = _lattice(vals, vals)
    o, d = _axial(pts, 2, -1.0, 2.0)
    ob, db = _axial(pts, 2, 1.0, -2.0)
    o, d = np.concatenate([o, ob]), np.concatenate([d, db])
    o, d = _pad(o, d, (-4.0, -4.0, -0.1), (4.0, 4.0, 0.1), 5)
    return o, oracle_lib.pack_unit_vectors(d), np.full(len(o), FAR, np.float32)


DEGENERATE = {
    "sphere-poles": Degenerate(degenerate_spheres, sphere_rays),
    "cube-edges": Degenerate(degenerate_cubes, cube_rays),
    "mesh-normals": Degenerate(degenerate_normals, normals_rays),
    "plane-coordinates": Degenerate(degenerate_plane, plane_rays),
}


# --- material parameter edges ------------------------------------------------------

GLASS = dict(AbbeNumber=40.0, Roughness=0.0, TransmissionColor=(0.9, 0.9, 0.9), TransmissionDepth=1.0)


def material_scene(pt, glass=None, scatter=None, metal=None, root=None, extra=None, camera=None):
    """A diffuse plane at z = -1, a glass sphere at (-0.6, 0, 0), a metal
    sphere of radius 0.7 at (0.9, 0, 0), whatever `extra` adds, and a pinhole
    camera in front."""
    s = pt.Scene.empty()
    d = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Floor", BaseColor=(0.8, 0.7, 0.6))
    s.create_entity(pt.ENTITY_PLANE, position=(0.0, 0.0, -1.0), material=d)
    if glass is not None:
        g = s.create_material(pt.MATERIAL_BASIC_TRANSLUCENT, "Glass", **glass)
        if scatter is not None:
            s.set_material_parameter(g, "ScatteringColor", scatter[0])
            s.set_material_parameter(g, "ScatteringAnisotropy", scatter[1])
        s.create_entity(pt.ENTITY_SPHERE, position=(-0.6, 0.0, 0.0), material=g)
    if metal is not None:
        m = s.create_material(pt.MATERIAL_BASIC_METAL, "Metal", **metal)
        s.create_entity(pt.ENTITY_SPHERE, position=(0.9, 0.0, 0.0), scale=(0.7, 0.7, 0.7), material=m)
    root = dict(root or {})
    if extra is not None:
        extra(s, pt, root)
    s.set_root(**root)
    if camera is None:
        _camera(s, pt, position=(0.0, -4.0, 0.3), rotation=(1.5, 0.0, 0.0))
    else:
        camera(s, pt)
    s.pack()
    return s


def _shells(s, pt, root):
    """Six concentric glass spheres: a path inside the fifth holds more
    shapes than the four active-shape entries."""
    for k in range(6):
        g = s.create_material(pt.MATERIAL_BASIC_TRANSLUCENT, f"Shell{k}", IOR=1.1 + 0.1 * k, AbbeNumber=40.0, Roughness=0.0,
                              TransmissionColor=(0.9, 0.9, 0.9), TransmissionDepth=1.0)
        r = 1.2 - 0.15 * k
        s.create_entity(pt.ENTITY_SPHERE, scale=(r, r, r), material=g)


def _overlap(s, pt, root):
    """Three glass spheres in a chain, each overlapping the next: a path
    leaves the first while inside the second, which empties active slot 0
    while slot 1 is held."""
    for k in range(3):
        g = s.create_material(pt.MATERIAL_BASIC_TRANSLUCENT, f"Lens{k}", IOR=1.2 + 0.15 * k, AbbeNumber=40.0, Roughness=0.0,
                              TransmissionColor=(0.9, 0.9, 0.9), TransmissionDepth=1.0)
        s.create_entity(pt.ENTITY_SPHERE, position=(-0.7 + 0.7 * k, 0.5 * k, 0.0), material=g)


def _black_sky(s, pt, root):
    img = np.zeros((8, 16, 4), np.float32)
    img[..., 3] = 1.0
    d = s.create_material(pt.MATERIAL_BASIC_DIFFUSE, "Ball", BaseColor=(0.8, 0.8, 0.8))
    s.create_entity(pt.ENTITY_SPHERE, material=d)
    root["skybox"] = s.create_texture("BlackSky", pt.TEXTURE_RADIANCE, img)


def _openpbr(**params):
    def extra(s, pt, root):
        m = s.create_material(pt.MATERIAL_OPENPBR, "Layered", **params)
        s.create_entity(pt.ENTITY_SPHERE, material=m)
    return extra


def _camera_above(s, pt):
    _camera(s, pt, position=(0.0, 0.0, 3.0), rotation=(0.0, 0.0, 0.0), fov=50.0)


def _lit_pole(s, pt, root):
    m = s.create_material(pt.MATERIAL_BASIC_METAL, "Brushed", BaseColor=(0.9, 0.8, 0.6), SpecularColor=(1.0, 1.0, 1.0),
                          Roughness=0.5, RoughnessAnisotropy=0.8)
    s.create_entity(pt.ENTITY_SPHERE, material=m)


def _mat(glass=None, scatter=None, metal=None, root=None, extra=None, camera=None, openpbr=False, flags=(3,), ptp=0.0,
         size=None, branches=()):
    def build(pt):
        return material_scene(pt, None if glass is None else dict(GLASS, **glass), scatter, metal, root, extra, camera)
    return Material(build, openpbr, flags, ptp, size, branches)


WHITE_METAL = dict(BaseColor=(1.0, 1.0, 1.0), SpecularColor=(1.0, 1.0, 1.0), Roughness=1.0, RoughnessAnisotropy=1.0)
BLACK_METAL = dict(BaseColor=(0.0, 0.0, 0.0), SpecularColor=(0.0, 0.0, 0.0), Roughness=1e-4, RoughnessAnisotropy=0.0)
FOG = dict(IOR=1.3, TransmissionDepth=0.3)

# branches: the path_restatement.STATS keys the scene is named for (each must
# be counted at least once by the CPU test).
MATERIALS = {
    # relative IOR exactly 1 (AbbeNumber 1e9 takes the dispersion away): Sq = Ci * RelIOR + Co = 0, J = inf
    "ior-one-smooth": _mat(dict(IOR=1.0), branches=("glass_dirac", "refract")),
    "ior-one-rough": _mat(dict(IOR=1.0, Roughness=0.3), branches=("glass", "refract")),
    "ior-one-no-dispersion": _mat(dict(IOR=1.0, Roughness=0.3, AbbeNumber=1e9), root=dict(skybox_sampling_probability=0.5),
                                  branches=("glass", "refract", "sq_zero")),
    "ior-below-one": _mat(dict(IOR=0.7, Roughness=0.2), branches=("glass", "reflect", "refract")),
    "abbe-zero": _mat(dict(IOR=1.5, AbbeNumber=0.0), branches=("glass_dirac",)),
    "abbe-one": _mat(dict(IOR=1.5, AbbeNumber=1.0, Roughness=0.2), branches=("glass", "reflect")),
    "roughness-one-anisotropy-one": _mat(dict(IOR=1.5, Roughness=1.0), metal=WHITE_METAL,
                                         branches=("glass", "metal")),
    "roughness-tiny": _mat(dict(IOR=1.5, Roughness=1e-4), metal=BLACK_METAL,
                           branches=("glass_dirac", "metal_dirac")),
    "hg-zero": _mat(FOG, scatter=((0.8, 0.8, 0.8), 0.0), branches=("medium",)),
    "hg-plus-one": _mat(FOG, scatter=((0.8, 0.8, 0.8), 1.0), branches=("medium_hg",)),
    "hg-minus-one": _mat(FOG, scatter=((1.0, 1.0, 1.0), -1.0), branches=("medium_hg",)),
    "depth-tiny": _mat(dict(IOR=1.3, TransmissionDepth=1e-6, TransmissionColor=(0.5, 0.5, 0.5)), branches=("refract",)),
    "transmission-black": _mat(dict(IOR=1.3, TransmissionColor=(0.0, 0.0, 0.0)), branches=("refract",)),
    "transmission-white": _mat(dict(IOR=1.3, TransmissionColor=(1.0, 1.0, 1.0)), scatter=((0.0, 0.0, 0.0), 0.5),
                               branches=("refract",)),
    "shells": _mat(extra=_shells, branches=("glass_dirac", "active_full")),
    "overlap": _mat(extra=_overlap, branches=("glass_dirac", "slot0_hole")),
    "black-sky": _mat(extra=_black_sky, root=dict(skybox_sampling_probability=1.0), branches=("light",)),
    "termination-one": _mat(dict(IOR=1.5, Roughness=1.0), metal=WHITE_METAL, ptp=1.0,
                            branches=("diffuse", "terminated")),
    # the OpenPBR twins (rendered with set_openpbr(True))
    "openpbr-ior-one": _mat(extra=_openpbr(BaseColor=(1.0, 1.0, 1.0), SpecularIOR=1.0, CoatWeight=1.0, CoatIOR=1.0,
                                           Roughness=0.0, CoatRoughness=0.0), openpbr=True,
                            branches=("coat_refract", "spec_refract")),
    "openpbr-bounce-zero": _mat(extra=_openpbr(BaseColor=(1.0, 1.0, 1.0), LayerBounceLimit=0, CoatWeight=1.0),
                                openpbr=True, branches=("openpbr_walk",)),
    "openpbr-roughness-one": _mat(extra=_openpbr(TransmissionWeight=1.0, Roughness=1.0, RoughnessAnisotropy=1.0,
                                                 TransmissionDepth=0.0, SpecularWeight=0.0), openpbr=True,
                                  branches=("openpbr_walk",)),
    "openpbr-black-metal": _mat(extra=_openpbr(BaseMetalness=1.0, BaseColor=(0.0, 0.0, 0.0), SpecularWeight=1.0,
                                               Roughness=1e-4), openpbr=True, branches=("spec_metal",)),
    "openpbr-weights-zero": _mat(extra=_openpbr(BaseWeight=0.0, SpecularWeight=0.0, CoatWeight=0.0, TransmissionWeight=0.0,
                                                BaseMetalness=0.0), openpbr=True, branches=("openpbr_walk", "spec_refract")),
    "openpbr-weights-one": _mat(extra=_openpbr(BaseWeight=1.0, SpecularWeight=1.0, CoatWeight=1.0, TransmissionWeight=1.0,
                                               BaseMetalness=1.0), openpbr=True,
                                branches=("coat_reflect", "spec_metal")),
    # a brushed metal sphere seen from straight above, without jitter, in a frame
    # of odd width and height: the centre pixel's ray runs down the axis and its
    # hit carries the pole's NaN tangent into Scatter's frame
    "lit-pole": _mat(extra=_lit_pole, camera=_camera_above, flags=(1, 3), size="odd", branches=("metal",)),
}


def frame_size(case, W, H):
    """The frame a MATERIALS case renders at: (W, H), or one pixel less each
    way where the case needs a centre pixel."""
    return (W - 1, H - 1) if case.size == "odd" else (W, H)


def material_types(scene):
    """The material types (MATERIAL_*) of the scene's shapes: more than one
    lets a renderer in tile groups shade through per-class lists."""
    a = scene.arrays()
    return {int(a["materials"][32 * int(m)]) for m in a["shapes"]["MaterialIndex"]}
