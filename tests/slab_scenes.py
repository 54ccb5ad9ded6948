"""Scenes at the boundaries of the fast slab division's two gates
(test_gpu_slab_domain.py; their host-side conditions in test_slab_cases.py).

The scene gate (rt_scene.hip FastDivBoxes, once per upload) needs every TLAS
and BLAS box coordinate to be 0 or in [2^-50, 2^40]; the ray gate
(pt_device.hpp FastDivRay, per ray and traversal level) needs every origin
component in that set and every velocity component in [2^-59, 2^27].  The
blob of fuzz_scenes.py as it comes does NOT pass the scene gate: a lat-long
sphere's sin(pi) and cos(pi / 2) leave coordinates near 1e-17 < 2^-50 in its
boxes, so every scene built on it traces with IEEE division.  clean_blob()
sets those to 0; the scenes here start from it.
"""
from __future__ import annotations

import numpy as np

import oracle_lib
import slab_cases as sc
from test_gpu_mesh_extend import blob, chain_mesh, mesh_scene, special_rays

F32 = np.float32
EDIT = (55, 0)     # the blob vertex and axis the controls edit: a value near 0 there is a bound of its leaf's box


def clean_blob(seed=3):
    pos, idx, nrm, uv = blob(seed)
    pos = pos.copy()
    pos[np.abs(pos) < 2.0 ** -50] = 0.0
    return pos, idx, nrm, uv


def box_gate(scene) -> bool:
    """The scene gate from the packed boxes, by DESIGN.md §2's statement of the range."""
    a = scene.arrays()
    return all(sc.boxes_in_range(a[k]["Minimum"], a[k]["Maximum"]).all() for k in ("shape_nodes", "mesh_nodes"))


def edited_blob_scene(pt, value=None, **transform):
    """The clean blob with one vertex coordinate replaced (None: as it is)."""
    pos, idx, nrm, uv = clean_blob()
    if value is not None:
        pos[EDIT] = value
    return mesh_scene(pt, (pos, idx, nrm, uv), **transform)


def below(x):
    return np.nextafter(F32(x), F32(0))


def above(x):
    return np.nextafter(F32(x), F32(np.inf))


# (name, the edited coordinate, the gate): the bounds themselves keep the gate on, one ulp outside turns it off
GATE_CASES = (
    ("clean", None, True),
    ("zero", F32(0.0), True),
    ("2^-50", F32(2.0 ** -50), True),
    ("below-2^-50", below(2.0 ** -50), False),
    ("2^-60", F32(2.0 ** -60), False),
    ("2^40", F32(2.0 ** 40), True),
    ("above-2^40", above(2.0 ** 40), False),
)


def long_chain_scene(pt, links):
    """chain_mesh(56) reaches 3 * 2^37; 59 links reach 3 * 2^40, beyond the range."""
    return mesh_scene(pt, chain_mesh(links), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.1), scale=(1.0, 1.0, 1.0))


def chain_rays(n=2048, seed=5):
    """Rays along the chain and at random (test_gpu_mesh_extend.test_stack_formats_and_spill)."""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), F32)
    o[:, 0] = rng.uniform(-40.0, -2.0, n)
    o[:, 1:] = rng.normal(0.0, 0.3, (n, 2)) + [0.0, 1.0]
    dirs = np.zeros((n, 3))
    dirs[:, 0] = 1.0
    dirs[:, 1:] = rng.normal(0.0, 0.02, (n, 2))
    dirs[n // 2:] = rng.normal(size=(n - n // 2, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return o, oracle_lib.pack_unit_vectors(dirs.astype(F32)), np.full(n, 1048576.0 * 4096.0 * 4096.0, F32)


STRADDLE = 2.0 ** 27


def straddle_scene(pt, instances=1):
    """The clean blob with its vertices times 2^27, instanced at scale
    2^-27 (1.3, 0.8, 1.7) and rotated: the same picture as the plain blob
    scene, but a unit world velocity becomes a mesh-space velocity of about
    2^27 / scale per component, on both sides of the ray gate's upper bound
    within one wave."""
    pos, idx, nrm, uv = clean_blob()
    scale = tuple(float(F32(k) * F32(1.0 / STRADDLE)) for k in (1.3, 0.8, 1.7))
    return mesh_scene(pt, ((pos * F32(STRADDLE)).astype(F32), idx, nrm, uv), scale=scale, instances=instances)


def local_rays(scene, origins, packed_velocities, shape=0):
    """The rays in the shape's space as the traversal forms them
    (mat4_mul_point / mat4_mul_vector of the packed From matrix, float32,
    left to right)."""
    m = scene.arrays()["shapes"][shape]["Transform"]["From"].reshape(-1).astype(F32)
    o = np.ascontiguousarray(origins, dtype=F32).reshape(-1, 3)
    v = oracle_lib.fp_eval("unpack_unit_vector", packed_velocities).view(F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        lo = np.stack([((m[r] * o[:, 0] + m[4 + r] * o[:, 1]) + m[8 + r] * o[:, 2]) + m[12 + r] * F32(1.0)
                       for r in range(3)], axis=1)
        lv = np.stack([((m[r] * v[:, 0] + m[4 + r] * v[:, 1]) + m[8 + r] * v[:, 2]) + m[12 + r] * F32(0.0)
                       for r in range(3)], axis=1)
    assert lo.dtype == F32 and lv.dtype == F32
    return lo, lv


def straddle_shares(scene, rays):
    """(share of the rays whose mesh-space ray passes the ray gate, share with
    a mesh-space velocity component above 2^27 and one below, share that hits
    by the oracle)."""
    o, v, d = rays
    lo, lv = local_rays(scene, o, v)
    exact = sc.expected_flag(lo, lv)
    m = np.abs(lv)
    both = (m > STRADDLE).any(axis=1) & (m < STRADDLE).any(axis=1)
    hit = oracle_lib.trace_rays(scene.packs(), o, v, d)["shape_material"] != 0xFFFFFFFF
    return float(exact.mean()), float(both.mean()), float(hit.mean())

