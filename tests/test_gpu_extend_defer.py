"""GPU: deferred hit attributes in the mesh-only extend loop (DESIGN.md §4
"Deferred hit attributes and pre-packed pushes"; traverse.hpp MeshStep,
MeshEnd).

The mesh-only loop carries, of a hit, only its time and its face; the rest of
the record (the coordinates and the packed vertex indices) is formed once
after the loop by testing that one face again.  Nothing of it may change a
result, so everything here is held to the CPU oracle bit for bit, records
compared as integers:

  * C3 at 80x48 and 64x16 over 42 rounds, in LENGTH order with the RUN block
    map and in OCTANT order with the TILE map; C2 (the general loop) at 64x64
    over 8 rounds; C1 in fused rounds at 64x64;
  * through the ray query, in the mesh-only and the general loop, on the three
    stack formats, and through the any-hit query:
      - rays that hit face 0 beside rays that miss, lane by lane in one wave
        (face 0 is a hit like any other: "no hit" is not a face index);
      - the bit-equal-time scenes of tests/edge_scenes.py: the face kept is
        the last one accepted, as before;
      - the 16-triangle mesh of tests/test_gpu_extend_lean.py: a winning face
        with |Det| at and beyond 2^126 (the division block, entered again
        after the loop), at PT_EPSILON, and a denormal |Det|;
      - a leaf with the 16-bit stack format's largest face count, 4095 faces
        of one centroid beside seven small faces (first face 7 = 2^3 - 1), and
        the same mesh one face over, which takes the 32-bit format;
      - a chain mesh deep enough to fill the 20 LDS rows and reach depth 32.
"""
from __future__ import annotations

import numpy as np
import pytest

import edge_scenes
import oracle_lib
from test_gpu_block_map import LENGTH, RUN, TILE, assert_oracle, close, oracle_after, renderer, snapshot
from test_gpu_extend_lean import lean_case
from test_gpu_mesh_extend import AUTO, FAR, GENERAL, MESH, blob, mesh_scene, upload
from test_gpu_parity import compare_hits, compare_state, render_pair, scene_for

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
OCTANT = 1                       # PT_RAY_ORDER_OCTANT
FORMATS = pytest.mark.parametrize("fmt", [0, 1, 2], ids=["stack16", "stack32-packed", "stack32-node-index"])
FORMS = pytest.mark.parametrize("form", [AUTO, GENERAL], ids=["mesh-loop", "general-loop"])
IDENTITY = dict(position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


# --- renders ------------------------------------------------------------------------

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
    close(r)


def test_c2_general_loop_8_rounds_equal_the_oracle(pt, dev):
    gs, os_, ga, oa = render_pair(pt, dev, 2, 64, 64, [2, 1, 1, 1, 1, 1, 1])
    compare_state(gs, os_)
    assert np.array_equal(ga.view(np.uint32), oa.view(np.uint32))


def test_c1_fused_rounds_equal_the_oracle(pt, dev):
    gs, os_, ga, oa = render_pair(pt, dev, 1, 64, 64, [2, 1, 1, 1], fused=2)
    compare_state(gs, os_)
    assert np.array_equal(ga.view(np.uint32), oa.view(np.uint32))


# --- ray sets -----------------------------------------------------------------------
#
# Each case: (scene, rays, the oracle's records), built once and left unchanged.

_cases = {}


def case(pt, name):
    if name not in _cases:
        _cases[name] = BUILD[name](pt)
    return _cases[name]


def with_oracle(s, rays):
    return s, rays, oracle_lib.trace_rays(s.packs(), *rays)


def face0_case(pt):
    """The blob, untransformed; even rays go straight at the centroid of the
    face the packed scene numbers 0, from just in front of it, odd rays start
    outside the mesh and fly away: hit, miss, hit, miss through three waves
    and a ragged fourth."""
    s = mesh_scene(pt, blob(), **IDENTITY)
    a = s.arrays()
    f = a["mesh_faces"][0]
    p = np.stack([f["Position0"], f["Position1"], f["Position2"]]).astype(np.float64)[:, :3]
    c = p.mean(axis=0)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    n /= np.linalg.norm(n)
    k = 201
    o = np.zeros((k, 3))
    d = np.zeros((k, 3))
    o[0::2], d[0::2] = c + 1e-3 * n, -n
    o[1::2], d[1::2] = c + 50.0 * n, n
    rays = (o.astype(np.float32), oracle_lib.pack_unit_vectors(d.astype(np.float32)), np.full(k, FAR, np.float32))
    s, rays, ref = with_oracle(s, rays)
    hit = ref["shape_material"] != NONE
    assert hit[0::2].all() and not hit[1::2].any()
    assert np.all(np.abs(ref["time"][0::2] - 1e-3) < 1e-4)          # nothing in between: face 0 is the hit
    return s, rays, ref


def tie_case(name):
    def build(pt):
        t = edge_scenes.TIES[name]
        s = t.build(pt)
        return with_oracle(s, edge_scenes.tie_rays(s, t))
    return build


def lean_all_case(pt):
    s, groups, allr, ref = lean_case(pt)
    for g in ("huge", "eps", "eps_above"):                          # the winners the name promises
        assert (groups[g][1]["shape_material"] != NONE).all()
    assert not (groups["denormal"][1]["shape_material"] != NONE).any()
    return s, allr, ref


CLUSTER = 4095                   # count < 2^(15 - F) at F = 3


def cluster_mesh(count):
    """Seven small triangles along -x and `count` triangles over one set of
    positions at +x (each with vertices of its own: other normals and UVs, so
    a record names the copy that won).  Faces of one centroid cannot be split:
    the copies are one leaf, the last in face order, starting at face 7."""
    pos, idx, nrm, uv = [], [], [], []
    for i in range(7):
        x = -10.0 + i
        pos += [(x, -0.25, 0.0), (x + 0.5, -0.25, 0.0), (x, 0.25, 0.0)]
    for i in range(count):
        pos += [(10.0, -1.0, 0.0), (12.0, -1.0, 0.0), (10.0, 1.0, 0.0)]
    for i in range(7 + count):
        idx.append((3 * i, 3 * i + 1, 3 * i + 2))
        a = 0.0005 * (i % 1024)
        nrm += [(np.sin(a), 0.0, np.cos(a))] * 3
        uv += [((i % 64) / 64.0, (i // 64) / 64.0)] * 3
    return np.array(pos, np.float32), np.array(idx, np.uint32), np.array(nrm, np.float32), np.array(uv, np.float32)


def cluster_rays():
    """Down onto the cluster and the small faces, past them, and oblique."""
    rng = np.random.default_rng(31)
    n = 193
    o = np.column_stack([rng.uniform(9.9, 11.3, n), rng.uniform(-1.1, 0.3, n), np.full(n, 2.0)])
    o[::3, 0] = rng.uniform(-10.5, -3.0, len(o[::3]))
    o[::3, 1] = rng.uniform(-0.4, 0.4, len(o[::3]))
    d = np.tile([0.0, 0.0, -1.0], (n, 1))
    d[1::4] += rng.normal(0.0, 0.1, (len(d[1::4]), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), oracle_lib.pack_unit_vectors(d.astype(np.float32)), np.full(n, FAR, np.float32)


def cluster_case(count):
    def build(pt):
        s = mesh_scene(pt, cluster_mesh(count), **IDENTITY)
        nodes = s.arrays()["mesh_nodes"]
        leaf = nodes[nodes["FaceEndIndex"] > 0]
        big = leaf[leaf["FaceEndIndex"] - leaf["FaceBeginOrNodeIndex"] == count]
        assert len(big) == 1 and big["FaceBeginOrNodeIndex"][0] == 7 and leaf["FaceBeginOrNodeIndex"].max() == 7
        s, rays, ref = with_oracle(s, cluster_rays())
        hit = ref["shape_material"] != NONE
        assert hit.sum() > 40 and (~hit).sum() > 40
        return s, rays, ref
    return build


def deep_chain_mesh(links=86, shift=48):
    """test_gpu_mesh_extend's chain with more links, every coordinate still 0
    or within the exact fast division's range [2^-50, 2^40]."""
    pos, idx = [], []
    for i in range(links):
        c, r = 3.0 * 2.0 ** (i - shift), 0.5 * 2.0 ** (i - shift)
        pos += [(c, -r, 1.0 - r), (c, r, 1.0 - r), (c, 0.0, 1.0 + r)]
        idx.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(pos, np.float32), np.array(idx, np.uint32)


def blas_depth(nodes, root=0):
    depth, todo = 0, [(root, 0)]
    while todo:
        i, d = todo.pop()
        depth = max(depth, d)
        if nodes["FaceEndIndex"][i] == 0:
            c = int(nodes["FaceBeginOrNodeIndex"][i])
            todo += [(c, d + 1), (c + 1, d + 1)]
    return depth


def deep_chain_case(pt):
    """A BVH deeper than the 32 stack entries, and rays along it that set a
    far child aside at every level."""
    s = mesh_scene(pt, deep_chain_mesh(), position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0))
    assert blas_depth(s.arrays()["mesh_nodes"]) > 32
    rng = np.random.default_rng(5)
    n = 515
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = rng.uniform(-40.0, -2.0, n)
    o[:, 1:] = rng.normal(0.0, 0.3, (n, 2)) + [0.0, 1.0]
    dirs = np.zeros((n, 3))
    dirs[:, 0] = 1.0
    dirs[:, 1:] = rng.normal(0.0, 0.02, (n, 2))
    dirs[n // 2:] = rng.normal(size=(n - n // 2, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = (o, oracle_lib.pack_unit_vectors(dirs.astype(np.float32)), np.full(n, FAR * 4096.0, np.float32))
    s, rays, ref = with_oracle(s, rays)
    assert (ref["shape_material"] != NONE).sum() > n // 8
    return s, rays, ref


BUILD = {
    "face0": face0_case,
    "tie-double-mesh": tie_case("double-mesh"),
    "tie-twin-instances": tie_case("twin-instances"),
    "lean": lean_all_case,
    "largest-leaf": cluster_case(CLUSTER),
    "leaf-one-over": cluster_case(CLUSTER + 1),
    "deep-chain": deep_chain_case,
}
ONE_MESH = {name: name != "tie-twin-instances" for name in BUILD}


@pytest.mark.parametrize("name", list(BUILD))
@FORMATS
@FORMS
def test_hit_records(pt, dev, name, form, fmt):
    s, rays, ref = case(pt, name)
    ds = upload(pt, dev, s, form=form, stack_format=fmt)
    assert ds.extend_form == (MESH if form == AUTO and ONE_MESH[name] else GENERAL)
    if name == "deep-chain":
        assert ds.stack_needed == 32
    if fmt == 0 and name == "largest-leaf":
        assert ds.node_cache_pairs > 0          # the LDS node cache rides with the 16-bit format
    if name == "leaf-one-over" or fmt != 0:
        assert ds.node_cache_pairs == 0         # one face over the bound: no 16-bit format
    compare_hits(ds.trace_rays(*rays), ref)
    ds.close()


@pytest.mark.parametrize("name", list(BUILD))
@FORMATS
@FORMS
def test_any_hit(pt, dev, name, form, fmt):
    s, rays, ref = case(pt, name)
    ds = upload(pt, dev, s, form=form, stack_format=fmt)
    assert np.array_equal(ds.occluded(*rays), ref["shape_material"] != NONE)
    ds.close()
