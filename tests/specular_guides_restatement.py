"""A numpy float32 restatement of the guides that follow mirrors and smooth
glass, written from the definition apart from
include/pt_guides.h and csrc/hip/denoise.hip (test infrastructure only;
tests/test_specular_guides.py, tests/test_gpu_specular_guides.py):

  guides      per bounce one oracle ray query (oracle_lib.trace_rays) over the
              pixels still in flight, as denoise_restatement.guides does for
              the first ray; then per hit the classification (a basic metal
              or basic translucent whose texturable roughness at the hit is
              < 1e-3, while bounces remain), the record of a hit that is not
              followed, or the new ray of one that is.
  direction   the world direction a followed hit sends its ray on: the mirror
              direction, or the refraction by the material's base index, with
              total internal reflection taking the mirror's.

Numerics: DESIGN.md §2's convention in numpy float32 (nothing fused, sums
left to right, IEEE sqrt and division)."""
from __future__ import annotations

import numpy as np

import denoise_restatement as dr
import kat
import oracle_lib
import path_restatement as pr
import preview_restatement as pvr

f32 = np.float32
NONE = 0xFFFFFFFF
MAX_BOUNCES = 8
METAL, TRANSLUCENT = 1, 2
ROUGHNESS_WORD = {METAL: 9, TRANSLUCENT: 3}     # PT_BASIC_METAL_ROUGHNESS, PT_BASIC_TRANSLUCENT_ROUGHNESS
IOR_WORD = 1                                    # PT_BASIC_TRANSLUCENT_IOR
DIRAC = f32(1e-3)
OFFSET = f32(1e-3)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2],
                     a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0],
                     a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1).astype(f32)


def local_in(translucent, eta, out):
    """In of the hit's frame for Out (n, 3): (-x, -y, z) for a mirror and
    under total internal reflection, the refracted direction otherwise."""
    translucent = np.asarray(translucent, bool)
    eta = np.asarray(eta, f32)
    out = np.asarray(out, f32).reshape(-1, 3)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        mirror = np.stack([-out[:, 0], -out[:, 1], out[:, 2]], axis=1).astype(f32)
        c = out[:, 2]
        rel = np.where(c < 0, eta, one / eta).astype(f32)
        k = one - (rel * rel) * (one - c * c)
        refract = translucent & (k > 0)
        cr = -np.sign(c).astype(f32) * np.sqrt(np.where(refract, k, one).astype(f32))
        bent = np.stack([-rel * out[:, 0], -rel * out[:, 1], cr], axis=1).astype(f32)
    return np.where(refract[:, None], bent, mirror).astype(f32), refract


def direction(translucent, eta, N, TX, V):
    """W (n, 3) and, per ray, whether it was refracted."""
    N, TX, V = (np.asarray(a, f32).reshape(-1, 3) for a in (N, TX, V))
    with np.errstate(all="ignore"):
        TY = _cross(N, TX)
        out = np.stack([-_dot(V, TX), -_dot(V, TY), -_dot(V, N)], axis=1).astype(f32)
        inn, refracted = local_in(translucent, eta, out)
        W = (inn[:, 0:1] * TX + inn[:, 1:2] * TY) + inn[:, 2:3] * N
    return W.astype(f32), refracted


def guides(scene, camera, W, H, max_bounces, trace=None):
    """(H, W) guide records of packed camera `camera` after chains of at most
    max_bounces followed hits.  trace: a dict that receives per-pixel (H, W)
    arrays: "bounces" (followed hits), "refracted" and "reflected" (how many
    of them took which branch) and "packed_velocity" (the last ray traced)."""
    assert 0 <= max_bounces <= MAX_BOUNCES
    cam = scene.arrays()["cameras"][camera]
    world = pr.World(scene)
    n = W * H
    out = np.zeros(n, dr.GUIDE_DTYPE)
    out["shape"] = NONE
    info = {k: np.zeros(n, np.uint32) for k in ("bounces", "refracted", "reflected")}
    if trace is not None:
        trace.update({k: v.reshape(H, W) for k, v in info.items()})
    rays = [dr.central_ray(cam, x, y, W, H) for y in range(H) for x in range(W)]
    if rays[0] is None:
        return out.reshape(H, W)
    O = np.array([r[0] for r in rays], f32)
    PV = np.array([r[1] for r in rays], np.uint32)
    total = np.zeros(n, f32)
    tag = np.zeros(n, np.uint32)
    live = np.arange(n)
    flat = {}   # base colour of a material without a base texture
    for b in range(max_bounces + 1):
        if live.size == 0:
            break
        hits = oracle_lib.trace_rays(scene.packs(), O[live], PV[live], np.full(live.size, pr.HIT_TIME_LIMIT, f32))
        V = kat.unpack_unit_vector(PV[live])
        N = kat.unpack_unit_vector(hits["packed_normal"])
        TX = kat.unpack_unit_vector(hits["packed_tangent"])
        follow = np.zeros(live.size, bool)
        glass = np.zeros(live.size, bool)
        eta = np.ones(live.size, f32)
        for j, p in enumerate(live):
            h = hits[j]
            sm = int(h["shape_material"])
            if sm == NONE:
                sky = pvr.observe_d65(world.sky_spectrum([f32(c) for c in V[j]]))
                out["albedo"][p] = pvr._mat3(pvr.XYZ_TO_SRGB, sky)
                continue
            s, m = sm >> 16, sm & 0xFFFF
            total[p] = h["time"] if b == 0 else total[p] + h["time"]
            typ = int(world.mat[32 * m])
            uv = [f32(h["u"]), f32(h["v"])]
            if b < max_bounces and typ in ROUGHNESS_WORD and world.value(m, ROUGHNESS_WORD[typ], uv) < DIRAC:
                follow[j] = True
                glass[j] = typ == TRANSLUCENT
                eta[j] = world.mfloat(m, IOR_WORD)
                if tag[p] == 0:
                    tag[p] = s + 1
                continue
            textured = typ in (0, 1) and int(world.mat[32 * m + 4]) != NONE
            if textured:
                col = pvr.base_color(world, m, uv)
            else:
                if m not in flat:
                    flat[m] = pvr.base_color(world, m, [f32(0.0), f32(0.0)])
                col = flat[m]
            out["normal"][p] = N[j]
            out["time"][p] = total[p]
            out["albedo"][p] = pvr._mat3(pvr.XYZ_TO_SRGB, col)
            out["shape"][p] = (int(tag[p]) << 16) | s
        if not follow.any():
            break
        f = np.flatnonzero(follow)
        pix = live[f]
        Wd, refracted = direction(glass[f], eta[f], N[f], TX[f], V[f])
        t = hits["time"][f].astype(f32)
        pos = O[pix] + t[:, None] * V[f]
        O[pix] = pos + OFFSET * Wd
        PV[pix] = kat.pack_unit_vector(Wd)
        info["bounces"][pix] += 1
        info["refracted"][pix] += refracted
        info["reflected"][pix] += ~refracted
        live = pix
    if trace is not None:
        trace["packed_velocity"] = PV.reshape(H, W)
    return out.reshape(H, W)
