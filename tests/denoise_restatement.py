"""A numpy float32 restatement of the denoiser, written from
the definition apart from csrc/scene/denoise.cpp and csrc/hip/denoise.hip
(test infrastructure only; tests/test_denoise.py, tests/test_gpu_denoise.py):

  denoise        the edge-avoiding a-trous filter: c_0 = xyz / w, then per
                 iteration i (step s = 2^i, colour sigma SigmaColor * 2^-i)
                 the 5x5 taps q = p + s (dx, dy), dy outer, dx inner; a tap
                 outside the image, empty or of another shape is skipped;
                 w = k[dx+2] k[dy+2] exp(-(((dc + da) + dn) + dz)); the three
                 channel sums and the weight sum accumulate in tap order.
  central_ray    GenerateCameraRay (scene.glsl.inc:613-655) at the pixel
                 centre through the lens centre, for the pinhole, thin-lens
                 and 360 models, with the integrator's packed velocity.
  guides         the guide records of a frame: Trace() of the central rays
                 (the oracle's ray query), the hit record's unpacked normal,
                 time and shape, the preview's base colour.

Numerics: DESIGN.md §2's convention in numpy float32 (nothing fused, sums
left to right); exp is the convention's own (the oracle's exported pt_exp),
min / max are IEEE minNum / maxNum (np.fmax)."""
from __future__ import annotations

import numpy as np

import kat
import oracle_lib
import path_restatement as pr
import preview_restatement as pvr

f32 = np.float32
NONE = 0xFFFFFFFF
K = [f32(1.0 / 16.0), f32(1.0 / 4.0), f32(3.0 / 8.0), f32(1.0 / 4.0), f32(1.0 / 16.0)]
GUIDE_DTYPE = np.dtype([("normal", "<f4", (3,)), ("time", "<f4"), ("albedo", "<f4", (3,)), ("shape", "<u4")])


def _exp(x):
    fn = oracle_lib.lib().oracle_fp_exp
    return np.array([fn(float(v)) for v in x.reshape(-1)], f32).reshape(x.shape)


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(accum, guides, iterations=5, sigma_color=1.0, sigma_normal=1.0, sigma_depth=1.0, sigma_albedo=1.0,
            return_all=False):
    """(H, W, 4) float32: the denoised mean and 1, zeros where empty.
    return_all: the list of results for Iterations = 0 .. iterations (an
    iteration's constants depend on its index only, so the chain is shared)."""
    with np.errstate(all="ignore"):
        out = _denoise(np.asarray(accum, f32), np.asarray(guides), iterations, f32(sigma_color), f32(sigma_normal),
                       f32(sigma_depth), f32(sigma_albedo))
    return out if return_all else out[-1]


def _image(c, valid):
    img = np.zeros(c.shape[:2] + (4,), f32)
    img[..., :3] = np.where(valid[..., None], c, f32(0.0))
    img[..., 3] = np.where(valid, f32(1.0), f32(0.0))
    return img


def _denoise(a, g, iterations, s_color, s_normal, s_depth, s_albedo):
    H, W = a.shape[:2]
    valid = a[..., 3] > 0
    c = np.zeros((H, W, 3), f32)
    c[valid] = a[valid][:, :3] / a[valid][:, 3:4]
    n, t, alb, shape = g["normal"].astype(f32), g["time"].astype(f32), g["albedo"].astype(f32), g["shape"]
    hit = shape != NONE
    ys, xs = np.mgrid[0:H, 0:W]
    results = [_image(c, valid)]
    for i in range(iterations):
        s = 1 << i
        sc = s_color * f32(2.0 ** -i)
        sc2 = sc * sc
        sa2 = s_albedo * s_albedo
        sums = np.zeros((H, W, 3), f32)
        sw = np.zeros((H, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                ok = valid & inside & valid[qyc, qxc] & (shape[qyc, qxc] == shape)
                if not ok.any():
                    continue
                py, px = ys[ok], xs[ok]
                ty, tx = qyc[ok], qxc[ok]
                cp, cq = c[py, px], c[ty, tx]
                dc = _dist2(cp, cq) / sc2
                da = _dist2(alb[py, px], alb[ty, tx]) / sa2
                np_, nq = n[py, px], n[ty, tx]
                d = (np_[:, 0] * nq[:, 0] + np_[:, 1] * nq[:, 1]) + np_[:, 2] * nq[:, 2]
                dn = np.fmax(f32(0.0), f32(1.0) - d) / s_normal
                tp, tq = t[py, px], t[ty, tx]
                dz = np.abs(tp - tq) / (s_depth * np.fmax(tp, f32(1e-6)))
                h_ = hit[py, px]
                dn = np.where(h_, dn, f32(0.0)).astype(f32)
                dz = np.where(h_, dz, f32(0.0)).astype(f32)
                w = (K[dx + 2] * K[dy + 2]) * _exp(-(((dc + da) + dn) + dz))
                sums[py, px] = sums[py, px] + w[:, None] * cq
                sw[py, px] = sw[py, px] + w
        c = np.where(valid[..., None], sums / sw[..., None], f32(0.0)).astype(f32)
        results.append(_image(c, valid))
    return results


# --- guides -----------------------------------------------------------------------

def central_ray(cam, x, y, W, H):
    """(origin [3], packed velocity) of the pixel's central camera ray."""
    half = f32(0.5)
    sx, sy = f32(x) + half, f32(y) + half
    nx, ny = sx / f32(W), sy / f32(H)
    model = int(cam["Model"])
    size = cam["SensorSize"].astype(f32)
    zero = f32(0.0)
    o = [zero, zero, zero]
    with np.errstate(all="ignore"):
        if model in (0, 1):
            sp = [-size[0] * (nx - half), -size[1] * (half - ny), f32(cam["SensorDistance"])]
            if model == 0:
                v = pr._normalize([o[k] - sp[k] for k in range(3)])
            else:
                fl = f32(cam["FocalLength"])
                den = sp[2] - fl
                op = [(-sp[k] * fl) / den for k in range(3)]
                v = pr._normalize([op[k] - o[k] for k in range(3)])
        elif model == 2:
            phi = (nx - half) * pr.TAU
            theta = (half - ny) * pr.PI
            ct, st = pr._fp("cos", theta), pr._fp("sin", theta)
            v = [ct * pr._fp("sin", phi), st, -ct * pr._fp("cos", phi)]
        else:
            return None
        to = cam["Transform"]["To"].astype(f32).reshape(16)
        O = pr._mat_vec(to, o, 1.0)
        V = pr._mat_vec(to, v, 0.0)
    return O, int(kat.pack_unit_vector(np.array([V], f32))[0])


def guides(scene, camera, W, H):
    """(H, W) guide records of packed camera `camera`."""
    cam = scene.arrays()["cameras"][camera]
    world = pr.World(scene)
    out = np.zeros((H, W), GUIDE_DTYPE)
    out["shape"] = NONE
    rays = [[central_ray(cam, x, y, W, H) for x in range(W)] for y in range(H)]
    if rays[0][0] is None:
        return out
    origins = np.array([r[0] for row in rays for r in row], f32)
    packed = np.array([r[1] for row in rays for r in row], np.uint32)
    hits = oracle_lib.trace_rays(scene.packs(), origins, packed, np.full(len(packed), pr.HIT_TIME_LIMIT, f32))
    hits = hits.reshape(H, W)
    velocities = kat.unpack_unit_vector(packed).reshape(H, W, 3)
    normals = kat.unpack_unit_vector(hits["packed_normal"].reshape(-1)).reshape(H, W, 3)
    flat = {}   # base colour of a material without a base texture
    for y in range(H):
        for x in range(W):
            h = hits[y, x]
            sm = int(h["shape_material"])
            if sm == NONE:
                sky = pvr.observe_d65(world.sky_spectrum([f32(c) for c in velocities[y, x]]))
                out["albedo"][y, x] = pvr._mat3(pvr.XYZ_TO_SRGB, sky)
                continue
            m = sm & 0xFFFF
            typ = int(world.mat[32 * m])
            textured = typ in (0, 1) and int(world.mat[32 * m + 4]) != NONE
            if textured:
                col = pvr.base_color(world, m, [f32(h["u"]), f32(h["v"])])
            else:
                if m not in flat:
                    flat[m] = pvr.base_color(world, m, [f32(0.0), f32(0.0)])
                col = flat[m]
            out["normal"][y, x] = normals[y, x]
            out["time"][y, x] = h["time"]
            out["albedo"][y, x] = pvr._mat3(pvr.XYZ_TO_SRGB, col)
            out["shape"][y, x] = sm >> 16
    return out
