"""A numpy float32 restatement of temporal reprojection,
written from the definition apart from include/pt_reproject.h (test
infrastructure only; tests/test_reproject.py, tests/test_gpu_reproject.py).
It reuses only denoise_restatement.central_ray, kat's unit-vector unpacking
and path_restatement's _fp (the convention's own atan2 / asin).

For every pixel (x, y) of the current w x h view:

  1  (O, V): the central camera ray of the current camera (central_ray, the
     velocity unpacked from its packed form).  No history for an unknown
     model or a thin lens whose sensor is not behind the focal plane (either
     camera).
  2  hit: P = O + V time, per component; miss: the direction V alone.
  3  L = From_prev (P, 1) or From_prev (V, 0).  Pinhole / thin lens: L.z < 0
     or no history; k = SensorDistance / -L.z, Nx = (L.x k) / SensorSize.x +
     0.5, Ny = 0.5 - (L.y k) / SensorSize.y.  360: Phi = atan2(L.x, -L.z),
     Theta = asin(L.y / |L|), Nx = Phi / TAU + 0.5, Ny = 0.5 - Theta / PI.
     u = Nx wp - 0.5, v = Ny hp - 0.5; outside (-1, wp) x (-1, hp), NaN
     included, no tap can lie in the image: no history.
  4  taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with x0 = floor(u),
     y0 = floor(v), weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  Valid:
     inside the previous image; four finite history components and w > 0;
     the same shape; on hits, dot(normals) >= NormalCosine and
     |time_prev - dist| <= DepthTolerance dist, dist = |P - origin_prev|.
  5  Wsum < MinWeight: zeros; else mean = sum w (xyz / w_hist) / Wsum, n =
     min(sum w w_hist / Wsum, MaxHistory), result (mean n, n).

Sums run in tap order, left to right; nothing is fused."""
from __future__ import annotations

import numpy as np

import denoise_restatement as dr
import kat
import path_restatement as pr

f32 = np.float32
NONE = 0xFFFFFFFF
# The starting values the definition came with; the cases of reproject_cases.py are built around them.
DEFAULTS = dict(normal_cosine=0.9, depth_tolerance=0.02, min_weight=0.25, max_history=64.0)
RULES = ("frame", "history", "shape", "normal", "depth")


def _apply(m, v, w):
    """Column-major 4x4 times (v, w), rows 0..2, summed left to right."""
    w = f32(w)
    return [((m[r] * v[0] + m[4 + r] * v[1]) + m[8 + r] * v[2]) + m[12 + r] * w for r in range(3)]


def camera_ok(cam):
    model = int(cam["Model"])
    if model in (0, 2):
        return True
    if model == 1:
        return bool(f32(cam["SensorDistance"]) > f32(cam["FocalLength"]))
    return False


def rays(cam, W, H):
    """(origin [3] of float32, velocities (H, W, 3)) of the view's central rays."""
    packed = np.zeros((H, W), np.uint32)
    origin = None
    for y in range(H):
        for x in range(W):
            origin, packed[y, x] = dr.central_ray(cam, x, y, W, H)
    return [f32(c) for c in origin], kat.unpack_unit_vector(packed.reshape(-1)).reshape(H, W, 3)


def project(cam, L):
    """(front, Nx, Ny) of camera-space points or directions L = [x, y, z] arrays."""
    half = f32(0.5)
    with np.errstate(all="ignore"):
        if int(cam["Model"]) == 2:
            length = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
            s = (L[1] / length).astype(f32)
            phi = np.array([pr._fp("atan2", a, b) for a, b in zip(L[0].reshape(-1), (-L[2]).reshape(-1))], f32)
            theta = np.array([pr._fp("asin", a) for a in s.reshape(-1)], f32)
            phi, theta = phi.reshape(L[0].shape), theta.reshape(L[0].shape)
            return np.ones(L[0].shape, bool), phi / pr.TAU + half, half - theta / pr.PI
        front = L[2] < 0
        size = cam["SensorSize"].astype(f32)
        k = f32(cam["SensorDistance"]) / -L[2]
        return front, (L[0] * k) / size[0] + half, half - (L[1] * k) / size[1]


def locate(prev_cam, cam, guides, wp, hp):
    """Steps 1-3: dict of located (H, W) bool, behind (the previous camera),
    u, v, dist."""
    H, W = guides.shape
    no = dict(located=np.zeros((H, W), bool), behind=np.zeros((H, W), bool), u=np.zeros((H, W), f32),
              v=np.zeros((H, W), f32), dist=np.zeros((H, W), f32))
    if not (camera_ok(cam) and camera_ok(prev_cam)):
        return no
    O, V = rays(cam, W, H)
    hit = guides["shape"] != NONE
    t = guides["time"].astype(f32)
    frm = prev_cam["Transform"]["From"].astype(f32).reshape(16)
    to = prev_cam["Transform"]["To"].astype(f32).reshape(16)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        P = [O[k] + V[..., k] * t for k in range(3)]
        Lh = _apply(frm, P, 1.0)
        Lm = _apply(frm, [V[..., k] for k in range(3)], 0.0)
        L = [np.where(hit, Lh[k], Lm[k]).astype(f32) for k in range(3)]
        Op = _apply(to, [zero, zero, zero], 1.0)
        d = [P[k] - Op[k] for k in range(3)]
        dist = np.where(hit, np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), zero).astype(f32)
        front, nx, ny = project(prev_cam, L)
        u = (nx * f32(wp) - f32(0.5)).astype(f32)
        v = (ny * f32(hp) - f32(0.5)).astype(f32)
        inside = (u > -1) & (u < f32(wp)) & (v > -1) & (v < f32(hp))
    return dict(located=front & inside, behind=~front, u=u, v=v, dist=dist)


def reproject(prev_accum, prev_guides, prev_cam, guides, cam, normal_cosine=0.9, depth_tolerance=0.02,
              min_weight=0.25, max_history=64.0, detail=False):
    """(H, W, 4) float32.  detail: also a dict with, per rule of RULES, a
    (4, H, W) bool array "tap i passes the rule" (evaluated wherever the pixel
    is located, whatever the other rules say; out-of-frame taps are judged on
    the nearest pixel of the image), `located`, `behind` and `wsum`."""
    prev_accum = np.asarray(prev_accum, f32)
    hp_, wp_ = prev_accum.shape[:2]
    H, W = guides.shape
    nc, dt, mw, mh = f32(normal_cosine), f32(depth_tolerance), f32(min_weight), f32(max_history)
    loc = locate(prev_cam, cam, guides, wp_, hp_)
    located, dist = loc["located"], loc["dist"]
    with np.errstate(all="ignore"):
        u = np.where(located, loc["u"], f32(0.0)).astype(f32)
        v = np.where(located, loc["v"], f32(0.0)).astype(f32)
        fu, fv = np.floor(u), np.floor(v)
        x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
        fx, fy = u - fu, v - fv
        one = f32(1.0)
        hit = guides["shape"] != NONE
        nrm = guides["normal"].astype(f32)
        sums = [np.zeros((H, W), f32) for _ in range(5)]        # x, y, z, n, w
        passes = {r: np.zeros((4, H, W), bool) for r in RULES}
        for i in range(4):
            qx, qy = x0 + (i & 1), y0 + (i >> 1)
            inside = (qx >= 0) & (qx < wp_) & (qy >= 0) & (qy < hp_)
            cx, cy = np.clip(qx, 0, wp_ - 1), np.clip(qy, 0, hp_ - 1)
            h = prev_accum[cy, cx]
            g = prev_guides[cy, cx]
            history = np.isfinite(h).all(axis=-1) & (h[..., 3] > 0)
            shape = g["shape"] == guides["shape"]
            gn = g["normal"].astype(f32)
            dot = (gn[..., 0] * nrm[..., 0] + gn[..., 1] * nrm[..., 1]) + gn[..., 2] * nrm[..., 2]
            normal = ~hit | (dot >= nc)
            depth = ~hit | (np.abs(g["time"].astype(f32) - dist) <= dt * dist)
            for r, ok in zip(RULES, (inside, history, shape, normal, depth)):
                passes[r][i] = ok
            ok = located & inside & history & shape & normal & depth
            w = ((fx if i & 1 else one - fx) * (fy if i >> 1 else one - fy)).astype(f32)
            hw = h[..., 3]
            terms = [w * (h[..., 0] / hw), w * (h[..., 1] / hw), w * (h[..., 2] / hw), w * hw, w]
            for k in range(5):
                sums[k] = np.where(ok, sums[k] + terms[k], sums[k]).astype(f32)
        sx, sy, sz, sn, sw = sums
        have = sw >= mw
        n = np.fmin(sn / sw, mh)
        out = np.zeros((H, W, 4), f32)
        for k, s in enumerate((sx, sy, sz)):
            out[..., k] = np.where(have, (s / sw) * n, f32(0.0))
        out[..., 3] = np.where(have, n, f32(0.0))
    if not detail:
        return out
    return out, dict(passes, located=located, behind=loc["behind"], wsum=sw)
