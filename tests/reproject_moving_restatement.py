"""A numpy float32 restatement of the moving-shape reprojection (DESIGN.md §6
row 9), written from the definition apart from include/pt_reproject.h and
csrc/scene/reproject.cpp (test infrastructure only;
tests/test_reproject_moving.py, tests/test_gpu_reproject_moving.py).  It
reuses reproject_restatement's unchanged steps: the rays, the projection, the
matrix product and the whole of row 8 for the pixels that take row 8's path.

The motion table, shape i of the current pack against shape i of the previous:

  - i beyond the previous array, another Type or MeshRootNodeIndex, or a
    non-finite value in either Transform: Flags = 2 (no history), zeros;
  - the two Transform records bytewise equal: Flags = 0, identities;
  - otherwise Flags = 1 (moved), Point = rows 0..2 of To_prev From_cur,
    Normal = the transpose of the linear part of To_cur From_prev; every
    product summed left to right.

The reprojection, per pixel, with s the guide's shape:

  - a miss: row 8;
  - s >= the table's length, or a record with bit 2: no history;
  - a record with bit 1 (and not bit 2): moved, below;
  - any other record: row 8.

Moved: P as in row 8; Pp = Point (P, 1); L = From_prev (Pp, 1); dist =
|Pp - origin_prev|; Ne = Normal n / sqrt(|Normal n|^2), no history unless that
squared length is > 0 and finite; taps as in row 8 with dot(n_prev, Ne) in the
normal rule."""
from __future__ import annotations

import numpy as np

import reproject_restatement as rr

f32 = np.float32
NONE = 0xFFFFFFFF
MOVED, NO_HISTORY = 1, 2
MOTION_DTYPE = np.dtype([("Point", "<f4", (12,)), ("Normal", "<f4", (9,)), ("Flags", "<u4"), ("Pad0", "<u4", (2,))])


def shape_motion(prev_shapes, shapes):
    out = np.zeros(len(shapes), MOTION_DTYPE)
    for i, c in enumerate(shapes):
        m = out[i]
        if i >= len(prev_shapes):
            m["Flags"] = NO_HISTORY
            continue
        p = prev_shapes[i]
        values = np.concatenate([p["Transform"]["To"], p["Transform"]["From"], c["Transform"]["To"],
                                 c["Transform"]["From"]])
        if (int(p["Type"]) != int(c["Type"]) or int(p["MeshRootNodeIndex"]) != int(c["MeshRootNodeIndex"])
                or not np.isfinite(values).all()):
            m["Flags"] = NO_HISTORY
            continue
        if p["Transform"].tobytes() == c["Transform"].tobytes():
            m["Point"][[0, 5, 10]] = 1
            m["Normal"][[0, 4, 8]] = 1
            continue
        m["Flags"] = MOVED
        Tp, Fp = p["Transform"]["To"].astype(f32), p["Transform"]["From"].astype(f32)
        Tc, Fc = c["Transform"]["To"].astype(f32), c["Transform"]["From"].astype(f32)
        with np.errstate(all="ignore"):
            for r in range(3):
                for k in range(4):
                    m["Point"][4 * r + k] = (((Tp[r] * Fc[4 * k] + Tp[4 + r] * Fc[4 * k + 1])
                                              + Tp[8 + r] * Fc[4 * k + 2]) + Tp[12 + r] * Fc[4 * k + 3])
            for i_ in range(3):
                for j in range(3):
                    b = (Tc[i_] * Fp[4 * j] + Tc[4 + i_] * Fp[4 * j + 1]) + Tc[8 + i_] * Fp[4 * j + 2]
                    m["Normal"][3 * j + i_] = b            # Normal[3r + c] = B[c][r]
    return out


def kinds(guides, motion):
    """(static, moved, none) masks of the current pixels, and each pixel's record index (0 where it has none)."""
    shape = guides["shape"]
    hit = shape != NONE
    n = len(motion)
    inside = hit & (shape < n)
    idx = np.where(inside, shape, 0).astype(np.int64)
    flags = motion["Flags"][idx] if n else np.zeros(shape.shape, np.uint32)
    none = hit & (~inside | ((flags & NO_HISTORY) != 0))
    moved = inside & ((flags & NO_HISTORY) == 0) & ((flags & MOVED) != 0)
    return ~none & ~moved, moved, none, idx


def _moved(prev_accum, prev_guides, prev_cam, guides, cam, point, normal, nc, dt, mw, mh):
    """Every pixel treated as a hit of a moved shape with its own (H, W, 12)
    Point and (H, W, 9) Normal.  Returns (out, valid (4, H, W), (x0, y0) of the first tap)."""
    hp_, wp_ = prev_accum.shape[:2]
    H, W = guides.shape
    out = np.zeros((H, W, 4), f32)
    valid = np.zeros((4, H, W), bool)
    if not (rr.camera_ok(cam) and rr.camera_ok(prev_cam)):
        return out, valid, (np.zeros((H, W), np.int64), np.zeros((H, W), np.int64))
    O, V = rr.rays(cam, W, H)
    t = guides["time"].astype(f32)
    frm = prev_cam["Transform"]["From"].astype(f32).reshape(16)
    to = prev_cam["Transform"]["To"].astype(f32).reshape(16)
    zero, one = f32(0.0), f32(1.0)
    with np.errstate(all="ignore"):
        P = [O[k] + V[..., k] * t for k in range(3)]
        Pp = [((point[..., 4 * r] * P[0] + point[..., 4 * r + 1] * P[1]) + point[..., 4 * r + 2] * P[2])
              + point[..., 4 * r + 3] for r in range(3)]
        L = [np.asarray(c, f32) for c in rr._apply(frm, Pp, 1.0)]
        Op = rr._apply(to, [zero, zero, zero], 1.0)
        d = [Pp[k] - Op[k] for k in range(3)]
        dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(f32)
        n = guides["normal"].astype(f32)
        Nv = [(normal[..., 3 * r] * n[..., 0] + normal[..., 3 * r + 1] * n[..., 1]) + normal[..., 3 * r + 2] * n[..., 2]
              for r in range(3)]
        q = ((Nv[0] * Nv[0] + Nv[1] * Nv[1]) + Nv[2] * Nv[2]).astype(f32)
        normal_ok = (q > 0) & np.isfinite(q)
        s = one / np.sqrt(q)
        Ne = [(Nv[k] * s).astype(f32) for k in range(3)]
        front, nx, ny = rr.project(prev_cam, L)
        u = (nx * f32(wp_) - f32(0.5)).astype(f32)
        v = (ny * f32(hp_) - f32(0.5)).astype(f32)
        located = front & normal_ok & (u > -1) & (u < f32(wp_)) & (v > -1) & (v < f32(hp_))
        u, v = np.where(located, u, zero).astype(f32), np.where(located, v, zero).astype(f32)
        fu, fv = np.floor(u), np.floor(v)
        x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
        fx, fy = u - fu, v - fv
        sums = [np.zeros((H, W), f32) for _ in range(5)]
        for i in range(4):
            qx, qy = x0 + (i & 1), y0 + (i >> 1)
            inside = (qx >= 0) & (qx < wp_) & (qy >= 0) & (qy < hp_)
            cx, cy = np.clip(qx, 0, wp_ - 1), np.clip(qy, 0, hp_ - 1)
            h = prev_accum[cy, cx]
            g = prev_guides[cy, cx]
            history = np.isfinite(h).all(axis=-1) & (h[..., 3] > 0)
            same = g["shape"] == guides["shape"]
            gn = g["normal"].astype(f32)
            dot = (gn[..., 0] * Ne[0] + gn[..., 1] * Ne[1]) + gn[..., 2] * Ne[2]
            depth = np.abs(g["time"].astype(f32) - dist) <= dt * dist
            ok = located & inside & history & same & (dot >= nc) & depth
            valid[i] = ok
            w = ((fx if i & 1 else one - fx) * (fy if i >> 1 else one - fy)).astype(f32)
            hw = h[..., 3]
            terms = [w * (h[..., 0] / hw), w * (h[..., 1] / hw), w * (h[..., 2] / hw), w * hw, w]
            for k in range(5):
                sums[k] = np.where(ok, sums[k] + terms[k], sums[k]).astype(f32)
        sx, sy, sz, sn, sw = sums
        have = sw >= mw
        cnt = np.fmin(sn / sw, mh)
        for k, c in enumerate((sx, sy, sz)):
            out[..., k] = np.where(have, (c / sw) * cnt, zero)
        out[..., 3] = np.where(have, cnt, zero)
    return out, valid, (x0, y0)


def reproject_moving(prev_accum, prev_guides, prev_cam, guides, cam, motion, normal_cosine=0.9, depth_tolerance=0.02,
                     min_weight=0.25, max_history=64.0, detail=False):
    """(H, W, 4) float32.  motion None: row 8.  detail: also a dict with the
    masks `static`, `moved`, `none` and `valid` (4, H, W): tap i of a moved
    pixel passes every rule, and `x0`, `y0`, a moved pixel's first tap."""
    prev_accum = np.asarray(prev_accum, f32)
    base = rr.reproject(prev_accum, prev_guides, prev_cam, guides, cam, normal_cosine, depth_tolerance, min_weight,
                        max_history)
    H, W = guides.shape
    if motion is None:
        everything = np.ones((H, W), bool)
        d = dict(static=everything, moved=~everything, none=~everything, valid=np.zeros((4, H, W), bool),
                 x0=np.zeros((H, W), np.int64), y0=np.zeros((H, W), np.int64))
        return (base, d) if detail else base
    motion = np.asarray(motion, MOTION_DTYPE).reshape(-1)
    static, moved, none, idx = kinds(guides, motion)
    out = base.copy()
    out[none] = 0
    valid = np.zeros((4, H, W), bool)
    x0 = y0 = np.zeros((H, W), np.int64)
    if moved.any():
        mv, valid, (x0, y0) = _moved(prev_accum, prev_guides, prev_cam, guides, cam, motion["Point"][idx].astype(f32),
                              motion["Normal"][idx].astype(f32), f32(normal_cosine), f32(depth_tolerance),
                              f32(min_weight), f32(max_history))
        out[moved] = mv[moved]
        valid = valid & moved[None]
    if not detail:
        return out
    return out, dict(static=static, moved=moved, none=none, valid=valid, x0=x0, y0=y0)
