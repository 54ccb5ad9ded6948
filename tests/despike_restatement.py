"""The firefly clamp (DESIGN.md §6 "Firefly clamp (row 12)") restated in numpy
float32, from the definition's text and not from include/pt_despike.h: the two
share the numerics convention only (IEEE binary32, one rounding per operation,
IEEE /).

Every tap of the window is one whole-image array operation; the order
statistic is a sort over the stacked taps, non-members standing at -inf, and
not an insertion.  A sort may leave either of two equal zeros of opposite sign
at the Rank-th place: the definition's `+ Floor` makes that invisible."""
from __future__ import annotations

import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
DEFAULTS = dict(radius=3, rank=3, min_neighbours=8, scale=1.0, floor=0.0, normal_cosine=0.9)


def ok(a):
    """Four finite components and .w > 0."""
    return np.isfinite(a).all(axis=-1) & (a[..., 3] > 0)


def value(a):
    """The largest component of a.xyz / a.w, by comparisons."""
    with np.errstate(all="ignore"):
        c = a[..., :3] / a[..., 3:4]
        v = c[..., 0]
        v = np.where(c[..., 1] > v, c[..., 1], v)
        v = np.where(c[..., 2] > v, c[..., 2], v)
    return v


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
    xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[yd, xd] = a[ys, xs]
    return b


def despike(src, guides, radius, rank, min_neighbours, scale, floor, normal_cosine, detail=False):
    src = np.asarray(src, F)
    H, W = guides.shape
    R, K = int(radius), int(rank)
    scale, floor, cosine = F(scale), F(floor), F(normal_cosine)
    shape, normal = guides["shape"], guides["normal"].astype(F)
    hit = shape != NONE
    usable = ok(src)
    v = value(src)

    # Step 3: the members, tap by tap; the centre is no member of its own window.
    values, m = [], np.zeros((H, W), np.int64)
    shape_cut, normal_cut = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            q_usable = _shift(usable, dy, dx, False)        # False outside the image
            q_shape = _shift(shape, dy, dx, 0)
            qn = _shift(normal, dy, dx, 0)
            with np.errstate(all="ignore"):
                d = (qn[..., 0] * normal[..., 0] + qn[..., 1] * normal[..., 1]) + qn[..., 2] * normal[..., 2]
            same_shape = q_shape == shape
            member = q_usable & same_shape & (~hit | (d >= cosine))
            values.append(np.where(member, _shift(v, dy, dx, 0), F(-np.inf)).astype(F))
            m += member
            shape_cut |= q_usable & ~same_shape
            normal_cut |= q_usable & same_shape & ~member

    # Step 5: the K-th largest of the multiset, the limit.
    ranked = np.sort(np.stack(values), axis=0)
    with np.errstate(all="ignore"):
        t = ranked[-K]
        L = scale * t + floor
        # Steps 4 and 6.
        tested = usable & (m >= min_neighbours)
        clamp = tested & (L >= 0) & (v > L)
        f = L / v
        scaled = src[..., :3] * f[..., None]
    out = src.copy()
    out[clamp, :3] = scaled[clamp]
    if not detail:
        return out
    with np.errstate(all="ignore"):
        floor_deciding = tested & (v > scale * t) & (scale * t >= 0) & ~(v > L)
    return out, dict(m=m, t=t, L=L, v=v, clamped=clamp, unclamped=tested & ~clamp, untested=usable & ~tested,
                     not_usable=~usable, shape_cut=shape_cut & tested, normal_cut=normal_cut & tested,
                     t_inf=tested & np.isposinf(t), zero_clamp=clamp & (t == 0) & (L == 0),
                     floor_deciding=floor_deciding)
