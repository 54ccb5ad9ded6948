"""History validation (DESIGN.md §6 "History validation (row 11)") restated in
numpy float32, from the definition's text and not from include/pt_rectify.h:
the two share the numerics convention only (IEEE binary32, one rounding per
operation, sums in window order, IEEE / and sqrt).

The window is walked tap by tap in row-major order, every tap as one
whole-image array operation, so each pixel's sums take their terms in the
definition's order.  `mutation` breaks one rule on purpose (tests/test_rectify.py
checks that each one is noticed)."""
from __future__ import annotations

import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
DEFAULTS = dict(radius=3, min_neighbours=25, sigma=1.0, clamped_history=8.0, normal_cosine=0.9)
MUTATIONS = ("min-neighbours-le", "column-off-by-one", "sample-variance")


def ok(a):
    """Four finite components and .w > 0."""
    return np.isfinite(a).all(axis=-1) & (a[..., 3] > 0)


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
    xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[yd, xd] = a[ys, xs]
    return b


def rectify(hist, cur, guides, radius, min_neighbours, sigma, clamped_history, normal_cosine, detail=False,
            mutation=None):
    hist, cur = np.asarray(hist, F), np.asarray(cur, F)
    H, W = guides.shape
    R = int(radius)
    sigma, clamped, cosine = F(sigma), F(clamped_history), F(normal_cosine)
    shape, normal = guides["shape"], guides["normal"].astype(F)
    hit = shape != NONE
    cur_ok = ok(cur)
    with np.errstate(all="ignore"):
        colour = cur[..., :3] / cur[..., 3:4]

        # Step 2: the window set, tap by tap.
        taps = []
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                sx = dx + 1 if mutation == "column-off-by-one" else dx
                inside = _shift(np.ones((H, W), bool), dy, sx, False)
                q_ok = _shift(cur_ok, dy, sx, False)
                q_shape = _shift(shape, dy, sx, 0)
                qn = _shift(normal, dy, sx, 0)
                d = (qn[..., 0] * normal[..., 0] + qn[..., 1] * normal[..., 1]) + qn[..., 2] * normal[..., 2]
                surface = (q_shape == shape) & (~hit | (d >= cosine))
                taps.append((inside & q_ok & surface, _shift(colour, dy, sx, 0), inside & q_ok,
                             q_shape == shape))
        m = np.zeros((H, W), np.int64)
        for member, *_ in taps:
            m += member

        # Step 4: the moments, in window order; a sum starts from its first member.
        S, started = np.zeros((H, W, 3), F), np.zeros((H, W), bool)
        for member, c, *_ in taps:
            S = np.where((member & ~started)[..., None], c, np.where(member[..., None], S + c, S))
            started |= member
        mf = np.maximum(m, 1).astype(F)[..., None]
        mu = S / mf
        D, started = np.zeros((H, W, 3), F), np.zeros((H, W), bool)
        for member, c, *_ in taps:
            t = (c - mu) * (c - mu)
            D = np.where((member & ~started)[..., None], t, np.where(member[..., None], D + t, D))
            started |= member
        if mutation == "sample-variance":
            sd = np.sqrt(D / np.maximum(m - 1, 1).astype(F)[..., None])
        else:
            sd = np.sqrt(D / mf)
        finite = np.isfinite(mu).all(axis=-1) & np.isfinite(sd).all(axis=-1)

        # Step 5: the clip.
        n = hist[..., 3:4]
        h = hist[..., :3] / n
        e = sigma * sd
        lo, hi = mu - e, mu + e
        t = np.where(h < lo, lo, h)              # min(max(h, lo), hi); h stays where it equals a bound
        hc = np.where(t > hi, hi, t)
        moved = ~(hc == h).all(axis=-1)
        nc = np.fmin(n, clamped)
        clipped = np.concatenate([hc * nc, nc], axis=-1).astype(F)

    # Step 3 and the order of the exits.
    hist_ok = ok(hist)
    few = m <= min_neighbours if mutation == "min-neighbours-le" else m < min_neighbours
    untested = hist_ok & few
    unstable = hist_ok & ~few & ~finite
    clip = hist_ok & ~few & finite & moved
    out = hist.copy()
    out[~hist_ok] = 0
    out[clip] = clipped[clip]
    if not detail:
        return out
    shape_cut = np.zeros((H, W), bool)
    normal_cut = np.zeros((H, W), bool)
    for member, _, usable, same_shape in taps:
        shape_cut |= usable & ~same_shape
        normal_cut |= usable & same_shape & ~member
    with np.errstate(all="ignore"):
        low = clip & (hc > h).any(axis=-1)
        high = clip & (hc < h).any(axis=-1)
    return out, dict(mu=mu, lo=lo, hi=hi, m=m, no_history=~hist_ok, untested=untested, unstable=unstable, clipped=clip, low=low, high=high,
                     unclipped=hist_ok & ~few & finite & ~moved,
                     centre_through_neighbours=hist_ok & ~few & ~cur_ok, shape_cut=shape_cut & ~few & hist_ok,
                     normal_cut=normal_cut & ~few & hist_ok,
                     count_cut=clip & (hist[..., 3] > clamped), count_kept=clip & (hist[..., 3] <= clamped))
