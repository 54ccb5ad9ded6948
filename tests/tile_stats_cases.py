"""Accumulators shared by the per-tile statistics tests (tests/test_tile_stats.py
on the CPU, tests/test_gpu_tile_stats.py on the device), for any size from
1 x 1 up: random frames, empty frames, and frames with NaN / inf / denormal /
negative-w pixels scattered over the tiles; second halves for the pair mode
with pixels whose relative half-difference is exactly 0 and exactly 1, so
that `r > threshold` and `r >= threshold` part at the thresholds 0 and 1."""
from __future__ import annotations

import numpy as np

F = np.float32
# One tile; one tile exactly; a second tile of one column / one row; 3 x 2
# tiles with 1-wide and 15-high edge tiles; 5 x 3 tiles with odd edges.
SIZES = [(1, 1), (16, 16), (17, 16), (16, 17), (33, 31), (67, 45)]
THRESHOLDS = [0.0, 0.1, 1.0, float("inf")]

NAN, INF = F(np.nan), F(np.inf)

SPECIAL = np.array([
    (NAN, 1, 1, 1), (1, NAN, 1, 1), (1, 1, 1, NAN),            # NaN in a component
    (1, INF, 1, 1), (-INF, 1, 1, 1), (1, 1, 1, INF),           # infinities
    (1, 1, 1, 0), (1, 1, 1, -0.0), (1, 1, 1, -2), (1, 1, 1, -1e-40),   # w = 0, -0, negative: empty
    (1, 1e-40, 1, 1), (1, 1, 1, 1e-40), (1, 1e-45, 1, 1e-45),  # denormal y, denormal w (filled: w > 0)
    (1, 3e38, 1, 1e-3),                                        # y / w overflows
    (1, -2, 1, 4), (1, 0, 1, 4),                               # dark but filled
    (1, 2, 3, 2.5), (1, 2, 3, 1e-3), (1, 2, 3, 1e3),           # the min / max of the counts
], F)


def random_frame(W, H, seed=0):
    """XYZ sums of w samples each, w an integer 1..64; one pixel in seven empty."""
    rng = np.random.default_rng(1000 + seed)
    w = rng.integers(1, 65, (H, W)).astype(F)
    a = np.empty((H, W, 4), F)
    a[..., :3] = rng.uniform(0.0, 2.0, (H, W, 3)).astype(F) * w[..., None]
    a[..., 3] = w
    a[rng.uniform(size=(H, W)) < 1.0 / 7.0] = 0
    return a


def scatter(a, pixels, seed):
    """`pixels` planted at distinct random positions (as many as fit)."""
    flat = a.reshape(-1, 4)
    rng = np.random.default_rng(2000 + seed)
    n = min(len(pixels), len(flat))
    flat[rng.choice(len(flat), n, replace=False)] = pixels[rng.permutation(len(pixels))[:n]]
    return a


def special(W, H, seed=0):
    return scatter(random_frame(W, H, seed), SPECIAL, seed)


def empty(W, H):
    return np.zeros((H, W, 4), F)


def pair(W, H, seed=0):
    """(A, B): two draws with their own special pixels, then pairs of pixels
    with r = 0 (equal halves), r = 1 (Y_B = 0), Y_A + Y_B = 0 (skipped), a sum
    that is not finite although the halves are, and filled in one half only."""
    a, b = special(W, H, seed), special(W, H, seed + 50)
    fa, fb = a.reshape(-1, 4), b.reshape(-1, 4)
    planted = [
        ((1.5, 1.5, 1.5, 1.5), (1.5, 1.5, 1.5, 1.5)),          # r = 0
        ((1, 3, 1, 2), (1, 0, 1, 2)),                          # r = 1
        ((1, 0, 1, 2), (1, 5, 1, 4)),                          # r = 1
        ((1, 2, 1, 4), (1, -1, 1, 2)),                         # Y_A + Y_B = 0: no pair pixel
        ((1, 3e38, 1, 4), (1, 3e38, 1, 4)),                    # a pair pixel whose sum is not finite
        ((1, 1, 1, 1), (0, 0, 0, 0)), ((0, 0, 0, 0), (1, 1, 1, 1)),   # filled in one half
        ((2, 2, 2, 2), (2, 2, 2, 2)),                          # r = 0
    ]
    rng = np.random.default_rng(3000 + seed)
    n = min(len(planted), len(fa))
    for k, i in zip(rng.permutation(len(planted))[:n], rng.choice(len(fa), n, replace=False)):
        fa[i], fb[i] = planted[k]
    return a, b


def cases(W, H):
    """{name: (A, B or None)} for one size."""
    a, b = pair(W, H, seed=W + H)
    c, d = pair(W, H, seed=W + H + 1)
    return {
        "random": (random_frame(W, H, W), None),
        "empty": (empty(W, H), None),
        "special": (special(W, H, W + 7), None),
        "pair": (a, b),
        "pair-2": (c, d),
        "pair-random": (random_frame(W, H, W), random_frame(W, H, W + 1)),
        "pair-empty": (empty(W, H), empty(W, H)),
    }
