"""Crafted accumulators shared by the frame-statistics tests
(tests/test_stats.py on the CPU, tests/test_gpu_stats.py on the device):
denoise_cases.accumulators with one pixel planted for every rule of the
definition, a constant and an empty image, and second
halves for the pair mode."""
from __future__ import annotations

import numpy as np

import denoise_cases as dc

F = np.float32
# 40x24; 67x45: a pixel count that is no multiple of 256; 1030x517: 532,510
# pixels, more than the statistics kernel's whole grid covers in one step
# (256 CUs x 1 block x 1024 threads x 2 pixels = 524,288), so its loop runs
# a second time in some blocks and not in others.
SIZES = [(40, 24), (67, 45)]
LARGE = (1030, 517)

NAN, INF = F(np.nan), F(np.inf)
BELOW = lambda v: np.nextafter(F(v), F(0))     # noqa: E731  the float32 just below v


def planted():
    """(x, y, z, w) of every special pixel.  w = 4 and y = 4 Y where Y must be
    exact (a power-of-two scale cannot round)."""
    px = [
        (1, 1, 1, 0), (1, 1, 1, -2),                                       # w = 0, w < 0: empty
        (NAN, 1, 1, 1), (1, NAN, 1, 1), (1, 1, NAN, 1), (1, 1, 1, NAN),    # NaN in each component
        (1, INF, 1, 1), (-INF, 1, 1, 1), (1, 1, 1, INF), (1, 1, INF, 0),   # +inf, -inf (also in an "empty" pixel)
        (1, -2, 1, 4), (1, 0, 1, 4), (1, -0.0, 1, 4),                      # Y < 0, Y = 0, Y = -0: dark
        (1, 3e38, 1, 1e-3),                                                # y / w overflows to +inf: bin 255
        (1, 1e-38, 1, 1e3), (1, 1.5e-45, 1, 1),                            # denormal Y: bin 0
        (1, 2, 3, 2.5), (0.3, 0.7, 0.1, 0.37),                             # non-integer w
    ]
    for k in (-31, -3, 0, 5, 31):                                          # Y exactly at bin edges
        for m in (1.0, 1.25, 1.5, 1.75):
            px.append((1, 4 * m * 2.0 ** k, 1, 4))
        px.append((1, 4 * float(BELOW(2.0 ** k)), 1, 4))                   # and just below one
    for v in (2.0 ** 32, 2.0 ** -32):                                      # the ends of the binned range
        px.append((1, 4 * v, 1, 4))
        px.append((1, 4 * float(BELOW(v)), 1, 4))
    px.append((1, 4 * 2.0 ** 40, 1, 4))                                    # far above: bin 255
    return np.array(px, F)


def crafted(W, H, seed=0):
    """denoise_cases.accumulators (random XYZ sums and counts, empty pixels,
    negative and x1e6 sums) with the planted pixels from row 3 on."""
    a = dc.accumulators(W, H, seed)
    p = planted()
    assert 3 * W + len(p) <= 7 * W
    a.reshape(-1, 4)[3 * W:3 * W + len(p)] = p
    return a


def constant(W, H, value=(0.5, 0.25, 0.125, 2.0)):
    a = np.empty((H, W, 4), F)
    a[...] = np.array(value, F)
    return a


def empty(W, H):
    return np.zeros((H, W, 4), F)


def pair(W, H, seed=0):
    """(A, B): A = crafted; B an independent draw with its own empty pixels,
    then pixels equal to A (r = 0), pixels with Y_A + Y_B <= 0, and sums that
    are not finite although both halves are."""
    a = crafted(W, H, seed)
    b = dc.accumulators(W, H, seed + 100)
    fa, fb = a.reshape(-1, 4), b.reshape(-1, 4)
    k = 8 * W                                       # rows 8 and 9: clear of the planted block
    fa[k:k + 6] = F(1.5)                            # filled, so that the copy below is a pair pixel
    fb[k:k + 6] = fa[k:k + 6]                       # equal halves: r = 0
    fa[k + 6], fb[k + 6] = (1, -2, 1, 4), (1, -1, 1, 2)          # Y_A + Y_B < 0: skipped
    fa[k + 7], fb[k + 7] = (1, 2, 1, 4), (1, -1, 1, 2)           # Y_A + Y_B = 0: skipped
    fa[k + 8], fb[k + 8] = (1, 3e38, 1, 4), (1, 3e38, 1, 4)      # finite halves, y overflows in the sum
    fa[k + 9], fb[k + 9] = (3e38, 1, 1, 4), (3e38, 2, 1, 4)      # the same in x: the pair still counts
    fa[k + 10], fb[k + 10] = (1, INF, 1, 4), (1, -INF, 1, 4)     # NaN only after the add
    fa[k + 11], fb[k + 11] = (1, 3e38, 1, 1e-3), (1, 1, 1, 1)    # Y_A = inf: r is NaN, skipped
    fa[k + 12], fb[k + 12] = (1, 1, 1, 1), (0, 0, 0, 0)          # filled in A only
    fa[k + 13], fb[k + 13] = (0, 0, 0, 0), (1, 1, 1, 1)          # filled in B only
    fa[k + 14], fb[k + 14] = (1, 3, 1, 2), (1, 0, 1, 2)          # Y_B = 0: r = 1
    return a, b


def cases(W, H):
    """{name: (A, B or None)} for one size."""
    a, b = pair(W, H, seed=W)
    return {
        "crafted": (crafted(W, H, seed=W), None),
        "constant": (constant(W, H), None),
        "empty": (empty(W, H), None),
        "pair": (a, b),
        "pair-constant": (constant(W, H), constant(W, H, (1.0, 0.75, 0.5, 2.0))),
        "pair-equal": (constant(W, H), constant(W, H).copy()),
        "pair-empty": (empty(W, H), empty(W, H)),
    }
