"""Crafted pairs of accumulators shared by the pair denoiser's tests
(tests/test_denoise_pair.py on the CPU, tests/test_gpu_denoise_pair.py on
the device): two of tests/denoise_cases.py's accumulators with different
seeds, patched so that one image holds pixels filled only in A, only in B and
in neither, a block where A and B are bit-identical (variance 0), negative
sums and x1e6 values.  Guides are denoise_cases.crafted_guides."""
from __future__ import annotations

import numpy as np

import denoise_cases as dc

F = np.float32
PARAMS = dict(sigma_luminance=3.0, sigma_normal=0.3, sigma_depth=0.4, sigma_albedo=0.5)


def pair(W, H, seed=0):
    """(A, B): every patch is clipped to the image, so (5, 3) keeps them all."""
    a, b = dc.accumulators(W, H, seed), dc.accumulators(W, H, seed + 7919)
    # Both carry denoise_cases' rows: empty in both at [0, :8], negative sums
    # in both at [1, :8], x1e6 in both at [2, :8], an empty run at H // 2.
    y0, x0 = H // 3, W // 3
    a[y0:y0 + 2, x0:x0 + 3, 3] = np.maximum(a[y0:y0 + 2, x0:x0 + 3, 3], 1)
    b[y0:y0 + 2, x0:x0 + 3] = 0                                # filled only in A
    y1, x1 = H - 1 - H // 4, W // 5
    b[y1:y1 + 2, x1:x1 + 3, 3] = np.maximum(b[y1:y1 + 2, x1:x1 + 3, 3], 1)
    a[y1:y1 + 2, x1:x1 + 3] = 0                                # filled only in B
    a[H - 1, W - 2:] = 0
    b[H - 1, W - 2:] = 0                                       # filled in neither
    y2, x2 = H // 2 + 1, W // 2
    a[y2:y2 + 4, x2:x2 + 5, 3] = np.maximum(a[y2:y2 + 4, x2:x2 + 5, 3], 1)
    b[y2:y2 + 4, x2:x2 + 5] = a[y2:y2 + 4, x2:x2 + 5]          # bit-identical: v = 0
    a[-1, 0, :3] = -np.abs(a[-1, 0, :3]) - 1                   # a negative sum in A alone
    a[-1, 0, 3] = 3
    b[-1, 1, :3] *= F(1e6)                                     # very bright in B alone
    b[-1, 1, 3] = 5
    return a, b


def features(a, b):
    """Which of the crafted features the pair holds (for the test of the cases)."""
    fa, fb = a[..., 3] > 0, b[..., 3] > 0
    same = fa & fb & (a.view(np.uint32) == b.view(np.uint32)).all(axis=-1)
    return {
        "only_a": bool((fa & ~fb).any()),
        "only_b": bool((~fa & fb).any()),
        "neither": bool((~fa & ~fb).any()),
        "both": bool((fa & fb).any()),
        "identical": bool(same.any()),
        "negative": bool(((a[..., :3] < 0).any(axis=-1) & fa).any() or ((b[..., :3] < 0).any(axis=-1) & fb).any()),
        "bright": bool(((a[..., :3] > 1e5).any(axis=-1) & fa).any() or ((b[..., :3] > 1e5).any(axis=-1) & fb).any()),
    }
