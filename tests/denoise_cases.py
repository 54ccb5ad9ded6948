"""Crafted inputs shared by the denoiser tests (tests/test_denoise.py on the
CPU, tests/test_gpu_denoise.py on the device): random accumulators in the
manner of tests/test_resolve.py::accumulators and guide images with the
features the filter's edge stops act on."""
from __future__ import annotations

import numpy as np

from denoise_restatement import GUIDE_DTYPE, NONE

F = np.float32
SIZES = [(40, 24), (67, 45)]          # (width, height)
PARAMS = dict(sigma_color=2.0, sigma_normal=0.3, sigma_depth=0.4, sigma_albedo=0.5)


def accumulators(W, H, seed=0):
    """XYZ sums + sample counts: rows with zero count, negative sums and
    x1e6 values among them, plus scattered empty pixels."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 4, size=(H, W, 4)).astype(F)
    a[..., 3] = rng.integers(0, 50, size=(H, W)).astype(F)   # some counts are 0
    a[0, :8] = 0                                   # no samples
    a[1, :8, :3] = -a[1, :8, :3]                   # negative XYZ sums
    a[2, :8, :3] *= 1e6                            # very bright
    a[H // 2, W // 2:] = 0                         # an empty run inside the image
    return a


def crafted_guides(W, H, seed=0):
    """Three shapes meeting at a vertical, a horizontal and a diagonal edge,
    a miss region, a normal discontinuity inside one shape, a depth ramp and
    an albedo checkerboard."""
    rng = np.random.default_rng(1000 + seed)
    g = np.zeros((H, W), GUIDE_DTYPE)
    ys, xs = np.mgrid[0:H, 0:W]
    shape = np.zeros((H, W), np.uint32)
    shape[:, W // 2:] = 1                                      # vertical edge 0 | 1
    shape[(ys >= H // 2) & (xs < W // 2)] = 2                  # horizontal edge 0 / 2
    shape[(xs >= W // 2) & (xs - W // 2 + ys > H)] = 2         # diagonal edge 1 \ 2
    miss = (xs >= W - W // 5) & (ys < H // 4)
    shape[miss] = NONE
    g["shape"] = shape
    n = np.zeros((H, W, 3), F)
    n[...] = (0.0, 0.0, 1.0)
    n[(shape == 0) & (xs < W // 4)] = (0.0, 0.6, 0.8)          # a crease inside shape 0
    n[shape == 1] = (0.6, 0.0, 0.8)
    n[shape == 2] = (-0.6, 0.0, 0.8)
    n = n + rng.uniform(-0.01, 0.01, size=n.shape).astype(F)   # not exactly unit: the filter must not care
    g["normal"] = n.astype(F)
    g["time"] = (F(1.0) + xs.astype(F) * F(0.05) + ys.astype(F) * F(0.2)).astype(F)      # depth ramp
    checker = ((xs // 3 + ys // 3) & 1).astype(F)
    g["albedo"] = (F(0.2) + F(0.6) * checker)[..., None] * np.array([1.0, 0.9, 0.8], F)
    g["normal"][miss] = 0
    g["time"][miss] = 0
    g["albedo"][miss] = (0.3, 0.5, 0.9)
    return g


def same_bits(a, b):
    """Elementwise: equal bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
