"""numpy restatement of the per-tile statistics, written from the definition
in DESIGN.md §6 row 10 (not from the C++): row 6's pixel classes and pair
rule (tests/stats_restatement.py) counted over the 16 x 16 tiles of the frame.
The second opinion the host implementation (ptsTileStatistics) is compared
with; the device kernel is compared with the host.

`over` and `origin` are the two places a one-token slip would hide; the tests
pass mutated ones (>= for >, an origin off by one) and require a mismatch."""
from __future__ import annotations

import operator

import numpy as np

from stats_restatement import classes

F = np.float32
TILE = 16
DTYPE = np.dtype([("filled", "<u4"), ("empty", "<u4"), ("nonfinite", "<u4"), ("pair", "<u4"), ("over", "<u4"),
                  ("min_count", "<f4"), ("max_count", "<f4"), ("reserved", "<u4")])


def tile_origin(t: int) -> int:
    return TILE * t


def tile_statistics(accum, other=None, threshold=0.1, over=operator.gt, origin=tile_origin) -> np.ndarray:
    a = np.ascontiguousarray(accum, F)
    H, W = a.shape[:2]
    flat = a.reshape(-1, 4)
    frame = flat
    pair = np.zeros(H * W, bool)
    above = np.zeros(H * W, bool)
    if other is not None:
        b = np.ascontiguousarray(other, F).reshape(-1, 4)
        with np.errstate(all="ignore"):
            frame = (flat + b).astype(F)
            _, _, fa, Ya = classes(flat)
            _, _, fb, Yb = classes(b)
            t = (Ya + Yb).astype(F)
            r = (np.abs(Ya - Yb) / t).astype(F)
            pair = fa & fb & (t > 0) & np.isfinite(r)
            above = pair & over(r, F(threshold))
    nonfinite, empty, filled, _ = classes(frame)
    w = frame[:, 3].reshape(H, W)
    planes = {"filled": filled, "empty": empty, "nonfinite": nonfinite, "pair": pair, "over": above}
    planes = {k: v.reshape(H, W) for k, v in planes.items()}
    tiles_y, tiles_x = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    out = np.zeros((tiles_y, tiles_x), DTYPE)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            box = (slice(origin(ty), min(origin(ty) + TILE, H)), slice(origin(tx), min(origin(tx) + TILE, W)))
            rec = out[ty, tx]
            for k, plane in planes.items():
                rec[k] = int(plane[box].sum())
            counts = w[box][planes["filled"][box]]
            if counts.size:
                rec["min_count"], rec["max_count"] = counts.min(), counts.max()
    return out
