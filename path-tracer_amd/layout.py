"""Pixel partitioning for one-process-per-GPU rendering, and the record
layout of the sky light gathered at points.

The image is cut into 16-row bands; band b belongs to rank b % nranks
(interleaved for load balance).  RNG streams are keyed on the
global pixel coordinate (basic_scatter.glsl:315-318), so the union of the
ranks' renders is bit-identical to a single-GPU render and the frame-end sum
over ranks is exact (disjoint supports).
"""
from __future__ import annotations

import numpy as np

BAND_ROWS = 16


def band_rows(height: int, rank: int, nranks: int) -> np.ndarray:
    """Image rows owned by `rank`."""
    rows = np.arange(height)
    return rows[(rows // BAND_ROWS) % nranks == rank]


def owned_pixels(width: int, height: int, rank: int, nranks: int) -> np.ndarray:
    """Boolean (height, width) mask of the pixels owned by `rank`."""
    mask = np.zeros((height, width), dtype=bool)
    mask[band_rows(height, rank, nranks)] = True
    return mask


# pt_sky_record (include/pt_packed.h): one point's gathered sky light
# (DeviceScene.gather_sky_light).  SH[i][c]: spherical
# harmonic i of bands 0..2, CIE XYZ channel c.
SKY_RECORD_DTYPE = np.dtype([("SH", "<f4", (9, 3)), ("Unoccluded", "<f4"), ("OccludedMask", "<u8"), ("Samples", "<f4"),
                             ("Reserved", "<u4", (1,))])
assert SKY_RECORD_DTYPE.itemsize == 128 and SKY_RECORD_DTYPE.fields["OccludedMask"][1] == 112
