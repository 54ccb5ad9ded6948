"""What runs in libptscene.so and needs no GPU: the frame and tile
statistics and the post-processing passes on saved accumulators, each the
implementation its device pass equals bit for bit (include/pt_scene.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._core import camera_struct, guide_image, image, image_like, motion_table, pts, tile_grid
from .params import (DenoiseParameters, DenoisePairParameters, DespikeParameters, RectifyParameters, ReprojectParameters,
                     SkyGatherParameters, VisibilityGatherParameters)
from .layout import SKY_RECORD_DTYPE


class FrameStatistics:
    """pt_frame_statistics (pt_packed.h): pixel classes,
    a 256-bin quarter-octave luminance histogram, luminance and sample-count
    range and, from a pair of half renders, the histogram of the relative
    half-difference r = |Y_A - Y_B| / (Y_A + Y_B).  Every field is an
    attribute (the histograms as uint32 arrays); the methods are pt_stats.h's
    double helpers, evaluated by libptscene.so."""

    _COUNTS = ("pixels", "filled", "empty", "nonfinite", "dark", "noise_pixels", "noise_skipped")
    _FLOATS = ("min_luminance", "max_luminance", "min_samples", "max_samples")
    _HISTOGRAMS = ("luminance_histogram", "noise_histogram")

    def __init__(self, struct: N.pt_frame_statistics):
        self._s = struct
        for f in self._COUNTS:
            setattr(self, f, int(getattr(struct, f)))
        for f in self._FLOATS:
            setattr(self, f, np.float32(getattr(struct, f)))
        for f in self._HISTOGRAMS:
            setattr(self, f, np.ctypeslib.as_array(getattr(struct, f)).astype(np.uint32))

    def as_struct(self) -> N.pt_frame_statistics:
        return self._s

    def tobytes(self) -> bytes:
        return bytes(self._s)

    def _histogram(self, which: str):
        return self._s.noise_histogram if which == "noise" else self._s.luminance_histogram

    def percentile(self, q: float, which: str = "luminance") -> int:
        """The smallest bin whose cumulative count reaches ceil(q * total) of
        the luminance (or "noise") histogram; -1 when it is empty."""
        return int(N.scene_lib().ptsStatsPercentileBin(self._histogram(which), float(q)))

    def log_average(self, q_lo: float = 0.01, q_hi: float = 0.99, which: str = "luminance") -> float:
        """Geometric mean of the bin centres between two percentile bins (0 when empty)."""
        return float(N.scene_lib().ptsStatsLogAverage(self._histogram(which), float(q_lo), float(q_hi)))

    def auto_brightness(self, key: float = 0.18, q_lo: float = 0.01, q_hi: float = 0.99) -> float:
        """key / log_average: ResolveParameters.Brightness is a linear scale
        in front of the tone curve.  1 for a frame without a binned pixel."""
        return float(N.scene_lib().ptsStatsAutoBrightness(C.byref(self._s), float(key), float(q_lo), float(q_hi)))

    def noise(self, q: float = 0.95) -> float:
        """An upper bound of the relative noise of a share q of the pair
        pixels: the upper edge of the noise histogram's percentile bin
        (inf without a pair pixel)."""
        return float(N.scene_lib().ptsStatsNoise(C.byref(self._s), float(q)))

    @staticmethod
    def bin_edges() -> np.ndarray:
        """The 257 bin edges (float64): bin b is [edges[b], edges[b + 1])."""
        L = N.scene_lib()
        return np.array([L.ptsStatsBinEdge(b) for b in range(N.STATS_BINS + 1)], dtype=np.float64)

    def __eq__(self, other):
        return isinstance(other, FrameStatistics) and self.tobytes() == other.tobytes()

    def __repr__(self):
        return (f"FrameStatistics(pixels={self.pixels}, filled={self.filled}, empty={self.empty}, "
                f"nonfinite={self.nonfinite}, dark={self.dark}, luminance=[{self.min_luminance}, "
                f"{self.max_luminance}], samples=[{self.min_samples}, {self.max_samples}], "
                f"noise_pixels={self.noise_pixels}, noise_skipped={self.noise_skipped})")


def _accumulators(accum, other):
    """(a, b or None, pointer to b or None): the statistics' one or two accumulators, neither empty."""
    a = image(accum, empty=False)
    if other is None:
        return a, None, None
    b = image(other, "second accumulator", empty=False)
    if b.shape != a.shape:
        raise ValueError(f"accumulators of shapes {a.shape} and {b.shape}")
    return a, b, N.fptr(b)


def frame_statistics_host(accum: np.ndarray, other: "np.ndarray | None" = None) -> FrameStatistics:
    """The frame statistics on the CPU (ptsFrameStatistics, libptscene.so):
    for saved accumulators on a machine without a GPU, and the implementation
    SampleBuffer.statistics equals bit for bit.  accum, other: (H, W, 4) XYZ
    sums + sample count; with `other`, an independent render of the same
    frame, the luminance part describes accum + other and the noise part the
    pair."""
    a, b, bp = _accumulators(accum, other)
    out = N.pt_frame_statistics()
    pts("ptsFrameStatistics", a.shape[1], a.shape[0], N.fptr(a), bp, C.byref(out))
    return FrameStatistics(out)


def tile_statistics_host(accum: np.ndarray, other: "np.ndarray | None" = None, threshold: float = 0.1) -> np.ndarray:
    """Per-tile statistics on the CPU (ptsTileStatistics, libptscene.so), which
    SampleBuffer.tile_statistics equals bit for bit: a (tiles_y, tiles_x) array
    of TILE_STATS_DTYPE records, one per 16 x 16 tile (clipped at the right and
    bottom edges).  accum, other: (H, W, 4) accumulators as for
    frame_statistics_host; without `other`, pair and over are 0.  over counts
    the pair pixels whose relative half-difference exceeds `threshold`."""
    a, b, bp = _accumulators(accum, other)
    out = np.zeros(tile_grid(a.shape[1], a.shape[0]), dtype=N.TILE_STATS_DTYPE)
    pts("ptsTileStatistics", a.shape[1], a.shape[0], N.fptr(a), bp, float(threshold), out.ctypes.data)
    return out


def tile_mask_of_region(width: int, height: int, x0: int, y0: int, x1: int, y1: int) -> np.ndarray:
    """The (tiles_y, tiles_x) uint8 mask of the 16 x 16 tiles of a width x
    height frame that hold a pixel of [x0, x1) x [y0, y1) (clipped to the
    frame): the argument of BasicRenderer.set_active_tiles that re-renders
    that region."""
    ty, tx = tile_grid(width, height)
    mask = np.zeros((ty, tx), dtype=np.uint8)
    x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), int(width)), min(int(y1), int(height))
    if x0 < x1 and y0 < y1:
        mask[y0 // N.TILE_SIZE:(y1 - 1) // N.TILE_SIZE + 1, x0 // N.TILE_SIZE:(x1 - 1) // N.TILE_SIZE + 1] = 1
    return mask


def denoise_host(accum: np.ndarray, guides: np.ndarray, params: "DenoiseParameters | None" = None) -> np.ndarray:
    """The denoiser on the CPU (ptsDenoise, libptscene.so): for saved
    accumulators on a machine without a GPU, and the implementation the
    device filter equals bit for bit.  accum: (H, W, 4) XYZ sums + sample
    count; guides: (H, W) DENOISE_GUIDE_DTYPE records.  Returns (H, W, 4):
    the denoised mean XYZ and 1 (zeros where the count is not positive)."""
    a = image(accum)
    g = guide_image(guides, a)
    out = np.zeros_like(a)
    p = (params or DenoiseParameters()).as_struct()
    pts("ptsDenoise", a.shape[1], a.shape[0], N.fptr(a), g.ctypes.data, C.byref(p), N.fptr(out))
    return out


def denoise_pair_host(accum_a: np.ndarray, accum_b: np.ndarray, guides: np.ndarray,
                      params: "DenoisePairParameters | None" = None) -> np.ndarray:
    """The variance-guided denoiser on the CPU (ptsDenoisePair,
    libptscene.so), which the device filter equals bit for bit.  accum_a,
    accum_b: (H, W, 4) accumulators of two independent renders of one frame
    (FrameIndex apart by 1 << 24); guides: (H, W) DENOISE_GUIDE_DTYPE records.
    Returns (H, W, 4): the denoised mean XYZ of a + b and 1 (zeros where the
    combined count is not positive)."""
    a, b = (np.ascontiguousarray(x, dtype=np.float32) for x in (accum_a, accum_b))   # both, before either is judged
    a = image(a)
    b = image_like(b, a, "second accumulator", "first")
    g = guide_image(guides, a)
    out = np.zeros_like(a)
    p = (params or DenoisePairParameters()).as_struct()
    pts("ptsDenoisePair", a.shape[1], a.shape[0], N.fptr(a), N.fptr(b), g.ctypes.data, C.byref(p), N.fptr(out))
    return out


def shape_motion(prev_shapes: np.ndarray, shapes: np.ndarray) -> np.ndarray:
    """The motion table between two packs of one scene (ptsShapeMotion,
    pt_scene.h): prev_shapes and shapes are the packed
    shape records (scene.arrays()["shapes"], DeviceScene.shapes) of the
    previous and the current frame; returns one SHAPE_MOTION_DTYPE record per
    current shape.  Shapes are matched by index: the set of entities must be
    the same in both packs (only a longer array is noticed)."""
    ps = np.ascontiguousarray(prev_shapes, dtype=N.SHAPE_DTYPE).reshape(-1)
    cs = np.ascontiguousarray(shapes, dtype=N.SHAPE_DTYPE).reshape(-1)
    out = np.zeros(cs.size, dtype=N.SHAPE_MOTION_DTYPE)
    pts("ptsShapeMotion", ps.ctypes.data if ps.size else None, ps.size, cs.ctypes.data if cs.size else None, cs.size,
        out.ctypes.data if cs.size else None)
    return out


def reproject_host(prev_accum: np.ndarray, prev_guides: np.ndarray, prev_camera, guides: np.ndarray, camera,
                   params: "ReprojectParameters | None" = None, motion: "np.ndarray | None" = None) -> np.ndarray:
    """Temporal reprojection on the CPU (ptsReproject, libptscene.so), which
    the device kernel equals bit for bit.  prev_accum: (Hp, Wp, 4) accumulator
    of the previous view; prev_guides: its (Hp, Wp) DENOISE_GUIDE_DTYPE
    records; guides: the current view's (H, W) records; prev_camera, camera:
    the packed camera records (scene.arrays()["cameras"][i]) the two guide
    images were rendered with.  Returns (H, W, 4): (mean XYZ * n, n) with n
    the carried sample count, zeros where the pixel has no history.  motion:
    a shape_motion() table; pixels of moved shapes then follow them
    (ptsReprojectMoving)."""
    a = image(prev_accum)
    pg = guide_image(prev_guides, a, "previous guides")
    g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.ndim != 2:
        raise ValueError(f"guides of shape {g.shape}, expected (H, W)")
    out = np.zeros(g.shape + (4,), np.float32)
    pc, c = camera_struct(prev_camera), camera_struct(camera)
    p = (params or ReprojectParameters()).as_struct()
    views = (a.shape[1], a.shape[0], N.fptr(a), pg.ctypes.data, C.byref(pc), g.shape[1], g.shape[0], g.ctypes.data,
             C.byref(c))
    if motion is not None:
        m, mp, mn = motion_table(motion)
        pts("ptsReprojectMoving", *views, mp, mn, C.byref(p), N.fptr(out))
    else:
        pts("ptsReproject", *views, C.byref(p), N.fptr(out))
    return out


def rectify_host(history: np.ndarray, current: np.ndarray, guides: np.ndarray,
                 params: "RectifyParameters | None" = None) -> np.ndarray:
    """History validation on the CPU (ptsRectifyHistory, libptscene.so), which
    the device kernel equals bit for bit.  history: (H, W, 4) accumulator in
    (mean * n, n) form, e.g. reproject_host's result; current: the (H, W, 4)
    accumulator of the new rounds alone; guides: the current view's (H, W)
    DENOISE_GUIDE_DTYPE records.  Returns the (H, W, 4) history with every
    pixel's mean pulled into the box its window of current samples allows and
    the count of a pulled pixel cut."""
    a = image(history, "history")
    b = image_like(current, a, "current accumulator", "history")
    g = guide_image(guides, a)
    out = np.zeros_like(a)
    p = (params or RectifyParameters()).as_struct()
    pts("ptsRectifyHistory", a.shape[1], a.shape[0], N.fptr(a), N.fptr(b), g.ctypes.data, C.byref(p), N.fptr(out))
    return out


def gather_visibility_rays_host(points: np.ndarray, normals: np.ndarray,
                                params: "VisibilityGatherParameters | None" = None):
    """The rays DeviceScene.gather_visibility traces, on the CPU
    (ptsGatherVisibilityRays, libptscene.so: include/pt_visibility.h compiled
    for the host), bit for bit.  points, normals: (n, 3).  Returns (origins
    (n Samples, 3), packed velocities, durations), point-major: ray i Samples +
    k is sample k of point i; the arguments of DeviceScene.occluded and
    trace_rays."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if len(p) != len(nrm):
        raise ValueError(f"{len(p)} points and {len(nrm)} normals")
    s = (params or VisibilityGatherParameters()).as_struct()
    rays = len(p) * s.Samples if 1 <= s.Samples <= N.AMBIENT_OCCLUSION_MAX_SAMPLES else 0
    o, v, d = np.zeros((rays, 3), np.float32), np.zeros(rays, np.uint32), np.zeros(rays, np.float32)
    pts("ptsGatherVisibilityRays", C.byref(s), len(p), N.fptr(p), N.fptr(nrm), N.fptr(o), N.u32ptr(v), N.fptr(d))
    return o, v, d


def gather_visibility_reduce_host(samples: int, packed_velocities: np.ndarray, occluded: np.ndarray) -> np.ndarray:
    """DeviceScene.gather_visibility's records from any answer to "is ray r
    blocked" over gather_visibility_rays_host's rays (ptsGatherVisibilityReduce,
    libptscene.so): the mask, the count and the bent vector by the device's
    summation tree.  packed_velocities: (n samples,); occluded: one bool per
    ray (DeviceScene.occluded's result, or a closest-hit query's "hit").
    Returns n VISIBILITY_RECORD_DTYPE records."""
    samples = int(samples)
    v = np.ascontiguousarray(packed_velocities, dtype=np.uint32).reshape(-1)
    occ = np.ascontiguousarray(occluded, dtype=bool).reshape(-1)
    if samples < 1 or len(v) % samples or len(occ) != len(v):
        raise ValueError(f"{len(v)} velocities and {len(occ)} bits for {samples} samples per point")
    bits = np.zeros((len(v) + 63) // 64 * 8, np.uint8)
    packed_bits = np.packbits(occ, bitorder="little")
    bits[:len(packed_bits)] = packed_bits
    out = np.zeros(len(v) // samples, dtype=N.VISIBILITY_RECORD_DTYPE)
    pts("ptsGatherVisibilityReduce", samples, len(out), N.u32ptr(v), bits.view(np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)),
        out.ctypes.data)
    return out


def sky_gather_rays_host(points: np.ndarray, normals: "np.ndarray | None" = None,
                         params: "SkyGatherParameters | None" = None):
    """The rays DeviceScene.gather_sky_light traces and each ray's normalised
    first wavelength L0, on the CPU (ptsSkyGatherRays, libptscene.so:
    include/pt_visibility.h compiled for the host), bit for bit, for both
    lobes.  points: (n, 3); normals: (n, 3), or None with the sphere lobe.
    Returns (origins (n Samples, 3), packed velocities, durations, L0),
    point-major."""
    s = (params or SkyGatherParameters()).as_struct()
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if len(p) != len(nrm):
            raise ValueError(f"{len(p)} points and {len(nrm)} normals")
    elif s.Lobe == N.SKY_GATHER_COSINE:
        raise ValueError("the cosine lobe needs normals")
    rays = len(p) * s.Samples if 1 <= s.Samples <= N.AMBIENT_OCCLUSION_MAX_SAMPLES else 0
    o, v = np.zeros((rays, 3), np.float32), np.zeros(rays, np.uint32)
    d, l0 = np.zeros(rays, np.float32), np.zeros(rays, np.float32)
    pts("ptsSkyGatherRays", C.byref(s), len(p), N.fptr(p), None if nrm is None else N.fptr(nrm), N.fptr(o), N.u32ptr(v),
        N.fptr(d), N.fptr(l0))
    return o, v, d, l0


def sky_gather_reduce_host(samples: int, packed_velocities: np.ndarray, occluded: np.ndarray,
                           contributions: np.ndarray) -> np.ndarray:
    """DeviceScene.gather_sky_light's records from any answer to "is ray r
    blocked" over sky_gather_rays_host's rays and any per-ray XYZ
    contributions (n samples, 3) (ptsSkyGatherReduce, libptscene.so): the
    basis at the unpacked velocities, the 27 products per ray (an occluded
    ray's contribution is taken as zero) and the device's summation tree.
    Returns n SKY_RECORD_DTYPE records."""
    samples = int(samples)
    v = np.ascontiguousarray(packed_velocities, dtype=np.uint32).reshape(-1)
    occ = np.ascontiguousarray(occluded, dtype=bool).reshape(-1)
    c = np.ascontiguousarray(contributions, dtype=np.float32).reshape(-1, 3)
    if samples < 1 or len(v) % samples or len(occ) != len(v) or len(c) != len(v):
        raise ValueError(f"{len(v)} velocities, {len(occ)} bits and {len(c)} contributions for {samples} samples "
                         f"per point")
    bits = np.zeros((len(v) + 63) // 64 * 8, np.uint8)
    packed_bits = np.packbits(occ, bitorder="little")
    bits[:len(packed_bits)] = packed_bits
    out = np.zeros(len(v) // samples, dtype=SKY_RECORD_DTYPE)
    pts("ptsSkyGatherReduce", samples, len(out), N.u32ptr(v), bits.view(np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)),
        N.fptr(c), out.ctypes.data)
    return out


SH9_Y0 = 0.28209479   # the band-0 harmonic as the device has it (pt_sky_gather_basis' float literal)


def sh9_basis(directions: np.ndarray) -> np.ndarray:
    """The nine real spherical harmonics of bands 0..2 (z up, the order and
    signs of pt_sky_gather_basis) at unit vectors (..., 3), in float64:
    (..., 9)."""
    d = np.asarray(directions, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k1, k2 = np.sqrt(3.0 / (4.0 * np.pi)), np.sqrt(15.0 / (4.0 * np.pi))
    return np.stack([np.full_like(x, np.sqrt(1.0 / (4.0 * np.pi))), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z,
                     np.sqrt(5.0 / (16.0 * np.pi)) * (3.0 * z * z - 1.0), k2 * x * z, 0.5 * k2 * (x * x - y * y)],
                    axis=-1)


def sky_irradiance(records: np.ndarray) -> np.ndarray:
    """The CIE XYZ irradiance from the sky at each point of cosine-lobe
    records, (n, 3) float64: pi SH[0] / (Y0 Samples).  Without the pi it is
    the pixel value the integrator converges to for direct sky light on a
    white Lambertian surface there."""
    r = np.asarray(records)
    return np.pi * r["SH"][..., 0, :].astype(np.float64) / (SH9_Y0 * r["Samples"].astype(np.float64))[..., None]


def sky_radiance_sh(records: np.ndarray) -> np.ndarray:
    """The SH9 coefficients of the visible sky's radiance around each point
    of sphere-lobe records, (n, 9, 3) float64: (4 pi / Samples) SH."""
    r = np.asarray(records)
    return 4.0 * np.pi * r["SH"].astype(np.float64) / r["Samples"].astype(np.float64)[..., None, None]


def sh9_irradiance(coeffs: np.ndarray, normals: np.ndarray) -> np.ndarray:
    """The irradiance on surfaces of unit normals (n, 3) under radiance given
    by SH9 coefficients (9, C) or (n, 9, C): the clamped-cosine convolution,
    sum_i A_band(i) coeffs[i] Y_i(normal) with A = pi, 2 pi / 3, pi / 4.
    Returns (n, C) float64."""
    A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    Y = sh9_basis(np.asarray(normals, np.float64).reshape(-1, 3))
    return np.einsum("ni,ic->nc" if np.ndim(coeffs) == 2 else "ni,nic->nc", Y * A, np.asarray(coeffs, np.float64))


def shape_surface_points(scene, shape_index: int):
    """One world-space point and unit normal per vertex of packed mesh shape
    `shape_index`, for baking visibility (DeviceScene.gather_visibility) on a
    mesh without restating the packs.  scene: a packed Scene, or the dict of
    its arrays().  The shape's packed mesh nodes are walked from
    MeshRootNodeIndex; every distinct VertexIndex of the faces below gives one
    entry, at its first occurrence: the face's position through the shape's
    Transform.To, and the vertex's unpacked normal through the transpose of
    From's 3 x 3, renormalised (the hit record's TransformNormal).  Returns
    (points (n, 3) float32, normals (n, 3) float32, vertex indices (n,)
    uint32)."""
    a = scene if isinstance(scene, dict) else scene.arrays()
    shapes = a["shapes"]
    if not 0 <= int(shape_index) < len(shapes):
        raise ValueError(f"shape index {shape_index} of {len(shapes)} shapes")
    shape = shapes[int(shape_index)]
    if int(shape["Type"]) != 0:   # PT_SHAPE_TYPE_MESH_INSTANCE
        raise ValueError(f"shape {shape_index} of type {int(shape['Type'])} is not a mesh instance")
    nodes, faces, vertices = a["mesh_nodes"], a["mesh_faces"], a["mesh_vertices"]
    ranges, stack = [], [int(shape["MeshRootNodeIndex"])]
    while stack:
        node = nodes[stack.pop()]
        begin, end = int(node["FaceBeginOrNodeIndex"]), int(node["FaceEndIndex"])
        if end > 0:
            ranges.append((begin, end))
        else:
            stack += [begin + 1, begin]
    ranges.sort()
    f = np.concatenate([faces[b:e] for b, e in ranges]) if ranges else faces[:0]
    index = np.stack([f["VertexIndex0"], f["VertexIndex1"], f["VertexIndex2"]], axis=1).reshape(-1)
    local = np.stack([f["Position0"], f["Position1"], f["Position2"]], axis=1).reshape(-1, 3).astype(np.float64)
    index, first = np.unique(index, return_index=True)
    local = local[first]
    # The packed matrices are column-major: element (row r, column c) at [4 c + r].
    to = shape["Transform"]["To"].astype(np.float64).reshape(4, 4).T
    from_t = shape["Transform"]["From"].astype(np.float64).reshape(4, 4)[:3, :3]
    points = local @ to[:3, :3].T + to[:3, 3]
    # UnpackUnitVector (octahedral snorm16 x 2).
    word = vertices["PackedNormal"][index]
    p = np.stack([(word & 0xFFFF).astype(np.uint16).view(np.int16), (word >> 16).astype(np.uint16).view(np.int16)],
                 axis=1).astype(np.float64) / 32767.0
    p = np.clip(p, -1.0, 1.0)
    z = 1.0 - np.abs(p[:, 0]) - np.abs(p[:, 1])
    fold = (1.0 - np.abs(p[:, ::-1])) * np.where(p >= 0, 1.0, -1.0)
    p = np.where((z < 0)[:, None], fold, p)
    n = np.concatenate([p, z[:, None]], axis=1) @ from_t.T
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return points.astype(np.float32), n.astype(np.float32), index.astype(np.uint32)


def despike_host(accum: np.ndarray, guides: np.ndarray, params: "DespikeParameters | None" = None) -> np.ndarray:
    """The firefly clamp on the CPU (ptsDespike, libptscene.so), which the
    device kernel equals bit for bit.  accum: (H, W, 4) XYZ sums + sample
    count; guides: the same view's (H, W) DENOISE_GUIDE_DTYPE records.
    Returns the (H, W, 4) accumulator with the colour sums of every pixel that
    stands out of its window scaled down onto the window's limit; every other
    pixel and every count keeps its bits."""
    a = image(accum)
    g = guide_image(guides, a)
    out = np.zeros_like(a)
    p = (params or DespikeParameters()).as_struct()
    pts("ptsDespike", a.shape[1], a.shape[0], N.fptr(a), g.ctypes.data, C.byref(p), N.fptr(out))
    return out
