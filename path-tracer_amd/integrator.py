"""Integrator entry points (mirror of src/integrator/basic.hpp:28-32 and
src/integrator/integrator.hpp:51-60) over libpathtracer.so.

    CreateSampleBuffer(device, W, H)          integrator.hpp:51
    CreateBasicRenderer(device, scene, sb)     basic.hpp:28
    ResetBasicRenderer(device, renderer)       basic.hpp:31
    RunBasicRenderer(device, renderer, rounds) basic.hpp:32

The renderer's CameraIndex / RenderFlags / PathLengthLimit /
PathTerminationProbability / FrameIndex are exposed as attributes, written
by the caller before Reset/Run exactly as application.cpp:104-107 does.
Everything runs in the HIP library; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


class PathTracerError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise PathTracerError(f"{what}: {N.hip_lib().ptGetLastError().decode()} (status {rc})")


def device_count() -> int:
    n = C.c_int(0)
    N.hip_lib().ptGetDeviceCount(C.byref(n))
    return n.value


class Device:
    """A HIP device + stream (replaces the reference's `vulkan` context)."""

    def __init__(self, hip_device: int = 0):
        L = N.hip_lib()
        self._h = L.ptCreateDevice(int(hip_device))
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())
        self.index = hip_device

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        _check(N.hip_lib().ptSynchronize(self._h), "ptSynchronize")

    def set_profiling(self, enable: bool, period: int = 1):
        """Kernel timing with HIP events; period > 1 times every period-th round only."""
        _check(N.hip_lib().ptSetProfiling(self._h, int(enable)), "ptSetProfiling")
        _check(N.hip_lib().ptSetProfilingPeriod(self._h, int(period)), "ptSetProfilingPeriod")

    def kernel_stats(self, kernel: int):
        n = C.c_uint64(0)
        ms = C.c_double(0)
        _check(N.hip_lib().ptGetKernelStats(self._h, kernel, C.byref(n), C.byref(ms)), "ptGetKernelStats")
        return int(n.value), float(ms.value)

    def kernel_rounds(self, kernel: int) -> int:
        """Rounds covered by the timed launches of `kernel` (a round batch
        covers several): total_ms / rounds is its time per round."""
        n = C.c_uint64(0)
        _check(N.hip_lib().ptGetKernelRounds(self._h, kernel, C.byref(n)), "ptGetKernelRounds")
        return int(n.value)

    def reset_kernel_stats(self):
        _check(N.hip_lib().ptResetKernelStats(self._h), "ptResetKernelStats")

    def set_statistics_variant(self, variant: int):
        """STATS_VARIANT_AUTO / _PLAIN / _UNIFORM: the statistics kernel's
        histogram update (identical results; ptSetFrameStatisticsVariant)."""
        _check(N.hip_lib().ptSetFrameStatisticsVariant(self._h, int(variant)), "ptSetFrameStatisticsVariant")

    def check_fast_division(self, n: int, seed: int = 1) -> int:
        m = C.c_uint64(0)
        _check(N.hip_lib().ptCheckFastDivision(self._h, n, seed, C.byref(m)), "ptCheckFastDivision")
        return int(m.value)

    def check_fast_reciprocal(self) -> int:
        m = C.c_uint64(0)
        _check(N.hip_lib().ptCheckFastReciprocal(self._h, C.byref(m)), "ptCheckFastReciprocal")
        return int(m.value)

    def eval_numerics(self, op, a, b=None, c=None) -> np.ndarray:
        """Test probe (ptEvalNumerics): operation `op` (a name of
        N.NUMERICS_OPS or its id) on the device over uint32 operand words
        (float bit patterns or integers).  Returns the result words, shape
        (n,) or (n, outputs) for an op with several."""
        name = N.NUMERICS_OPS[op] if isinstance(op, int) else op
        arrays = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (a, b, c)]
        n = len(arrays[0])
        outputs = N.NUMERICS_OUTPUTS.get(name, 1)
        out = np.zeros(n * outputs, dtype=np.uint32)
        ptrs = [None if x is None else N.u32ptr(x) for x in arrays]
        _check(N.hip_lib().ptEvalNumerics(self._h, N.NUMERICS_OPS.index(name), n, *ptrs, N.u32ptr(out)),
               "ptEvalNumerics")
        return out if outputs == 1 else out.reshape(n, outputs)

    def close(self):
        if self._h:
            N.hip_lib().ptDestroyDevice(self._h)
            self._h = None


class DeviceScene:
    """Device copy of a packed scene (CreateVulkanScene / UpdateVulkanScene)."""

    def __init__(self, device: Device):
        L = N.hip_lib()
        self.device = device
        self.cameras = np.zeros(0, dtype=N.CAMERA_DTYPE)
        self.shapes = np.zeros(0, dtype=N.SHAPE_DTYPE)
        self._h = L.ptCreateScene(device.handle)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())

    @property
    def handle(self):
        return self._h

    def set_stack_format(self, fmt: int):
        """PT_STACK_FORMAT_* (0 auto, 1 packed 32-bit words, 2 node indices); next update()."""
        _check(N.hip_lib().ptSetSceneStackFormat(self._h, int(fmt)), "ptSetSceneStackFormat")

    def set_hit_record_form(self, form: int):
        """PT_HIT_RECORD_* (0 auto, 1 face index); next update()."""
        _check(N.hip_lib().ptSetSceneHitRecordForm(self._h, int(form)), "ptSetSceneHitRecordForm")

    def set_extend_form(self, form: int):
        """PT_EXTEND_FORM_* (0 auto, 1 general traversal loop); next update()."""
        _check(N.hip_lib().ptSetSceneExtendForm(self._h, int(form)), "ptSetSceneExtendForm")

    @property
    def extend_form(self) -> int:
        """The extend form the uploaded scene runs: 1 general, 2 mesh-only (ptGetSceneExtendForm)."""
        v = C.c_uint32(0)
        _check(N.hip_lib().ptGetSceneExtendForm(self._h, C.byref(v)), "ptGetSceneExtendForm")
        return int(v.value)

    def update(self, scene, dirty_flags: int = 0xFFFFFFFF):
        packs = scene.packs() if hasattr(scene, "packs") else scene
        _check(N.hip_lib().ptUpdateScene(self.device.handle, self._h, C.byref(packs), dirty_flags), "ptUpdateScene")
        # The packed camera records as uploaded (FrameHistory keeps a frame's own).
        self.cameras = np.zeros(0, dtype=N.CAMERA_DTYPE)
        if packs.camera_count and packs.cameras:
            buf = (C.c_char * (packs.camera_count * N.CAMERA_DTYPE.itemsize)).from_address(packs.cameras)
            self.cameras = np.frombuffer(buf, dtype=N.CAMERA_DTYPE).copy()
        # And the packed shapes (FrameHistory(follow_shapes=True) compares two frames' transforms).
        self.shapes = np.zeros(0, dtype=N.SHAPE_DTYPE)
        if packs.shape_count and packs.shapes:
            buf = (C.c_char * (packs.shape_count * N.SHAPE_DTYPE.itemsize)).from_address(packs.shapes)
            self.shapes = np.frombuffer(buf, dtype=N.SHAPE_DTYPE).copy()

    def length_table(self) -> dict:
        """{classes, trained, rounds}: the scene's traversal-length table, one
        class 0..6 per ray key, whether it was trained since the last clear and
        the LENGTH rounds counted since then (diagnostic, ptReadSceneLengthTable)."""
        cls = np.zeros(N.RAYKEY_COUNT, dtype=np.uint8)
        t, n = C.c_uint32(0), C.c_uint64(0)
        _check(N.hip_lib().ptReadSceneLengthTable(self.device.handle, self._h, cls.ctypes.data, C.byref(t), C.byref(n)),
               "ptReadSceneLengthTable")
        return {"classes": cls, "trained": bool(t.value), "rounds": int(n.value)}

    @property
    def stack_needed(self) -> int:
        """Traversal stack entries the uploaded scene can need (TLAS + BLAS depth)."""
        v = C.c_uint32(0)
        _check(N.hip_lib().ptSceneStackNeeded(self._h, C.byref(v)), "ptSceneStackNeeded")
        return int(v.value)

    @property
    def node_cache_pairs(self) -> int:
        """BLAS child pairs the extend kernel keeps in LDS (0: none; ptSceneNodeCache)."""
        v = C.c_uint32(0)
        _check(N.hip_lib().ptSceneNodeCache(self._h, C.byref(v)), "ptSceneNodeCache")
        return int(v.value)

    def trace_rays(self, origins: np.ndarray, packed_velocities: np.ndarray, durations: np.ndarray) -> np.ndarray:
        """Bit-exact Trace() of a ray batch (scene.glsl.inc:522-611)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(packed_velocities, dtype=np.uint32).reshape(-1)
        d = np.ascontiguousarray(durations, dtype=np.float32).reshape(-1)
        out = np.zeros(len(v), dtype=N.HIT_RECORD_DTYPE)
        _check(N.hip_lib().ptTraceRays(self.device.handle, self._h, len(v), N.fptr(o), N.u32ptr(v), N.fptr(d),
                                       out.ctypes.data), "ptTraceRays")
        return out

    def sample_textures(self, texture_index: np.ndarray, uv: np.ndarray, wrap: int = 0) -> np.ndarray:
        """Test probe (ptSampleTextures): SampleTexture of the uploaded scene
        at (n, 2) UVs; wrap 0 = remainder, 1 = the lean kernel's two-select
        form (refused when a placement leaves [0, 1]).  Returns (n, 4)."""
        t = np.ascontiguousarray(texture_index, dtype=np.uint32).reshape(-1)
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        assert len(u) == len(t)
        out = np.zeros((len(t), 4), dtype=np.float32)
        _check(N.hip_lib().ptSampleTextures(self.device.handle, self._h, len(t), N.u32ptr(t), N.fptr(u), int(wrap),
                                            N.fptr(out)), "ptSampleTextures")
        return out

    def trace_rays_stats(self, origins: np.ndarray, packed_velocities: np.ndarray, durations: np.ndarray):
        """Traversal counters (ptExtendStats keys) and per-ray step counts of a
        ray batch (diagnostic, ptTraceRaysStats)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(packed_velocities, dtype=np.uint32).reshape(-1)
        d = np.ascontiguousarray(durations, dtype=np.float32).reshape(-1)
        out = (C.c_uint64 * 14)()
        steps = np.zeros(len(v), dtype=np.uint32)
        _check(N.hip_lib().ptTraceRaysStats(self.device.handle, self._h, len(v), N.fptr(o), N.u32ptr(v), N.fptr(d),
                                            out, steps.ctypes.data), "ptTraceRaysStats")
        keys = ("rays", "lane_steps", "wave_steps_x64", "internal_nodes", "blas_leaves", "faces", "pops",
                "tlas_leaves", "waves")
        stats = dict(zip(keys, (int(x) for x in out)))
        stats["simd_efficiency"] = stats["lane_steps"] / max(stats["wave_steps_x64"], 1)
        return stats, steps

    def close(self):
        if self._h:
            N.hip_lib().ptDestroyScene(self.device.handle, self._h)
            self._h = None


class ResolveParameters:
    """resolve_parameters (integrator.hpp:43-48) with the reference defaults."""

    def __init__(self, Brightness: float = 1.0, ToneMappingMode: int = N.TONE_MAPPING_CLAMP,
                 ToneMappingWhiteLevel: float = 1.0):
        self.Brightness = float(Brightness)
        self.ToneMappingMode = int(ToneMappingMode)
        self.ToneMappingWhiteLevel = float(ToneMappingWhiteLevel)

    def as_struct(self) -> N.pt_resolve_parameters:
        return N.pt_resolve_parameters(self.Brightness, self.ToneMappingMode, self.ToneMappingWhiteLevel)

    @classmethod
    def auto(cls, stats: "FrameStatistics", key: float = 0.18, q_lo: float = 0.01, q_hi: float = 0.99,
             **kw) -> "ResolveParameters":
        """Resolve parameters whose Brightness puts the frame's log-average
        luminance at `key` (FrameStatistics.auto_brightness); **kw are the
        other fields, e.g. ToneMappingMode."""
        return cls(Brightness=stats.auto_brightness(key, q_lo, q_hi), **kw)


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


def _accumulator(a, what="accumulator") -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or a.size == 0:
        raise ValueError(f"{what} of shape {a.shape}, expected (H, W, 4)")
    return a


def frame_statistics_host(accum: np.ndarray, other: "np.ndarray | None" = None) -> FrameStatistics:
    """The frame statistics on the CPU (ptsFrameStatistics, libptscene.so):
    for saved accumulators on a machine without a GPU, and the implementation
    SampleBuffer.statistics equals bit for bit.  accum, other: (H, W, 4) XYZ
    sums + sample count; with `other`, an independent render of the same
    frame, the luminance part describes accum + other and the noise part the
    pair."""
    a = _accumulator(accum)
    b = None
    if other is not None:
        b = _accumulator(other, "second accumulator")
        if b.shape != a.shape:
            raise ValueError(f"accumulators of shapes {a.shape} and {b.shape}")
    out = N.pt_frame_statistics()
    rc = N.scene_lib().ptsFrameStatistics(a.shape[1], a.shape[0], N.fptr(a), N.fptr(b) if b is not None else None,
                                          C.byref(out))
    if rc != 0:
        raise PathTracerError(f"ptsFrameStatistics: bad arguments (status {rc})")
    return FrameStatistics(out)


def _tile_grid(width: int, height: int):
    """(tiles_y, tiles_x) of a width x height frame's 16 x 16 tiles."""
    return (int(height) + N.TILE_SIZE - 1) // N.TILE_SIZE, (int(width) + N.TILE_SIZE - 1) // N.TILE_SIZE


def tile_statistics_host(accum: np.ndarray, other: "np.ndarray | None" = None, threshold: float = 0.1) -> np.ndarray:
    """Per-tile statistics on the CPU (ptsTileStatistics, libptscene.so), which
    SampleBuffer.tile_statistics equals bit for bit: a (tiles_y, tiles_x) array
    of TILE_STATS_DTYPE records, one per 16 x 16 tile (clipped at the right and
    bottom edges).  accum, other: (H, W, 4) accumulators as for
    frame_statistics_host; without `other`, pair and over are 0.  over counts
    the pair pixels whose relative half-difference exceeds `threshold`."""
    a = _accumulator(accum)
    b = None
    if other is not None:
        b = _accumulator(other, "second accumulator")
        if b.shape != a.shape:
            raise ValueError(f"accumulators of shapes {a.shape} and {b.shape}")
    out = np.zeros(_tile_grid(a.shape[1], a.shape[0]), dtype=N.TILE_STATS_DTYPE)
    rc = N.scene_lib().ptsTileStatistics(a.shape[1], a.shape[0], N.fptr(a), N.fptr(b) if b is not None else None,
                                         float(threshold), out.ctypes.data)
    if rc != 0:
        raise PathTracerError(f"ptsTileStatistics: bad arguments (status {rc})")
    return out


def tile_mask_of_region(width: int, height: int, x0: int, y0: int, x1: int, y1: int) -> np.ndarray:
    """The (tiles_y, tiles_x) uint8 mask of the 16 x 16 tiles of a width x
    height frame that hold a pixel of [x0, x1) x [y0, y1) (clipped to the
    frame): the argument of BasicRenderer.set_active_tiles that re-renders
    that region."""
    ty, tx = _tile_grid(width, height)
    mask = np.zeros((ty, tx), dtype=np.uint8)
    x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), int(width)), min(int(y1), int(height))
    if x0 < x1 and y0 < y1:
        mask[y0 // N.TILE_SIZE:(y1 - 1) // N.TILE_SIZE + 1, x0 // N.TILE_SIZE:(x1 - 1) // N.TILE_SIZE + 1] = 1
    return mask


# refine_tiles' floor on the rounds of a tile (tools/exp_active_tiles.py;
# DESIGN.md §6 row 10).
REFINE_MIN_ROUNDS = 128


def refine_tiles(renderer_a: "BasicRenderer", renderer_b: "BasicRenderer", threshold: float, q: float = 0.95,
                 min_rounds: int = REFINE_MIN_ROUNDS, rounds_per_step: int = 8, max_rounds: int = 1024,
                 min_count: "float | None" = None):
    """Go on rendering a frame's two halves on the tiles that still need it.
    renderer_a and renderer_b are full-frame renderers on one device, on
    sample buffers of one size, FrameIndex apart by 1 << 24, already Reset
    (and, after a camera move, with FrameHistory.begin_frame's history in
    place); rounds continue from their current state.  In steps of
    `rounds_per_step` rounds (run_rounds on both, under one active tile set)
    the per-tile pair statistics of the two sample buffers are computed in one
    device pass, and a tile stays active while
      - it has run fewer than `min_rounds` rounds here, or
      - no pixel of it is a pair pixel yet (pair == 0), or
      - over > (1 - q) * pair: more than a share 1 - q of its pair pixels have
        a relative half-difference above `threshold`, or
      - `min_count` is given and some filled pixel of a + b has fewer samples
        (the tile's min_count; disoccluded pixels after a reprojection).
    It ends when no tile is active or after `max_rounds` rounds.  Returns
    (rounds, stats): the rounds run here per tile, (tiles_y, tiles_x) int64,
    and the last tile statistics.  The renderers' active tile sets are
    cleared on return, on an error too.

    min_rounds is a floor against a bias, not a tuning knob: a tile frozen
    after n rounds holds only the paths that completed within n rounds, the
    short ones, so it is darker than the converged tile wherever long paths
    carry light -- the bias of cutting a whole frame early, here local to
    the frozen tiles, where neighbours that ran longer make it visible.  The
    default is the value chosen in DESIGN.md §6 row 10."""
    if rounds_per_step < 1 or min_rounds < 0 or max_rounds < 1:
        raise ValueError("rounds_per_step >= 1, min_rounds >= 0 and max_rounds >= 1 are required")
    if not 0.0 < q <= 1.0:
        raise ValueError("q must lie in (0, 1]")
    sa, sb = renderer_a.sample_buffer, renderer_b.sample_buffer
    if (sa.width, sa.height) != (sb.width, sb.height):
        raise ValueError("the two renderers' sample buffers differ in size")
    active = np.ones(_tile_grid(sa.width, sa.height), dtype=bool)
    rounds = np.zeros(active.shape, dtype=np.int64)
    done, stats = 0, None
    try:
        while True:
            step = min(rounds_per_step, max_rounds - done)
            if done < min_rounds:
                step = min(step, min_rounds - done)   # every tile stops at min_rounds exactly, if it stops there
            for r in (renderer_a, renderer_b):
                r.set_active_tiles(None if active.all() else active)
                r.run_rounds(step)
            done += step
            rounds[active] += step
            stats = sa.tile_statistics(sb, threshold)
            need = (stats["pair"] == 0) | (stats["over"] > (1.0 - q) * stats["pair"])
            if min_count is not None:
                need |= (stats["filled"] > 0) & (stats["min_count"] < np.float32(min_count))
            if done < min_rounds:
                need[:] = True
            active &= need
            if not active.any() or done >= max_rounds:
                return rounds, stats
    finally:
        for r in (renderer_a, renderer_b):
            r.set_active_tiles(None)


def render_until_noise(renderer_a: "BasicRenderer", renderer_b: "BasicRenderer", threshold: float, q: float = 0.95,
                       check_every: int = 8, min_pair_fraction: float = 0.99, max_rounds: int = 1024):
    """Render one frame as two independent halves until it is converged:
    renderer_b.FrameIndex := renderer_a.FrameIndex + (1 << 24) (the stream
    offset), both are Reset, run Run(2) and then Run(1) rounds in lockstep;
    every `check_every` rounds the pair statistics of their two sample
    buffers are computed (sa.statistics(sb)), and the loop ends when at least
    `min_pair_fraction` of the pixels are filled in both halves and
    noise(q) <= threshold, or after `max_rounds` rounds.  The renderers are on
    one device, on sample buffers of one size that the caller has left empty
    (new ones are); RenderFlags should include ACCUMULATE.  Returns (rounds
    per half, the last FrameStatistics); sa.accumulate(sb) then makes sa the
    combined frame those statistics describe."""
    if check_every < 1 or max_rounds < 2:
        raise ValueError("check_every >= 1 and max_rounds >= 2 are required")
    sa, sb = renderer_a.sample_buffer, renderer_b.sample_buffer
    renderer_b.FrameIndex = renderer_a.FrameIndex + (1 << 24)
    for r in (renderer_a, renderer_b):
        r.reset()
    for r in (renderer_a, renderer_b):
        r.run(2)
    rounds, stats = 2, None
    while True:
        if rounds % check_every == 0 or rounds >= max_rounds:
            stats = sa.statistics(sb)
            if rounds >= max_rounds or (stats.noise_pixels >= min_pair_fraction * stats.pixels and
                                        stats.noise(q) <= threshold):
                return rounds, stats
        for r in (renderer_a, renderer_b):
            r.run(1)
        rounds += 1


class DenoiseParameters:
    """pt_denoise_parameters (pt_packed.h): the a-trous filter's iteration
    count (steps 1, 2, 4, ... 2^(Iterations-1)) and edge-stopping sigmas.  The
    defaults are the ones chosen on configs 1 and 3, 8 spp against 512 spp
    (DESIGN.md §6)."""

    def __init__(self, Iterations: int = 5, SigmaColor: float = 0.5, SigmaNormal: float = 0.25,
                 SigmaDepth: float = 0.3, SigmaAlbedo: float = 0.1):
        self.Iterations = int(Iterations)
        self.SigmaColor, self.SigmaNormal = float(SigmaColor), float(SigmaNormal)
        self.SigmaDepth, self.SigmaAlbedo = float(SigmaDepth), float(SigmaAlbedo)

    def as_struct(self) -> N.pt_denoise_parameters:
        return N.pt_denoise_parameters(self.Iterations, self.SigmaColor, self.SigmaNormal, self.SigmaDepth,
                                       self.SigmaAlbedo)


def denoise_host(accum: np.ndarray, guides: np.ndarray, params: "DenoiseParameters | None" = None) -> np.ndarray:
    """The denoiser on the CPU (ptsDenoise, libptscene.so): for saved
    accumulators on a machine without a GPU, and the implementation the
    device filter equals bit for bit.  accum: (H, W, 4) XYZ sums + sample
    count; guides: (H, W) DENOISE_GUIDE_DTYPE records.  Returns (H, W, 4):
    the denoised mean XYZ and 1 (zeros where the count is not positive)."""
    a = np.ascontiguousarray(accum, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"accumulator of shape {a.shape}, expected (H, W, 4)")
    g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.shape != a.shape[:2]:
        raise ValueError(f"guides of shape {g.shape}, accumulator {a.shape[:2]}")
    out = np.zeros_like(a)
    p = (params or DenoiseParameters()).as_struct()
    rc = N.scene_lib().ptsDenoise(a.shape[1], a.shape[0], N.fptr(a), g.ctypes.data, C.byref(p), N.fptr(out))
    if rc != 0:
        raise PathTracerError(f"ptsDenoise: bad arguments (status {rc})")
    return out


class DenoisePairParameters:
    """pt_denoise_pair_parameters (pt_packed.h): the variance-guided filter
    over two half renders.  SigmaLuminance is in standard deviations of the
    pixel's luminance, estimated from the two halves; the other sigmas are
    DenoiseParameters'.  The defaults are the ones chosen on configs 1, 2, 3
    and 5 at 2x4, 2x32 and 2x128 rounds against 2048."""

    def __init__(self, Iterations: int = 5, SigmaLuminance: float = 4.0, SigmaNormal: float = 0.25,
                 SigmaDepth: float = 0.3, SigmaAlbedo: float = 0.1):
        self.Iterations = int(Iterations)
        self.SigmaLuminance, self.SigmaNormal = float(SigmaLuminance), float(SigmaNormal)
        self.SigmaDepth, self.SigmaAlbedo = float(SigmaDepth), float(SigmaAlbedo)

    def as_struct(self) -> N.pt_denoise_pair_parameters:
        return N.pt_denoise_pair_parameters(self.Iterations, self.SigmaLuminance, self.SigmaNormal, self.SigmaDepth,
                                            self.SigmaAlbedo)


def denoise_pair_host(accum_a: np.ndarray, accum_b: np.ndarray, guides: np.ndarray,
                      params: "DenoisePairParameters | None" = None) -> np.ndarray:
    """The variance-guided denoiser on the CPU (ptsDenoisePair,
    libptscene.so), which the device filter equals bit for bit.  accum_a,
    accum_b: (H, W, 4) accumulators of two independent renders of one frame
    (FrameIndex apart by 1 << 24); guides: (H, W) DENOISE_GUIDE_DTYPE records.
    Returns (H, W, 4): the denoised mean XYZ of a + b and 1 (zeros where the
    combined count is not positive)."""
    a = np.ascontiguousarray(accum_a, dtype=np.float32)
    b = np.ascontiguousarray(accum_b, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"accumulator of shape {a.shape}, expected (H, W, 4)")
    if b.shape != a.shape:
        raise ValueError(f"second accumulator of shape {b.shape}, first {a.shape}")
    g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.shape != a.shape[:2]:
        raise ValueError(f"guides of shape {g.shape}, accumulator {a.shape[:2]}")
    out = np.zeros_like(a)
    p = (params or DenoisePairParameters()).as_struct()
    rc = N.scene_lib().ptsDenoisePair(a.shape[1], a.shape[0], N.fptr(a), N.fptr(b), g.ctypes.data, C.byref(p),
                                      N.fptr(out))
    if rc != 0:
        raise PathTracerError(f"ptsDenoisePair: bad arguments (status {rc})")
    return out


class ReprojectParameters:
    """pt_reproject_parameters (pt_packed.h): which taps of the previous
    frame still show a pixel's surface (NormalCosine, DepthTolerance), how
    much valid bilinear weight makes a history (MinWeight) and the cap on the
    carried sample count (MaxHistory; inf: none).  The defaults are the ones
    settled on configs 1 and 3 after a small pan, 128 rounds of history and 2
    or 8 new ones against 4096."""

    def __init__(self, NormalCosine: float = 0.9, DepthTolerance: float = 0.05, MinWeight: float = 0.25,
                 MaxHistory: float = 64.0):
        self.NormalCosine, self.DepthTolerance = float(NormalCosine), float(DepthTolerance)
        self.MinWeight, self.MaxHistory = float(MinWeight), float(MaxHistory)

    def as_struct(self) -> N.pt_reproject_parameters:
        return N.pt_reproject_parameters(self.NormalCosine, self.DepthTolerance, self.MinWeight, self.MaxHistory)


def _camera_struct(camera) -> N.pt_packed_camera:
    """A packed camera record (scene.arrays()["cameras"][i]) as the C struct."""
    if isinstance(camera, N.pt_packed_camera):
        return camera
    c = np.asarray(camera, dtype=N.CAMERA_DTYPE)
    if c.shape != ():
        raise ValueError(f"one camera record expected, got shape {c.shape}")
    return N.pt_packed_camera.from_buffer_copy(c.tobytes())


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
    rc = N.scene_lib().ptsShapeMotion(ps.ctypes.data if ps.size else None, ps.size, cs.ctypes.data if cs.size else None,
                                      cs.size, out.ctypes.data if cs.size else None)
    if rc != 0:
        raise PathTracerError(f"ptsShapeMotion: bad arguments (status {rc})")
    return out


def _motion_table(motion):
    """(array kept alive, pointer or None, count) of an optional motion table."""
    if motion is None:
        return None, None, 0
    m = np.ascontiguousarray(motion, dtype=N.SHAPE_MOTION_DTYPE).reshape(-1)
    if m.size == 0:                      # an empty table is still a table: every hit is beyond it
        m = np.zeros(1, dtype=N.SHAPE_MOTION_DTYPE)
        return m, m.ctypes.data, 0
    return m, m.ctypes.data, m.size


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
    a = np.ascontiguousarray(prev_accum, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"accumulator of shape {a.shape}, expected (H, W, 4)")
    pg = np.ascontiguousarray(prev_guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if pg.shape != a.shape[:2]:
        raise ValueError(f"previous guides of shape {pg.shape}, accumulator {a.shape[:2]}")
    g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.ndim != 2:
        raise ValueError(f"guides of shape {g.shape}, expected (H, W)")
    out = np.zeros(g.shape + (4,), np.float32)
    pc, c = _camera_struct(prev_camera), _camera_struct(camera)
    p = (params or ReprojectParameters()).as_struct()
    if motion is not None:
        m, mp, mn = _motion_table(motion)
        rc = N.scene_lib().ptsReprojectMoving(a.shape[1], a.shape[0], N.fptr(a), pg.ctypes.data, C.byref(pc),
                                              g.shape[1], g.shape[0], g.ctypes.data, C.byref(c), mp, mn, C.byref(p),
                                              N.fptr(out))
        if rc != 0:
            raise PathTracerError(f"ptsReprojectMoving: bad arguments (status {rc})")
        return out
    rc = N.scene_lib().ptsReproject(a.shape[1], a.shape[0], N.fptr(a), pg.ctypes.data, C.byref(pc), g.shape[1],
                                    g.shape[0], g.ctypes.data, C.byref(c), C.byref(p), N.fptr(out))
    if rc != 0:
        raise PathTracerError(f"ptsReproject: bad arguments (status {rc})")
    return out


class RectifyParameters:
    """pt_rectify_parameters (pt_packed.h): the window of new samples a
    carried history is held against (Radius; MinNeighbours members or the
    pixel stays untested; NormalCosine between a member's normal and the
    centre's), the half width of the allowed box in standard deviations
    (Sigma) and the cap on a clipped pixel's sample count (ClampedHistory;
    inf: none).  The defaults are the setting tools/exp_rectify.py's rule
    chose; MinNeighbours 25 is meant for Radius 3's 49
    pixels: lower it with the radius (a Radius 1 window has 9)."""

    def __init__(self, Radius: int = 3, MinNeighbours: int = 25, Sigma: float = 1.0, ClampedHistory: float = 8.0,
                 NormalCosine: float = 0.9):
        self.Radius, self.MinNeighbours = int(Radius), int(MinNeighbours)
        self.Sigma, self.ClampedHistory, self.NormalCosine = float(Sigma), float(ClampedHistory), float(NormalCosine)

    def as_struct(self) -> N.pt_rectify_parameters:
        # Out-of-range counts reach the library's check instead of ctypes' wrap-around.
        return N.pt_rectify_parameters(min(max(self.Radius, 0), 0xFFFFFFFF), min(max(self.MinNeighbours, 0), 0xFFFFFFFF),
                                       self.Sigma, self.ClampedHistory, self.NormalCosine)


def rectify_host(history: np.ndarray, current: np.ndarray, guides: np.ndarray,
                 params: "RectifyParameters | None" = None) -> np.ndarray:
    """History validation on the CPU (ptsRectifyHistory, libptscene.so), which
    the device kernel equals bit for bit.  history: (H, W, 4) accumulator in
    (mean * n, n) form, e.g. reproject_host's result; current: the (H, W, 4)
    accumulator of the new rounds alone; guides: the current view's (H, W)
    DENOISE_GUIDE_DTYPE records.  Returns the (H, W, 4) history with every
    pixel's mean pulled into the box its window of current samples allows and
    the count of a pulled pixel cut."""
    a = np.ascontiguousarray(history, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"history of shape {a.shape}, expected (H, W, 4)")
    b = np.ascontiguousarray(current, dtype=np.float32)
    if b.shape != a.shape:
        raise ValueError(f"current accumulator of shape {b.shape}, history {a.shape}")
    g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.shape != a.shape[:2]:
        raise ValueError(f"guides of shape {g.shape}, accumulator {a.shape[:2]}")
    out = np.zeros_like(a)
    p = (params or RectifyParameters()).as_struct()
    rc = N.scene_lib().ptsRectifyHistory(a.shape[1], a.shape[0], N.fptr(a), N.fptr(b), g.ctypes.data, C.byref(p),
                                         N.fptr(out))
    if rc != 0:
        raise PathTracerError(f"ptsRectifyHistory: bad arguments (status {rc})")
    return out


class DespikeParameters:
    """pt_despike_parameters (pt_packed.h): the firefly clamp's window
    (Radius; MinNeighbours members or the pixel stays untested; NormalCosine
    between a member's normal and the centre's), which neighbour is the
    yardstick (the Rank-th largest value, so that Rank - 1 fireflies in a
    window do not raise it) and the limit Scale * yardstick + Floor above
    which a pixel is scaled down.  The defaults are the setting
    tools/exp_despike.py's rule chose: Scale 1 clamps
    every pixel above its window's third brightest neighbour, 7 to 8 % of a
    frame, and removes 1 to 20 % of a noisy frame's energy; Scale 2 touches
    fireflies only.  MinNeighbours 8 suits every radius (a Radius 1 window
    has 8 neighbours)."""

    def __init__(self, Radius: int = 3, Rank: int = 3, MinNeighbours: int = 8, Scale: float = 1.0, Floor: float = 0.0,
                 NormalCosine: float = 0.9):
        self.Radius, self.Rank, self.MinNeighbours = int(Radius), int(Rank), int(MinNeighbours)
        self.Scale, self.Floor, self.NormalCosine = float(Scale), float(Floor), float(NormalCosine)

    def as_struct(self) -> N.pt_despike_parameters:
        # Out-of-range counts reach the library's check instead of ctypes' wrap-around.
        u = [min(max(v, 0), 0xFFFFFFFF) for v in (self.Radius, self.Rank, self.MinNeighbours)]
        return N.pt_despike_parameters(u[0], u[1], u[2], self.Scale, self.Floor, self.NormalCosine)


def despike_host(accum: np.ndarray, guides: np.ndarray, params: "DespikeParameters | None" = None) -> np.ndarray:
    """The firefly clamp on the CPU (ptsDespike, libptscene.so), which the
    device kernel equals bit for bit.  accum: (H, W, 4) XYZ sums + sample
    count; guides: the same view's (H, W) DENOISE_GUIDE_DTYPE records.
    Returns the (H, W, 4) accumulator with the colour sums of every pixel that
    stands out of its window scaled down onto the window's limit; every other
    pixel and every count keeps its bits."""
    a = np.ascontiguousarray(accum, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"accumulator of shape {a.shape}, expected (H, W, 4)")
    g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.shape != a.shape[:2]:
        raise ValueError(f"guides of shape {g.shape}, accumulator {a.shape[:2]}")
    out = np.zeros_like(a)
    p = (params or DespikeParameters()).as_struct()
    rc = N.scene_lib().ptsDespike(a.shape[1], a.shape[0], N.fptr(a), g.ctypes.data, C.byref(p), N.fptr(out))
    if rc != 0:
        raise PathTracerError(f"ptsDespike: bad arguments (status {rc})")
    return out


class DenoiseGuides:
    """Per-pixel primary-hit records of the scene camera's central rays
    (normal, hit time, base colour, shape) that steer the denoiser, plus the
    filter's intermediate image (ptCreateDenoiseGuides)."""

    def __init__(self, device: "Device", width: int, height: int):
        L = N.hip_lib()
        self.device = device
        self.width, self.height = int(width), int(height)
        self._h = L.ptCreateDenoiseGuides(device.handle, self.width, self.height)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())

    @property
    def handle(self):
        return self._h

    def render(self, scene: "DeviceScene", camera_index: int = 0, specular_bounces: int = 0):
        """One central camera ray per pixel of packed camera `camera_index` (enqueues).
        specular_bounces (up to GUIDE_MAX_BOUNCES): the ray is followed through
        that many perfect mirrors and smooth glass surfaces, and the record
        describes the surface the pixel shows (ptRenderDenoiseGuidesSpecular;
        DESIGN.md §6 row 13).  0: the primary hit (ptRenderDenoiseGuides)."""
        if int(specular_bounces) == 0:
            _check(N.hip_lib().ptRenderDenoiseGuides(self.device.handle, scene.handle, self._h, int(camera_index)),
                   "ptRenderDenoiseGuides")
            return
        if int(specular_bounces) < 0:
            raise ValueError(f"specular_bounces: {specular_bounces}")
        _check(N.hip_lib().ptRenderDenoiseGuidesSpecular(self.device.handle, scene.handle, self._h, int(camera_index),
                                                         int(specular_bounces)), "ptRenderDenoiseGuidesSpecular")

    def read(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), dtype=N.DENOISE_GUIDE_DTYPE)
        _check(N.hip_lib().ptReadDenoiseGuides(self.device.handle, self._h, out.ctypes.data), "ptReadDenoiseGuides")
        return out

    def write(self, guides: np.ndarray):
        g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
        if g.size != self.width * self.height:
            raise ValueError(f"guides have {g.size} pixels, the object {self.width * self.height}")
        _check(N.hip_lib().ptWriteDenoiseGuides(self.device.handle, self._h, g.ctypes.data), "ptWriteDenoiseGuides")

    def set_variant(self, variant: int):
        """DENOISE_VARIANT_AUTO / _GATHER / _LATTICE: the filter kernel used
        (identical results; ptSetDenoiseVariant)."""
        _check(N.hip_lib().ptSetDenoiseVariant(self._h, int(variant)), "ptSetDenoiseVariant")

    def close(self):
        if self._h:
            N.hip_lib().ptDestroyDenoiseGuides(self.device.handle, self._h)
            self._h = None


class SampleBuffer:
    """rgba32f accumulator: CIE XYZ sums + sample count (integrator.cpp:15-87)."""

    def __init__(self, device: Device, width: int, height: int):
        L = N.hip_lib()
        self.device = device
        self.width, self.height = int(width), int(height)
        self._h = L.ptCreateSampleBuffer(device.handle, self.width, self.height)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())

    @property
    def handle(self):
        return self._h

    def read(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(N.hip_lib().ptReadSampleBuffer(self.device.handle, self._h, N.fptr(out)), "ptReadSampleBuffer")
        return out

    def write(self, rgba: np.ndarray):
        """Overwrite the accumulator (resume accumulation from a saved one)."""
        a = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.height, self.width, 4)
        _check(N.hip_lib().ptWriteSampleBuffer(self.device.handle, self._h, N.fptr(a)), "ptWriteSampleBuffer")

    def render(self, params: "ResolveParameters | None" = None, **kw):
        """RenderSampleBuffer (integrator.hpp:55-60): resolve on the device."""
        p = (params or ResolveParameters(**kw)).as_struct()
        _check(N.hip_lib().ptRenderSampleBuffer(self.device.handle, self._h, C.byref(p)), "ptRenderSampleBuffer")

    def denoise(self, guides: "DenoiseGuides", params: "DenoiseParameters | None" = None,
                out: "SampleBuffer | None" = None) -> "SampleBuffer":
        """The edge-avoiding a-trous filter on the device (ptDenoiseSampleBuffer;
        enqueues): `out` (a new sample buffer of this size when None) receives
        the denoised mean XYZ and a sample count of 1, so out.render(...) and
        out.read() work as on any sample buffer.  This buffer is not written."""
        dst = out if out is not None else SampleBuffer(self.device, self.width, self.height)
        p = (params or DenoiseParameters()).as_struct()
        try:
            _check(N.hip_lib().ptDenoiseSampleBuffer(self.device.handle, self._h, guides.handle, C.byref(p),
                                                     dst.handle), "ptDenoiseSampleBuffer")
        except PathTracerError:
            if out is None:
                dst.close()
            raise
        return dst

    def denoise_pair(self, other: "SampleBuffer", guides: "DenoiseGuides",
                     params: "DenoisePairParameters | None" = None,
                     out: "SampleBuffer | None" = None) -> "SampleBuffer":
        """The variance-guided filter on the device (ptDenoiseSampleBufferPair;
        enqueues) over this buffer and `other`, two independent renders of one
        frame (e.g. render_until_noise's halves): `out` (a new sample buffer
        of this size when None) receives the denoised mean XYZ of this + other
        and a sample count of 1, as denoise() leaves it.  Neither input is
        written."""
        dst = out if out is not None else SampleBuffer(self.device, self.width, self.height)
        p = (params or DenoisePairParameters()).as_struct()
        try:
            _check(N.hip_lib().ptDenoiseSampleBufferPair(self.device.handle, self._h, other.handle, guides.handle,
                                                         C.byref(p), dst.handle), "ptDenoiseSampleBufferPair")
        except PathTracerError:
            if out is None:
                dst.close()
            raise
        return dst

    def despike(self, guides: "DenoiseGuides", params: "DespikeParameters | None" = None,
                out: "SampleBuffer | None" = None) -> "SampleBuffer":
        """The firefly clamp on the device (ptDespikeSampleBuffer; enqueues):
        `out` (a new sample buffer of this size when None; never this buffer)
        receives this accumulator with the pixels that stand out of their
        window scaled down onto the window's limit, counts unchanged, so that
        out.denoise(...), out.denoise_pair(...), other.accumulate(out) and
        rectify work on it as on any accumulator.  One call per buffer: for
        two halves, a.despike(g) and b.despike(g) before denoise_pair.  This
        buffer and the guides are not written."""
        dst = out if out is not None else SampleBuffer(self.device, self.width, self.height)
        p = (params or DespikeParameters()).as_struct()
        try:
            _check(N.hip_lib().ptDespikeSampleBuffer(self.device.handle, self._h, guides.handle, C.byref(p),
                                                     dst.handle), "ptDespikeSampleBuffer")
        except PathTracerError:
            if out is None:
                dst.close()
            raise
        return dst

    def reproject(self, prev_guides: "DenoiseGuides", prev_camera, guides: "DenoiseGuides", camera,
                  params: "ReprojectParameters | None" = None, out: "SampleBuffer | None" = None,
                  motion: "np.ndarray | None" = None) -> "SampleBuffer":
        """Temporal reprojection on the device (ptReprojectSampleBuffer;
        enqueues): this buffer is the previous view's accumulator, prev_guides
        and prev_camera its guides and packed camera record, guides and camera
        the current view's.  `out` (a new sample buffer of the guides' size
        when None) receives (mean XYZ * n, n) per pixel, zeros where the pixel
        is disoccluded; a renderer with RENDER_FLAG_ACCUMULATE adds its
        samples on top.  This buffer and both guides are not written.
        motion: a shape_motion() table; pixels of moved shapes then follow
        them (ptReprojectSampleBufferMoving)."""
        dst = out if out is not None else SampleBuffer(self.device, guides.width, guides.height)
        pc, c = _camera_struct(prev_camera), _camera_struct(camera)
        p = (params or ReprojectParameters()).as_struct()
        try:
            if motion is not None:
                m, mp, mn = _motion_table(motion)
                _check(N.hip_lib().ptReprojectSampleBufferMoving(self.device.handle, self._h, prev_guides.handle,
                                                                 C.byref(pc), guides.handle, C.byref(c), mp, mn,
                                                                 C.byref(p), dst.handle),
                       "ptReprojectSampleBufferMoving")
            else:
                _check(N.hip_lib().ptReprojectSampleBuffer(self.device.handle, self._h, prev_guides.handle,
                                                           C.byref(pc), guides.handle, C.byref(c), C.byref(p),
                                                           dst.handle),
                       "ptReprojectSampleBuffer")
        except PathTracerError:
            if out is None:
                dst.close()
            raise
        return dst

    def rectify(self, current: "SampleBuffer", guides: "DenoiseGuides", params: "RectifyParameters | None" = None,
                out: "SampleBuffer | None" = None) -> "SampleBuffer":
        """History validation on the device (ptRectifyHistory; enqueues): this
        buffer is a carried history in (mean * n, n) form, `current` the
        accumulator of the new rounds alone, `guides` the current view's.
        `out` (this buffer itself when None: in place) receives the history
        pulled into the box each pixel's window of current samples allows,
        with the count of a pulled pixel cut; current.accumulate(out) then
        gives the frame to go on rendering into.  current and guides are not
        written."""
        dst = out if out is not None else self
        p = (params or RectifyParameters()).as_struct()
        _check(N.hip_lib().ptRectifyHistory(self.device.handle, self._h, current.handle, guides.handle, C.byref(p),
                                            dst.handle), "ptRectifyHistory")
        return dst

    def statistics(self, other: "SampleBuffer | None" = None) -> FrameStatistics:
        """Frame statistics on the device (ptComputeFrameStatistics; blocks):
        of this buffer, or, with `other` (an independent render of the same
        frame), of this + other with the noise histogram of the pair.
        Neither buffer is written."""
        out = N.pt_frame_statistics()
        _check(N.hip_lib().ptComputeFrameStatistics(self.device.handle, self._h,
                                                    other.handle if other is not None else None, C.byref(out)),
               "ptComputeFrameStatistics")
        return FrameStatistics(out)

    def tile_statistics(self, other: "SampleBuffer | None" = None, threshold: float = 0.1) -> np.ndarray:
        """Per-tile statistics on the device (ptComputeTileStatistics; blocks,
        one launch): a (tiles_y, tiles_x) array of TILE_STATS_DTYPE records of
        this buffer's 16 x 16 tiles, or, with `other`, of this + other with
        the pair counts (over: pair pixels whose relative half-difference
        exceeds `threshold`).  Neither buffer is written."""
        out = np.zeros(_tile_grid(self.width, self.height), dtype=N.TILE_STATS_DTYPE)
        _check(N.hip_lib().ptComputeTileStatistics(self.device.handle, self._h,
                                                   other.handle if other is not None else None, float(threshold),
                                                   out.ctypes.data), "ptComputeTileStatistics")
        return out

    def accumulate(self, src: "SampleBuffer"):
        """This accumulator += src's, per component in float32, on the device
        (ptAccumulateSampleBuffer; enqueues).  src is not written."""
        _check(N.hip_lib().ptAccumulateSampleBuffer(self.device.handle, self._h, src.handle),
               "ptAccumulateSampleBuffer")

    def read_resolved(self) -> np.ndarray:
        """OutColor of the last render(): (H, W, 4) float32, alpha 1."""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(N.hip_lib().ptReadResolvedImage(self.device.handle, self._h, N.fptr(out)), "ptReadResolvedImage")
        return out

    def read_srgb8(self) -> np.ndarray:
        """The resolved image as B8G8R8A8_SRGB stores it: (H, W, 4) uint8, RGBA order."""
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        _check(N.hip_lib().ptReadResolvedImageSRGB8(self.device.handle, self._h,
                                                    out.ctypes.data_as(C.POINTER(C.c_uint8))),
               "ptReadResolvedImageSRGB8")
        return out

    def close(self):
        if self._h:
            N.hip_lib().ptDestroySampleBuffer(self.device.handle, self._h)
            self._h = None


class FrameHistory:
    """Keeps the last frame (its sample buffer, guides, camera record and, with
    follow_shapes, packed shapes) so
    that the next one starts from it: begin_frame() renders the new view's
    guides and reprojects the stored frame into the new sample buffer.  Thin
    glue over DenoiseGuides.render and SampleBuffer.reproject."""

    def __init__(self, device: "Device", width: int, height: int, params: "ReprojectParameters | None" = None,
                 follow_shapes: bool = False, validate: "RectifyParameters | bool | None" = None,
                 specular_bounces: int = 0):
        """follow_shapes: also keep the frame's packed shapes and reproject
        with the motion table between the two frames (shape_motion), so that
        a moved object keeps its history.  The scene's entities must be the
        same from frame to frame.
        validate: True (default RectifyParameters) or a RectifyParameters:
        the history is held against the new frame's own samples before it
        counts, so that shading that changed without
        any geometry changing loses its weight.  begin_frame() then
        reprojects into a buffer this object owns and leaves the frame's
        sample buffer cleared; merge() joins the two after the frame's first
        run().
        specular_bounces: passed to every guide render this object makes
        (DenoiseGuides.render).  With follow_shapes a
        pixel seen through a mirror or smooth glass then carries a tagged shape
        word, which no motion record covers: it gets no history."""
        self.device = device
        self.width, self.height = int(width), int(height)
        self.params = params
        self.specular_bounces = int(specular_bounces)
        self.follow_shapes = bool(follow_shapes)
        if validate is None or validate is False:
            self.validate = None
        elif validate is True:
            self.validate = RectifyParameters()
        elif isinstance(validate, RectifyParameters):
            self.validate = validate
        else:
            raise ValueError(f"validate: True or a RectifyParameters expected, got {validate!r}")
        self.held = None           # validate: the reprojected history until merge() (owned)
        self._unmerged = False      # validate: begin_frame() was called and merge() not yet
        self._carried = False       # the last begin_frame() carried a history
        self.shapes = None          # the last frame's packed shapes (follow_shapes)
        self._spare = DenoiseGuides(device, self.width, self.height)
        self.guides = None          # the current frame's guides (after begin_frame)
        self.buffer = None          # the sample buffer passed to the last begin_frame (non-owning)
        self.camera = None          # its packed camera record

    def begin_frame(self, ds: "DeviceScene", camera_index: int, sample_buffer: "SampleBuffer") -> bool:
        """Call after ds.update(scene) and after the frame's renderer.reset()
        (a Reset clears its sample buffer, pixel by pixel, as the reference's
        restart does), before its run(): the new rounds then accumulate on
        top of the history.  sample_buffer is of this history's size and not
        the last call's buffer.  True: it now holds the reprojected history;
        False (first call): it was left as it is.  The buffer passed here
        must stay alive until the next call, which reads what the renderer
        has accumulated in it by then.
        With validate the reprojected history goes into a buffer this object
        holds and sample_buffer is left as the Reset cleared it; the return
        value is the same.  Call merge(sample_buffer) after the frame's first
        run(): a history that is never merged is dropped."""
        if sample_buffer.width != self.width or sample_buffer.height != self.height:
            raise ValueError(f"sample buffer {sample_buffer.width}x{sample_buffer.height}, history "
                             f"{self.width}x{self.height}")
        camera = ds.cameras[int(camera_index)].copy()
        guides = self._spare
        guides.render(ds, camera_index, self.specular_bounces)
        carried = self.buffer is not None
        shapes = ds.shapes.copy() if self.follow_shapes else None
        if carried:
            motion = shape_motion(self.shapes, shapes) if self.follow_shapes else None
            dst = sample_buffer
            if self.validate is not None:
                if self.held is None:
                    self.held = SampleBuffer(self.device, self.width, self.height)
                dst = self.held
            self.buffer.reproject(self.guides, self.camera, guides, camera, self.params, out=dst, motion=motion)
        self.shapes = shapes
        if self.guides is None:
            self._spare = DenoiseGuides(self.device, self.width, self.height)
        else:
            self._spare = self.guides
        self.guides, self.buffer, self.camera = guides, sample_buffer, camera
        self._carried, self._unmerged = carried, self.validate is not None
        return carried

    def merge(self, sample_buffer: "SampleBuffer"):
        """With validate, after the frame's first run(k): holds the history
        begin_frame() reprojected against the k rounds sample_buffer now
        holds (SampleBuffer.rectify, in place) and adds it to them
        (sample_buffer.accumulate); both enqueue.  Further run() calls then
        accumulate on top, and refine_tiles(min_count=...) goes on rendering
        where the count was cut.  Does nothing on the first frame, which
        carried nothing.  sample_buffer is begin_frame()'s."""
        if self.validate is None:
            raise ValueError("merge: this FrameHistory was created without validate")
        if not self._unmerged:
            raise ValueError("merge: no begin_frame() since the last merge()")
        if sample_buffer is not self.buffer:
            raise ValueError("merge: not the sample buffer passed to begin_frame()")
        self._unmerged = False
        if not self._carried:
            return
        self.held.rectify(sample_buffer, self.guides, self.validate)
        sample_buffer.accumulate(self.held)

    def close(self):
        for g in (self._spare, self.guides, self.held):
            if g is not None:
                g.close()
        self._spare = self.guides = self.buffer = self.held = None
        self._unmerged = False


class BasicRenderer:
    """basic_renderer (basic.hpp:6-26) running the HIP wavefront kernels."""

    _FIELDS = ("FrameIndex", "CameraIndex", "RenderFlags", "PathLengthLimit", "PathTerminationProbability")

    def __init__(self, device: Device, scene: DeviceScene, sample_buffer: SampleBuffer, rank: int = 0, nranks: int = 1,
                 streams: int = 1):
        """rank / nranks: the 16-row pixel bands owned (b % nranks == rank);
        streams: independent paths per owned pixel, stream k seeded at
        FrameIndex + (k << 24) (ptCreateBasicRendererStreams)."""
        L = N.hip_lib()
        self.device, self.scene, self.sample_buffer = device, scene, sample_buffer
        self.rank, self.nranks, self.streams = rank, nranks, streams
        self._h = L.ptCreateBasicRendererStreams(device.handle, scene.handle, sample_buffer.handle, rank, nranks,
                                                 streams)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())
        self._params = L.ptBasicRendererParams(self._h)

    def __getattr__(self, name):
        if name in BasicRenderer._FIELDS:
            return getattr(self._params.contents, name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in BasicRenderer._FIELDS:
            setattr(self._params.contents, name, value)
        else:
            object.__setattr__(self, name, value)

    @property
    def handle(self):
        return self._h

    @property
    def slot_count(self) -> int:
        return int(N.hip_lib().ptBasicRendererSlotCount(self._h))

    def merge_streams(self):
        """The sample buffer's owned pixels := the sum of every stream's
        accumulator, stream 0 included, in stream order
        ((A0 + A1) + A2 ...; ptMergeBasicRendererStreams).  The streams are
        not cleared and keep accumulating, so a later merge writes the new
        totals (not deltas).  A no-op for one stream."""
        _check(N.hip_lib().ptMergeBasicRendererStreams(self.device.handle, self._h), "ptMergeBasicRendererStreams")

    def set_fused_rounds(self, mode: int):
        """0 never / 1 automatic / 2 whenever possible (ptSetBasicRendererFusedRounds)."""
        _check(N.hip_lib().ptSetBasicRendererFusedRounds(self._h, int(mode)), "ptSetBasicRendererFusedRounds")

    def set_round_batch(self, rounds: int):
        """Rounds per launch for consecutive Run(1) rounds (run_rounds,
        render_frame): 0 automatic (16 when every tile fits on the GPU at
        once), 1 never (one launch per round), R >= 2 always R."""
        _check(N.hip_lib().ptSetBasicRendererRoundBatch(self._h, int(rounds)), "ptSetBasicRendererRoundBatch")

    def set_split(self, groups: int):
        """Tile groups of consecutive rounds, each on its own HIP stream
        (ptSetBasicRendererSplit): 0 automatic, 1 off, 2..MAX_SPLIT that many.
        Results are identical for every value."""
        _check(N.hip_lib().ptSetBasicRendererSplit(self._h, int(groups)), "ptSetBasicRendererSplit")

    def split(self) -> dict:
        """{groups, timed_tiles, tiles}: the tile groups consecutive rounds use
        now, group 0's tiles (the launches kernel profiling times) and all
        tiles (ptGetBasicRendererSplit)."""
        g, t0, t = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(N.hip_lib().ptGetBasicRendererSplit(self._h, C.byref(g), C.byref(t0), C.byref(t)),
               "ptGetBasicRendererSplit")
        return {"groups": int(g.value), "timed_tiles": int(t0.value), "tiles": int(t.value)}

    def set_class_lists(self, mode: int):
        """Class-pure shade inside tile groups (ptSetBasicRendererClassLists):
        0 automatic, 1 off.  Results are identical either way."""
        _check(N.hip_lib().ptSetBasicRendererClassLists(self._h, int(mode)), "ptSetBasicRendererClassLists")

    def class_lists(self) -> bool:
        """Whether consecutive rounds shade through per-class lists now."""
        u = C.c_uint32(0)
        _check(N.hip_lib().ptGetBasicRendererClassLists(self._h, C.byref(u)), "ptGetBasicRendererClassLists")
        return bool(u.value)

    def set_ray_order(self, order: int):
        """Where a tile's new rays sit (ptSetBasicRendererRayOrder): 0
        automatic, 1 by direction octant, 2 by predicted traversal length.
        Results are identical in every order."""
        _check(N.hip_lib().ptSetBasicRendererRayOrder(self._h, int(order)), "ptSetBasicRendererRayOrder")

    def ray_order(self) -> dict:
        """{order, used}: the order set and the one the next unfused rounds
        use, 1 octant or 2 length (ptGetBasicRendererRayOrder)."""
        o, u = C.c_uint32(0), C.c_uint32(0)
        _check(N.hip_lib().ptGetBasicRendererRayOrder(self._h, C.byref(o), C.byref(u)), "ptGetBasicRendererRayOrder")
        return {"order": int(o.value), "used": int(u.value)}

    def ray_positions(self) -> np.ndarray:
        """Per slot, the position of its ray (high byte) and of its last hit
        (low byte) within its tile (diagnostic, ptReadBasicRendererRayPositions)."""
        out = np.zeros(self._slot_count(), dtype=np.uint16)
        _check(N.hip_lib().ptReadBasicRendererRayPositions(self.device.handle, self._h, out.ctypes.data),
               "ptReadBasicRendererRayPositions")
        return out

    def set_active_tiles(self, mask: "np.ndarray | None"):
        """The tiles the following rounds run on (ptSetBasicRendererActiveTiles):
        a (tiles_y, tiles_x) array, non-zero = active (tile_mask_of_region
        builds one), or None for every tile.  An active tile's results equal
        an unmasked render's bit for bit; an inactive tile is not touched.
        Full-frame, single-stream renderers only; render_frame is refused
        while a mask is set.  Waits for the device."""
        if mask is None:
            _check(N.hip_lib().ptSetBasicRendererActiveTiles(self.device.handle, self._h, None, 0),
                   "ptSetBasicRendererActiveTiles")
            return
        m = np.asarray(mask)
        grid = _tile_grid(self.sample_buffer.width, self.sample_buffer.height)
        if m.shape != grid:
            raise ValueError(f"mask of shape {m.shape}, the frame has {grid} tiles")
        m = np.ascontiguousarray(m != 0, dtype=np.uint8)
        _check(N.hip_lib().ptSetBasicRendererActiveTiles(self.device.handle, self._h, m.ctypes.data, m.size),
               "ptSetBasicRendererActiveTiles")

    def active_tiles(self) -> dict:
        """{active, tiles}: the tiles the next round launches and all tiles
        (ptGetBasicRendererActiveTiles)."""
        a, t = C.c_uint32(0), C.c_uint32(0)
        _check(N.hip_lib().ptGetBasicRendererActiveTiles(self._h, C.byref(a), C.byref(t)),
               "ptGetBasicRendererActiveTiles")
        return {"active": int(a.value), "tiles": int(t.value)}

    def run_rounds(self, count: int):
        """count consecutive Run(1) calls (one new FrameIndex each), batched
        per set_round_batch (ptRunBasicRendererRounds)."""
        _check(N.hip_lib().ptRunBasicRendererRounds(self.device.handle, self._h, int(count)),
               "ptRunBasicRendererRounds")

    def set_openpbr(self, enable: bool):
        """Shade OpenPBR materials (ptSetBasicRendererOpenPBR); off by default,
        as in the reference, where an OpenPBR hit ends the path."""
        _check(N.hip_lib().ptSetBasicRendererOpenPBR(self._h, int(bool(enable))), "ptSetBasicRendererOpenPBR")

    def reset(self):
        _check(N.hip_lib().ptResetBasicRenderer(self.device.handle, self._h), "ptResetBasicRenderer")

    def run(self, rounds: int = 1):
        _check(N.hip_lib().ptRunBasicRenderer(self.device.handle, self._h, int(rounds)), "ptRunBasicRenderer")

    def render_frame(self, target_samples: int, max_rounds: int = 1 << 30):
        """Benchmark-mode frame (ptRenderFrame): Reset,
        Run(2), then Run(1) rounds until target_samples paths completed since
        the Reset.  Blocks; returns (rounds, samples)."""
        rounds, samples = C.c_uint32(0), C.c_uint64(0)
        _check(N.hip_lib().ptRenderFrame(self.device.handle, self._h, int(target_samples), int(max_rounds),
                                         C.byref(rounds), C.byref(samples)), "ptRenderFrame")
        return int(rounds.value), int(samples.value)

    def stats(self):
        """(rays traced, paths completed) since the last Reset (ptGetStats)."""
        rays, samples = C.c_uint64(0), C.c_uint64(0)
        _check(N.hip_lib().ptGetStats(self.device.handle, self._h, C.byref(rays), C.byref(samples)), "ptGetStats")
        return int(rays.value), int(samples.value)

    def extend_stats(self) -> dict:
        """Traversal counters of the current rays (diagnostic, ptExtendStats)."""
        out = (C.c_uint64 * 14)()
        _check(N.hip_lib().ptExtendStats(self.device.handle, self._h, out), "ptExtendStats")
        keys = ("rays", "lane_steps", "wave_steps_x64", "internal_nodes", "blas_leaves", "faces", "pops",
                "tlas_leaves", "waves", "blas_steps_distinct1", "blas_steps_distinct2", "blas_steps_distinct3_4",
                "blas_steps_distinct5_8", "blas_steps_distinct9_")
        d = dict(zip(keys, (int(x) for x in out)))
        d["simd_efficiency"] = d["lane_steps"] / max(d["wave_steps_x64"], 1)
        for k in ("lane_steps", "internal_nodes", "blas_leaves", "faces", "pops", "tlas_leaves"):
            d[k + "_per_ray"] = d[k] / max(d["rays"], 1)
        return d

    def _slot_count(self) -> int:
        sb = self.sample_buffer
        tiles_x, bands = (sb.width + 15) // 16, (sb.height + 15) // 16
        owned = (bands - self.rank + self.nranks - 1) // self.nranks if bands > self.rank else 0
        return owned * tiles_x * 256 * self.streams

    def extend_step_counts(self) -> np.ndarray:
        """Traversal steps of every current ray, per ray position (diagnostic)."""
        out = np.zeros(self._slot_count(), dtype=np.uint32)
        _check(N.hip_lib().ptExtendStepCounts(self.device.handle, self._h, out.ctypes.data), "ptExtendStepCounts")
        return out

    def read_state(self, stream: int = 0) -> np.ndarray:
        """Per-pixel state of one path stream, image order (owned pixels)."""
        sb = self.sample_buffer
        out = np.zeros(sb.width * sb.height, dtype=N.PIXEL_STATE_DTYPE)
        _check(N.hip_lib().ptReadBasicRendererStreamState(self.device.handle, self._h, int(stream), out.ctypes.data),
               "ptReadBasicRendererStreamState")
        return out.reshape(sb.height, sb.width)

    def write_state(self, state: np.ndarray, stream: int = 0):
        """Resume: restore every owned pixel's live path of one stream from a
        saved read_state() (ptWriteBasicRendererStreamState): the next ray and
        the path record; the trace record is not needed (the next run traces
        first).  With the sample buffer (SampleBuffer.write) and FrameIndex
        restored too, later runs equal the uninterrupted render bit for bit."""
        sb = self.sample_buffer
        a = np.ascontiguousarray(state, dtype=N.PIXEL_STATE_DTYPE).reshape(-1)
        if a.size != sb.width * sb.height:
            raise ValueError(f"state has {a.size} pixels, the sample buffer {sb.width * sb.height}")
        _check(N.hip_lib().ptWriteBasicRendererStreamState(self.device.handle, self._h, int(stream), a.ctypes.data),
               "ptWriteBasicRendererStreamState")

    def read_accumulator(self, stream: int = 0) -> np.ndarray:
        """One path stream's own accumulator (H, W, 4) (the sample buffer for one stream)."""
        sb = self.sample_buffer
        out = np.zeros((sb.height, sb.width, 4), dtype=np.float32)
        _check(N.hip_lib().ptReadBasicRendererStreamAccumulator(self.device.handle, self._h, int(stream), N.fptr(out)),
               "ptReadBasicRendererStreamAccumulator")
        return out

    def write_accumulator(self, rgba: np.ndarray, stream: int = 0):
        """Restore one path stream's own accumulator (resume of a multi-stream render)."""
        sb = self.sample_buffer
        a = np.ascontiguousarray(rgba, dtype=np.float32).reshape(sb.height, sb.width, 4)
        _check(N.hip_lib().ptWriteBasicRendererStreamAccumulator(self.device.handle, self._h, int(stream), N.fptr(a)),
               "ptWriteBasicRendererStreamAccumulator")

    def shade_info(self) -> dict:
        """The shade variant this renderer runs (diagnostic, ptGetBasicRendererShadeInfo):
        scene / kernel PT_SHADE_* masks, completion queue, grey path records."""
        info = N.pt_shade_info()
        _check(N.hip_lib().ptGetBasicRendererShadeInfo(self._h, C.byref(info)), "ptGetBasicRendererShadeInfo")
        return {"scene_mask": int(info.scene_mask), "kernel_mask": int(info.kernel_mask),
                "completion_queue": bool(info.completion_queue), "grey_records": bool(info.grey_records),
                "ray_order": int(info.ray_order), "length_trained": bool(info.length_trained)}

    def close(self):
        if self._h:
            N.hip_lib().ptDestroyBasicRenderer(self.device.handle, self._h)
            self._h = None


class PreviewParameters:
    """preview_parameters (preview_render.hpp:22-33).  camera_to: the camera's
    4x4 world transform (column-major 16 floats or a (4,4) array, like
    packed_transform.To); From is not read by the preview."""

    def __init__(self, camera_to, RenderMode=0, Brightness=1.0, SelectedShapeIndex=0xFFFFFFFF,
                 RenderSizeX=640, RenderSizeY=360, MouseX=0xFFFFFFFF, MouseY=0xFFFFFFFF):
        m = np.asarray(camera_to, dtype=np.float32)
        self.camera_to = (m.T.reshape(-1) if m.shape == (4, 4) else m.reshape(-1)).copy()
        self.RenderMode, self.Brightness, self.SelectedShapeIndex = int(RenderMode), float(Brightness), int(SelectedShapeIndex)
        self.RenderSizeX, self.RenderSizeY, self.MouseX, self.MouseY = int(RenderSizeX), int(RenderSizeY), int(MouseX), int(MouseY)

    def as_struct(self) -> N.pt_preview_parameters:
        p = N.pt_preview_parameters()
        p.CameraTransform.To[:] = [float(x) for x in self.camera_to]
        p.RenderMode, p.Brightness, p.SelectedShapeIndex = self.RenderMode, self.Brightness, self.SelectedShapeIndex
        p.RenderSizeX, p.RenderSizeY, p.MouseX, p.MouseY = self.RenderSizeX, self.RenderSizeY, self.MouseX, self.MouseY
        return p


class PreviewRenderContext:
    """preview_render_context (preview_render.hpp:15-20): primary-ray preview,
    AOVs and pick queries over a DeviceScene."""

    def __init__(self, device: Device, scene: DeviceScene):
        L = N.hip_lib()
        self.device, self.scene = device, scene
        self._h = L.ptCreatePreviewRenderContext(device.handle, scene.handle)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())
        self._size = (0, 0)

    def render(self, params: PreviewParameters):
        _check(N.hip_lib().ptRenderPreview(self.device.handle, self._h, C.byref(params.as_struct())), "ptRenderPreview")
        self._size = (params.RenderSizeY, params.RenderSizeX)

    def query(self) -> int:
        """RetrievePreviewQueryResult: shape index under the mouse (0xFFFFFFFF = none)."""
        v = C.c_uint32(0)
        _check(N.hip_lib().ptRetrievePreviewQueryResult(self.device.handle, self._h, C.byref(v)),
               "ptRetrievePreviewQueryResult")
        return int(v.value)

    def image(self) -> np.ndarray:
        out = np.zeros(self._size + (4,), dtype=np.float32)
        _check(N.hip_lib().ptReadPreviewImage(self.device.handle, self._h, N.fptr(out)), "ptReadPreviewImage")
        return out

    def aovs(self) -> np.ndarray:
        out = np.zeros(self._size, dtype=N.PREVIEW_AOV_DTYPE)
        _check(N.hip_lib().ptReadPreviewAOVs(self.device.handle, self._h, out.ctypes.data), "ptReadPreviewAOVs")
        return out

    def close(self):
        if self._h:
            N.hip_lib().ptDestroyPreviewRenderContext(self.device.handle, self._h)
            self._h = None


class Comm:
    """RCCL communicator (one process per GPU) for the frame-end reduce."""

    def __init__(self, device: Device, nranks: int, rank: int, unique_id: bytes):
        L = N.hip_lib()
        buf = (C.c_uint8 * 128)(*unique_id)
        self.device = device
        self._h = L.ptCommCreate(device.handle, nranks, rank, buf)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())

    def set_timeout(self, seconds: float):
        """Deadline of a device-stream wait while this communicator is live
        (ptCommSetTimeout; default 600 s).  Past it the communicators are
        aborted and the waiting call raises (PT_ERROR_TIMEOUT)."""
        _check(N.hip_lib().ptCommSetTimeout(self._h, float(seconds)), "ptCommSetTimeout")

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(N.hip_lib().ptCommGetUniqueId(buf), "ptCommGetUniqueId")
        return bytes(buf)

    def reduce_sample_buffer(self, sample_buffer: SampleBuffer, root: int = 0):
        _check(N.hip_lib().ptCommReduceSampleBuffer(self.device.handle, self._h, sample_buffer.handle, root),
               "ptCommReduceSampleBuffer")

    def reduce_sample_buffer_into(self, sample_buffer: SampleBuffer, total: SampleBuffer | None, root: int = 0):
        """Sample sharding: `total` on `root` = sum over ranks of their own
        accumulators (ptCommReduceSampleBufferInto); `total` may be None
        on the other ranks."""
        _check(N.hip_lib().ptCommReduceSampleBufferInto(self.device.handle, self._h, sample_buffer.handle,
                                                         total.handle if total is not None else None, root),
               "ptCommReduceSampleBufferInto")

    def gather_sample_buffer(self, sample_buffer: SampleBuffer, root: int = 0):
        """Each rank's own bands, point-to-point to `root` (1/N of the reduce's traffic)."""
        _check(N.hip_lib().ptCommGatherSampleBuffer(self.device.handle, self._h, sample_buffer.handle, root),
               "ptCommGatherSampleBuffer")

    def close(self):
        if self._h:
            N.hip_lib().ptCommDestroy(self._h)
            self._h = None


# Reference-named free functions ------------------------------------------------

def CreateSampleBuffer(device: Device, width: int, height: int) -> SampleBuffer:
    return SampleBuffer(device, width, height)


def CreateBasicRenderer(device: Device, scene: DeviceScene, sample_buffer: SampleBuffer) -> BasicRenderer:
    return BasicRenderer(device, scene, sample_buffer)


def ResetBasicRenderer(device: Device, renderer: BasicRenderer):
    renderer.reset()


def RunBasicRenderer(device: Device, renderer: BasicRenderer, rounds: int):
    renderer.run(rounds)


def DestroyBasicRenderer(device: Device, renderer: BasicRenderer):
    renderer.close()


def DestroySampleBuffer(device: Device, sample_buffer: SampleBuffer):
    sample_buffer.close()


def RenderSampleBuffer(device: Device, sample_buffer: SampleBuffer, parameters: ResolveParameters):
    sample_buffer.render(parameters)


def CreatePreviewRenderContext(device: Device, scene: DeviceScene) -> PreviewRenderContext:
    return PreviewRenderContext(device, scene)


def RenderPreview(device: Device, context: PreviewRenderContext, parameters: PreviewParameters):
    context.render(parameters)


def RetrievePreviewQueryResult(device: Device, context: PreviewRenderContext) -> int:
    return context.query()
