"""The basic renderer and the loops that drive a pair of them
(libpathtracer.so; include/pt_api.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._core import U32, U64, Handle, extend_stats, hip, hip_get, tile_grid
from .device import Device, DeviceScene
from .frame import SampleBuffer

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
    active = np.ones(tile_grid(sa.width, sa.height), dtype=bool)
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


class BasicRenderer(Handle):
    """basic_renderer (basic.hpp:6-26) running the HIP wavefront kernels."""

    _destroy = "ptDestroyBasicRenderer"
    _FIELDS = ("FrameIndex", "CameraIndex", "RenderFlags", "PathLengthLimit", "PathTerminationProbability")

    def __init__(self, device: Device, scene: DeviceScene, sample_buffer: SampleBuffer, rank: int = 0, nranks: int = 1,
                 streams: int = 1):
        """rank / nranks: the 16-row pixel bands owned (b % nranks == rank);
        streams: independent paths per owned pixel, stream k seeded at
        FrameIndex + (k << 24) (ptCreateBasicRendererStreams)."""
        self.device, self.scene, self.sample_buffer = device, scene, sample_buffer
        self.rank, self.nranks, self.streams = rank, nranks, streams
        self._create("ptCreateBasicRendererStreams", device.handle, scene.handle, sample_buffer.handle, rank, nranks,
                     streams)
        self._params = N.hip_lib().ptBasicRendererParams(self._h)

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
    def slot_count(self) -> int:
        return int(N.hip_lib().ptBasicRendererSlotCount(self._h))

    def merge_streams(self):
        """The sample buffer's owned pixels := the sum of every stream's
        accumulator, stream 0 included, in stream order
        ((A0 + A1) + A2 ...; ptMergeBasicRendererStreams).  The streams are
        not cleared and keep accumulating, so a later merge writes the new
        totals (not deltas).  A no-op for one stream."""
        hip("ptMergeBasicRendererStreams", self.device.handle, self._h)

    def set_fused_rounds(self, mode: int):
        """0 never / 1 automatic / 2 whenever possible (ptSetBasicRendererFusedRounds)."""
        hip("ptSetBasicRendererFusedRounds", self._h, int(mode))

    def set_round_batch(self, rounds: int):
        """Rounds per launch for consecutive Run(1) rounds (run_rounds,
        render_frame): 0 automatic (16 when every tile fits on the GPU at
        once), 1 never (one launch per round), R >= 2 always R."""
        hip("ptSetBasicRendererRoundBatch", self._h, int(rounds))

    def set_split(self, groups: int):
        """Tile groups of consecutive rounds, each on its own HIP stream
        (ptSetBasicRendererSplit): 0 automatic, 1 off, 2..MAX_SPLIT that many.
        Results are identical for every value."""
        hip("ptSetBasicRendererSplit", self._h, int(groups))

    def split(self) -> dict:
        """{groups, timed_tiles, tiles}: the tile groups consecutive rounds use
        now, group 0's tiles (the launches kernel profiling times) and all
        tiles (ptGetBasicRendererSplit)."""
        return dict(zip(("groups", "timed_tiles", "tiles"),
                        hip_get("ptGetBasicRendererSplit", self._h, types=(U32, U32, U32))))

    def set_class_lists(self, mode: int):
        """Class-pure shade inside tile groups (ptSetBasicRendererClassLists):
        0 automatic, 1 off.  Results are identical either way."""
        hip("ptSetBasicRendererClassLists", self._h, int(mode))

    def class_lists(self) -> bool:
        """Whether consecutive rounds shade through per-class lists now."""
        return bool(hip_get("ptGetBasicRendererClassLists", self._h))

    def set_ray_order(self, order: int):
        """Where a tile's new rays sit (ptSetBasicRendererRayOrder): 0
        automatic, 1 by direction octant, 2 by predicted traversal length.
        Results are identical in every order."""
        hip("ptSetBasicRendererRayOrder", self._h, int(order))

    def ray_order(self) -> dict:
        """{order, used}: the order set and the one the next unfused rounds
        use, 1 octant or 2 length (ptGetBasicRendererRayOrder)."""
        return dict(zip(("order", "used"), hip_get("ptGetBasicRendererRayOrder", self._h, types=(U32, U32))))

    def set_block_map(self, block_map: int):
        """Which extend block traces which ray positions
        (ptSetBasicRendererBlockMap): 0 automatic, 1 tile (a tile's four
        quarters), 2 run (one quarter of four neighbouring tiles, under LENGTH
        order).  Results are identical under every map."""
        hip("ptSetBasicRendererBlockMap", self._h, int(block_map))

    def block_map(self) -> dict:
        """{map, used}: the map set (0 automatic) and the one the next rounds
        use, 1 tile or 2 run (ptGetBasicRendererBlockMap)."""
        return dict(zip(("map", "used"), hip_get("ptGetBasicRendererBlockMap", self._h, types=(U32, U32))))

    def ray_positions(self) -> np.ndarray:
        """Per slot, the position of its ray (high byte) and of its last hit
        (low byte) within its tile (diagnostic, ptReadBasicRendererRayPositions)."""
        out = np.zeros(self.slot_count, dtype=np.uint16)
        hip("ptReadBasicRendererRayPositions", self.device.handle, self._h, out.ctypes.data)
        return out

    def set_active_tiles(self, mask: "np.ndarray | None"):
        """The tiles the following rounds run on (ptSetBasicRendererActiveTiles):
        a (tiles_y, tiles_x) array, non-zero = active (tile_mask_of_region
        builds one), or None for every tile.  An active tile's results equal
        an unmasked render's bit for bit; an inactive tile is not touched.
        Full-frame, single-stream renderers only; render_frame is refused
        while a mask is set.  Waits for the device."""
        if mask is None:
            hip("ptSetBasicRendererActiveTiles", self.device.handle, self._h, None, 0)
            return
        m = np.asarray(mask)
        grid = tile_grid(self.sample_buffer.width, self.sample_buffer.height)
        if m.shape != grid:
            raise ValueError(f"mask of shape {m.shape}, the frame has {grid} tiles")
        m = np.ascontiguousarray(m != 0, dtype=np.uint8)
        hip("ptSetBasicRendererActiveTiles", self.device.handle, self._h, m.ctypes.data, m.size)

    def active_tiles(self) -> dict:
        """{active, tiles}: the tiles the next round launches and all tiles
        (ptGetBasicRendererActiveTiles)."""
        return dict(zip(("active", "tiles"), hip_get("ptGetBasicRendererActiveTiles", self._h, types=(U32, U32))))

    def run_rounds(self, count: int):
        """count consecutive Run(1) calls (one new FrameIndex each), batched
        per set_round_batch (ptRunBasicRendererRounds)."""
        hip("ptRunBasicRendererRounds", self.device.handle, self._h, int(count))

    def set_openpbr(self, enable: bool):
        """Shade OpenPBR materials (ptSetBasicRendererOpenPBR); off by default,
        as in the reference, where an OpenPBR hit ends the path."""
        hip("ptSetBasicRendererOpenPBR", self._h, int(bool(enable)))

    def reset(self):
        hip("ptResetBasicRenderer", self.device.handle, self._h)

    def run(self, rounds: int = 1):
        hip("ptRunBasicRenderer", self.device.handle, self._h, int(rounds))

    def render_frame(self, target_samples: int, max_rounds: int = 1 << 30):
        """Benchmark-mode frame (ptRenderFrame): Reset,
        Run(2), then Run(1) rounds until target_samples paths completed since
        the Reset.  Blocks; returns (rounds, samples)."""
        return hip_get("ptRenderFrame", self.device.handle, self._h, int(target_samples), int(max_rounds),
                       types=(U32, U64))

    def stats(self):
        """(rays traced, paths completed) since the last Reset (ptGetStats)."""
        return hip_get("ptGetStats", self.device.handle, self._h, types=(U64, U64))

    def extend_stats(self) -> dict:
        """Traversal counters of the current rays (diagnostic, ptExtendStats)."""
        out = (C.c_uint64 * 14)()
        hip("ptExtendStats", self.device.handle, self._h, out)
        d = extend_stats(out)
        for k in ("lane_steps", "internal_nodes", "blas_leaves", "faces", "pops", "tlas_leaves"):
            d[k + "_per_ray"] = d[k] / max(d["rays"], 1)
        return d

    def extend_step_counts(self) -> np.ndarray:
        """Traversal steps of every current ray, per ray position (diagnostic)."""
        out = np.zeros(self.slot_count, dtype=np.uint32)
        hip("ptExtendStepCounts", self.device.handle, self._h, out.ctypes.data)
        return out

    def read_state(self, stream: int = 0) -> np.ndarray:
        """Per-pixel state of one path stream, image order (owned pixels)."""
        sb = self.sample_buffer
        out = np.zeros(sb.width * sb.height, dtype=N.PIXEL_STATE_DTYPE)
        hip("ptReadBasicRendererStreamState", self.device.handle, self._h, int(stream), out.ctypes.data)
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
        hip("ptWriteBasicRendererStreamState", self.device.handle, self._h, int(stream), a.ctypes.data)

    def read_accumulator(self, stream: int = 0) -> np.ndarray:
        """One path stream's own accumulator (H, W, 4) (the sample buffer for one stream)."""
        sb = self.sample_buffer
        out = np.zeros((sb.height, sb.width, 4), dtype=np.float32)
        hip("ptReadBasicRendererStreamAccumulator", self.device.handle, self._h, int(stream), N.fptr(out))
        return out

    def write_accumulator(self, rgba: np.ndarray, stream: int = 0):
        """Restore one path stream's own accumulator (resume of a multi-stream render)."""
        sb = self.sample_buffer
        a = np.ascontiguousarray(rgba, dtype=np.float32).reshape(sb.height, sb.width, 4)
        hip("ptWriteBasicRendererStreamAccumulator", self.device.handle, self._h, int(stream), N.fptr(a))

    def shade_info(self) -> dict:
        """The shade variant this renderer runs (diagnostic, ptGetBasicRendererShadeInfo):
        scene / kernel PT_SHADE_* masks, completion queue, grey path records."""
        info = N.pt_shade_info()
        hip("ptGetBasicRendererShadeInfo", self._h, C.byref(info))
        return {"scene_mask": int(info.scene_mask), "kernel_mask": int(info.kernel_mask),
                "completion_queue": bool(info.completion_queue), "grey_records": bool(info.grey_records),
                "ray_order": int(info.ray_order), "length_trained": bool(info.length_trained),
                "block_map": int(info.block_map)}
