"""The device, the device copy of a scene and the communicator
(libpathtracer.so; include/pt_api.h)."""
from __future__ import annotations

import ctypes as C
from typing import TYPE_CHECKING

import numpy as np

from . import _native as N
from ._core import U32, U64, F64, Handle, extend_stats, hip, hip_get
from .layout import SKY_RECORD_DTYPE
from .params import SkyGatherParameters, VisibilityGatherParameters

if TYPE_CHECKING:
    from .frame import SampleBuffer


def device_count() -> int:
    n = C.c_int(0)
    N.hip_lib().ptGetDeviceCount(C.byref(n))
    return n.value


class Device(Handle):
    """A HIP device + stream (replaces the reference's `vulkan` context)."""

    _destroy, _destroy_takes_device = "ptDestroyDevice", False

    def __init__(self, hip_device: int = 0):
        self._create("ptCreateDevice", int(hip_device))
        self.index = hip_device

    def synchronize(self):
        hip("ptSynchronize", self._h)

    def set_profiling(self, enable: bool, period: int = 1):
        """Kernel timing with HIP events; period > 1 times every period-th round only."""
        hip("ptSetProfiling", self._h, int(enable))
        hip("ptSetProfilingPeriod", self._h, int(period))

    def kernel_stats(self, kernel: int):
        return hip_get("ptGetKernelStats", self._h, kernel, types=(U64, F64))

    def kernel_rounds(self, kernel: int) -> int:
        """Rounds covered by the timed launches of `kernel` (a round batch
        covers several): total_ms / rounds is its time per round."""
        return hip_get("ptGetKernelRounds", self._h, kernel, types=(U64,))

    def reset_kernel_stats(self):
        hip("ptResetKernelStats", self._h)

    def set_statistics_variant(self, variant: int):
        """STATS_VARIANT_AUTO / _PLAIN / _UNIFORM: the statistics kernel's
        histogram update (identical results; ptSetFrameStatisticsVariant)."""
        hip("ptSetFrameStatisticsVariant", self._h, int(variant))

    def check_fast_division(self, n: int, seed: int = 1) -> int:
        return hip_get("ptCheckFastDivision", self._h, n, seed, types=(U64,))

    def check_fast_reciprocal(self) -> int:
        return hip_get("ptCheckFastReciprocal", self._h, types=(U64,))

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
        hip("ptEvalNumerics", self._h, N.NUMERICS_OPS.index(name), n, *ptrs, N.u32ptr(out))
        return out if outputs == 1 else out.reshape(n, outputs)

    def eval_slab_test(self, origin, velocity, reach, box_min, box_max, scene_gate: int = 1):
        """Test probe (ptEvalSlabTest): the traversal's slab test of n rays
        ((n, 3) origins and velocities, (n,) reaches) against n boxes ((n, 3)
        minima and maxima), the level ray set as the kernels set it under a
        scene whose box-coordinate gate is `scene_gate`.  Returns (entry time
        bit patterns, fast-division flags), each uint32 of shape (n,)."""
        o, v, lo, hi = (np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3) for x in (origin, velocity, box_min, box_max))
        r = np.ascontiguousarray(reach, dtype=np.float32).reshape(-1)
        n = len(r)
        if not (len(o) == len(v) == len(lo) == len(hi) == n):
            raise ValueError("eval_slab_test: arrays of different lengths")
        entry, exact = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        hip("ptEvalSlabTest", self._h, n, N.fptr(o), N.fptr(v), N.fptr(r), N.fptr(lo), N.fptr(hi), int(scene_gate),
            N.u32ptr(entry), N.u32ptr(exact))
        return entry, exact


def _records(pointer, count: int, dtype: np.dtype) -> np.ndarray:
    """A copy of `count` packed records at `pointer` (none for a null pointer)."""
    if not (count and pointer):
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(pointer), dtype=dtype).copy()


def _ray_batch(origins, packed_velocities, durations):
    """(origins (n, 3), packed velocities (n,), durations (n,)) as the trace entry points read them."""
    return (np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3),
            np.ascontiguousarray(packed_velocities, dtype=np.uint32).reshape(-1),
            np.ascontiguousarray(durations, dtype=np.float32).reshape(-1))


class DeviceScene(Handle):
    """Device copy of a packed scene (CreateVulkanScene / UpdateVulkanScene)."""

    _destroy = "ptDestroyScene"

    def __init__(self, device: Device):
        self.device = device
        self.cameras = np.zeros(0, dtype=N.CAMERA_DTYPE)
        self.shapes = np.zeros(0, dtype=N.SHAPE_DTYPE)
        self._create("ptCreateScene", device.handle)

    def set_stack_format(self, fmt: int):
        """PT_STACK_FORMAT_* (0 auto, 1 packed 32-bit words, 2 node indices); next update()."""
        hip("ptSetSceneStackFormat", self._h, int(fmt))

    def set_hit_record_form(self, form: int):
        """PT_HIT_RECORD_* (0 auto, 1 face index); next update()."""
        hip("ptSetSceneHitRecordForm", self._h, int(form))

    def set_extend_form(self, form: int):
        """PT_EXTEND_FORM_* (0 auto, 1 general traversal loop); next update()."""
        hip("ptSetSceneExtendForm", self._h, int(form))

    @property
    def extend_form(self) -> int:
        """The extend form the uploaded scene runs: 1 general, 2 mesh-only (ptGetSceneExtendForm)."""
        return hip_get("ptGetSceneExtendForm", self._h)

    def update(self, scene, dirty_flags: int = 0xFFFFFFFF):
        packs = scene.packs() if hasattr(scene, "packs") else scene
        hip("ptUpdateScene", self.device.handle, self._h, C.byref(packs), dirty_flags)
        # The packed camera records as uploaded (FrameHistory keeps a frame's own).
        self.cameras = _records(packs.cameras, packs.camera_count, N.CAMERA_DTYPE)
        # And the packed shapes (FrameHistory(follow_shapes=True) compares two frames' transforms).
        self.shapes = _records(packs.shapes, packs.shape_count, N.SHAPE_DTYPE)

    def length_table(self) -> dict:
        """{classes, trained, rounds}: the scene's traversal-length table, one
        class 0..6 per ray key, whether it was trained since the last clear and
        the LENGTH rounds counted since then (diagnostic, ptReadSceneLengthTable)."""
        cls = np.zeros(N.RAYKEY_COUNT, dtype=np.uint8)
        t, n = hip_get("ptReadSceneLengthTable", self.device.handle, self._h, cls.ctypes.data, types=(U32, U64))
        return {"classes": cls, "trained": bool(t), "rounds": n}

    @property
    def stack_needed(self) -> int:
        """Traversal stack entries the uploaded scene can need (TLAS + BLAS depth)."""
        return hip_get("ptSceneStackNeeded", self._h)

    @property
    def fast_division(self) -> bool:
        """Whether the uploaded scene's box tests take the exact fast slab
        division (every box coordinate 0 or in [2^-50, 2^40]; ptSceneFastDivision)."""
        return bool(hip_get("ptSceneFastDivision", self._h))

    @property
    def node_cache_pairs(self) -> int:
        """BLAS child pairs the extend kernel keeps in LDS (0: none; ptSceneNodeCache)."""
        return hip_get("ptSceneNodeCache", self._h)

    def trace_rays(self, origins: np.ndarray, packed_velocities: np.ndarray, durations: np.ndarray) -> np.ndarray:
        """Bit-exact Trace() of a ray batch (scene.glsl.inc:522-611)."""
        o, v, d = _ray_batch(origins, packed_velocities, durations)
        out = np.zeros(len(v), dtype=N.HIT_RECORD_DTYPE)
        hip("ptTraceRays", self.device.handle, self._h, len(v), N.fptr(o), N.u32ptr(v), N.fptr(d), out.ctypes.data)
        return out

    def occluded(self, origins: np.ndarray, packed_velocities: np.ndarray, durations: np.ndarray) -> np.ndarray:
        """The any-hit query (ptOccludedRays): per ray of
        a trace_rays batch, whether anything lies within its duration.  A bool
        array equal to trace_rays(...)["shape_material"] != 0xFFFFFFFF, from
        one launch and one bit per ray read back."""
        o, v, d = _ray_batch(origins, packed_velocities, durations)
        n = len(v)
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        hip("ptOccludedRays", self.device.handle, self._h, n, N.fptr(o), N.u32ptr(v), N.fptr(d),
            words.ctypes.data_as(C.POINTER(C.c_uint64)))
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)

    def occluded_stats(self, origins: np.ndarray, packed_velocities: np.ndarray, durations: np.ndarray):
        """trace_rays_stats' counters and per-ray step counts for the any-hit
        traversal of the batch (diagnostic, ptOccludedRaysStats)."""
        o, v, d = _ray_batch(origins, packed_velocities, durations)
        out = (C.c_uint64 * 14)()
        steps = np.zeros(len(v), dtype=np.uint32)
        hip("ptOccludedRaysStats", self.device.handle, self._h, len(v), N.fptr(o), N.u32ptr(v), N.fptr(d), out,
            steps.ctypes.data)
        return extend_stats(out, 9), steps

    def gather_visibility(self, points: np.ndarray, normals: np.ndarray, samples: int = 16,
                          radius: float = float("inf"), seed: int = 0, offset: float = 1e-3, first_index: int = 0,
                          params: "VisibilityGatherParameters | None" = None) -> np.ndarray:
        """How open the hemisphere is at caller-given points (ptGatherVisibility;
        DESIGN.md §6 row 15): mesh vertices, lightmap texels, probe positions.
        points, normals: (n, 3); a normal is used as given.  Each point traces
        `samples` rays (a power of two up to 64) of the ambient-occlusion
        pass's cosine lobe around its normal, from `offset` along the ray to
        `radius`, drawn from stream first_index + i of frame `seed`.  Returns n
        VISIBILITY_RECORD_DTYPE records: OccludedMask (bit k: ray k is
        blocked), Unoccluded (the open rays; / Samples is the visibility) and
        Bent, the sum of the open rays' directions (normalise it for the bent
        normal).  Blocks."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if len(p) != len(nrm):
            raise ValueError(f"{len(p)} points and {len(nrm)} normals")
        s = (params or VisibilityGatherParameters(samples, radius, seed, offset, first_index)).as_struct()
        out = np.zeros(len(p), dtype=N.VISIBILITY_RECORD_DTYPE)
        hip("ptGatherVisibility", self.device.handle, self._h, len(p), N.fptr(p), N.fptr(nrm), C.byref(s),
            out.ctypes.data)
        return out

    def gather_sky_light(self, points: np.ndarray, normals: "np.ndarray | None" = None, samples: int = 16,
                         radius: float = float("inf"), seed: int = 0, offset: float = 1e-3, first_index: int = 0,
                         lobe: "int | str" = "cosine", params: "SkyGatherParameters | None" = None) -> np.ndarray:
        """The sky's light that reaches caller-given points (ptGatherSkyLight;
        DESIGN.md §6 row 16), in the integrator's own units.  points: (n, 3).
        lobe "cosine": gather_visibility's rays around `normals` (n, 3), for
        irradiance at texels or vertices; lobe "sphere": rays uniform over the
        sphere, normals unused (None), for a light probe.  Each open ray adds
        the sky's radiance along it (CIE XYZ, at four wavelengths of its own
        draw) times the nine real spherical harmonics of bands 0..2.  Returns
        n SKY_RECORD_DTYPE records: SH (9, 3), OccludedMask, Unoccluded,
        Samples; sky_irradiance (cosine) and sky_radiance_sh (sphere) read
        them.  Blocks."""
        s = (params or SkyGatherParameters(samples, radius, seed, offset, first_index, lobe)).as_struct()
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            if len(p) != len(nrm):
                raise ValueError(f"{len(p)} points and {len(nrm)} normals")
        elif s.Lobe == N.SKY_GATHER_COSINE:
            raise ValueError("the cosine lobe needs normals")
        out = np.zeros(len(p), dtype=SKY_RECORD_DTYPE)
        hip("ptGatherSkyLight", self.device.handle, self._h, len(p), N.fptr(p), None if nrm is None else N.fptr(nrm),
            C.byref(s), out.ctypes.data)
        return out

    def sample_textures(self, texture_index: np.ndarray, uv: np.ndarray, wrap: int = 0) -> np.ndarray:
        """Test probe (ptSampleTextures): SampleTexture of the uploaded scene
        at (n, 2) UVs; wrap 0 = remainder, 1 = the lean kernel's two-select
        form (refused when a placement leaves [0, 1]).  Returns (n, 4)."""
        t = np.ascontiguousarray(texture_index, dtype=np.uint32).reshape(-1)
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        assert len(u) == len(t)
        out = np.zeros((len(t), 4), dtype=np.float32)
        hip("ptSampleTextures", self.device.handle, self._h, len(t), N.u32ptr(t), N.fptr(u), int(wrap), N.fptr(out))
        return out

    def trace_rays_stats(self, origins: np.ndarray, packed_velocities: np.ndarray, durations: np.ndarray):
        """Traversal counters (ptExtendStats keys) and per-ray step counts of a
        ray batch (diagnostic, ptTraceRaysStats)."""
        o, v, d = _ray_batch(origins, packed_velocities, durations)
        out = (C.c_uint64 * 14)()
        steps = np.zeros(len(v), dtype=np.uint32)
        hip("ptTraceRaysStats", self.device.handle, self._h, len(v), N.fptr(o), N.u32ptr(v), N.fptr(d), out,
            steps.ctypes.data)
        return extend_stats(out, 9), steps


class Comm(Handle):
    """RCCL communicator (one process per GPU) for the frame-end reduce."""

    _destroy, _destroy_takes_device = "ptCommDestroy", False

    def __init__(self, device: Device, nranks: int, rank: int, unique_id: bytes):
        buf = (C.c_uint8 * 128)(*unique_id)
        self.device = device
        self._create("ptCommCreate", device.handle, nranks, rank, buf)

    def set_timeout(self, seconds: float):
        """Deadline of a device-stream wait while this communicator is live
        (ptCommSetTimeout; default 600 s).  Past it the communicators are
        aborted and the waiting call raises (PT_ERROR_TIMEOUT)."""
        hip("ptCommSetTimeout", self._h, float(seconds))

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        hip("ptCommGetUniqueId", buf)
        return bytes(buf)

    def reduce_sample_buffer(self, sample_buffer: SampleBuffer, root: int = 0):
        hip("ptCommReduceSampleBuffer", self.device.handle, self._h, sample_buffer.handle, root)

    def reduce_sample_buffer_into(self, sample_buffer: SampleBuffer, total: SampleBuffer | None, root: int = 0):
        """Sample sharding: `total` on `root` = sum over ranks of their own
        accumulators (ptCommReduceSampleBufferInto); `total` may be None
        on the other ranks."""
        hip("ptCommReduceSampleBufferInto", self.device.handle, self._h, sample_buffer.handle,
            total.handle if total is not None else None, root)

    def gather_sample_buffer(self, sample_buffer: SampleBuffer, root: int = 0):
        """Each rank's own bands, point-to-point to `root` (1/N of the reduce's traffic)."""
        hip("ptCommGatherSampleBuffer", self.device.handle, self._h, sample_buffer.handle, root)
