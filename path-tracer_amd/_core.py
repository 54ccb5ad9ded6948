"""What the modules of the Python mirror share (integrator.py lists them):
the error type, a library call by entry-point name, the handle base class and
the argument coercers, each written once."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

U32, U64, F64 = C.c_uint32, C.c_uint64, C.c_double


class PathTracerError(RuntimeError):
    pass


def hip(name, *args):
    """libpathtracer.so's `name`(*args); a non-zero status raises with the library's message."""
    L = N.hip_lib()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise PathTracerError(f"{name}: {L.ptGetLastError().decode()} (status {rc})")


def hip_get(name, *args, types=(U32,)):
    """hip(name, *args, one out-parameter per type): the value written, or the tuple of them."""
    out = [t() for t in types]
    hip(name, *args, *(C.byref(v) for v in out))
    return out[0].value if len(out) == 1 else tuple(v.value for v in out)


def pts(name, *args):
    """libptscene.so's `name`(*args), a host pass that answers with a status."""
    rc = getattr(N.scene_lib(), name)(*args)
    if rc != 0:
        raise PathTracerError(f"{name}: bad arguments (status {rc})")


class Handle:
    """An object of libpathtracer.so behind `_h`.  A class names its destroy
    entry point and whether that takes the device in front of the handle."""

    _destroy, _destroy_takes_device = None, True

    def _create(self, name, *args):
        L = N.hip_lib()
        self._h = getattr(L, name)(*args)
        if not self._h:
            raise PathTracerError(L.ptGetLastError().decode())

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            args = (self.device.handle, self._h) if self._destroy_takes_device else (self._h,)
            getattr(N.hip_lib(), self._destroy)(*args)
            self._h = None


def image(a, what="accumulator", empty=True) -> np.ndarray:
    """An (H, W, 4) float32 image; empty=False refuses one without a pixel too."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or not (empty or a.size):
        raise ValueError(f"{what} of shape {a.shape}, expected (H, W, 4)")
    return a


def image_like(b, a: np.ndarray, what: str, first: str) -> np.ndarray:
    """A second float32 image of the shape of `a`, which the message calls `first`."""
    b = np.ascontiguousarray(b, dtype=np.float32)
    if b.shape != a.shape:
        raise ValueError(f"{what} of shape {b.shape}, {first} {a.shape}")
    return b


def guide_image(g, a: np.ndarray, what="guides") -> np.ndarray:
    """The (H, W) DENOISE_GUIDE_DTYPE records that go with the (H, W, 4) image `a`."""
    g = np.ascontiguousarray(g, dtype=N.DENOISE_GUIDE_DTYPE)
    if g.shape != a.shape[:2]:
        raise ValueError(f"{what} of shape {g.shape}, accumulator {a.shape[:2]}")
    return g


def tile_grid(width: int, height: int):
    """(tiles_y, tiles_x) of a width x height frame's 16 x 16 tiles."""
    return (int(height) + N.TILE_SIZE - 1) // N.TILE_SIZE, (int(width) + N.TILE_SIZE - 1) // N.TILE_SIZE


def camera_struct(camera) -> N.pt_packed_camera:
    """A packed camera record (scene.arrays()["cameras"][i]) as the C struct."""
    if isinstance(camera, N.pt_packed_camera):
        return camera
    c = np.asarray(camera, dtype=N.CAMERA_DTYPE)
    if c.shape != ():
        raise ValueError(f"one camera record expected, got shape {c.shape}")
    return N.pt_packed_camera.from_buffer_copy(c.tobytes())


def motion_table(motion):
    """(array kept alive, pointer or None, count) of an optional motion table."""
    if motion is None:
        return None, None, 0
    m = np.ascontiguousarray(motion, dtype=N.SHAPE_MOTION_DTYPE).reshape(-1)
    if m.size == 0:                      # an empty table is still a table: every hit is beyond it
        m = np.zeros(1, dtype=N.SHAPE_MOTION_DTYPE)
        return m, m.ctypes.data, 0
    return m, m.ctypes.data, m.size


# ptExtendStats' counters in order; ptTraceRaysStats fills the first nine.
EXTEND_STATS_KEYS = ("rays", "lane_steps", "wave_steps_x64", "internal_nodes", "blas_leaves", "faces", "pops",
                     "tlas_leaves", "waves", "blas_steps_distinct1", "blas_steps_distinct2", "blas_steps_distinct3_4",
                     "blas_steps_distinct5_8", "blas_steps_distinct9_")


def extend_stats(counters, count=len(EXTEND_STATS_KEYS)) -> dict:
    """The first `count` counters by name, and the SIMD efficiency they give."""
    d = dict(zip(EXTEND_STATS_KEYS[:count], (int(x) for x in counters)))
    d["simd_efficiency"] = d["lane_steps"] / max(d["wave_steps_x64"], 1)
    return d
