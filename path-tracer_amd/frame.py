"""A frame's device images: the sample buffer with its post-processing
passes, the denoise guides, and the history that carries one frame into the
next (libpathtracer.so; include/pt_api.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._core import Handle, PathTracerError, camera_struct, hip, motion_table, tile_grid
from .device import Device, DeviceScene
from .host import FrameStatistics, shape_motion
from .params import (AmbientOcclusionParameters, DenoiseParameters, DenoisePairParameters, DespikeParameters,
                     RectifyParameters, ReprojectParameters, ResolveParameters)


class DenoiseGuides(Handle):
    """Per-pixel primary-hit records of the scene camera's central rays
    (normal, hit time, base colour, shape) that steer the denoiser, plus the
    filter's intermediate image (ptCreateDenoiseGuides)."""

    _destroy = "ptDestroyDenoiseGuides"

    def __init__(self, device: "Device", width: int, height: int):
        self.device = device
        self.width, self.height = int(width), int(height)
        self._create("ptCreateDenoiseGuides", device.handle, self.width, self.height)

    def render(self, scene: "DeviceScene", camera_index: int = 0, specular_bounces: int = 0):
        """One central camera ray per pixel of packed camera `camera_index` (enqueues).
        specular_bounces (up to GUIDE_MAX_BOUNCES): the ray is followed through
        that many perfect mirrors and smooth glass surfaces, and the record
        describes the surface the pixel shows (ptRenderDenoiseGuidesSpecular;
        DESIGN.md §6 row 13).  0: the primary hit (ptRenderDenoiseGuides)."""
        if int(specular_bounces) == 0:
            hip("ptRenderDenoiseGuides", self.device.handle, scene.handle, self._h, int(camera_index))
            return
        if int(specular_bounces) < 0:
            raise ValueError(f"specular_bounces: {specular_bounces}")
        hip("ptRenderDenoiseGuidesSpecular", self.device.handle, scene.handle, self._h, int(camera_index),
            int(specular_bounces))

    def read(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), dtype=N.DENOISE_GUIDE_DTYPE)
        hip("ptReadDenoiseGuides", self.device.handle, self._h, out.ctypes.data)
        return out

    def write(self, guides: np.ndarray):
        g = np.ascontiguousarray(guides, dtype=N.DENOISE_GUIDE_DTYPE)
        if g.size != self.width * self.height:
            raise ValueError(f"guides have {g.size} pixels, the object {self.width * self.height}")
        hip("ptWriteDenoiseGuides", self.device.handle, self._h, g.ctypes.data)

    def set_variant(self, variant: int):
        """DENOISE_VARIANT_AUTO / _GATHER / _LATTICE: the filter kernel used
        (identical results; ptSetDenoiseVariant)."""
        hip("ptSetDenoiseVariant", self._h, int(variant))


class SampleBuffer(Handle):
    """rgba32f accumulator: CIE XYZ sums + sample count (integrator.cpp:15-87)."""

    _destroy = "ptDestroySampleBuffer"

    def __init__(self, device: Device, width: int, height: int):
        self.device = device
        self.width, self.height = int(width), int(height)
        self._create("ptCreateSampleBuffer", device.handle, self.width, self.height)

    def read(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        hip("ptReadSampleBuffer", self.device.handle, self._h, N.fptr(out))
        return out

    def write(self, rgba: np.ndarray):
        """Overwrite the accumulator (resume accumulation from a saved one)."""
        a = np.ascontiguousarray(rgba, dtype=np.float32).reshape(self.height, self.width, 4)
        hip("ptWriteSampleBuffer", self.device.handle, self._h, N.fptr(a))

    def render(self, params: "ResolveParameters | None" = None, **kw):
        """RenderSampleBuffer (integrator.hpp:55-60): resolve on the device."""
        p = (params or ResolveParameters(**kw)).as_struct()
        hip("ptRenderSampleBuffer", self.device.handle, self._h, C.byref(p))

    def _into(self, out: "SampleBuffer | None", size, name: str, *args) -> "SampleBuffer":
        """The pass `name`(device, this buffer, *args, dst): dst is `out` or a
        new sample buffer of `size`, which is closed again if the pass is
        refused.  Returns dst."""
        dst = out if out is not None else SampleBuffer(self.device, *size)
        try:
            hip(name, self.device.handle, self._h, *args, dst.handle)
        except PathTracerError:
            if out is None:
                dst.close()
            raise
        return dst

    def denoise(self, guides: "DenoiseGuides", params: "DenoiseParameters | None" = None,
                out: "SampleBuffer | None" = None) -> "SampleBuffer":
        """The edge-avoiding a-trous filter on the device (ptDenoiseSampleBuffer;
        enqueues): `out` (a new sample buffer of this size when None) receives
        the denoised mean XYZ and a sample count of 1, so out.render(...) and
        out.read() work as on any sample buffer.  This buffer is not written."""
        p = (params or DenoiseParameters()).as_struct()
        return self._into(out, (self.width, self.height), "ptDenoiseSampleBuffer", guides.handle, C.byref(p))

    def denoise_pair(self, other: "SampleBuffer", guides: "DenoiseGuides",
                     params: "DenoisePairParameters | None" = None,
                     out: "SampleBuffer | None" = None) -> "SampleBuffer":
        """The variance-guided filter on the device (ptDenoiseSampleBufferPair;
        enqueues) over this buffer and `other`, two independent renders of one
        frame (e.g. render_until_noise's halves): `out` (a new sample buffer
        of this size when None) receives the denoised mean XYZ of this + other
        and a sample count of 1, as denoise() leaves it.  Neither input is
        written."""
        p = (params or DenoisePairParameters()).as_struct()
        return self._into(out, (self.width, self.height), "ptDenoiseSampleBufferPair", other.handle, guides.handle,
                          C.byref(p))

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
        p = (params or DespikeParameters()).as_struct()
        return self._into(out, (self.width, self.height), "ptDespikeSampleBuffer", guides.handle, C.byref(p))

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
        pc, c = camera_struct(prev_camera), camera_struct(camera)
        p = (params or ReprojectParameters()).as_struct()
        views = (prev_guides.handle, C.byref(pc), guides.handle, C.byref(c))
        size = (guides.width, guides.height)
        if motion is not None:
            m, mp, mn = motion_table(motion)
            return self._into(out, size, "ptReprojectSampleBufferMoving", *views, mp, mn, C.byref(p))
        return self._into(out, size, "ptReprojectSampleBuffer", *views, C.byref(p))

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
        hip("ptRectifyHistory", self.device.handle, self._h, current.handle, guides.handle, C.byref(p), dst.handle)
        return dst

    def statistics(self, other: "SampleBuffer | None" = None) -> FrameStatistics:
        """Frame statistics on the device (ptComputeFrameStatistics; blocks):
        of this buffer, or, with `other` (an independent render of the same
        frame), of this + other with the noise histogram of the pair.
        Neither buffer is written."""
        out = N.pt_frame_statistics()
        hip("ptComputeFrameStatistics", self.device.handle, self._h, other.handle if other is not None else None,
            C.byref(out))
        return FrameStatistics(out)

    def tile_statistics(self, other: "SampleBuffer | None" = None, threshold: float = 0.1) -> np.ndarray:
        """Per-tile statistics on the device (ptComputeTileStatistics; blocks,
        one launch): a (tiles_y, tiles_x) array of TILE_STATS_DTYPE records of
        this buffer's 16 x 16 tiles, or, with `other`, of this + other with
        the pair counts (over: pair pixels whose relative half-difference
        exceeds `threshold`).  Neither buffer is written."""
        out = np.zeros(tile_grid(self.width, self.height), dtype=N.TILE_STATS_DTYPE)
        hip("ptComputeTileStatistics", self.device.handle, self._h, other.handle if other is not None else None,
            float(threshold), out.ctypes.data)
        return out

    def accumulate(self, src: "SampleBuffer"):
        """This accumulator += src's, per component in float32, on the device
        (ptAccumulateSampleBuffer; enqueues).  src is not written."""
        hip("ptAccumulateSampleBuffer", self.device.handle, self._h, src.handle)

    def render_ambient_occlusion(self, device_scene: "DeviceScene", camera_index: int = 0, samples: int = 16,
                                 radius: float = float("inf"), seed: int = 0,
                                 params: "AmbientOcclusionParameters | None" = None):
        """The ambient-occlusion / sky-visibility image of packed camera
        `camera_index` into this buffer (ptRenderAmbientOcclusion; enqueues):
        every pixel becomes (u, u, u, samples), u of its `samples` cosine-lobe
        rays of length `radius` from the primary hit being unoccluded (a miss:
        u = samples).  An accumulator: render() shows the visible fraction,
        accumulate() adds images of other seeds, the denoisers take it.  The
        value is .y; the image is data, not colour.  DESIGN.md §6 row 14."""
        p = (params or AmbientOcclusionParameters(samples, radius, seed)).as_struct()
        hip("ptRenderAmbientOcclusion", self.device.handle, device_scene.handle, int(camera_index), C.byref(p), self._h)

    def read_resolved(self) -> np.ndarray:
        """OutColor of the last render(): (H, W, 4) float32, alpha 1."""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        hip("ptReadResolvedImage", self.device.handle, self._h, N.fptr(out))
        return out

    def read_srgb8(self) -> np.ndarray:
        """The resolved image as B8G8R8A8_SRGB stores it: (H, W, 4) uint8, RGBA order."""
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        hip("ptReadResolvedImageSRGB8", self.device.handle, self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out


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
