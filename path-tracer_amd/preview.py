"""The primary-ray preview (mirror of src/application/preview_render.hpp)
over libpathtracer.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._core import Handle, hip, hip_get
from .device import Device, DeviceScene


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


class PreviewRenderContext(Handle):
    """preview_render_context (preview_render.hpp:15-20): primary-ray preview,
    AOVs and pick queries over a DeviceScene."""

    _destroy = "ptDestroyPreviewRenderContext"

    def __init__(self, device: Device, scene: DeviceScene):
        self.device, self.scene = device, scene
        self._create("ptCreatePreviewRenderContext", device.handle, scene.handle)
        self._size = (0, 0)

    def render(self, params: PreviewParameters):
        hip("ptRenderPreview", self.device.handle, self._h, C.byref(params.as_struct()))
        self._size = (params.RenderSizeY, params.RenderSizeX)

    def query(self) -> int:
        """RetrievePreviewQueryResult: shape index under the mouse (0xFFFFFFFF = none)."""
        return hip_get("ptRetrievePreviewQueryResult", self.device.handle, self._h)

    def image(self) -> np.ndarray:
        out = np.zeros(self._size + (4,), dtype=np.float32)
        hip("ptReadPreviewImage", self.device.handle, self._h, N.fptr(out))
        return out

    def aovs(self) -> np.ndarray:
        out = np.zeros(self._size, dtype=N.PREVIEW_AOV_DTYPE)
        hip("ptReadPreviewAOVs", self.device.handle, self._h, out.ctypes.data)
        return out
