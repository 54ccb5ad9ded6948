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

from ._core import PathTracerError
from .device import Comm, Device, DeviceScene, device_count
from .frame import DenoiseGuides, FrameHistory, SampleBuffer
from .host import (FrameStatistics, denoise_host, denoise_pair_host, despike_host, frame_statistics_host,
                   gather_visibility_rays_host, gather_visibility_reduce_host, rectify_host, reproject_host,
                   sh9_basis, sh9_irradiance, shape_motion, shape_surface_points, sky_gather_rays_host,
                   sky_gather_reduce_host, sky_irradiance, sky_radiance_sh, tile_mask_of_region, tile_statistics_host)
from .params import (AmbientOcclusionParameters, DenoiseParameters, DenoisePairParameters, DespikeParameters,
                     RectifyParameters, ReprojectParameters, ResolveParameters, SkyGatherParameters,
                     VisibilityGatherParameters)
from .preview import PreviewParameters, PreviewRenderContext
from .renderer import REFINE_MIN_ROUNDS, BasicRenderer, refine_tiles, render_until_noise


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
