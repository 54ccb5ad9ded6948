"""The parameter records of the resolve and post-processing passes
(include/pt_packed.h, include/pt_api.h), each with its defaults."""
from __future__ import annotations

from typing import TYPE_CHECKING

from . import _native as N

if TYPE_CHECKING:
    from .host import FrameStatistics


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


class AmbientOcclusionParameters:
    """pt_ambient_occlusion_parameters (pt_packed.h): the rays per pixel of
    the ambient-occlusion image (Samples, 1..64), how far an occluder may lie
    (Radius > 0; inf: visibility of the sky) and the integrator frame whose
    random stream draws them (Seed).  DESIGN.md §6 row 14."""

    def __init__(self, Samples: int = 16, Radius: float = float("inf"), Seed: int = 0):
        self.Samples, self.Radius, self.Seed = int(Samples), float(Radius), int(Seed)

    def as_struct(self) -> N.pt_ambient_occlusion_parameters:
        # An out-of-range count reaches the library's check instead of ctypes' wrap-around.
        return N.pt_ambient_occlusion_parameters(min(max(self.Samples, 0), 0xFFFFFFFF), self.Radius,
                                                 self.Seed & 0xFFFFFFFF)


class VisibilityGatherParameters:
    """pt_visibility_gather_parameters (pt_packed.h): the rays per point of
    DeviceScene.gather_visibility (Samples, a power of two up to 64), how far
    an occluder may lie (Radius > 0; inf: visibility of the sky), the
    integrator frame whose random streams draw them (Seed), how far along its
    direction a ray starts (Offset, finite and >= 0; the default is the
    integrator's restart offset) and the stream of the first point
    (FirstIndex: point i draws from stream FirstIndex + i, so a batch cut in
    pieces gives the whole batch's records).  DESIGN.md §6 row 15."""

    def __init__(self, Samples: int = 16, Radius: float = float("inf"), Seed: int = 0, Offset: float = 1e-3,
                 FirstIndex: int = 0):
        self.Samples, self.Radius, self.Seed = int(Samples), float(Radius), int(Seed)
        self.Offset, self.FirstIndex = float(Offset), int(FirstIndex)

    def as_struct(self) -> N.pt_visibility_gather_parameters:
        # An out-of-range count reaches the library's check instead of ctypes' wrap-around.
        if not 0 <= self.FirstIndex <= 0xFFFFFFFF:
            raise ValueError(f"FirstIndex {self.FirstIndex} outside 0..2^32 - 1")
        return N.pt_visibility_gather_parameters(min(max(self.Samples, 0), 0xFFFFFFFF), self.Radius,
                                                 self.Seed & 0xFFFFFFFF, self.Offset, self.FirstIndex)


class SkyGatherParameters:
    """pt_sky_gather_parameters (pt_packed.h): VisibilityGatherParameters'
    Samples, Radius, Seed, Offset and FirstIndex, with the same ranges, and
    the Lobe the rays of DeviceScene.gather_sky_light are drawn from:
    "cosine" (0; the cosine lobe around the point's normal, exactly
    DeviceScene.gather_visibility's rays: irradiance) or "sphere" (1; uniform
    over the sphere, no normal: a light probe).  DESIGN.md §6 row 16."""

    LOBES = {"cosine": N.SKY_GATHER_COSINE, "sphere": N.SKY_GATHER_SPHERE}

    def __init__(self, Samples: int = 16, Radius: float = float("inf"), Seed: int = 0, Offset: float = 1e-3,
                 FirstIndex: int = 0, Lobe: "int | str" = "cosine"):
        self.Samples, self.Radius, self.Seed = int(Samples), float(Radius), int(Seed)
        self.Offset, self.FirstIndex = float(Offset), int(FirstIndex)
        if isinstance(Lobe, str):
            if Lobe not in self.LOBES:
                raise ValueError(f"lobe {Lobe!r} is neither 'cosine' nor 'sphere'")
            Lobe = self.LOBES[Lobe]
        self.Lobe = int(Lobe)

    def as_struct(self) -> N.pt_sky_gather_parameters:
        # An out-of-range count or lobe reaches the library's check instead of ctypes' wrap-around.
        if not 0 <= self.FirstIndex <= 0xFFFFFFFF:
            raise ValueError(f"FirstIndex {self.FirstIndex} outside 0..2^32 - 1")
        return N.pt_sky_gather_parameters(min(max(self.Samples, 0), 0xFFFFFFFF), self.Radius, self.Seed & 0xFFFFFFFF,
                                          self.Offset, self.FirstIndex, min(max(self.Lobe, 0), 0xFFFFFFFF))
