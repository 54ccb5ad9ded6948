"""ctypes bindings of the C ABI (include/pt_api.h, include/pt_scene.h).

The libraries are built in-tree by path-tracer_amd/build.py.  There is no
fallback: if libpathtracer.so cannot be loaded, every device entry point
raises, so a GPU run can never silently take a CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
SCENE_LIB_PATH = PKG / "libptscene.so"
HIP_LIB_PATH = PKG / "libpathtracer.so"


class NativeLibraryMissing(RuntimeError):
    pass


# --- structs (include/pt_packed.h, include/pt_api.h) ---------------------------

class pt_scene_packs(C.Structure):
    _fields_ = [
        ("globals", C.c_void_p),
        ("textures", C.c_void_p), ("texture_count", C.c_uint32),
        ("material_data", C.c_void_p), ("material_word_count", C.c_uint32),
        ("shapes", C.c_void_p), ("shape_count", C.c_uint32),
        ("shape_nodes", C.c_void_p), ("shape_node_count", C.c_uint32),
        ("mesh_faces", C.c_void_p), ("mesh_face_count", C.c_uint32),
        ("mesh_vertices", C.c_void_p), ("mesh_vertex_count", C.c_uint32),
        ("mesh_nodes", C.c_void_p), ("mesh_node_count", C.c_uint32),
        ("cameras", C.c_void_p), ("camera_count", C.c_uint32),
        ("atlas", C.c_void_p),
        ("atlas_width", C.c_uint32), ("atlas_height", C.c_uint32), ("atlas_layer_count", C.c_uint32),
    ]


class pt_shade_info(C.Structure):
    """pt_shade_info (include/pt_api.h): the shade variant a renderer runs."""
    _fields_ = [("scene_mask", C.c_uint32), ("kernel_mask", C.c_uint32), ("completion_queue", C.c_uint32),
                ("grey_records", C.c_uint32), ("ray_order", C.c_uint32), ("length_trained", C.c_uint32),
                ("block_map", C.c_uint32)]


RAY_ORDER_AUTO, RAY_ORDER_OCTANT, RAY_ORDER_LENGTH = 0, 1, 2   # PT_RAY_ORDER_*
BLOCK_MAP_AUTO, BLOCK_MAP_TILE, BLOCK_MAP_RUN = 0, 1, 2        # PT_BLOCK_MAP_*
RAYKEY_COUNT = 32768                                            # PT_RAYKEY_COUNT (include/pt_raykey.h)


SHADE_DIFFUSE, SHADE_METAL, SHADE_TRANSLUCENT, SHADE_SCATTER = 1, 2, 4, 8
SHADE_OPENPBR, SHADE_PRIMS, SHADE_SKY, SHADE_TEXWRAP = 16, 32, 64, 128


class pt_basic_renderer_params(C.Structure):
    _fields_ = [
        ("FrameIndex", C.c_uint32),
        ("CameraIndex", C.c_uint32),
        ("RenderFlags", C.c_uint32),
        ("PathLengthLimit", C.c_uint32),
        ("PathTerminationProbability", C.c_float),
    ]


class pts_load_model_options(C.Structure):
    """load_model_options (src/scene/scene.hpp:383-391) + openpbr_as_diffuse."""
    _fields_ = [
        ("name", C.c_char_p), ("directory_path", C.c_char_p),
        ("vertex_transform", C.c_float * 16), ("normal_transform", C.c_float * 16),
        ("texcoord_transform", C.c_float * 9), ("openpbr_as_diffuse", C.c_int),
    ]


class pt_resolve_parameters(C.Structure):
    """resolve_parameters (src/integrator/integrator.hpp:43-48)."""
    _fields_ = [
        ("Brightness", C.c_float),
        ("ToneMappingMode", C.c_uint32),
        ("ToneMappingWhiteLevel", C.c_float),
    ]


class pt_denoise_parameters(C.Structure):
    """pt_denoise_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Iterations", C.c_uint32),
        ("SigmaColor", C.c_float),
        ("SigmaNormal", C.c_float),
        ("SigmaDepth", C.c_float),
        ("SigmaAlbedo", C.c_float),
    ]


class pt_denoise_pair_parameters(C.Structure):
    """pt_denoise_pair_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Iterations", C.c_uint32),
        ("SigmaLuminance", C.c_float),
        ("SigmaNormal", C.c_float),
        ("SigmaDepth", C.c_float),
        ("SigmaAlbedo", C.c_float),
    ]


class pt_reproject_parameters(C.Structure):
    """pt_reproject_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("NormalCosine", C.c_float),
        ("DepthTolerance", C.c_float),
        ("MinWeight", C.c_float),
        ("MaxHistory", C.c_float),
    ]


class pt_rectify_parameters(C.Structure):
    """pt_rectify_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Radius", C.c_uint32),
        ("MinNeighbours", C.c_uint32),
        ("Sigma", C.c_float),
        ("ClampedHistory", C.c_float),
        ("NormalCosine", C.c_float),
    ]


assert C.sizeof(pt_rectify_parameters) == 20


class pt_despike_parameters(C.Structure):
    """pt_despike_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Radius", C.c_uint32),
        ("Rank", C.c_uint32),
        ("MinNeighbours", C.c_uint32),
        ("Scale", C.c_float),
        ("Floor", C.c_float),
        ("NormalCosine", C.c_float),
    ]


assert C.sizeof(pt_despike_parameters) == 24


class pt_ambient_occlusion_parameters(C.Structure):
    """pt_ambient_occlusion_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Samples", C.c_uint32),
        ("Radius", C.c_float),
        ("Seed", C.c_uint32),
    ]


assert C.sizeof(pt_ambient_occlusion_parameters) == 12
AMBIENT_OCCLUSION_MAX_SAMPLES = 64   # PT_AMBIENT_OCCLUSION_MAX_SAMPLES (include/pt_visibility.h)


class pt_visibility_gather_parameters(C.Structure):
    """pt_visibility_gather_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Samples", C.c_uint32),
        ("Radius", C.c_float),
        ("Seed", C.c_uint32),
        ("Offset", C.c_float),
        ("FirstIndex", C.c_uint32),
    ]


assert C.sizeof(pt_visibility_gather_parameters) == 20
# pt_visibility_record (include/pt_packed.h): one point's gathered visibility.
VISIBILITY_RECORD_DTYPE = np.dtype([("Bent", "<f4", (3,)), ("Unoccluded", "<f4"), ("OccludedMask", "<u8"),
                                    ("Samples", "<f4"), ("Reserved", "<u4")])
assert VISIBILITY_RECORD_DTYPE.itemsize == 32
VISIBILITY_GATHER_MAX_POINTS = 1 << 26   # PT_VISIBILITY_GATHER_MAX_POINTS (include/pt_visibility.h)
VISIBILITY_GATHER_MAX_LANES = 1 << 22    # PT_VISIBILITY_GATHER_MAX_LANES


class pt_sky_gather_parameters(C.Structure):
    """pt_sky_gather_parameters (include/pt_packed.h)."""
    _fields_ = [
        ("Samples", C.c_uint32),
        ("Radius", C.c_float),
        ("Seed", C.c_uint32),
        ("Offset", C.c_float),
        ("FirstIndex", C.c_uint32),
        ("Lobe", C.c_uint32),
    ]


assert C.sizeof(pt_sky_gather_parameters) == 24
SKY_GATHER_COSINE = 0   # PT_SKY_GATHER_COSINE (include/pt_packed.h)
SKY_GATHER_SPHERE = 1   # PT_SKY_GATHER_SPHERE

STATS_BINS = 256


class pt_frame_statistics(C.Structure):
    """pt_frame_statistics (include/pt_packed.h)."""
    _fields_ = [
        ("pixels", C.c_uint64),
        ("filled", C.c_uint64),
        ("empty", C.c_uint64),
        ("nonfinite", C.c_uint64),
        ("dark", C.c_uint64),
        ("luminance_histogram", C.c_uint32 * STATS_BINS),
        ("min_luminance", C.c_float),
        ("max_luminance", C.c_float),
        ("min_samples", C.c_float),
        ("max_samples", C.c_float),
        ("noise_pixels", C.c_uint64),
        ("noise_skipped", C.c_uint64),
        ("noise_histogram", C.c_uint32 * STATS_BINS),
    ]


# pt_tile_statistics (include/pt_packed.h): one 32-byte record per 16 x 16 tile.
TILE_SIZE = 16
TILE_STATS_DTYPE = np.dtype([("filled", "<u4"), ("empty", "<u4"), ("nonfinite", "<u4"), ("pair", "<u4"),
                             ("over", "<u4"), ("min_count", "<f4"), ("max_count", "<f4"), ("reserved", "<u4")])
assert TILE_STATS_DTYPE.itemsize == 32


class pt_packed_transform(C.Structure):
    _fields_ = [("To", C.c_float * 16), ("From", C.c_float * 16)]


class pt_packed_camera(C.Structure):
    """pt_packed_camera (include/pt_packed.h); CAMERA_DTYPE is the same record in numpy."""
    _fields_ = [
        ("Model", C.c_uint32),
        ("FocalLength", C.c_float),
        ("ApertureRadius", C.c_float),
        ("SensorDistance", C.c_float),
        ("SensorSize", C.c_float * 2),
        ("Pad0", C.c_uint32 * 2),
        ("Transform", pt_packed_transform),
    ]


class pt_preview_parameters(C.Structure):
    """preview_parameters (src/application/preview_render.hpp:22-33)."""
    _fields_ = [
        ("CameraTransform", pt_packed_transform),
        ("RenderMode", C.c_uint32),
        ("Brightness", C.c_float),
        ("SelectedShapeIndex", C.c_uint32),
        ("RenderSizeX", C.c_uint32), ("RenderSizeY", C.c_uint32),
        ("MouseX", C.c_uint32), ("MouseY", C.c_uint32),
    ]


class pts_config_info(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("camera_count", C.c_uint32),
        ("render_flags", C.c_uint32), ("termination_probability", C.c_float),
        ("mesh_face_count", C.c_uint32), ("shape_count", C.c_uint32),
    ]


HIT_RECORD_DTYPE = np.dtype([
    ("time", "<f4"), ("shape_material", "<u4"), ("packed_normal", "<u4"),
    ("packed_tangent", "<u4"), ("u", "<f4"), ("v", "<f4"),
])
assert HIT_RECORD_DTYPE.itemsize == 24

PIXEL_STATE_DTYPE = np.dtype([
    ("origin", "<f4", (3,)), ("packed_velocity", "<u4"),
    ("hit", HIT_RECORD_DTYPE),
    ("lambda0", "<f4"), ("throughput", "<f4", (4,)), ("probability", "<f4", (4,)),
    ("sample", "<f4", (3,)), ("active01", "<u4"), ("active23", "<u4"),
])
assert PIXEL_STATE_DTYPE.itemsize == 96

PREVIEW_AOV_DTYPE = np.dtype([
    ("time", "<f4"), ("shape_index", "<u4"), ("material_index", "<u4"), ("primitive_index", "<u4"),
    ("mesh_complexity", "<u4"), ("scene_complexity", "<u4"), ("normal", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"),
    ("reserved", "<u4"),
])
assert PREVIEW_AOV_DTYPE.itemsize == 48

# pt_denoise_guide (include/pt_packed.h): a pixel's primary-hit record for the denoiser.
DENOISE_GUIDE_DTYPE = np.dtype([("normal", "<f4", (3,)), ("time", "<f4"), ("albedo", "<f4", (3,)), ("shape", "<u4")])
assert DENOISE_GUIDE_DTYPE.itemsize == 32

# Packed scene layouts (include/pt_packed.h) as numpy dtypes, for tests.
SHAPE_NODE_DTYPE = np.dtype([("Minimum", "<f4", (3,)), ("ChildNodeIndices", "<u4"),
                             ("Maximum", "<f4", (3,)), ("ShapeIndex", "<u4")])
MESH_NODE_DTYPE = np.dtype([("Minimum", "<f4", (3,)), ("FaceBeginOrNodeIndex", "<u4"),
                            ("Maximum", "<f4", (3,)), ("FaceEndIndex", "<u4")])
MESH_FACE_DTYPE = np.dtype([("Position0", "<f4", (3,)), ("VertexIndex0", "<u4"),
                            ("Position1", "<f4", (3,)), ("VertexIndex1", "<u4"),
                            ("Position2", "<f4", (3,)), ("VertexIndex2", "<u4")])
MESH_VERTEX_DTYPE = np.dtype([("PackedNormal", "<u4"), ("PackedUV", "<u4")])
TRANSFORM_DTYPE = np.dtype([("To", "<f4", (16,)), ("From", "<f4", (16,))])
SHAPE_DTYPE = np.dtype([("Type", "<i4"), ("MaterialIndex", "<u4"), ("MeshRootNodeIndex", "<u4"),
                        ("Pad0", "<u4"), ("Transform", TRANSFORM_DTYPE)])
CAMERA_DTYPE = np.dtype([("Model", "<u4"), ("FocalLength", "<f4"), ("ApertureRadius", "<f4"),
                         ("SensorDistance", "<f4"), ("SensorSize", "<f4", (2,)), ("Pad0", "<u4", (2,)),
                         ("Transform", TRANSFORM_DTYPE)])
TEXTURE_DTYPE = np.dtype([("AtlasPlacementMinimum", "<f4", (2,)), ("AtlasPlacementMaximum", "<f4", (2,)),
                          ("AtlasImageIndex", "<u4"), ("Type", "<u4"), ("Flags", "<u4"), ("Unused0", "<u4")])
GLOBALS_DTYPE = np.dtype([("SkyboxMeanDirection", "<f4", (3,)), ("SkyboxConcentration", "<f4"),
                          ("SkyboxSamplingProbability", "<f4"), ("SkyboxBrightness", "<f4"),
                          ("SkyboxTextureIndex", "<u4"), ("ShapeCount", "<u4"), ("SceneScatterRate", "<f4"),
                          ("Pad0", "<u4", (3,))])
assert SHAPE_NODE_DTYPE.itemsize == 32 and MESH_NODE_DTYPE.itemsize == 32 and MESH_FACE_DTYPE.itemsize == 48
assert SHAPE_DTYPE.itemsize == 144 and CAMERA_DTYPE.itemsize == 160 and GLOBALS_DTYPE.itemsize == 48
assert TEXTURE_DTYPE.itemsize == 32
# pt_shape_motion (include/pt_packed.h): one shape's motion between two packed scenes (ptsShapeMotion).
SHAPE_MOTION_DTYPE = np.dtype([("Point", "<f4", (12,)), ("Normal", "<f4", (9,)), ("Flags", "<u4"),
                               ("Pad0", "<u4", (2,))])
assert SHAPE_MOTION_DTYPE.itemsize == 96
SHAPE_MOTION_MOVED, SHAPE_MOTION_NO_HISTORY = 1, 2

KERNEL_RAYGEN, KERNEL_EXTEND, KERNEL_SHADE, KERNEL_RESOLVE = 0, 1, 2, 3
TONE_MAPPING_CLAMP, TONE_MAPPING_REINHARD, TONE_MAPPING_HABLE, TONE_MAPPING_ACES = 0, 1, 2, 3
(PREVIEW_RENDER_MODE_BASE_COLOR, PREVIEW_RENDER_MODE_BASE_COLOR_SHADED, PREVIEW_RENDER_MODE_NORMAL,
 PREVIEW_RENDER_MODE_MATERIAL_INDEX, PREVIEW_RENDER_MODE_PRIMITIVE_INDEX, PREVIEW_RENDER_MODE_MESH_COMPLEXITY,
 PREVIEW_RENDER_MODE_SCENE_COMPLEXITY) = range(7)
KERNEL_PREVIEW = 4
KERNEL_ROUND = 5     # fused extend + shade (partitions that fit the GPU at once)
KERNEL_ROUNDS = 6    # a round batch: several rounds of every tile in one launch (PT_KERNEL_ROUNDS)
MAX_SPLIT = 4        # PT_MAX_SPLIT: tile groups of ptSetBasicRendererSplit
KERNEL_DENOISE = 7   # one a-trous iteration; ptDespikeSampleBuffer's launch (PT_KERNEL_DENOISE)
KERNEL_GUIDES = 8    # ptRenderDenoiseGuides (PT_KERNEL_GUIDES)
GUIDE_MAX_BOUNCES = 8  # ptRenderDenoiseGuidesSpecular (PT_GUIDE_MAX_BOUNCES)
DENOISE_MAX_ITERATIONS = 8
DENOISE_VARIANT_AUTO, DENOISE_VARIANT_GATHER, DENOISE_VARIANT_LATTICE = 0, 1, 2
KERNEL_STATS = 9     # the frame and tile statistics passes and the sample-buffer add (PT_KERNEL_STATS)
STATS_VARIANT_AUTO, STATS_VARIANT_PLAIN, STATS_VARIANT_UNIFORM = 0, 1, 2
KERNEL_REPROJECT = 10   # ptReprojectSampleBuffer[Moving] and ptRectifyHistory (PT_KERNEL_REPROJECT)

# The numerics probe's operations (include/pt_numerics.h PT_NUM_*: the index is the id).
NUMERICS_OPS = (
    "add", "mul", "div", "sqrt", "fma", "min", "max", "clamp", "floor", "fract", "rint", "round_half_away", "mix",
    "exp", "log", "pow", "sin", "cos", "atan2", "asin", "u32_to_float", "floor_to_int", "random", "random01",
    "pack_snorm16", "unpack_snorm16", "half_to_float", "pack_unit_vector", "unpack_unit_vector", "fast_rcp", "xdiv",
)
NUMERICS_OPERANDS = {"fma": 3, "clamp": 3, "mix": 3, "pack_unit_vector": 3, "add": 2, "mul": 2, "div": 2, "min": 2,
                     "max": 2, "pow": 2, "atan2": 2, "xdiv": 2}   # every other op reads one operand
NUMERICS_OUTPUTS = {"random": 2, "unpack_unit_vector": 3}          # every other op writes one word
NUMERICS_DEVICE_ONLY = ("fast_rcp", "xdiv")                        # pt_device.hpp forms without a host counterpart

_vp = C.c_void_p
_u32 = C.c_uint32
_f32 = C.c_float
_i32 = C.c_int
_fptr = C.POINTER(C.c_float)
_u32ptr = C.POINTER(C.c_uint32)

# name: (restype, argtypes)
SCENE_API = {
    "ptsGetLastError": (C.c_char_p, []),
    "ptsCreateScene": (_vp, []),
    "ptsCreateEmptyScene": (_vp, []),
    "ptsCreateConfigScene": (_vp, [_i32, C.POINTER(pts_config_info)]),
    "ptsDestroyScene": (None, [_vp]),
    "ptsSceneRoot": (_vp, [_vp]),
    "ptsCreateEntity": (_vp, [_vp, _i32, _vp]),
    "ptsSetEntityTransform": (None, [_vp, _vp, _fptr, _fptr, _fptr]),
    "ptsSetEntityActive": (None, [_vp, _vp, _i32]),
    "ptsSetEntityMaterial": (None, [_vp, _vp, _vp]),
    "ptsSetEntityMesh": (None, [_vp, _vp, _vp]),
    "ptsEntityPackedShapeIndex": (_u32, [_vp]),
    "ptsSetCameraPinhole": (None, [_vp, _vp, _f32, _f32]),
    "ptsSetCameraThinLens": (None, [_vp, _vp, _f32, _f32, _f32, _f32, _f32]),
    "ptsSetCamera360": (None, [_vp, _vp]),
    "ptsFindCamera": (_vp, [_vp, _u32]),
    "ptsSetCameraTransform": (None, [_vp, _vp, _fptr, _fptr]),
    "ptsSetRootParameters": (None, [_vp, _f32, _f32, _f32, _vp]),
    "ptsCreateMaterial": (_vp, [_vp, _i32, C.c_char_p]),
    "ptsSetMaterialParameter": (_i32, [_vp, _vp, C.c_char_p, _fptr, _i32]),
    "ptsSetMaterialTexture": (_i32, [_vp, _vp, C.c_char_p, _vp]),
    "ptsMaterialPackedIndex": (_u32, [_vp]),
    "ptsCreateCheckerTexture": (_vp, [_vp, C.c_char_p, _i32, _fptr, _fptr]),
    "ptsCreateTexture": (_vp, [_vp, C.c_char_p, _i32, _u32, _u32, _fptr, _i32]),
    "ptsCreateMesh": (_vp, [_vp, C.c_char_p, _u32, _fptr, _fptr, _fptr, _u32, _u32ptr]),
    "ptsMeshDepth": (_u32, [_vp]),
    "ptsMeshNodeCount": (_u32, [_vp]),
    "ptsMeshFaces": (None, [_vp, _u32ptr]),
    "ptsDefaultLoadModelOptions": (None, [C.POINTER(pts_load_model_options)]),
    "ptsLoadTexture": (_vp, [_vp, C.c_char_p, _i32, C.c_char_p]),
    "ptsLoadImageRGBA8": (_i32, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _vp]),
    "ptsLoadModelAsPrefab": (_vp, [_vp, C.c_char_p, C.POINTER(pts_load_model_options)]),
    "ptsInstantiatePrefab": (_vp, [_vp, _vp, _vp]),
    "ptsLoadScene": (_vp, [C.c_char_p]),
    "ptsSaveScene": (_i32, [_vp, C.c_char_p]),
    "ptsSceneTextureCount": (_u32, [_vp]),
    "ptsSceneMaterialCount": (_u32, [_vp]),
    "ptsSceneMeshCount": (_u32, [_vp]),
    "ptsScenePrefabCount": (_u32, [_vp]),
    "ptsPrefabMeshCount": (_u32, [_vp]),
    "ptsPrefabMesh": (_vp, [_vp, _u32, C.POINTER(_vp), _fptr]),
    "ptsMeshVertexCount": (_u32, [_vp]),
    "ptsMeshFaceCount": (_u32, [_vp]),
    "ptsMeshVertices": (None, [_vp, _fptr]),
    "ptsMaterialType": (_i32, [_vp]),
    "ptsPackSceneData": (_u32, [_vp]),
    "ptsGetScenePacks": (None, [_vp, C.POINTER(pt_scene_packs)]),
    "ptsMarkDirty": (None, [_vp, _u32]),
    "ptsGetParametricSpectrumCoefficients": (_i32, [_fptr, _fptr]),
    "ptsBuildSpectrumTable": (_i32, [_i32]),
    "ptsSaveSpectrumTable": (_i32, [C.c_char_p]),
    "ptsLoadSpectrumTable": (_i32, [C.c_char_p]),
    "ptsSetSpectrumTablePath": (None, [C.c_char_p]),
    "ptsDenoise": (_i32, [_u32, _u32, _fptr, _vp, C.POINTER(pt_denoise_parameters), _fptr]),
    "ptsDenoisePair": (_i32, [_u32, _u32, _fptr, _fptr, _vp, C.POINTER(pt_denoise_pair_parameters), _fptr]),
    "ptsReproject": (_i32, [_u32, _u32, _fptr, _vp, C.POINTER(pt_packed_camera), _u32, _u32, _vp,
                            C.POINTER(pt_packed_camera), C.POINTER(pt_reproject_parameters), _fptr]),
    "ptsShapeMotion": (_i32, [_vp, _u32, _vp, _u32, _vp]),
    "ptsReprojectMoving": (_i32, [_u32, _u32, _fptr, _vp, C.POINTER(pt_packed_camera), _u32, _u32, _vp,
                                  C.POINTER(pt_packed_camera), _vp, _u32, C.POINTER(pt_reproject_parameters), _fptr]),
    "ptsRectifyHistory": (_i32, [_u32, _u32, _fptr, _fptr, _vp, C.POINTER(pt_rectify_parameters), _fptr]),
    "ptsDespike": (_i32, [_u32, _u32, _fptr, _vp, C.POINTER(pt_despike_parameters), _fptr]),
    "ptsCentralCameraRay": (_i32, [C.POINTER(pt_packed_camera), _u32, _u32, _u32, _u32, _fptr, _fptr]),
    "ptsAmbientOcclusionRays": (_i32, [C.POINTER(pt_ambient_occlusion_parameters), _u32, _u32, _fptr, _fptr, _f32,
                                       _fptr, _fptr, _u32ptr, _fptr]),
    "ptsGatherVisibilityRays": (_i32, [C.POINTER(pt_visibility_gather_parameters), _u32, _fptr, _fptr, _fptr, _u32ptr,
                                       _fptr]),
    "ptsGatherVisibilityReduce": (_i32, [_u32, _u32, _u32ptr, C.POINTER(C.c_uint64), _vp]),
    "ptsVisibilitySkip": (_u32, [_u32, _u32]),
    "ptsSkyGatherRays": (_i32, [C.POINTER(pt_sky_gather_parameters), _u32, _fptr, _fptr, _fptr, _u32ptr, _fptr, _fptr]),
    "ptsSkyGatherReduce": (_i32, [_u32, _u32, _u32ptr, C.POINTER(C.c_uint64), _fptr, _vp]),
    "ptsSkyGatherBasis": (_i32, [_u32, _u32ptr, _fptr]),
    "ptsFrameStatistics": (_i32, [_u32, _u32, _fptr, _fptr, C.POINTER(pt_frame_statistics)]),
    "ptsTileStatistics": (_i32, [_u32, _u32, _fptr, _fptr, _f32, _vp]),
    "ptsStatsBin": (_i32, [C.c_float]),
    "ptsStatsBinEdge": (C.c_double, [_i32]),
    "ptsStatsPercentileBin": (_i32, [_u32ptr, C.c_double]),
    "ptsStatsLogAverage": (C.c_double, [_u32ptr, C.c_double, C.c_double]),
    "ptsStatsAutoBrightness": (C.c_double, [C.POINTER(pt_frame_statistics), C.c_double, C.c_double, C.c_double]),
    "ptsStatsNoise": (C.c_double, [C.POINTER(pt_frame_statistics), C.c_double]),
    "ptsRayKey": (_u32, [_fptr, _fptr, _fptr, _fptr]),
    "ptsFaceTest": (_i32, [_u32, _fptr, _fptr, _fptr, _fptr, _fptr, _u32ptr, _fptr, _fptr, _fptr, _u32ptr]),
}

HIP_API = {
    "ptGetLastError": (C.c_char_p, []),
    "ptGetDeviceCount": (_i32, [C.POINTER(_i32)]),
    "ptCreateDevice": (_vp, [_i32]),
    "ptDestroyDevice": (None, [_vp]),
    "ptSynchronize": (_i32, [_vp]),
    "ptCreateScene": (_vp, [_vp]),
    "ptUpdateScene": (_i32, [_vp, _vp, C.POINTER(pt_scene_packs), _u32]),
    "ptSetSceneStackFormat": (_i32, [_vp, _u32]),
    "ptSetSceneHitRecordForm": (_i32, [_vp, _u32]),
    "ptSetSceneExtendForm": (_i32, [_vp, _u32]),
    "ptGetSceneExtendForm": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "ptDestroyScene": (None, [_vp, _vp]),
    "ptCreateSampleBuffer": (_vp, [_vp, _u32, _u32]),
    "ptDestroySampleBuffer": (None, [_vp, _vp]),
    "ptReadSampleBuffer": (_i32, [_vp, _vp, _fptr]),
    "ptWriteSampleBuffer": (_i32, [_vp, _vp, _fptr]),
    "ptRenderSampleBuffer": (_i32, [_vp, _vp, C.POINTER(pt_resolve_parameters)]),
    "ptReadResolvedImage": (_i32, [_vp, _vp, _fptr]),
    "ptReadResolvedImageSRGB8": (_i32, [_vp, _vp, C.POINTER(C.c_uint8)]),
    "ptCreateBasicRenderer": (_vp, [_vp, _vp, _vp]),
    "ptCreateBasicRendererPartitioned": (_vp, [_vp, _vp, _vp, _u32, _u32]),
    "ptCreateBasicRendererStreams": (_vp, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "ptMergeBasicRendererStreams": (_i32, [_vp, _vp]),
    "ptBasicRendererStreams": (_u32, [_vp]),
    "ptReadBasicRendererStreamState": (_i32, [_vp, _vp, _u32, _vp]),
    "ptWriteBasicRendererState": (_i32, [_vp, _vp, _vp]),
    "ptWriteBasicRendererStreamState": (_i32, [_vp, _vp, _u32, _vp]),
    "ptReadBasicRendererStreamAccumulator": (_i32, [_vp, _vp, _u32, _fptr]),
    "ptWriteBasicRendererStreamAccumulator": (_i32, [_vp, _vp, _u32, _fptr]),
    "ptGetBasicRendererShadeInfo": (_i32, [_vp, C.POINTER(pt_shade_info)]),
    "ptDestroyBasicRenderer": (None, [_vp, _vp]),
    "ptBasicRendererParams": (C.POINTER(pt_basic_renderer_params), [_vp]),
    "ptResetBasicRenderer": (_i32, [_vp, _vp]),
    "ptRunBasicRenderer": (_i32, [_vp, _vp, _u32]),
    "ptBasicRendererSlotCount": (_u32, [_vp]),
    "ptSetBasicRendererFusedRounds": (_i32, [_vp, _i32]),
    "ptRunBasicRendererRounds": (_i32, [_vp, _vp, _u32]),
    "ptSetBasicRendererRoundBatch": (_i32, [_vp, _u32]),
    "ptSetBasicRendererSplit": (_i32, [_vp, _u32]),
    "ptSetBasicRendererClassLists": (_i32, [_vp, _u32]),
    "ptGetBasicRendererClassLists": (_i32, [_vp, _u32ptr]),
    "ptGetBasicRendererSplit": (_i32, [_vp, _u32ptr, _u32ptr, _u32ptr]),
    "ptSetBasicRendererRayOrder": (_i32, [_vp, _u32]),
    "ptGetBasicRendererRayOrder": (_i32, [_vp, _u32ptr, _u32ptr]),
    "ptSetBasicRendererBlockMap": (_i32, [_vp, _u32]),
    "ptGetBasicRendererBlockMap": (_i32, [_vp, _u32ptr, _u32ptr]),
    "ptBlockMapGroupTileCount": (_u32, [_u32, _u32, _u32, _u32]),
    "ptBlockMapGroupTile": (_u32, [_u32, _u32, _u32, _u32, _u32]),
    "ptBlockMapGroupTileStart": (_u32, [_u32, _u32, _u32, _u32]),
    "ptBlockMapGroupUnitCount": (_u32, [_u32, _u32, _u32, _u32]),
    "ptBlockMapGroupUnit": (_u32, [_u32, _u32, _u32, _u32, _u32]),
    "ptBlockMapGroupUnitStart": (_u32, [_u32, _u32, _u32, _u32]),
    "ptBlockMapUnitTile": (_u32, [_u32, _u32, _u32]),
    "ptBlockMapUnitQuarter": (_u32, [_u32, _u32, _u32]),
    "ptReadSceneLengthTable": (_i32, [_vp, _vp, _vp, _u32ptr, C.POINTER(C.c_uint64)]),
    "ptReadBasicRendererRayPositions": (_i32, [_vp, _vp, _vp]),
    "ptSetBasicRendererOpenPBR": (_i32, [_vp, _i32]),
    "ptGetStats": (_i32, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ptTraceRaysStats": (_i32, [_vp, _vp, _u32, _fptr, _u32ptr, _fptr, C.POINTER(C.c_uint64), _vp]),
    "ptRenderFrame": (_i32, [_vp, _vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ptReadBasicRendererState": (_i32, [_vp, _vp, _vp]),
    "ptTraceRays": (_i32, [_vp, _vp, _u32, _fptr, _u32ptr, _fptr, _vp]),
    "ptOccludedRays": (_i32, [_vp, _vp, _u32, _fptr, _u32ptr, _fptr, C.POINTER(C.c_uint64)]),
    "ptOccludedRaysStats": (_i32, [_vp, _vp, _u32, _fptr, _u32ptr, _fptr, C.POINTER(C.c_uint64), _vp]),
    "ptRenderAmbientOcclusion": (_i32, [_vp, _vp, _u32, C.POINTER(pt_ambient_occlusion_parameters), _vp]),
    "ptGatherVisibility": (_i32, [_vp, _vp, _u32, _fptr, _fptr, C.POINTER(pt_visibility_gather_parameters), _vp]),
    "ptGatherVisibilityChunked": (_i32, [_vp, _vp, _u32, _fptr, _fptr, C.POINTER(pt_visibility_gather_parameters),
                                         _u32, _vp]),
    "ptGatherSkyLight": (_i32, [_vp, _vp, _u32, _fptr, _fptr, C.POINTER(pt_sky_gather_parameters), _vp]),
    "ptGatherSkyLightChunked": (_i32, [_vp, _vp, _u32, _fptr, _fptr, C.POINTER(pt_sky_gather_parameters), _u32, _vp]),
    "ptCreatePreviewRenderContext": (_vp, [_vp, _vp]),
    "ptDestroyPreviewRenderContext": (None, [_vp, _vp]),
    "ptRenderPreview": (_i32, [_vp, _vp, C.POINTER(pt_preview_parameters)]),
    "ptRetrievePreviewQueryResult": (_i32, [_vp, _vp, C.POINTER(C.c_uint32)]),
    "ptReadPreviewImage": (_i32, [_vp, _vp, _fptr]),
    "ptReadPreviewAOVs": (_i32, [_vp, _vp, _vp]),
    "ptCreateDenoiseGuides": (_vp, [_vp, _u32, _u32]),
    "ptDestroyDenoiseGuides": (None, [_vp, _vp]),
    "ptRenderDenoiseGuides": (_i32, [_vp, _vp, _vp, _u32]),
    "ptRenderDenoiseGuidesSpecular": (_i32, [_vp, _vp, _vp, _u32, _u32]),
    "ptReadDenoiseGuides": (_i32, [_vp, _vp, _vp]),
    "ptWriteDenoiseGuides": (_i32, [_vp, _vp, _vp]),
    "ptDenoiseSampleBuffer": (_i32, [_vp, _vp, _vp, C.POINTER(pt_denoise_parameters), _vp]),
    "ptSetDenoiseVariant": (_i32, [_vp, _u32]),
    "ptDenoiseSampleBufferPair": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(pt_denoise_pair_parameters), _vp]),
    "ptReprojectSampleBuffer": (_i32, [_vp, _vp, _vp, C.POINTER(pt_packed_camera), _vp, C.POINTER(pt_packed_camera),
                                       C.POINTER(pt_reproject_parameters), _vp]),
    "ptReprojectSampleBufferMoving": (_i32, [_vp, _vp, _vp, C.POINTER(pt_packed_camera), _vp,
                                             C.POINTER(pt_packed_camera), _vp, _u32,
                                             C.POINTER(pt_reproject_parameters), _vp]),
    "ptRectifyHistory": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(pt_rectify_parameters), _vp]),
    "ptDespikeSampleBuffer": (_i32, [_vp, _vp, _vp, C.POINTER(pt_despike_parameters), _vp]),
    "ptComputeFrameStatistics": (_i32, [_vp, _vp, _vp, C.POINTER(pt_frame_statistics)]),
    "ptComputeTileStatistics": (_i32, [_vp, _vp, _vp, _f32, _vp]),
    "ptSetBasicRendererActiveTiles": (_i32, [_vp, _vp, _vp, _u32]),
    "ptGetBasicRendererActiveTiles": (_i32, [_vp, _u32ptr, _u32ptr]),
    "ptAccumulateSampleBuffer": (_i32, [_vp, _vp, _vp]),
    "ptSetFrameStatisticsVariant": (_i32, [_vp, _u32]),
    "ptCheckFastDivision": (_i32, [_vp, C.c_uint64, _u32, C.POINTER(C.c_uint64)]),
    "ptCheckFastReciprocal": (_i32, [_vp, C.POINTER(C.c_uint64)]),
    "ptEvalNumerics": (_i32, [_vp, _u32, _u32, _u32ptr, _u32ptr, _u32ptr, _u32ptr]),
    "ptSampleTextures": (_i32, [_vp, _vp, _u32, _u32ptr, _fptr, _u32, _fptr]),
    "ptEvalSlabTest": (_i32, [_vp, _u32, _fptr, _fptr, _fptr, _fptr, _fptr, _u32, _u32ptr, _u32ptr]),
    "ptExtendStats": (_i32, [_vp, _vp, C.POINTER(C.c_uint64)]),
    "ptExtendStepCounts": (_i32, [_vp, _vp, _vp]),
    "ptSetProfilingPeriod": (_i32, [_vp, C.c_uint32]),
    "ptSceneStackNeeded": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "ptSceneFastDivision": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "ptSceneNodeCache": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "ptSetProfiling": (_i32, [_vp, _i32]),
    "ptGetKernelStats": (_i32, [_vp, _i32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "ptGetKernelRounds": (_i32, [_vp, _i32, C.POINTER(C.c_uint64)]),
    "ptResetKernelStats": (_i32, [_vp]),
    "ptCommGetUniqueId": (_i32, [C.POINTER(C.c_uint8)]),
    "ptCommCreate": (_vp, [_vp, _i32, _i32, C.POINTER(C.c_uint8)]),
    "ptCommDestroy": (None, [_vp]),
    "ptCommSetTimeout": (_i32, [_vp, C.c_double]),
    "ptCommReduceSampleBuffer": (_i32, [_vp, _vp, _vp, _i32]),
    "ptCommGatherSampleBuffer": (_i32, [_vp, _vp, _vp, _i32]),
    "ptCommReduceSampleBufferInto": (_i32, [_vp, _vp, _vp, _vp, _i32]),
}

_scene_lib = None
_hip_lib = None


def _bind(lib, table, required=True):
    """Set every entry point's ctypes signature.  required=False (a
    PT_HIP_LIB experiment build of an older tree, A/B timing only) skips the
    entry points that build lacks; calling one then raises AttributeError.
    The in-tree library must export all of them (tests/test_abi.py)."""
    for name, (res, args) in table.items():
        if not required and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def scene_lib():
    """libptscene.so (host only)."""
    global _scene_lib
    if _scene_lib is None:
        if not SCENE_LIB_PATH.exists():
            raise NativeLibraryMissing(f"{SCENE_LIB_PATH} not built (run __graft_entry__.build())")
        lib = C.CDLL(str(SCENE_LIB_PATH))
        _scene_lib = _bind(lib, SCENE_API)
        table = os.environ.get("PT_SPECTRUM_TABLE")
        if table and Path(table).exists():
            _scene_lib.ptsLoadSpectrumTable(table.encode())
    return _scene_lib


def hip_lib():
    """libpathtracer.so (HIP kernels for gfx950).  Raises if absent."""
    global _hip_lib
    if _hip_lib is None:
        # PT_HIP_LIB: an alternative build of the same library (compiler-flag
        # experiments, tools/build_variant.py); the default is the in-tree one.
        path = Path(os.environ.get("PT_HIP_LIB", str(HIP_LIB_PATH)))
        if not path.exists():
            raise NativeLibraryMissing(f"{path} not built (run __graft_entry__.build())")
        lib = C.CDLL(str(path))
        _hip_lib = _bind(lib, HIP_API, required="PT_HIP_LIB" not in os.environ)
    return _hip_lib


def fptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_fptr)


def u32ptr(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags.c_contiguous
    return a.ctypes.data_as(_u32ptr)
