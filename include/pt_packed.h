/*
 * pt_packed.h — byte layouts of the flattened scene buffers that feed the
 * integrator.  These are exactly the std430 structs the reference packs in
 * PackSceneData (src/scene/scene.hpp:80-173, device mirror
 * src/scene/scene.glsl.inc:30-99), so a scene packed by the reference's
 * src/scene code can be handed to ptUpdateScene() unchanged.
 *
 * Matrices are column-major float[16] (glm::mat4 memory order).
 */
#ifndef PT_PACKED_H
#define PT_PACKED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SHAPE_INDEX_NONE   0xFFFFFFFFu
#define PT_TEXTURE_INDEX_NONE 0xFFFFFFFFu

enum {
    PT_SHAPE_TYPE_MESH_INSTANCE = 0,
    PT_SHAPE_TYPE_PLANE         = 1,
    PT_SHAPE_TYPE_SPHERE        = 2,
    PT_SHAPE_TYPE_CUBE          = 3,
};

enum {
    PT_TEXTURE_TYPE_RAW                    = 0,
    PT_TEXTURE_TYPE_REFLECTANCE_WITH_ALPHA = 1,
    PT_TEXTURE_TYPE_RADIANCE               = 2,
};

#define PT_TEXTURE_FLAG_FILTER_NEAREST 1u

enum {
    PT_MATERIAL_TYPE_BASIC_DIFFUSE     = 0,
    PT_MATERIAL_TYPE_BASIC_METAL       = 1,
    PT_MATERIAL_TYPE_BASIC_TRANSLUCENT = 2,
    PT_MATERIAL_TYPE_OPENPBR           = 3,
};

enum {
    PT_CAMERA_MODEL_PINHOLE   = 0,
    PT_CAMERA_MODEL_THIN_LENS = 1,
    PT_CAMERA_MODEL_360       = 2,
};

/* scene_dirty_flag, src/scene/scene.hpp:323-333 */
enum {
    PT_SCENE_DIRTY_GLOBALS        = 1u << 0,
    PT_SCENE_DIRTY_TEXTURES       = 1u << 1,
    PT_SCENE_DIRTY_MATERIALS      = 1u << 2,
    PT_SCENE_DIRTY_SHAPES         = 1u << 3,
    PT_SCENE_DIRTY_MESHES         = 1u << 4,
    PT_SCENE_DIRTY_CAMERAS        = 1u << 5,
    PT_SCENE_DIRTY_SKYBOX_TEXTURE = 1u << 6,
    PT_SCENE_DIRTY_ALL            = 0xFFFFFFFFu,
};

/* Material attribute slots (src/scene/basic_*.glsl.inc, first lines). */
#define PT_MATERIAL_SLOT_WORDS 32
#define PT_BASIC_DIFFUSE_BASE_SPECTRUM            1
#define PT_BASIC_METAL_BASE_SPECTRUM              1
#define PT_BASIC_METAL_SPECULAR_SPECTRUM          5
#define PT_BASIC_METAL_ROUGHNESS                  9
#define PT_BASIC_METAL_ROUGHNESS_ANISOTROPY       11
#define PT_BASIC_TRANSLUCENT_IOR                  1
#define PT_BASIC_TRANSLUCENT_ABBE_NUMBER          2
#define PT_BASIC_TRANSLUCENT_ROUGHNESS            3
#define PT_BASIC_TRANSLUCENT_ROUGHNESS_ANISOTROPY 5
#define PT_BASIC_TRANSLUCENT_TRANSMISSION_SPECTRUM 7
#define PT_BASIC_TRANSLUCENT_TRANSMISSION_DEPTH   10
#define PT_BASIC_TRANSLUCENT_SCATTERING_SPECTRUM  11
#define PT_BASIC_TRANSLUCENT_SCATTERING_ANISOTROPY 14
/* OpenPBR (src/scene/openpbr.glsl.inc:1-27): 64 words, two slots. */
#define PT_OPENPBR_LAYER_BOUNCE_LIMIT                  1
#define PT_OPENPBR_BASE_WEIGHT                         2
#define PT_OPENPBR_BASE_SPECTRUM                       3
#define PT_OPENPBR_BASE_SPECTRUM_TEXTURE_INDEX         6
#define PT_OPENPBR_BASE_METALNESS                      7
#define PT_OPENPBR_BASE_DIFFUSE_ROUGHNESS              8
#define PT_OPENPBR_SPECULAR_WEIGHT                     9
#define PT_OPENPBR_SPECULAR_SPECTRUM                   10
#define PT_OPENPBR_SPECULAR_IOR                        13
#define PT_OPENPBR_SPECULAR_ROUGHNESS                  14
#define PT_OPENPBR_SPECULAR_ROUGHNESS_TEXTURE_INDEX    15
#define PT_OPENPBR_SPECULAR_ROUGHNESS_ANISOTROPY       16
#define PT_OPENPBR_TRANSMISSION_SPECTRUM               17
#define PT_OPENPBR_TRANSMISSION_WEIGHT                 20
#define PT_OPENPBR_TRANSMISSION_SCATTER_SPECTRUM       21
#define PT_OPENPBR_TRANSMISSION_SCATTER_ANISOTROPY     24
#define PT_OPENPBR_TRANSMISSION_DEPTH                  25
#define PT_OPENPBR_TRANSMISSION_DISPERSION_ABBE_NUMBER 26
#define PT_OPENPBR_EMISSION_SPECTRUM                   27
#define PT_OPENPBR_EMISSION_SPECTRUM_TEXTURE_INDEX     30
#define PT_OPENPBR_EMISSION_LUMINANCE                  31
#define PT_OPENPBR_COAT_WEIGHT                         32
#define PT_OPENPBR_COAT_COLOR_SPECTRUM                 33
#define PT_OPENPBR_COAT_IOR                            36
#define PT_OPENPBR_COAT_ROUGHNESS                      37
#define PT_OPENPBR_COAT_ROUGHNESS_ANISOTROPY           38
#define PT_OPENPBR_COAT_DARKENING                      39

typedef struct pt_packed_transform {   /* scene.hpp:82-86 */
    float To[16];
    float From[16];
} pt_packed_transform;

typedef struct pt_packed_texture {     /* scene.hpp:90-98 */
    float AtlasPlacementMinimum[2];
    float AtlasPlacementMaximum[2];
    uint32_t AtlasImageIndex;
    uint32_t Type;
    uint32_t Flags;
    uint32_t Unused0;
} pt_packed_texture;

typedef struct pt_packed_shape {       /* scene.hpp:102-108 */
    int32_t  Type;
    uint32_t MaterialIndex;
    uint32_t MeshRootNodeIndex;
    uint32_t Pad0;
    pt_packed_transform Transform;
} pt_packed_shape;

typedef struct pt_packed_shape_node {  /* scene.hpp:112-118 */
    float    Minimum[3];
    uint32_t ChildNodeIndices;         /* A | B << 16; 0 = leaf */
    float    Maximum[3];
    uint32_t ShapeIndex;
} pt_packed_shape_node;

typedef struct pt_packed_mesh_face {   /* scene.hpp:122-130 */
    float    Position0[3];
    uint32_t VertexIndex0;
    float    Position1[3];
    uint32_t VertexIndex1;
    float    Position2[3];
    uint32_t VertexIndex2;
} pt_packed_mesh_face;

typedef struct pt_packed_mesh_vertex { /* scene.hpp:134-138 */
    uint32_t PackedNormal;             /* octahedral snorm16x2 */
    uint32_t PackedUV;                 /* half2 */
} pt_packed_mesh_vertex;

typedef struct pt_packed_mesh_node {   /* scene.hpp:142-148 */
    float    Minimum[3];
    uint32_t FaceBeginOrNodeIndex;
    float    Maximum[3];
    uint32_t FaceEndIndex;             /* > 0 = leaf */
} pt_packed_mesh_node;

typedef struct pt_packed_scene_globals { /* scene.hpp:152-162 (std140 UBO) */
    float    SkyboxMeanDirection[3];
    float    SkyboxConcentration;
    float    SkyboxSamplingProbability;
    float    SkyboxBrightness;
    uint32_t SkyboxTextureIndex;
    uint32_t ShapeCount;
    float    SceneScatterRate;
    uint32_t Pad0[3];
} pt_packed_scene_globals;

typedef struct pt_packed_camera {      /* scene.hpp:166-174 */
    uint32_t Model;
    float    FocalLength;
    float    ApertureRadius;
    float    SensorDistance;
    float    SensorSize[2];
    uint32_t Pad0[2];
    pt_packed_transform Transform;
} pt_packed_camera;

/* All flattened scene data, as plain arrays.  Replaces the 11 descriptor
 * bindings of src/scene/scene.glsl.inc:121-179.  The texture atlas is
 * atlas_layer_count layers of atlas_width x atlas_height rgba32f texels
 * (the reference's 4096x4096 sampler2DArray, scene.cpp:1122-1227). */
typedef struct pt_scene_packs {
    const pt_packed_scene_globals* globals;
    const pt_packed_texture*       textures;       uint32_t texture_count;
    const uint32_t*                material_data;  uint32_t material_word_count;
    const pt_packed_shape*         shapes;         uint32_t shape_count;
    const pt_packed_shape_node*    shape_nodes;    uint32_t shape_node_count;
    const pt_packed_mesh_face*     mesh_faces;     uint32_t mesh_face_count;
    const pt_packed_mesh_vertex*   mesh_vertices;  uint32_t mesh_vertex_count;
    const pt_packed_mesh_node*     mesh_nodes;     uint32_t mesh_node_count;
    const pt_packed_camera*        cameras;        uint32_t camera_count;
    const float*                   atlas;
    uint32_t atlas_width, atlas_height, atlas_layer_count;
} pt_scene_packs;

/* Denoiser records (no reference counterpart), shared by the
 * device filter (pt_api.h) and the host one (pt_scene.h).
 *
 * pt_denoise_guide: the primary hit of a pixel's central camera ray. */
typedef struct pt_denoise_guide {
    float    normal[3];                /* UnpackUnitVector(hit.packed_normal); 0,0,0 on a miss */
    float    time;                     /* hit.time; 0 on a miss */
    float    albedo[3];                /* linear sRGB base colour (sky colour on a miss) */
    uint32_t shape;                    /* hit.shape_material >> 16; 0xFFFFFFFF on a miss */
} pt_denoise_guide;

#define PT_DENOISE_MAX_ITERATIONS 8

typedef struct pt_denoise_parameters {
    uint32_t Iterations;               /* 0..8, default 5: steps 1, 2, 4, 8, 16 */
    float    SigmaColor;               /* > 0; halved every iteration */
    float    SigmaNormal;              /* > 0 */
    float    SigmaDepth;               /* > 0 */
    float    SigmaAlbedo;              /* > 0 */
} pt_denoise_parameters;

/* The variance-guided filter over two half renders. */
typedef struct pt_denoise_pair_parameters {
    uint32_t Iterations;               /* 0..8, default 5: steps 1, 2, 4, 8, 16 */
    float    SigmaLuminance;           /* > 0; in standard deviations of the pixel's luminance, every iteration */
    float    SigmaNormal;              /* > 0 */
    float    SigmaDepth;               /* > 0 */
    float    SigmaAlbedo;              /* > 0 */
} pt_denoise_pair_parameters;

/* Temporal reprojection (arithmetic in pt_reproject.h):
 * which taps of the previous frame still show the current pixel's surface,
 * and how much history a pixel may carry. */
typedef struct pt_reproject_parameters {
    float    NormalCosine;             /* in (-1, 1], default 0.9: smallest dot product of the two normals */
    float    DepthTolerance;           /* > 0, default 0.05: largest relative mismatch of the distance */
    float    MinWeight;                /* in (0, 1], default 0.25: smallest sum of valid bilinear weights */
    float    MaxHistory;               /* > 0, default 64 (+inf: none): cap on the carried sample count */
} pt_reproject_parameters;

/* History validation (arithmetic in pt_rectify.h): the
 * window of new samples a carried history is held against, how far from
 * their mean it may lie and what a clipped pixel keeps of its count. */
typedef struct pt_rectify_parameters {
    uint32_t Radius;                   /* 1..3, default 3: the window is (2 Radius + 1)^2 pixels */
    uint32_t MinNeighbours;            /* 1..49, default 25: fewer window members leave the history untested */
    float    Sigma;                    /* finite, >= 0, default 1: half width of the box in standard deviations */
    float    ClampedHistory;           /* > 0, default 8 (+inf: no cut): cap on a clipped pixel's sample count */
    float    NormalCosine;             /* in (-1, 1], default 0.9: smallest dot product with a member's normal */
} pt_rectify_parameters;

/* Firefly clamp (arithmetic in pt_despike.h): the window
 * of neighbours a pixel's brightest colour component is held against, which
 * of their values is the yardstick and how far above it a pixel may lie. */
typedef struct pt_despike_parameters {
    uint32_t Radius;                   /* 1..3, default 3: the window is (2 Radius + 1)^2 pixels */
    uint32_t Rank;                     /* 1..4, default 3: the yardstick is the Rank-th largest neighbour */
    uint32_t MinNeighbours;            /* Rank..(2 Radius + 1)^2 - 1, default 8: fewer members leave the pixel untested */
    float    Scale;                    /* finite, >= 0, default 1: the limit is Scale * yardstick + Floor */
    float    Floor;                    /* finite, >= 0 and not -0, default 0: nothing at or below it is clamped */
    float    NormalCosine;             /* in (-1, 1], default 0.9: smallest dot product with a member's normal */
} pt_despike_parameters;

/* Ambient occlusion / sky visibility (arithmetic in
 * pt_visibility.h): how many cosine-lobe rays leave a pixel's primary hit, how
 * far an occluder may lie and which random stream draws them. */
typedef struct pt_ambient_occlusion_parameters {
    uint32_t Samples;                  /* 1..64, default 16: rays per pixel */
    float    Radius;                   /* > 0, default +inf; at or beyond PT_HIT_TIME_LIMIT (+inf): visibility of the sky */
    uint32_t Seed;                     /* default 0: the integrator's FrameIndex of the stream the rays are drawn from */
} pt_ambient_occlusion_parameters;

/* Visibility gathered at caller-given points (arithmetic
 * in pt_visibility.h): row 14's cosine lobe around each point's normal, and
 * which random stream each point draws from. */
typedef struct pt_visibility_gather_parameters {
    uint32_t Samples;                  /* 1, 2, 4, 8, 16, 32 or 64, default 16: rays per point */
    float    Radius;                   /* > 0, default +inf; at or beyond PT_HIT_TIME_LIMIT (+inf): visibility of the sky */
    uint32_t Seed;                     /* default 0: the integrator's FrameIndex of the streams the rays are drawn from */
    float    Offset;                   /* finite, >= 0, default 1e-3: a ray starts at P + Offset * W */
    uint32_t FirstIndex;               /* default 0: point i draws from stream FirstIndex + i; FirstIndex + n <= 2^32 */
} pt_visibility_gather_parameters;

/* One point's answer.  Bit k of OccludedMask: the point's ray k found
 * something within its duration (bits at and above Samples are 0).  Bent: the
 * sum of the traced velocities of the unoccluded rays, by the fixed pairwise
 * tree of pt_visibility_reduce. */
typedef struct pt_visibility_record {
    float    Bent[3];
    float    Unoccluded;               /* Samples - popcount(OccludedMask) */
    uint64_t OccludedMask;
    float    Samples;
    uint32_t Reserved;                 /* 0 */
} pt_visibility_record;

/* Sky light gathered at caller-given points (arithmetic
 * in pt_visibility.h): row 15's rays, or rays uniform over the sphere, each
 * open one weighted by the sky's radiance along it. */
#define PT_SKY_GATHER_COSINE 0u        /* row 15's cosine lobe around the point's normal */
#define PT_SKY_GATHER_SPHERE 1u        /* uniform over the sphere; the normal is not read */

typedef struct pt_sky_gather_parameters {
    uint32_t Samples;                  /* 1, 2, 4, 8, 16, 32 or 64, default 16: rays per point */
    float    Radius;                   /* > 0, default +inf; at or beyond PT_HIT_TIME_LIMIT (+inf): every occluder counts */
    uint32_t Seed;                     /* default 0: the integrator's FrameIndex of the streams the rays are drawn from */
    float    Offset;                   /* finite, >= 0, default 1e-3: a ray starts at P + Offset * W */
    uint32_t FirstIndex;               /* default 0: point i draws from stream FirstIndex + i; FirstIndex + n <= 2^32 */
    uint32_t Lobe;                     /* PT_SKY_GATHER_COSINE (default) or PT_SKY_GATHER_SPHERE */
} pt_sky_gather_parameters;

/* One point's answer.  SH[i][c]: the sum over the point's rays of (the open
 * ray's escape contribution in CIE XYZ channel c) * (real spherical harmonic i
 * of bands 0..2 along the ray, pt_sky_gather_basis), by the fixed pairwise
 * tree of pt_sky_gather_reduce.  OccludedMask, Unoccluded, Samples: as in
 * pt_visibility_record. */
typedef struct pt_sky_record {
    float    SH[9][3];
    float    Unoccluded;               /* Samples - popcount(OccludedMask) */
    uint64_t OccludedMask;             /* at byte 112 */
    float    Samples;
    uint32_t Reserved[1];              /* 0 */
} pt_sky_record;

/* One shape's motion between two packed scenes, filled
 * by ptsShapeMotion (pt_scene.h) and read by the moving-shape reprojection
 * (pt_reproject.h).  Point: rows 0..2 of the affine map from the current
 * world to the previous one (To_prev From_cur), row-major, Point[4r + c].
 * Normal: takes a current world normal into the previous world frame, before
 * normalisation (the inverse transpose of Point's linear part), Normal[3r + c]. */
#define PT_SHAPE_MOTION_MOVED      1u  /* the transform changed: Point and Normal hold the motion */
#define PT_SHAPE_MOTION_NO_HISTORY 2u  /* another or a new shape, or a non-finite transform: matrices are zero */

typedef struct pt_shape_motion {
    float    Point[12];
    float    Normal[9];
    uint32_t Flags;                    /* 0: unmoved (identity matrices, row 8's path) */
    uint32_t Pad0[2];
} pt_shape_motion;

/* Frame statistics (no reference counterpart; definition in DESIGN.md §6 row
 * 6, arithmetic in pt_stats.h): integer counts and float min/max of one
 * accumulator, or of the sum A + B of two with the noise fields taken from
 * the pair.  Computed by ptComputeFrameStatistics (pt_api.h) and
 * ptsFrameStatistics (pt_scene.h), bit for bit alike.
 * filled + empty + nonfinite = pixels; dark pixels are filled ones. */
#define PT_STATS_BINS 256

typedef struct pt_frame_statistics {
    uint64_t pixels;                   /* width * height */
    uint64_t filled;                   /* all four components finite, w > 0 */
    uint64_t empty;                    /* all finite, w <= 0 */
    uint64_t nonfinite;                /* a NaN or an infinity in any component */
    uint64_t dark;                     /* filled with Y = y / w <= 0: counted, not binned */
    uint32_t luminance_histogram[PT_STATS_BINS];   /* pt_stats_bin(Y) of filled pixels with Y > 0 */
    float    min_luminance, max_luminance;         /* over filled pixels with Y > 0; 0, 0 without any */
    float    min_samples, max_samples;             /* w over filled pixels; 0, 0 without any */
    uint64_t noise_pixels;             /* pair: filled in A and in B, Y_A + Y_B > 0, r finite */
    uint64_t noise_skipped;            /* pair: filled in A and in B, not counted above */
    uint32_t noise_histogram[PT_STATS_BINS];       /* pt_stats_bin(r), r = |Y_A - Y_B| / (Y_A + Y_B) */
} pt_frame_statistics;

/* Per-tile statistics (no reference counterpart): row
 * 6's classes and pair rule counted per 16 x 16 tile.  Tile (tx, ty) covers
 * the pixels [16 tx, 16 tx + 16) x [16 ty, 16 ty + 16) clipped to the image
 * and has index ty * ceil(width / 16) + tx, a full-frame renderer's tile
 * number.  Computed by ptComputeTileStatistics (pt_api.h) and
 * ptsTileStatistics (pt_scene.h), bit for bit alike.
 * filled + empty + nonfinite = the tile's pixels. */
#define PT_TILE_SIZE 16

typedef struct pt_tile_statistics {
    uint32_t filled, empty, nonfinite; /* pt_stats_classify of a, or of a + b (each component added in binary32) */
    uint32_t pair;                     /* filled in a and in b and pt_stats_pair_noise(Y_A, Y_B, &r) returns 1 */
    uint32_t over;                     /* of those, r > noise_threshold */
    float    min_count, max_count;     /* the classified accumulator's .w over filled pixels; 0, 0 without any */
    uint32_t reserved;                 /* 0 */
} pt_tile_statistics;

#ifdef __cplusplus
}
static_assert(sizeof(pt_frame_statistics) == 2120, "frame_statistics");
static_assert(sizeof(pt_tile_statistics) == 32, "tile_statistics");
static_assert(sizeof(pt_denoise_guide) == 32, "denoise_guide");
static_assert(sizeof(pt_denoise_parameters) == 20, "denoise_parameters");
static_assert(sizeof(pt_denoise_pair_parameters) == 20, "denoise_pair_parameters");
static_assert(sizeof(pt_reproject_parameters) == 16, "reproject_parameters");
static_assert(sizeof(pt_rectify_parameters) == 20, "rectify_parameters");
static_assert(sizeof(pt_despike_parameters) == 24, "despike_parameters");
static_assert(sizeof(pt_ambient_occlusion_parameters) == 12, "ambient_occlusion_parameters");
static_assert(sizeof(pt_visibility_gather_parameters) == 20, "visibility_gather_parameters");
static_assert(sizeof(pt_visibility_record) == 32, "visibility_record");
static_assert(sizeof(pt_sky_gather_parameters) == 24, "sky_gather_parameters");
static_assert(sizeof(pt_sky_record) == 128, "sky_record");
static_assert(sizeof(pt_shape_motion) == 96, "shape_motion");
static_assert(sizeof(pt_packed_transform) == 128, "packed_transform");
static_assert(sizeof(pt_packed_texture) == 32, "packed_texture");
static_assert(sizeof(pt_packed_shape) == 144, "packed_shape");
static_assert(sizeof(pt_packed_shape_node) == 32, "packed_shape_node");
static_assert(sizeof(pt_packed_mesh_face) == 48, "packed_mesh_face");
static_assert(sizeof(pt_packed_mesh_vertex) == 8, "packed_mesh_vertex");
static_assert(sizeof(pt_packed_mesh_node) == 32, "packed_mesh_node");
static_assert(sizeof(pt_packed_scene_globals) == 48, "packed_scene_globals");
static_assert(sizeof(pt_packed_camera) == 160, "packed_camera");
#endif

#endif /* PT_PACKED_H */
