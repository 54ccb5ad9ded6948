/*
 * pt_scene.h — C ABI of the host scene library (libptscene.so).
 *
 * Wraps the restatement of the reference's src/scene object / material /
 * camera API (src/scene/scene.hpp:410-442) and of PackSceneData
 * (src/scene/scene.cpp:1115-1621), which produce the flattened buffers the
 * integrator consumes (pt_scene_packs, include/pt_packed.h).  The entity,
 * material and camera fields keep the reference's names and meaning:
 *
 *   ptsCreateScene            scene.hpp:432  CreateScene (checker plane + camera)
 *   ptsCreateEntity           scene.hpp:413  CreateEntity(Scene, Type, Parent)
 *   ptsCreateMaterial         scene.hpp:418  CreateMaterial(Scene, Type, Name)
 *   ptsCreateCheckerTexture   scene.hpp:422  CreateCheckerTexture
 *   ptsCreateMesh             scene.cpp:790-866 (mesh + BuildMeshNode BVH)
 *   ptsPackSceneData          scene.hpp:436  PackSceneData (returns dirty flags)
 *   ptsGetParametricSpectrumCoefficients  spectrum.hpp:17
 *
 * Host only: no GPU is touched.  Material parameter names are the reference's
 * field names (basic_diffuse.hpp, basic_metal.hpp, basic_translucent.hpp).
 */
#ifndef PT_SCENE_H
#define PT_SCENE_H

#include <stdint.h>
#include "pt_packed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pts_scene pts_scene;
typedef struct pts_entity pts_entity;
typedef struct pts_material pts_material;
typedef struct pts_texture pts_texture;
typedef struct pts_mesh pts_mesh;
typedef struct pts_prefab pts_prefab;

enum {   /* entity_type, scene.hpp:228-238 */
    PTS_ENTITY_ROOT = 0,
    PTS_ENTITY_CONTAINER = 1,
    PTS_ENTITY_CAMERA = 2,
    PTS_ENTITY_MESH_INSTANCE = 3,
    PTS_ENTITY_PLANE = 4,
    PTS_ENTITY_SPHERE = 5,
    PTS_ENTITY_CUBE = 6,
};

/* Benchmark configurations (BASELINE.json "configs"). */
enum {
    PTS_CONFIG_C1_SPHERE_PLANE = 1,   /* 256x256, 16 spp */
    PTS_CONFIG_C2_CORNELL_SKY  = 2,   /* 1024x1024, 256 spp */
    PTS_CONFIG_C3_ROOM         = 3,   /* 1920x1080, 1024 spp */
    PTS_CONFIG_C4_ROOM_4K      = 4,   /* 3840x2160, 4096 spp, 8 GPUs */
    PTS_CONFIG_C5_LENS_360     = 5,   /* 2048x1024, 8192 spp */
};

typedef struct pts_config_info {
    uint32_t width, height;
    uint32_t spp;
    uint32_t camera_count;
    uint32_t render_flags;
    float    termination_probability;
    uint32_t mesh_face_count;
    uint32_t shape_count;
} pts_config_info;

/* load_model_options (scene.hpp:383-391). */
typedef struct pts_load_model_options {
    const char* name;                     /* NULL: file stem */
    const char* directory_path;           /* NULL: "." (textures and .mtl are looked up here) */
    float vertex_transform[16];           /* mat4, column-major */
    float normal_transform[16];
    float texcoord_transform[9];          /* mat3, column-major */
    int   openpbr_as_diffuse;             /* extension: BasicDiffuse instead of OpenPBR (K9) */
} pts_load_model_options;

const char* ptsGetLastError(void);

pts_scene*  ptsCreateScene(void);
pts_scene*  ptsCreateEmptyScene(void);
pts_scene*  ptsCreateConfigScene(int config, pts_config_info* info);
void        ptsDestroyScene(pts_scene* scene);

pts_entity* ptsSceneRoot(pts_scene* scene);
pts_entity* ptsCreateEntity(pts_scene* scene, int type, pts_entity* parent);
void        ptsSetEntityTransform(pts_scene* scene, pts_entity* e, const float position[3], const float rotation[3],
                                  const float scale[3]);
void        ptsSetEntityActive(pts_scene* scene, pts_entity* e, int active);
void        ptsSetEntityMaterial(pts_scene* scene, pts_entity* e, pts_material* m);
void        ptsSetEntityMesh(pts_scene* scene, pts_entity* e, pts_mesh* mesh);
uint32_t    ptsEntityPackedShapeIndex(pts_entity* e);
void        ptsSetCameraPinhole(pts_scene* scene, pts_entity* camera, float fov_degrees, float aperture_mm);
void        ptsSetCameraThinLens(pts_scene* scene, pts_entity* camera, float sensor_w_mm, float sensor_h_mm,
                                 float focal_length_mm, float aperture_mm, float focus_distance);
void        ptsSetCamera360(pts_scene* scene, pts_entity* camera);
/* The camera entity packed at `packed_index` by the last PackSceneData (NULL
 * if none), and a camera move as the editor's fly controls make it
 * (application.cpp:52-66): position / rotation (may be NULL) and only
 * SCENE_DIRTY_CAMERAS set. */
pts_entity* ptsFindCamera(pts_scene* scene, uint32_t packed_index);
void        ptsSetCameraTransform(pts_scene* scene, pts_entity* camera, const float position[3], const float rotation[3]);
/* root_entity fields (scene.hpp:254-262). */
void        ptsSetRootParameters(pts_scene* scene, float scatter_rate, float skybox_brightness,
                                 float skybox_sampling_probability, pts_texture* skybox);

pts_material* ptsCreateMaterial(pts_scene* scene, int type, const char* name);
/* name: BaseColor, SpecularColor, Roughness, RoughnessAnisotropy, IOR, AbbeNumber,
 * TransmissionColor, TransmissionDepth, ScatteringColor, ScatteringAnisotropy. */
int ptsSetMaterialParameter(pts_scene* scene, pts_material* m, const char* name, const float* values, int count);
/* name: BaseTexture, SpecularTexture, RoughnessTexture, RoughnessAnisotropyTexture. */
int ptsSetMaterialTexture(pts_scene* scene, pts_material* m, const char* name, pts_texture* t);
uint32_t ptsMaterialPackedIndex(pts_material* m);

pts_texture* ptsCreateCheckerTexture(pts_scene* scene, const char* name, int type, const float a[4], const float b[4]);
pts_texture* ptsCreateTexture(pts_scene* scene, const char* name, int type, uint32_t width, uint32_t height,
                              const float* rgba, int nearest_filtering);

/* positions/normals: 3 floats per vertex, uvs: 2 (normals/uvs may be NULL),
 * indices: 3 per face.  Builds the binned-SAH BVH (scene.cpp:435-599). */
pts_mesh* ptsCreateMesh(pts_scene* scene, const char* name, uint32_t vertex_count, const float* positions,
                        const float* normals, const float* uvs, uint32_t face_count, const uint32_t* indices);
uint32_t  ptsMeshDepth(pts_mesh* mesh);
uint32_t  ptsMeshNodeCount(pts_mesh* mesh);
/* Face vertex indices in BVH order (3 per face). */
void      ptsMeshFaces(pts_mesh* mesh, uint32_t* indices);

/* Scene ingestion: LoadTexture (scene.cpp:294-313; PNG / Radiance HDR with
 * stbi_loadf semantics), LoadModelAsPrefab (scene.cpp:601-903; Wavefront
 * OBJ + MTL), CreateEntity(Scene, Prefab, Parent) (scene.cpp:251-254). */
void        ptsDefaultLoadModelOptions(pts_load_model_options* options);
pts_texture* ptsLoadTexture(pts_scene* scene, const char* path, int type, const char* name);
/* The 8-bit RGBA samples LoadTexture linearises (JPEG / PNG / BMP / TGA;
 * stb_image's stbi_load(..., 4) semantics), for tests: returns 0 and the size
 * in *width, *height; `rgba` (may be NULL for a size query) receives
 * width*height*4 bytes. */
int ptsLoadImageRGBA8(const char* path, uint32_t* width, uint32_t* height, uint8_t* rgba);
pts_prefab* ptsLoadModelAsPrefab(pts_scene* scene, const char* path, const pts_load_model_options* options);
pts_entity* ptsInstantiatePrefab(pts_scene* scene, pts_prefab* prefab, pts_entity* parent);
uint32_t    ptsPrefabMeshCount(pts_prefab* prefab);
pts_mesh*   ptsPrefabMesh(pts_prefab* prefab, uint32_t index, pts_material** material, float position[3]);
uint32_t    ptsMeshVertexCount(pts_mesh* mesh);
uint32_t    ptsMeshFaceCount(pts_mesh* mesh);
/* vertices: 8 floats each (position, normal, uv). */
void        ptsMeshVertices(pts_mesh* mesh, float* vertices);
int         ptsMaterialType(pts_material* material);

/* Scene files: LoadScene / SaveScene (serializer.cpp:511-529): <path> is the
 * scene JSON; textures (<name>.texture), meshes (<name>.mesh) and the
 * spectrum table (spectrum.dat) sit beside it.  Load returns NULL on error. */
pts_scene*  ptsLoadScene(const char* path);
int         ptsSaveScene(pts_scene* scene, const char* path);
uint32_t    ptsSceneTextureCount(pts_scene* scene);
uint32_t    ptsSceneMaterialCount(pts_scene* scene);
uint32_t    ptsSceneMeshCount(pts_scene* scene);
uint32_t    ptsScenePrefabCount(pts_scene* scene);

uint32_t ptsPackSceneData(pts_scene* scene);
void     ptsGetScenePacks(pts_scene* scene, pt_scene_packs* out);
void     ptsMarkDirty(pts_scene* scene, uint32_t flags);

/* Spectral upsampling table (src/core/spectrum.cpp). */
int  ptsGetParametricSpectrumCoefficients(const float rgb[3], float beta[3]);
int  ptsBuildSpectrumTable(int threads);
int  ptsSaveSpectrumTable(const char* path);
int  ptsLoadSpectrumTable(const char* path);
void ptsSetSpectrumTablePath(const char* path);

/* Edge-avoiding a-trous denoiser on the host (no reference counterpart;
 * definition in DESIGN.md §6): the CPU path for saved accumulators and the
 * implementation ptDenoiseSampleBuffer (pt_api.h) is compared with, bit for
 * bit.  accum_rgba: width*height*4 floats as ptReadSampleBuffer returns them
 * (XYZ sums + sample count); guides: one record per pixel; out_rgba receives
 * the denoised mean XYZ and 1 (0, 0, 0, 0 where the count is not positive).
 * Returns non-zero, leaving out_rgba untouched, on a NULL argument, an empty
 * image, Iterations > 8 or a sigma that is not > 0.  Single-threaded. */
int  ptsDenoise(uint32_t width, uint32_t height, const float* accum_rgba, const pt_denoise_guide* guides,
                const pt_denoise_parameters* params, float* out_rgba);
/* The variance-guided filter over two half renders on the host (definition in
 * DESIGN.md §6 row 7): the CPU path and the implementation
 * ptDenoiseSampleBufferPair (pt_api.h) is compared with, bit for bit.
 * accum_a, accum_b: two independent renders of one frame (renderers whose
 * FrameIndex differ by 1 << 24), as ptReadSampleBuffer returns them; the
 * filter works on A + B, its luminance edge-stop scaled by the standard
 * deviation estimated from A - B.  out_rgba as for ptsDenoise.  Returns
 * non-zero, leaving out_rgba untouched, on a NULL argument, an empty image,
 * accum_a == accum_b, Iterations > 8 or a sigma that is not > 0.
 * Single-threaded. */
int  ptsDenoisePair(uint32_t width, uint32_t height, const float* accum_a, const float* accum_b,
                    const pt_denoise_guide* guides, const pt_denoise_pair_parameters* params, float* out_rgba);

/* Temporal reprojection on the host (no reference counterpart; definition in
 * DESIGN.md §6 row 8, arithmetic in pt_reproject.h): the CPU path and the
 * implementation ptReprojectSampleBuffer (pt_api.h) is compared with, bit for
 * bit.  prev_accum, prev_guides, prev_camera: the previous view's accumulator
 * (prev_width x prev_height), guide records and packed camera; guides,
 * camera: the current view's (width x height).  out_rgba receives
 * (mean XYZ * n, n) per current pixel, 0, 0, 0, 0 without a history.  Returns
 * non-zero, leaving out_rgba untouched, on a NULL argument, an empty image,
 * prev_accum == out_rgba, prev_guides == guides or a parameter outside its
 * range (pt_packed.h).  Single-threaded. */
int  ptsReproject(uint32_t prev_width, uint32_t prev_height, const float* prev_accum,
                  const pt_denoise_guide* prev_guides, const pt_packed_camera* prev_camera, uint32_t width,
                  uint32_t height, const pt_denoise_guide* guides, const pt_packed_camera* camera,
                  const pt_reproject_parameters* params, float* out_rgba);
/* The motion table of the moving-shape reprojection:
 * out[i], i < count, is shape i's motion between two packs of one scene,
 * prev_shapes (prev_count records) and shapes (count records), in binary32
 * without contraction, matrices column-major as everywhere.
 *   - i >= prev_count, another Type, another MeshRootNodeIndex, or a
 *     non-finite value in either Transform: Flags = PT_SHAPE_MOTION_NO_HISTORY,
 *     zero matrices;
 *   - the two 128-byte Transform records bytewise equal: Flags = 0, identity
 *     matrices (the pixel takes row 8's path and gets row 8's bits);
 *   - otherwise Flags = PT_SHAPE_MOTION_MOVED, Point = rows 0..2 of
 *     To_prev From_cur, Normal = the transpose of the linear part of
 *     To_cur From_prev (the inverse transpose of Point's linear part; no
 *     inverse is computed).
 * Shapes are matched by their index in the packed array: the caller
 * guarantees that the set of entities, and so their order, is the same in
 * both packs.  After an entity was added or removed the indices shift and
 * the table is wrong without any flag showing it; only the indices beyond
 * prev_count are NO_HISTORY.  Non-zero on a NULL array with a non-zero count. */
int  ptsShapeMotion(const pt_packed_shape* prev_shapes, uint32_t prev_count, const pt_packed_shape* shapes,
                    uint32_t count, pt_shape_motion* out);
/* ptsReproject with a motion table (ptsShapeMotion): a
 * hit pixel whose shape's record is MOVED looks for its history where that
 * surface point was, and expects the normal the shape had there; a shape
 * index >= motion_count or a NO_HISTORY record gives no history; everything
 * else is ptsReproject, bit for bit.  motion == NULL with motion_count == 0:
 * no table, ptsReproject itself.  Equals ptReprojectSampleBufferMoving
 * (pt_api.h) bit for bit.  Non-zero, leaving out_rgba untouched, on
 * ptsReproject's errors and on motion == NULL with motion_count > 0. */
int  ptsReprojectMoving(uint32_t prev_width, uint32_t prev_height, const float* prev_accum,
                        const pt_denoise_guide* prev_guides, const pt_packed_camera* prev_camera, uint32_t width,
                        uint32_t height, const pt_denoise_guide* guides, const pt_packed_camera* camera,
                        const pt_shape_motion* motion, uint32_t motion_count, const pt_reproject_parameters* params,
                        float* out_rgba);
/* History validation on the host (no reference counterpart; definition in
 * DESIGN.md §6 row 11, arithmetic in pt_rectify.h): the CPU path and the
 * implementation ptRectifyHistory (pt_api.h) is compared with, bit for bit.
 * history: an accumulator in (mean * n, n) form, e.g. ptsReproject's output;
 * current: the accumulator of the new rounds alone; guides: the current
 * view's records; all width x height.  out_rgba receives the history with
 * every pixel's mean colour pulled into mean +- Sigma deviations of the
 * current samples around it that show the same surface, and the count of a
 * pulled pixel cut to ClampedHistory; pixels that could not be tested keep
 * their bits, pixels without a usable history become 0, 0, 0, 0.  out_rgba
 * may be history.  Returns non-zero, leaving out_rgba untouched, on a NULL
 * argument, an empty image, history == current, out_rgba == current or a
 * parameter outside its range (pt_packed.h).  Single-threaded. */
int  ptsRectifyHistory(uint32_t width, uint32_t height, const float* history, const float* current,
                       const pt_denoise_guide* guides, const pt_rectify_parameters* params, float* out_rgba);
/* The firefly clamp on the host (no reference counterpart; definition in
 * DESIGN.md §6 row 12, arithmetic in pt_despike.h): the CPU path and the
 * implementation ptDespikeSampleBuffer (pt_api.h) is compared with, bit for
 * bit.  accum: an accumulator (XYZ sums + sample count); guides: the same
 * view's records; both width x height.  out_rgba receives accum with the
 * colour sums of every pixel whose value (the largest component of its mean
 * colour) exceeds Scale * (the Rank-th largest value among the window's
 * pixels of the same surface) + Floor scaled onto that limit; every other
 * pixel, and every sample count, keeps its bits.  Returns non-zero, leaving
 * out_rgba untouched, on a NULL argument, an empty image, out_rgba == accum or
 * a parameter outside its range (pt_packed.h).  Single-threaded. */
int  ptsDespike(uint32_t width, uint32_t height, const float* accum, const pt_denoise_guide* guides,
                const pt_despike_parameters* params, float* out_rgba);
/* pt_reproject.h's central camera ray of pixel (x, y) of a width x height
 * frame (the guide kernel's ray: pixel centre, lens centre, the velocity
 * after its packed round trip).  Non-zero on a NULL argument, an empty frame
 * or an unknown camera model. */
int  ptsCentralCameraRay(const pt_packed_camera* camera, uint32_t x, uint32_t y, uint32_t width, uint32_t height,
                         float origin[3], float velocity[3]);
/* pt_visibility.h's sample rays of pixel (x, y) on the host (DESIGN.md §6 row
 * 14; what ptRenderAmbientOcclusion (pt_api.h) traces, bit for bit): the
 * pixel's primary ray (origin, velocity) hit at `time` a surface whose guide
 * normal is `normal`; out_origins receives 3 * Samples floats, out_velocities
 * the Samples packed velocities, and *out_duration, if not NULL, the rays'
 * duration.  Non-zero, writing nothing, on a NULL argument (out_duration
 * excepted) or parameters outside their range (pt_packed.h). */
int  ptsAmbientOcclusionRays(const pt_ambient_occlusion_parameters* params, uint32_t x, uint32_t y,
                             const float origin[3], const float velocity[3], float time, const float normal[3],
                             float* out_origins, uint32_t* out_velocities, float* out_duration);
/* The rays of ptGatherVisibility (pt_api.h) on the host,
 * bit for bit, point-major: ray i * Samples + k is sample k of point i.
 * points, normals: 3 floats per point.  out_origins receives 3 floats per ray,
 * out_velocities the packed velocities and out_durations the durations, n *
 * Samples rays.  Non-zero, writing nothing, on a NULL argument (the arrays
 * with n > 0) or parameters outside their range (pt_packed.h; n <= 2^26). */
int  ptsGatherVisibilityRays(const pt_visibility_gather_parameters* params, uint32_t n, const float* points,
                             const float* normals, float* out_origins, uint32_t* out_velocities,
                             float* out_durations);
/* ptGatherVisibility's records from a one-bit-per-ray answer over those rays
 * (ptOccludedRays' mask layout: ray r is bit r % 64 of word r / 64), with the
 * device's summation tree.  packed: the rays' packed velocities.  Non-zero,
 * writing nothing, on samples not a power of two in 1..64, n > 2^26 or a NULL
 * array with n > 0. */
int  ptsGatherVisibilityReduce(uint32_t samples, uint32_t n, const uint32_t* packed, const uint64_t* occluded_bits,
                               pt_visibility_record* out);
/* pt_visibility_skip as a library call: `state` after `steps` steps of the
 * random stream's generator. */
uint32_t ptsVisibilitySkip(uint32_t state, uint32_t steps);
/* The rays of ptGatherSkyLight (pt_api.h) on the host, bit
 * for bit, point-major, for both lobes: as ptsGatherVisibilityRays, and
 * out_lambda0 receives each ray's normalised first wavelength L0 (the path's
 * four wavelengths are PathLambda(L0)).  normals may be NULL with Lobe SPHERE.
 * Non-zero, writing nothing, on a NULL argument (the arrays with n > 0) or
 * parameters outside their range. */
int  ptsSkyGatherRays(const pt_sky_gather_parameters* params, uint32_t n, const float* points, const float* normals,
                      float* out_origins, uint32_t* out_velocities, float* out_durations, float* out_lambda0);
/* ptGatherSkyLight's records from a one-bit-per-ray answer over those rays
 * (ptOccludedRays' mask layout) and any per-ray XYZ contributions (3 floats
 * per ray; an occluded ray's is taken as zero): the basis, the products and
 * the device's summation tree.  The sky evaluation is not part of this
 * library.  Non-zero, writing nothing, on samples not a power of two in
 * 1..64, n > 2^26 or a NULL array with n > 0. */
int  ptsSkyGatherReduce(uint32_t samples, uint32_t n, const uint32_t* packed, const uint64_t* occluded_bits,
                        const float* contributions, pt_sky_record* out);
/* pt_sky_gather_basis as a library call: 9 floats per packed unit vector, at
 * the unpacked vector. */
int  ptsSkyGatherBasis(uint32_t n, const uint32_t* packed, float* out);

/* Frame statistics on the host (no reference counterpart; definition in
 * DESIGN.md §6 row 6, arithmetic in pt_stats.h): the CPU path for saved
 * accumulators and the implementation ptComputeFrameStatistics (pt_api.h) is
 * compared with, bit for bit.  accum_a: width*height*4 floats as
 * ptReadSampleBuffer returns them.  accum_b NULL: the statistics of A, noise
 * fields 0.  accum_b given (an independent render of the same frame): the
 * luminance part describes A + B, each component added in binary32, and the
 * noise part the pixels filled in both.  Returns non-zero, leaving *out
 * untouched, on a NULL accum_a or out, an empty image or accum_b == accum_a.
 * Single-threaded. */
int  ptsFrameStatistics(uint32_t width, uint32_t height, const float* accum_a, const float* accum_b,
                        pt_frame_statistics* out);
/* Per-tile statistics on the host (pt_tile_statistics in
 * pt_packed.h): out holds ceil(width / 16) * ceil(height / 16) records, tile
 * (tx, ty) at ty * ceil(width / 16) + tx.  accum_b NULL: pair and over are 0.
 * Equals ptComputeTileStatistics (pt_api.h) bit for bit.  Returns non-zero,
 * leaving out untouched, on a NULL accum_a or out, an empty image, accum_b ==
 * accum_a, or a noise_threshold that is NaN or negative.  Single-threaded. */
int  ptsTileStatistics(uint32_t width, uint32_t height, const float* accum_a, const float* accum_b,
                       float noise_threshold, pt_tile_statistics* out);
/* pt_stats.h's bin function and double helpers as library calls (for callers
 * that cannot include the header): the bin of a value; the lower edge of bin
 * 0..256 (0 outside); the percentile bin of a 256-bin histogram (-1 when
 * empty); its log-average between two percentiles; key / log-average of the
 * luminance histogram (1 when empty); the upper edge of the noise histogram's
 * percentile bin (+infinity when empty). */
int    ptsStatsBin(float value);
double ptsStatsBinEdge(int bin);
int    ptsStatsPercentileBin(const uint32_t* histogram, double q);
double ptsStatsLogAverage(const uint32_t* histogram, double q_lo, double q_hi);
double ptsStatsAutoBrightness(const pt_frame_statistics* stats, double key, double q_lo, double q_hi);
double ptsStatsNoise(const pt_frame_statistics* stats, double q);
/* pt_raykey.h's key (0 .. 32 767) of the ray (origin, velocity) over the 8^3
 * grid of the world bounds [lo, hi]: what the device's length table is
 * indexed by (pt_api.h ptSetBasicRendererRayOrder).  0xFFFFFFFF on a NULL
 * argument. */
uint32_t ptsRayKey(const float origin[3], const float velocity[3], const float lo[3], const float hi[3]);

/* pt_facetest.h's lean face test from the determinant on, over n operand
 * sets: u, w, t = (1 / det) * num_u, num_w, num_t, with 1 / det taken as the
 * device takes it (the fast reciprocal's Newton step inside its range, the
 * IEEE quotient where pt_face_needs_division asks for it), and miss[i] the
 * folded flag pt_face_miss against time[i]; divides[i] is what
 * pt_face_needs_division answered for det[i].  0, or -1 on a NULL argument. */
int ptsFaceTest(uint32_t n, const float* det, const float* num_u, const float* num_w, const float* num_t,
                const float* time, uint32_t* miss, float* u, float* w, float* t, uint32_t* divides);

#ifdef __cplusplus
}
#endif

#endif /* PT_SCENE_H */
