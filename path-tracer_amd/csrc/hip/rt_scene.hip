// rt_scene.hip — host side of libpathtracer.so: pack validation and scene upload.
// Scene packs are validated on the host before upload so that no index in them
// can send a kernel out of bounds or into a cycle.
#include "runtime.hpp"

#include <cmath>

using namespace ptrt;

namespace {

// --- pack validation --------------------------------------------------------------

bool TexOk(uint32_t t, uint32_t n) { return t == PT_TEXTURE_INDEX_NONE || t < n; }

// Depth (edges on the longest root-leaf path) of the TLAS, or -1 if malformed.
int TlasDepth(const pt_scene_packs* p)
{
    uint32_t n = p->shape_node_count;
    struct item { uint32_t node, depth; };
    std::vector<item> st{{0, 0}};
    int maxd = 0;
    size_t visits = 0;
    while (!st.empty()) {
        item it = st.back(); st.pop_back();
        if (++visits > (size_t)n) return -1;   // cycle or shared children
        const pt_packed_shape_node& N = p->shape_nodes[it.node];
        maxd = std::max<int>(maxd, (int)it.depth);
        if (N.ChildNodeIndices == 0) {
            if (N.ShapeIndex >= p->shape_count) return -1;
        } else {
            uint32_t a = N.ChildNodeIndices & 0xFFFF, b = N.ChildNodeIndices >> 16;
            if (a >= n || b >= n) return -1;
            st.push_back({a, it.depth + 1});
            st.push_back({b, it.depth + 1});
        }
    }
    return maxd;
}

int BlasDepth(const pt_scene_packs* p, uint32_t root)
{
    uint32_t n = p->mesh_node_count;
    if (root >= n) return -1;
    struct item { uint32_t node, depth; };
    std::vector<item> st{{root, 0}};
    int maxd = 0;
    size_t visits = 0;
    while (!st.empty()) {
        item it = st.back(); st.pop_back();
        if (++visits > (size_t)n) return -1;
        const pt_packed_mesh_node& N = p->mesh_nodes[it.node];
        maxd = std::max<int>(maxd, (int)it.depth);
        if (N.FaceEndIndex > 0) {
            if (N.FaceBeginOrNodeIndex > N.FaceEndIndex || N.FaceEndIndex > p->mesh_face_count) return -1;
        } else {
            uint32_t c = N.FaceBeginOrNodeIndex;
            if (c + 1 >= n || c + 1 < c) return -1;
            st.push_back({c, it.depth + 1});
            st.push_back({c + 1, it.depth + 1});
        }
    }
    return maxd;
}

bool MaterialOk(const pt_scene_packs* p, uint32_t m)
{
    if ((uint64_t)m * 32 + 32 > p->material_word_count) return false;
    const uint32_t* A = p->material_data + 32 * m;
    uint32_t nt = p->texture_count;
    switch (A[0]) {
        case PT_MATERIAL_TYPE_BASIC_DIFFUSE: return TexOk(A[PT_BASIC_DIFFUSE_BASE_SPECTRUM + 3], nt);
        case PT_MATERIAL_TYPE_BASIC_METAL:
            return TexOk(A[PT_BASIC_METAL_BASE_SPECTRUM + 3], nt) && TexOk(A[PT_BASIC_METAL_SPECULAR_SPECTRUM + 3], nt) &&
                   TexOk(A[PT_BASIC_METAL_ROUGHNESS + 1], nt) && TexOk(A[PT_BASIC_METAL_ROUGHNESS_ANISOTROPY + 1], nt);
        case PT_MATERIAL_TYPE_BASIC_TRANSLUCENT:
            return TexOk(A[PT_BASIC_TRANSLUCENT_ROUGHNESS + 1], nt) && TexOk(A[PT_BASIC_TRANSLUCENT_ROUGHNESS_ANISOTROPY + 1], nt);
        default: return true;   // not shaded by the integrator
    }
}

int ValidatePacks(const pt_scene_packs* p, uint32_t* stack_needed)
{
    if (!p || !p->globals) { SetError("packs: globals missing"); return -1; }
    const pt_packed_scene_globals& g = *p->globals;
    if (g.ShapeCount != 0) {
        if (g.ShapeCount != p->shape_count) { SetError("packs: ShapeCount %u != shape_count %u", g.ShapeCount, p->shape_count); return -1; }
        if (p->shape_node_count == 0) { SetError("packs: no shape nodes"); return -1; }
    }
    if (p->shape_count > 65535 || p->shape_node_count > 65536) { SetError("packs: more than 65535 shapes (16-bit indices)"); return -1; }
    if (!TexOk(g.SkyboxTextureIndex, p->texture_count)) { SetError("packs: bad skybox texture"); return -1; }
    if (p->texture_count > 0 && (!p->atlas || p->atlas_layer_count == 0 || p->atlas_width == 0 || p->atlas_height == 0)) {
        SetError("packs: textures without atlas"); return -1;
    }
    for (uint32_t i = 0; i < p->mesh_face_count; i++) {
        const pt_packed_mesh_face& F = p->mesh_faces[i];
        if (F.VertexIndex0 >= p->mesh_vertex_count || F.VertexIndex1 >= p->mesh_vertex_count ||
            F.VertexIndex2 >= p->mesh_vertex_count) { SetError("packs: face %u vertex out of range", i); return -1; }
    }
    int blas = 0;
    for (uint32_t i = 0; i < p->shape_count; i++) {
        const pt_packed_shape& S = p->shapes[i];
        if (S.Type < 0 || S.Type > 3) { SetError("packs: shape %u bad type", i); return -1; }
        if (!MaterialOk(p, S.MaterialIndex)) { SetError("packs: shape %u bad material %u", i, S.MaterialIndex); return -1; }
        if (S.Type == PT_SHAPE_TYPE_MESH_INSTANCE) {
            int d = BlasDepth(p, S.MeshRootNodeIndex);
            if (d < 0) { SetError("packs: shape %u mesh BVH malformed", i); return -1; }
            blas = std::max(blas, d);
        }
    }
    int tlas = 0;
    if (g.ShapeCount != 0) {
        tlas = TlasDepth(p);
        if (tlas < 0) { SetError("packs: shape BVH malformed"); return -1; }
    }
    *stack_needed = (uint32_t)(std::min(tlas, 32) + std::min(blas, 32));
    return 0;
}

}  // namespace

// A scene whose Trace() is one mesh traversal (dscene::single_mesh): one
// shape, the TLAS root a leaf that names it, and that shape a mesh instance.
static bool OneMeshScene(const pt_scene_packs* p)
{
    return p->globals->ShapeCount == 1 && p->shape_count == 1 && p->shape_node_count >= 1 &&
           p->shape_nodes[0].ChildNodeIndices == 0 && p->shape_nodes[0].ShapeIndex == 0 &&
           p->shapes[0].Type == PT_SHAPE_TYPE_MESH_INSTANCE;
}

// Box-coordinate condition of the extend kernel's exact fast slab division
// (pt_device.hpp, IntersectBoundingBox): every TLAS / BLAS bound is 0 or has
// magnitude in [2^-50, 2^40].  Scenes outside it trace with IEEE division.
static bool FastDivBoxes(const pt_scene_packs* p)
{
    auto ok = [](float c) {
        float m = std::fabs(c);
        return m == 0.0f || (m >= 0x1p-50f && m <= 0x1p40f);
    };
    for (uint32_t i = 0; i < p->shape_node_count; i++)
        for (int k = 0; k < 3; k++)
            if (!ok(p->shape_nodes[i].Minimum[k]) || !ok(p->shape_nodes[i].Maximum[k])) return false;
    for (uint32_t i = 0; i < p->mesh_node_count; i++)
        for (int k = 0; k < 3; k++)
            if (!ok(p->mesh_nodes[i].Minimum[k]) || !ok(p->mesh_nodes[i].Maximum[k])) return false;
    return true;
}

// Whether every BLAS node's index words fit one packed stack entry
// (PackBlasEntry): leaves with <= 31 faces starting below 2^26, child-pair
// indices below 2^31.
static bool BlasWordsPackable(const pt_scene_packs* p)
{
    for (uint32_t i = 0; i < p->mesh_node_count; i++) {
        const pt_packed_mesh_node& n = p->mesh_nodes[i];
        if (n.FaceEndIndex > 0) {
            if (n.FaceBeginOrNodeIndex >= (1u << 26) || n.FaceEndIndex < n.FaceBeginOrNodeIndex ||
                n.FaceEndIndex - n.FaceBeginOrNodeIndex > 31)
                return false;
        } else if (n.FaceBeginOrNodeIndex >= 0x80000000u) {
            return false;
        }
    }
    return true;
}

// The 16-bit stack format (PackBlasEntry16): returns the bits F of a leaf's
// first face index, or 0 if some entry does not fit.  Internal entries are
// child-pair indices < 2^15; a leaf needs first < 2^F and count < 2^(15-F)
// for one F; TLAS entries are node indices < 2^16 (ValidatePacks).
static uint32_t BlasWords16FirstBits(const pt_scene_packs* p)
{
    if (p->shape_node_count > 65536) return 0;
    uint32_t max_first = 0, max_count = 0;
    for (uint32_t i = 0; i < p->mesh_node_count; i++) {
        const pt_packed_mesh_node& n = p->mesh_nodes[i];
        if (n.FaceEndIndex > 0) {
            if (n.FaceEndIndex < n.FaceBeginOrNodeIndex) return 0;
            max_first = std::max(max_first, n.FaceBeginOrNodeIndex);
            max_count = std::max(max_count, n.FaceEndIndex - n.FaceBeginOrNodeIndex);
        } else if (n.FaceBeginOrNodeIndex >= 0x8000u) {
            return 0;
        }
    }
    for (uint32_t F = 1; F < 15; F++)
        if (max_first < (1u << F) && max_count < (1u << (15 - F))) return F;
    return 0;
}

// Whether shading a hit on material m reads the hit's texture coordinates:
// some texture index among the fields its BSDF reads (MaterialOk's list, and
// OpenPBR's base colour and specular roughness textures) is set.  Hits on
// other materials skip computing their UV (HitAttributesV).
static bool MaterialReadsUV(const pt_scene_packs* p, uint32_t m)
{
    const uint32_t* A = p->material_data + 32 * (size_t)m;
    auto tx = [&](uint32_t w) { return A[w] != PT_TEXTURE_INDEX_NONE; };
    switch (A[0]) {
        case PT_MATERIAL_TYPE_BASIC_DIFFUSE: return tx(PT_BASIC_DIFFUSE_BASE_SPECTRUM + 3);
        case PT_MATERIAL_TYPE_BASIC_METAL:
            return tx(PT_BASIC_METAL_BASE_SPECTRUM + 3) || tx(PT_BASIC_METAL_SPECULAR_SPECTRUM + 3) ||
                   tx(PT_BASIC_METAL_ROUGHNESS + 1) || tx(PT_BASIC_METAL_ROUGHNESS_ANISOTROPY + 1);
        case PT_MATERIAL_TYPE_BASIC_TRANSLUCENT:
            return tx(PT_BASIC_TRANSLUCENT_ROUGHNESS + 1) || tx(PT_BASIC_TRANSLUCENT_ROUGHNESS_ANISOTROPY + 1);
        case PT_MATERIAL_TYPE_OPENPBR:
            return tx(PT_OPENPBR_BASE_SPECTRUM_TEXTURE_INDEX) || tx(PT_OPENPBR_SPECULAR_ROUGHNESS_TEXTURE_INDEX);
        default: return false;   // not shaded: the path ends
    }
}

// LDS node cache layout (the extend kernel's NodeCacheFill, pt_device.hpp
// PT_NODE_CACHE_PAIRS): the BLAS child pairs in breadth-first order from every
// mesh root -- the top levels, which most node fetches of a frame read (C3:
// the first 6 levels, 120 pairs, take 59 % of the internal-node visits) --
// the first PT_NODE_CACHE_PAIRS of them moved to the front of the device node
// array (pair j at nodes 2j, 2j+1), every other node after them in its
// original order, child-pair and root indices remapped.  The numbering enters
// no result: the traversal's decisions read only the nodes' bounds and face
// ranges, so a renumbered BVH is traversed in the same order to the same
// hits.  Returns the cached pair count, 0 (and the identity layout) when some
// node is the first child of one pair and the second of another, which no
// layout of adjacent pairs can hold.
static uint32_t NodeCacheLayout(const pt_scene_packs* p, std::vector<pt_packed_mesh_node>& out,
                                std::vector<uint32_t>& remap)
{
    const uint32_t n = p->mesh_node_count;
    const pt_packed_mesh_node* in = p->mesh_nodes;
    out.assign(in, in + n);
    remap.resize(n);
    for (uint32_t i = 0; i < n; i++) remap[i] = i;
    if (n < 3) return 0;
    std::vector<uint8_t> role(n, 0);   // 1: first node of a child pair, 2: second
    for (uint32_t i = 0; i < n; i++) {
        if (in[i].FaceEndIndex > 0) continue;
        const uint32_t c = in[i].FaceBeginOrNodeIndex;
        if (c + 1 >= n) return 0;
        role[c] |= 1;
        role[c + 1] |= 2;
    }
    for (uint32_t i = 0; i < n; i++)
        if (role[i] == 3) return 0;
    std::vector<uint32_t> cached, queue;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t k = 0; k < p->shape_count; k++) {
        if (p->shapes[k].Type != PT_SHAPE_TYPE_MESH_INSTANCE) continue;
        const uint32_t r = p->shapes[k].MeshRootNodeIndex;
        if (r < n && in[r].FaceEndIndex == 0) queue.push_back(in[r].FaceBeginOrNodeIndex);
    }
    for (size_t h = 0; h < queue.size() && cached.size() < PT_NODE_CACHE_PAIRS; h++) {
        const uint32_t c = queue[h];
        if (seen[c]) continue;
        seen[c] = 1;
        cached.push_back(c);
        for (uint32_t m = c; m <= c + 1; m++)
            if (in[m].FaceEndIndex == 0) queue.push_back(in[m].FaceBeginOrNodeIndex);
    }
    if (cached.empty()) return 0;
    std::vector<uint8_t> moved(n, 0);
    for (uint32_t j = 0; j < cached.size(); j++) {
        remap[cached[j]] = 2 * j;
        remap[cached[j] + 1] = 2 * j + 1;
        moved[cached[j]] = moved[cached[j] + 1] = 1;
    }
    uint32_t next = 2 * (uint32_t)cached.size();
    for (uint32_t i = 0; i < n; i++)
        if (!moved[i]) remap[i] = next++;
    for (uint32_t i = 0; i < n; i++) {
        pt_packed_mesh_node N = in[i];
        if (N.FaceEndIndex == 0) N.FaceBeginOrNodeIndex = remap[N.FaceBeginOrNodeIndex];
        out[remap[i]] = N;
    }
    return (uint32_t)cached.size();
}

// Material types reachable by a hit (every shape's material), whether any
// medium can scatter, whether any shape is not a mesh instance and whether sky
// light sampling is on: selects the shade kernel instantiation (shade.hip
// pt_shade_mats).
static uint32_t SceneMaterialMask(const pt_scene_packs* p)
{
    uint32_t m = 0;
    for (uint32_t i = 0; i < p->shape_count; i++) {
        uint32_t type = p->material_data[32 * p->shapes[i].MaterialIndex];
        if (type == PT_MATERIAL_TYPE_BASIC_DIFFUSE) m |= PT_MATS_DIFFUSE;
        else if (type == PT_MATERIAL_TYPE_BASIC_METAL) m |= PT_MATS_METAL;
        else if (type == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT) m |= PT_MATS_TRANSLUCENT;
        else if (type == PT_MATERIAL_TYPE_OPENPBR) m |= PT_MATS_OPENPBR;
    }
    if ((m & PT_MATS_TRANSLUCENT) || p->globals->SceneScatterRate > 0.0f) m |= PT_MATS_SCATTER;
    for (uint32_t i = 0; i < p->shape_count; i++)
        if (p->shapes[i].Type != PT_SHAPE_TYPE_MESH_INSTANCE) m |= PT_MATS_PRIMS;
    // PT_MATS_SKY clear: the light is never chosen and its pdf term is an
    // exact +0, so the shade kernel drops the sky lobe and the sky pdf
    // (SampleSurfaceIntegrand).  That needs SkyboxSamplingProbability == +0
    // (bit pattern 0: LP * pdf is then +0) and a finite pdf for every
    // direction: the constant 1/(4 pi) below PT_EPSILON, else a finite norm,
    // Kappa <= 1000 and |SkyboxMeanDirection|^2 <= 1.01 (so Kappa (Mu.In - 1)
    // stays far below exp's overflow).
    {
        const pt_packed_scene_globals& G = *p->globals;
        const float K = G.SkyboxConcentration;
        const float* D = G.SkyboxMeanDirection;
        const float norm = ptd::VmfConstants(K).norm;
        const bool pdf_finite = (K < PT_EPSILON) || (std::isfinite(norm) && K <= 1000.0f &&
                                                     D[0] * D[0] + D[1] * D[1] + D[2] * D[2] <= 1.01f);
        uint32_t ssp;
        std::memcpy(&ssp, &G.SkyboxSamplingProbability, 4);
        if (ssp != 0u || !pdf_finite) m |= PT_MATS_SKY;
    }
    // The lean instantiation's two-select texel wrap is exact when every
    // atlas placement lies in [0, 1] (the atlas packer's always do).
    for (uint32_t i = 0; i < p->texture_count; i++)
        for (int k = 0; k < 2; k++) {
            const float a = p->textures[i].AtlasPlacementMinimum[k], b = p->textures[i].AtlasPlacementMaximum[k];
            if (!((a >= 0.0f) & (a <= 1.0f) & (b >= 0.0f) & (b <= 1.0f))) m |= PT_MATS_TEXWRAP;
        }
    return m;
}

extern "C" {

pt_scene* ptCreateScene(pt_device* d)
{
    if (!d) { SetError("null device"); return nullptr; }
    pt_scene* s = new pt_scene;
    s->dev = d;
    return s;
}

void ptDestroyScene(pt_device* d, pt_scene* s)
{
    if (!s) return;
    if (d) (void)hipSetDevice(d->id);
    delete s;
}

int ptSetSceneStackFormat(pt_scene* s, uint32_t format)
{
    if (!s || format > PT_STACK_FORMAT_NODE_INDEX) { SetError("ptSetSceneStackFormat: bad argument"); return -1; }
    s->stack_format = format;
    return 0;
}

int ptSetSceneHitRecordForm(pt_scene* s, uint32_t form)
{
    if (!s || form > PT_HIT_RECORD_FACE_INDEX) { SetError("ptSetSceneHitRecordForm: bad argument"); return -1; }
    s->hit_record = form;
    return 0;
}

int ptSetSceneExtendForm(pt_scene* s, uint32_t form)
{
    if (!s || form > PT_EXTEND_FORM_GENERAL) { SetError("ptSetSceneExtendForm: bad argument"); return -1; }
    s->extend_form = form;
    return 0;
}

int ptGetSceneExtendForm(pt_scene* s, uint32_t* form)
{
    if (!s || !form) { SetError("null argument"); return -1; }
    *form = (s->valid && s->d.single_mesh) ? PT_EXTEND_FORM_MESH : PT_EXTEND_FORM_GENERAL;
    return 0;
}

// UpdateVulkanScene (scene.cpp:1692-2006): synchronous upload of the packs.
int ptUpdateScene(pt_device* d, pt_scene* s, const pt_scene_packs* p, uint32_t dirty)
{
    if (!d || !s) { SetError("null device/scene"); return -1; }
    uint32_t need = 0;
    if (ValidatePacks(p, &need) != 0) { s->valid = false; return -1; }
    PT_HIP(hipSetDevice(d->id));
    PT_WAIT(d);   // like vkDeviceWaitIdle (scene.cpp:1704)
    bool first = !s->valid;
    if (first || (dirty & PT_SCENE_DIRTY_TEXTURES)) {
        PT_HIP(s->textures.upload(p->textures, p->texture_count));
        s->texture_count = p->texture_count;
        size_t atlas_floats = (size_t)p->atlas_width * p->atlas_height * 4 * p->atlas_layer_count;
        s->atlas_tiled = p->atlas && p->atlas_width % 4 == 0 && p->atlas_height % 2 == 0;
        if (s->atlas_tiled) {
            // Upload row-major, then re-lay the texels in 4x2 blocks
            // (AtlasIndex, pt_device.hpp) on the device.
            dbuf<float> stage;
            PT_HIP(stage.upload(p->atlas, atlas_floats));
            PT_HIP(s->atlas.alloc(atlas_floats));
            PT_HIP(pt_launch_atlas_tile(reinterpret_cast<const float4*>(stage.ptr), reinterpret_cast<float4*>(s->atlas.ptr),
                                        p->atlas_width, p->atlas_height, p->atlas_layer_count, d->stream));
            PT_WAIT(d);
        } else {
            PT_HIP(s->atlas.upload(p->atlas, p->atlas ? atlas_floats : 0));
        }
    }
    if (first || (dirty & PT_SCENE_DIRTY_MATERIALS)) PT_HIP(s->material.upload(p->material_data, p->material_word_count));
    if (first || (dirty & PT_SCENE_DIRTY_SHAPES)) PT_HIP(s->shape_nodes.upload(p->shape_nodes, p->shape_node_count));
    // The device BLAS node array in the LDS node cache's layout (the shapes'
    // root indices follow it).
    const bool relayout = first || (dirty & (PT_SCENE_DIRTY_SHAPES | PT_SCENE_DIRTY_MATERIALS | PT_SCENE_DIRTY_MESHES));
    std::vector<pt_packed_mesh_node> nodes;
    std::vector<uint32_t> remap;
    if (relayout) s->cached_pairs = NodeCacheLayout(p, nodes, remap);
    if (relayout) {
        // The device's shape records carry, in their unused Pad0 word, whether
        // the shape's material reads texture coordinates (HitAttributesV).
        std::vector<pt_packed_shape> sh(p->shapes, p->shapes + p->shape_count);
        for (pt_packed_shape& S : sh) {
            S.Pad0 = MaterialReadsUV(p, S.MaterialIndex) ? ptd::PT_SHAPE_FLAG_UV : 0u;
            if (S.Type == PT_SHAPE_TYPE_MESH_INSTANCE) S.MeshRootNodeIndex = remap[S.MeshRootNodeIndex];
        }
        PT_HIP(s->shapes.upload(sh.data(), sh.size()));
        PT_HIP(s->mesh_nodes.upload(nodes.data(), nodes.size()));
        // One-mesh scenes: what the mesh-only extend loop's prologue reads of
        // the shape and of the mesh root (device node layout) rides in the
        // kernel arguments.  A property of the uploaded scene, so it follows
        // every upload that touches shapes or meshes.
        s->one_mesh = OneMeshScene(p) && sh[0].MeshRootNodeIndex < nodes.size();
        if (s->one_mesh) {
            const pt_packed_mesh_node& root = nodes[sh[0].MeshRootNodeIndex];
            s->d.mesh_root[0] = root.FaceBeginOrNodeIndex;
            s->d.mesh_root[1] = root.FaceEndIndex;
            std::memcpy(s->d.mesh_from, sh[0].Transform.From, sizeof s->d.mesh_from);
        }
    }
    if (first || (dirty & PT_SCENE_DIRTY_MESHES)) {
        // Device face records carry {Position0, Edge1, Edge2} (traverse.hpp
        // LaneMeshFace): the reference's per-test edge subtractions
        // (scene.glsl.inc:307-308) done once here, same IEEE f32 operations.
        std::vector<pt_packed_mesh_face> ef(p->mesh_faces, p->mesh_faces + p->mesh_face_count);
        for (pt_packed_mesh_face& F : ef)
            for (int k = 0; k < 3; k++) {
                float p0 = F.Position0[k];
                F.Position1[k] = F.Position1[k] - p0;
                F.Position2[k] = F.Position2[k] - p0;
            }
        PT_HIP(s->faces.upload(ef.data(), ef.size()));
        PT_HIP(s->vertices.upload(p->mesh_vertices, p->mesh_vertex_count));
        PT_HIP(s->vertex_attr.alloc(std::max<size_t>(p->mesh_vertex_count, 1)));
        PT_HIP(s->vertex_v.alloc(std::max<size_t>(p->mesh_vertex_count, 1)));
        PT_HIP(pt_launch_vertex_decode(reinterpret_cast<const uint2*>(s->vertices.ptr), p->mesh_vertex_count,
                                       s->vertex_attr.ptr, s->vertex_v.ptr, d->stream));
    }
    if (first || (dirty & PT_SCENE_DIRTY_CAMERAS)) PT_HIP(s->cameras.upload(p->cameras, p->camera_count));
    // The traversal-length table describes the geometry: a change of shapes or
    // meshes clears it and re-lays the key grid over the new world bounds (the
    // TLAS root's box; an axis without a finite extent gets one cell).
    if (first || (dirty & (PT_SCENE_DIRTY_SHAPES | PT_SCENE_DIRTY_MESHES))) {
        float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        if (p->shape_node_count && p->shape_nodes)
            for (int k = 0; k < 3; k++) { lo[k] = p->shape_nodes[0].Minimum[k]; hi[k] = p->shape_nodes[0].Maximum[k]; }
        s->len_bounds = pt_raykey_make_bounds(lo, hi);
        PT_HIP(s->len_sum.alloc(PT_RAYKEY_COUNT));
        PT_HIP(s->len_cnt.alloc(PT_RAYKEY_COUNT));
        PT_HIP(s->len_cls.alloc(PT_RAYKEY_COUNT));
        PT_HIP(hipMemsetAsync(s->len_sum.ptr, 0, PT_RAYKEY_COUNT * sizeof(uint32_t), d->stream));
        PT_HIP(hipMemsetAsync(s->len_cnt.ptr, 0, PT_RAYKEY_COUNT * sizeof(uint32_t), d->stream));
        PT_HIP(hipMemsetAsync(s->len_cls.ptr, PT_RAYKEY_CLASSES / 2, PT_RAYKEY_COUNT, d->stream));
        s->len_trained = false;
        s->len_pending = false;
        s->len_rounds = 0;
    }

    ptd::dscene& D = s->d;
    D.g = *p->globals;
    {
        ptd::vmf_consts K = ptd::VmfConstants(D.g.SkyboxConcentration);
        D.vmf_inv_kappa = K.inv_kappa;
        D.vmf_exp_m2k = K.exp_m2k;
        D.vmf_norm = K.norm;
        D.sky_flat = ptd::SkyFlat();
    }
    D.textures = s->textures.ptr;
    D.material = s->material.ptr;
    D.shapes = s->shapes.ptr;
    D.shape_nodes = reinterpret_cast<const float4*>(s->shape_nodes.ptr);
    D.mesh_faces = reinterpret_cast<const float4*>(s->faces.ptr);
    D.mesh_vertices = reinterpret_cast<const uint2*>(s->vertices.ptr);
    D.vertex_attr = s->vertex_attr.ptr;
    D.vertex_v = s->vertex_v.ptr;
    D.mesh_nodes = reinterpret_cast<const float4*>(s->mesh_nodes.ptr);
    D.cameras = s->cameras.ptr;
    D.atlas = reinterpret_cast<const float4*>(s->atlas.ptr);
    D.atlas_w = p->atlas_width;
    D.atlas_h = p->atlas_height;
    D.atlas_layers = p->atlas ? p->atlas_layer_count : 0;
    D.atlas_tiled = s->atlas_tiled ? 1u : 0u;
    D.fast_div = FastDivBoxes(p) ? 1u : 0u;
    s->mats = SceneMaterialMask(p);
    uint32_t types = s->mats & (PT_MATS_DIFFUSE | PT_MATS_METAL | PT_MATS_TRANSLUCENT | PT_MATS_OPENPBR);
    D.mat_classes = (types & (types - 1)) != 0 ? 1u : 0u;   // more than one material type
    // Hit records carry a mesh face's vertex indices when every index fits
    // 21 bits (PackVertexIndices, traverse.hpp); ptSetSceneHitRecordForm can
    // force the face-index form that larger scenes use.
    D.vidx21 = (p->mesh_vertex_count <= (1u << 21) && s->hit_record != PT_HIT_RECORD_FACE_INDEX) ? 1u : 0u;
    // Traversal stack entries: 16-bit when every entry fits, else packed
    // 32-bit BLAS words, else node indices (ptSetSceneStackFormat can force
    // the wider forms, which larger scenes need).
    // (On the device node layout: its child-pair indices are what the
    // stack entries hold.)
    pt_scene_packs pd = *p;
    if (relayout) pd.mesh_nodes = nodes.data();
    D.blas_words = (s->stack_format != PT_STACK_FORMAT_NODE_INDEX && (relayout ? BlasWordsPackable(&pd) : s->blas_packable)) ? 1u : 0u;
    D.blas_firstbits = 0;
    D.stack16 = 0;
    uint32_t F16 = s->stack_format == PT_STACK_FORMAT_AUTO ? (relayout ? BlasWords16FirstBits(&pd) : s->blas16_bits) : 0u;
    if (relayout) {
        s->blas_packable = BlasWordsPackable(&pd);
        s->blas16_bits = BlasWords16FirstBits(&pd);
    }
    if (uint32_t F = F16) {   // every stack entry fits 16 bits
        D.blas_words = 2;
        D.blas_firstbits = F;
        D.stack16 = 1;
    }
    // The LDS node cache rides with the u16 stack (variants.hpp HasNodeCache).
    D.node_cache = D.stack16 ? 2 * s->cached_pairs : 0u;
    // Extend's form: the mesh-only loop for a one-mesh scene, unless
    // ptSetSceneExtendForm asks for the general one (identical results).
    D.single_mesh = (s->one_mesh && s->extend_form == PT_EXTEND_FORM_AUTO) ? 1u : 0u;
    s->camera_count = p->camera_count;
    s->stack_needed = need;
    s->valid = true;
    return 0;
}

int ptSceneStackNeeded(pt_scene* s, uint32_t* entries)
{
    if (!s || !entries) { SetError("null argument"); return -1; }
    *entries = s->stack_needed;
    return 0;
}

int ptSceneFastDivision(pt_scene* s, uint32_t* enabled)
{
    if (!s || !enabled) { SetError("null argument"); return -1; }
    *enabled = s->valid ? s->d.fast_div : 0u;
    return 0;
}

int ptSceneNodeCache(pt_scene* s, uint32_t* pairs)
{
    if (!s || !pairs) { SetError("null argument"); return -1; }
    *pairs = s->valid ? s->d.node_cache / 2 : 0u;
    return 0;
}

int ptReadSceneLengthTable(pt_device* d, pt_scene* s, uint8_t* classes, uint32_t* trained, uint64_t* rounds)
{
    if (!d || !s) { SetError("ptReadSceneLengthTable: null argument"); return -1; }
    if (!s->valid) { SetError("scene has no valid packs (call ptUpdateScene)"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    PT_WAIT(d);
    if (classes) PT_HIP(hipMemcpy(classes, s->len_cls.ptr, PT_RAYKEY_COUNT, hipMemcpyDeviceToHost));
    if (trained) *trained = s->len_trained ? 1u : 0u;
    if (rounds) *rounds = s->len_rounds;
    return 0;
}

}  // extern "C"
