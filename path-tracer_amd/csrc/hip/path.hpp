// path.hpp — what every kernel of the wavefront integrator shares: the slot /
// pixel mapping, the path state, the ray order of a tile (TileOrder),
// GenerateNewPath and Scatter.  Used by extend.hpp and shade.hpp.
//
// Slot state is SoA-of-float4 indexed by slot (16-byte coalesced accesses):
//   ray  = {origin.xyz, packed velocity}, hit = {time, shape|mat, n, t},
//   uv, throughput, probability, {sample.xyz, lambda0}, active-shape stack.
// Slot s covers pixel (tx*16 + s%16, band*16 + (s%256)/16) of the tile
// t = s/256, so a renderer can own an arbitrary set of 16-row bands.
//
// Ray order (TileOrder): the path arrays (thr, prob, lam, act) are indexed by
// slot, the ray and hit arrays by POSITION within the same tile.  Whenever a
// block of 256 slots (one tile) emits its rays, it sorts them by direction
// octant with a block counting sort and stores slot s's ray at position
// pos(s); extend runs one thread per position, so a wave traces rays of one
// octant from one 16x16 pixel tile (0.91x extend time on C3 vs pixel order,
// tools/exp_reorder.py).  Every ray is still traced and shaded with its own
// slot's data, so results do not depend on the order.  In LENGTH order
// (dslots::len_order; one-mesh diffuse scenes) the same sort runs on other
// keys: new camera rays first, then continuing rays by the traversal length a
// per-scene table predicts for them, so that a tile's short rays share waves
// (TileOrderLengthKey; C3 extend 0.84x vs the octant order).
#pragma once

#include "pt_device.hpp"
#include "traverse.hpp"
#include "kernels.hpp"
#include "bsdf.hpp"

namespace ptd {

// --- slot / pixel mapping ---------------------------------------------------

// t / tiles_x by the host-computed reciprocal (exact for t * tiles_x < 2^32).
// (tiles_x == 1: the reciprocal 2^32 does not fit, the row is t itself.)
PT_DEV uint32_t TileRow(const dframe& F, uint32_t t)
{
    return F.tiles_x == 1 ? t : __umulhi(t, F.tiles_x_magic);
}

// Path stream of tile t, and t's tile within its stream.
PT_DEV uint32_t TileStream(const dframe& F, uint32_t& t)
{
    if (F.streams == 1) return 0;
    const uint32_t k = __umulhi(t, F.stream_magic);
    t -= k * F.stream_tiles;
    return k;
}

// The seed of slot s's stream (FrameIndex + (stream << 24)) and its
// accumulator.
PT_DEV uint32_t StreamSeed(uint32_t seed, uint32_t stream) { return seed + (stream << 24); }
PT_DEV float4* StreamAccum(const dframe& F, uint32_t stream)
{
    return F.streams == 1 ? F.accum : F.accx + (size_t)stream * F.width * F.height;
}

PT_DEV bool SlotPixel(const dframe& F, uint32_t s, uint32_t& x, uint32_t& y, uint32_t& stream)
{
    uint32_t t = s >> 8, l = s & 255u;
    stream = TileStream(F, t);
    uint32_t k = TileRow(F, t);
    uint32_t tx = t - k * F.tiles_x;
    uint32_t band = F.rank + k * F.nranks;
    x = tx * 16 + (l & 15u);
    y = band * 16 + (l >> 4);
    return x < F.width && y < F.height;
}

// Valid positions of a tile are the first (pixels of the tile inside the
// image): TileOrder sorts the slots outside the image to the end.
PT_DEV bool SlotPixel(const dframe& F, uint32_t s, uint32_t& x, uint32_t& y)
{
    uint32_t stream;
    return SlotPixel(F, s, x, y, stream);
}

PT_DEV bool PositionValid(const dframe& F, uint32_t q)
{
    uint32_t t = q >> 8;
    (void)TileStream(F, t);
    uint32_t k = TileRow(F, t);
    uint32_t tx = t - k * F.tiles_x;
    uint32_t band = F.rank + k * F.nranks;
    uint32_t nx = min(16u, F.width - tx * 16u);
    uint32_t ny = band * 16u < F.height ? min(16u, F.height - band * 16u) : 0u;
    return (q & 255u) < nx * ny;
}

// Position of slot s's current ray / last traced hit.
PT_DEV uint32_t RayPos(const dslots& L, uint32_t s, uint32_t p16) { return (s & ~255u) | (p16 >> 8); }
PT_DEV uint32_t HitPos(const dslots& L, uint32_t s, uint32_t p16) { return (s & ~255u) | (p16 & 255u); }

// --- path state ----------------------------------------------------------------


struct path {
    float Lambda0;
    pt4 Throughput, Probability;
    pt3 Sample;
    uint32_t Active[4];
};

// The path's four wavelengths from its normalized Lambda0
// (basic_scatter.glsl:118-122).
PT_DEV pt4 PathLambda(float L0)
{
    return v4(pt_mix(PT_CIE_LAMBDA_MIN, PT_CIE_LAMBDA_MAX, L0),
              pt_mix(PT_CIE_LAMBDA_MIN, PT_CIE_LAMBDA_MAX, pt_fract(L0 + 0.25f)),
              pt_mix(PT_CIE_LAMBDA_MIN, PT_CIE_LAMBDA_MAX, pt_fract(L0 + 0.50f)),
              pt_mix(PT_CIE_LAMBDA_MIN, PT_CIE_LAMBDA_MAX, pt_fract(L0 + 0.75f)));
}

// An escaped path's contribution (basic_scatter.glsl:165-173): the sky's
// radiance along V times the throughput, observed (CIE XYZ) and divided by
// the cluster PDF.
PT_DEV pt3 EscapeContribution(const dscene& S, pt3 V, pt4 Lambda, pt4 Throughput, float ClusterPDF)
{
    pt4 Emission = SampleSkyboxRadiance(S, V, Lambda);
    pt4 E = Emission * Throughput;
    // Left-to-right sum over the four wavelengths (the reference's
    // expression order) as a rolled loop: one observer evaluation's
    // registers at a time.
    float Lv[4] = {Lambda.x, Lambda.y, Lambda.z, Lambda.w};
    float Ev[4] = {E.x, E.y, E.z, E.w};
    pt3 XYZ = SampleStandardObserver(Lv[0]) * Ev[0];
#pragma unroll 1
    for (int I = 1; I < 4; I++) XYZ = XYZ + SampleStandardObserver(Lv[I]) * Ev[I];
    return XYZ / ClusterPDF;
}

// Path record (basic.glsl.inc:159-198 StorePathVertex) minus Sample: Scatter
// adds to Sample only on escape, and the escape zeroes Probability, which
// ends the path in the same shade (its Sample goes to the accumulator and a
// new path starts with Sample = 0).  So every path alive between rounds has
// Sample == 0 and only lambda0 is stored (4 bytes instead of 16); the state
// readback reports the zero.
// `act_none`: the slot's stored active-shape stack is already empty (all
// four entries NONE), as a new path's is, so its 8-byte record is not
// rewritten (a partial-line store for every completed path otherwise).
//
// GreyRecord: when the renderer's shade mask has no translucent and no
// OpenPBR material (pt_grey_mats), every factor Scatter multiplies into a
// path's Probability is the same for the four wavelengths -- the diffuse and
// metal pdfs are scalars (basic_diffuse.glsl.inc:30-33, basic_metal.glsl.inc),
// the sky pdf too, the medium density of the vacuum-or-scene-fog medium is
// v4(SceneScatterRate) based (basic_scatter.glsl:137-163), the roulette
// factor is a scalar (:295-298) -- and a new path starts at vec4(1); so the
// four components are the same bits, and the slot stores one float
// (L.prob1).  The active-shape stack can only grow on a refraction into a
// shape (In.z * Out.z < 0 with Out.z > 0, :266-282), which needs a
// translucent (or OpenPBR) BSDF: diffuse / metal directions have In.z >= 0,
// a sky sample below the surface ends the path, and a non-real hit seen from
// outside cannot occur with an empty stack; so it stays empty and is neither
// read nor written.  The host switches a renderer's live paths between the
// forms (pt_launch_grey_convert) when its shade mask changes.
PT_DEV void StorePathVertex(const dslots& L, uint32_t s, const path& P, bool act_none = false)
{
    L.thr[s] = make_float4(P.Throughput.x, P.Throughput.y, P.Throughput.z, P.Throughput.w);
    if (L.prob1) L.prob1[s] = P.Probability.x;
    else L.prob[s] = make_float4(P.Probability.x, P.Probability.y, P.Probability.z, P.Probability.w);
    L.lam[s] = P.Lambda0;
    if (!act_none) L.act[s] = make_uint2((P.Active[1] << 16) | P.Active[0], (P.Active[3] << 16) | P.Active[2]);
}

// Position of the k-th set bit (k < popcount) of a 64-bit word: a 6-step
// binary search over popcounts of the low halves.
PT_DEV uint32_t SelectBit64(uint64_t m, uint32_t k)
{
    uint32_t pos = 0;
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    uint32_t c = (uint32_t)__popc(lo);
    uint32_t w = lo;
    if (k >= c) { k -= c; w = hi; pos = 32; }
#pragma unroll
    for (uint32_t width = 16; width >= 1; width >>= 1) {
        uint32_t cw = (uint32_t)__popc(w & ((1u << width) - 1u));
        if (k >= cw) { k -= cw; w >>= width; pos += width; }
    }
    return pos;
}

// ShadeOrder: the position shaded by thread u of a tile: the positions of
// outcome class 0 first (in position order), then class 1, ... (miss last),
// from the tile's class masks (extend).  Tile-uniform mask words (scalar
// loads and counts), no barrier.
// Two classes (single-material scenes): hits first, then the miss mask.
PT_DEV uint32_t ShadePosition2(const uint64_t* miss, uint32_t u)
{
    uint64_t m0 = miss[0], m1 = miss[1], m2 = miss[2], m3 = miss[3];
    uint32_t c0 = (uint32_t)__popcll(~m0), c1 = (uint32_t)__popcll(~m1), c2 = (uint32_t)__popcll(~m2);
    uint32_t nhit = c0 + c1 + c2 + (uint32_t)__popcll(~m3);
    bool hit = u < nhit;
    uint32_t k = hit ? u : u - nhit;
    uint64_t w0 = hit ? ~m0 : m0, w1 = hit ? ~m1 : m1, w2 = hit ? ~m2 : m2, w3 = hit ? ~m3 : m3;
    uint32_t n0 = hit ? c0 : 64u - c0, n1 = hit ? c1 : 64u - c1, n2 = hit ? c2 : 64u - c2;
    uint32_t word = 0;
    uint64_t w = w0;
    if (k >= n0) { k -= n0; word = 1; w = w1;
        if (k >= n1) { k -= n1; word = 2; w = w2;
            if (k >= n2) { k -= n2; word = 3; w = w3; } } }
    return word * 64 + SelectBit64(w, k);
}

PT_DEV uint32_t ShadePosition(const uint64_t* mask, uint32_t u)
{
    uint32_t cnt[PT_OUTCOME_CLASSES][4], before = 0;
    uint32_t cls = 0, k = u;
#pragma unroll
    for (uint32_t c = 0; c < PT_OUTCOME_CLASSES; c++) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            cnt[c][w] = (uint32_t)__popcll(mask[4 * c + w]);
            n += cnt[c][w];
        }
        if (u >= before) { cls = c; k = u - before; }   // last class whose start is <= u
        before += n;
    }
    // Empty classes share their start with the next class, so the last
    // class starting at or before u holds u.
    uint32_t word = 0;
    uint32_t c0 = cnt[0][0], c1 = cnt[0][1], c2 = cnt[0][2];
#pragma unroll
    for (uint32_t c = 1; c < PT_OUTCOME_CLASSES; c++)
        if (cls == c) { c0 = cnt[c][0]; c1 = cnt[c][1]; c2 = cnt[c][2]; }
    if (k >= c0) { k -= c0; word = 1;
        if (k >= c1) { k -= c1; word = 2;
            if (k >= c2) { k -= c2; word = 3; } } }
    return word * 64 + SelectBit64(mask[4 * cls + word], k);
}

// TileOrder: called by all 256 threads of a block (one tile) once their new
// rays are known.  Sort key: direction octant (0-7) for valid slots, 8 for
// slots outside the image.  Per wave, a ballot per key gives each lane its
// rank among the wave's lanes of that key; one wave-wide exclusive scan of the
// 4 x 9 (key-major) counts gives every (key, wave) its base.  `hitbyte` is
// the position of the slot's last traced hit (shade: the ray it just
// consumed, where extend wrote the hit; raygen: unchanged).
PT_DEV uint32_t TileOrderKey(bool valid, pt3 V)
{
    return valid ? ((V.x < 0.0f ? 1u : 0u) | (V.y < 0.0f ? 2u : 0u) | (V.z < 0.0f ? 4u : 0u)) : 8u;
}

// LENGTH order (dslots::len_order; DESIGN.md §4 "Length classes"): the same
// ranking with other keys, so that a tile's short rays share waves and those
// waves end early.  0 for a new camera ray (every raygen ray, shade's
// completed paths), 1 + the length class of the ray's key in the scene's
// table (include/pt_raykey.h) for a continuing ray, 8 outside the image.
// Camera rays therefore sit at the tile's first positions; their count goes
// to len_cam, and a training extend skips them (their few shared keys would
// serialise its atomics).  Until the table is trained a continuing ray's class
// is its octant, the last two sharing one, which keeps the camera rays first.
PT_DEV uint32_t TileOrderLengthKey(const dslots& L, bool valid, bool camera, pt3 O, pt3 V)
{
    if (!valid) return 8u;
    if (camera) return 0u;
    if (!L.len_cls) return 1u + min(TileOrderKey(true, V), PT_RAYKEY_CLASSES - 1u);
    return 1u + L.len_cls[pt_ray_key(O.x, O.y, O.z, V.x, V.y, V.z, &L.len_bounds)];
}

// The same for a ray already packed ({O.xyz, PackUnitVector(V)}) with its key.
template <bool LEN = false>
PT_DEV void TileOrderStoreKeyed(const dslots& L, uint32_t s, uint32_t key, float4 ray, uint32_t hitbyte)
{
    __shared__ uint32_t cnt[64];
    uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t k = 0; k < 9; k++) {
        uint64_t m = __ballot(key == k);
        uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (key == k) rank = below;
        if (lane == 0) cnt[k * 4 + w] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t v = lane < 36 ? cnt[lane] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
        if ((int)lane >= o) incl += t;
    }
    uint32_t base = (uint32_t)__shfl((int)(incl - v), (int)(key * 4 + w), 64);
    uint32_t p = base + rank;
    uint32_t q = (s & ~255u) | p;
    L.ray[q] = ray;
    L.pos[s] = (uint16_t)((p << 8) | hitbyte);
    L.slotof[q] = (uint8_t)(s & 255u);
    if constexpr (LEN) {
        // Key 0's four counts end at lane 3 of the scan: the tile's camera rays.
        if (threadIdx.x == 3) L.len_cam[s >> 8] = (uint16_t)incl;
    }
}

// camera: the ray starts a new path (read in LENGTH order only).
template <bool LEN = false>
PT_DEV void TileOrderStoreRay(const dslots& L, uint32_t s, bool valid, bool camera, pt3 O, pt3 V, uint32_t hitbyte)
{
    uint32_t key;
    if constexpr (LEN) key = TileOrderLengthKey(L, valid, camera, O, V);
    else key = TileOrderKey(valid, V);
    TileOrderStoreKeyed<LEN>(L, s, key, make_float4(O.x, O.y, O.z, __uint_as_float(PackUnitVector(V))), hitbyte);
}

// GenerateNewPath (basic_scatter.glsl:7-42) + GenerateCameraRay (scene.glsl.inc:613-655)
PT_DEV void GenerateNewPath(const dscene& S, const dslots& L, const dframe& F, const dparams& Pm, rng& G, uint32_t s,
                            uint32_t x, uint32_t y, pt3& RO, pt3& RV, bool act_none = false)
{
    float SPx = (float)x, SPy = (float)y;
    if (Pm.render_flags & PT_RENDER_FLAG_SAMPLE_JITTER) {
        float JX = G.R01();
        float JY = G.R01();
        SPx = SPx + JX; SPy = SPy + JY;
    } else {
        SPx = SPx + 0.5f; SPy = SPy + 0.5f;
    }
    float Nx = SPx / (float)F.width, Ny = SPy / (float)F.height;
    const pt_packed_camera* Cam = &S.cameras[Pm.camera_index];
    uint32_t Model = Cam->Model;
    pt3 O, V;
    if (Model == PT_CAMERA_MODEL_PINHOLE || Model == PT_CAMERA_MODEL_THIN_LENS) {
        pt3 SP = v3(-Cam->SensorSize[0] * (Nx - 0.5f), -Cam->SensorSize[1] * (0.5f - Ny), Cam->SensorDistance);
        if (Model == PT_CAMERA_MODEL_PINHOLE) {
            pt2 D = Cam->ApertureRadius * RandomPointOnDisk(G);
            O = v3(D.x, D.y, 0);
            V = normalize(O - SP);
        } else {
            pt3 OP = -SP * Cam->FocalLength / (SP.z - Cam->FocalLength);
            pt2 D = Cam->ApertureRadius * RandomPointOnDisk(G);
            O = v3(D.x, D.y, 0);
            V = normalize(OP - O);
        }
    } else if (Model == PT_CAMERA_MODEL_360) {
        float Phi = (Nx - 0.5f) * PT_TAU;
        float Theta = (0.5f - Ny) * PT_PI;
        O = v3(0, 0, 0);
        V = v3(pt_cos(Theta) * pt_sin(Phi), pt_sin(Theta), -pt_cos(Theta) * pt_cos(Phi));
    } else {
        O = v3s(0); V = v3s(0);
    }
    const float* To = Cam->Transform.To;
    RO = mat4_mul_point(To, O);
    RV = mat4_mul_vector(To, V);
    path P;
    P.Lambda0 = G.R01();
    P.Throughput = v4s(1.0f);
    P.Probability = v4s(1.0f);
    P.Sample = v3s(0.0f);
    P.Active[0] = P.Active[1] = P.Active[2] = P.Active[3] = SHAPE_INDEX_NONE;
    StorePathVertex(L, s, P, act_none);
}

// Scatter (basic_scatter.glsl:114-310).  Returns true if an extension ray was
// produced (written to O, V).
template <uint32_t MATS, uint32_t CLS = 0xFFFFFFFFu>
PT_DEV bool Scatter(const dscene& S, rng& G, float PTP, path& Path, pt3& O, pt3& V, uint32_t HitShape,
                    uint32_t HitMaterial, float HitTime, uint32_t PN, uint32_t PT, pt2 UV)
{
    pt4 Lambda = PathLambda(Path.Lambda0);

    uint32_t Active = SHAPE_INDEX_NONE;
    for (int I = 0; I < 4; I++) Active = pt_umin(Active, Path.Active[I]);

    medium Md = ResolveMedium<MATS>(S, Active, Lambda);
    // Without translucent (or shaded OpenPBR) materials every medium is vacuum: exp(-0 * t) = 1
    // exactly, so the multiply is an identity and is skipped.
    if (MATS & (PT_MATS_TRANSLUCENT | PT_MATS_OPENPBR)) Path.Throughput = Path.Throughput * vexp(-Md.AbsorptionRate * HitTime);

    float ScatteringTime = PT_HIT_TIME_LIMIT;
    if ((MATS & PT_MATS_SCATTER) && Md.ScatteringRate.x > 0.0f) ScatteringTime = -pt_log(G.R01()) / Md.ScatteringRate.x;

    if (HitTime >= ScatteringTime) {
        if (ScatteringTime < PT_HIT_TIME_LIMIT) {
            ShadeMark(SM_MEDIUM_EVENT);
            O = O + V * ScatteringTime;
            pt3 X, Y, Z = V;
            ComputeCoordinateFrame(Z, X, Y);
            float U1 = G.R01();
            float U2 = G.R01();
            pt3 Sc = SampleDirectionHG(Md.ScatteringAnisotropy, U1, U2);
            pt4 Density = Md.ScatteringRate * vexp(-Md.ScatteringRate * ScatteringTime);
            Density = Density / pt_max(PT_EPSILON, max4(Density));
            Path.Throughput = Path.Throughput * Density;
            Path.Probability = Path.Probability * Density;
            V = normalize(X * Sc.x + Y * Sc.y + Z * Sc.z);
        } else {
            ShadeMark(SM_ESCAPE);
            float ClusterPDF = Path.Probability.x + Path.Probability.y + Path.Probability.z + Path.Probability.w;
            Path.Sample = Path.Sample + EscapeContribution(S, V, Lambda, Path.Throughput, ClusterPDF);
            Path.Probability = v4s(0.0f);
        }
        return max4(Path.Probability) > PT_EPSILON;
    }

    ShadeMark(SM_SURFACE);
    pt3 Nrm = UnpackUnitVector(PN);
    pt3 TX = UnpackUnitVector(PT);
    pt3 TY = cross(Nrm, TX);
    pt3 Position = O + HitTime * V;

    pt3 Out = -v3(dot(V, TX), dot(V, TY), dot(V, Nrm));
    bool IsReal;
    pt4 ExteriorIOR = v4s(1.0f);
    uint32_t ShapePriority = HitShape;
    if (Out.z > 0) {
        IsReal = Md.Priority > ShapePriority;
        if (IsReal) ExteriorIOR = Md.IOR;
    } else {
        IsReal = Md.Priority == ShapePriority;
        if (IsReal) {
            ShadeMark(SM_EXTERIOR_MEDIUM);
            uint32_t Ext = SHAPE_INDEX_NONE;
            for (int I = 0; I < 4; I++) {
                if (Path.Active[I] == Active) continue;
                Ext = pt_umin(Ext, Path.Active[I]);
            }
            ExteriorIOR = ResolveMedium<MATS>(S, Ext, Lambda).IOR;
        }
    }

    pt3 In;
    if (IsReal) {
        ShadeMark(SM_REAL);
        bsdf_parameters P;
        P.MaterialIndex = HitMaterial;
        P.TextureUV = UV;
        P.Lambda = Lambda;
        P.ExteriorIOR = ExteriorIOR;
        pt4 T, Pr;
        if (!SampleSurfaceIntegrand<MATS, CLS>(S, G, Nrm, TX, TY, P, Out, In, T, Pr)) return false;
        float Scale = 1.0f / pt_max(PT_EPSILON, max4(Pr));
        Path.Throughput = Path.Throughput * (T * Scale);
        Path.Probability = Path.Probability * (Pr * Scale);
    } else {
        ShadeMark(SM_NOT_REAL);
        In = -Out;
    }

    // Active-shape stack update (basic_scatter.glsl:266-282): first free slot
    // on entry, first matching slot on exit; constant indices keep the four
    // slots in registers.
    if (In.z * Out.z < 0) {
        uint32_t* A = Path.Active;
        if (Out.z > 0) {
            if (A[0] == SHAPE_INDEX_NONE) A[0] = HitShape;
            else if (A[1] == SHAPE_INDEX_NONE) A[1] = HitShape;
            else if (A[2] == SHAPE_INDEX_NONE) A[2] = HitShape;
            else if (A[3] == SHAPE_INDEX_NONE) A[3] = HitShape;
        } else {
            if (A[0] == HitShape) A[0] = SHAPE_INDEX_NONE;
            else if (A[1] == HitShape) A[1] = SHAPE_INDEX_NONE;
            else if (A[2] == HitShape) A[2] = SHAPE_INDEX_NONE;
            else if (A[3] == HitShape) A[3] = SHAPE_INDEX_NONE;
        }
    }

    ShadeMark(SM_ROULETTE);
    if (G.R01() < PTP) return false;
    Path.Probability = Path.Probability * (1.0f - PTP);

    V = In.x * TX + In.y * TY + In.z * Nrm;
    O = Position + 1e-3f * V;
    return max4(Path.Probability) > PT_EPSILON;
}

}  // namespace ptd
