// bsdf.hpp — the materials of the shade kernels: the basic BSDFs, the opt-in
// OpenPBR sampler, the media and SampleSurfaceIntegrand, with the branch
// marks of the shade statistics build.  Used through path.hpp.
#pragma once

#include "pt_device.hpp"
#include "kernels.hpp"

namespace ptd {

// --- shade branch statistics (experiment build only) ---------------------------
//
// Built with -DPT_SHADE_STATS=1 (tools/shade_stats.py via tools/build_variant.py),
// each mark ShadeMark(k) records, once per wave that reaches it, the number of
// lanes active there: waves[k] and lanes[k] summed over the launch, so
// lanes[k] / waves[k] is the SIMD occupancy of that branch of Scatter.  The
// product build compiles every mark to nothing.  A mark touches LDS only;
// shade_kernel clears the block's counts and adds them to the launch's
// (shade.hip ShadeStatsBegin / ShadeStatsEnd).
#ifndef PT_SHADE_STATS
#define PT_SHADE_STATS 0
#endif
enum : uint32_t {
    SM_ENTRY, SM_HIT, SM_ESCAPE, SM_MEDIUM_EVENT, SM_SURFACE, SM_REAL, SM_LIGHT, SM_LIGHT_BELOW,
    SM_DIFFUSE_COSINE, SM_DIFFUSE_EVAL, SM_METAL_EVAL, SM_METAL_SAMPLE, SM_TRANS_EVAL, SM_TRANS_SAMPLE,
    SM_TRANS_REFLECT, SM_TRANS_REFRACT, SM_OPENPBR, SM_NOT_REAL, SM_ROULETTE, SM_COMPLETED, SM_CONTINUE,
    SM_EXTERIOR_MEDIUM, SM_MESH_HIT, SM_SPHERE_HIT, SM_CUBE_HIT, SM_PLANE_HIT, SM_COUNT
};
#if PT_SHADE_STATS
PT_DEV uint32_t* ShadeStatLds()
{
    __shared__ uint32_t a[2 * 32];
    return a;
}
PT_DEV void ShadeMark(uint32_t k)
{
    const uint64_t m = __ballot(1);
    const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    if ((threadIdx.x & 63u) == first) {
        atomicAdd(&ShadeStatLds()[2 * k], 1u);
        atomicAdd(&ShadeStatLds()[2 * k + 1], (uint32_t)__popcll(m));
    }
}
#else
PT_DEV void ShadeMark(uint32_t) {}
#endif
// --- materials ---------------------------------------------------------------

struct bsdf_parameters { uint32_t MaterialIndex; pt2 TextureUV; pt4 Lambda; pt4 ExteriorIOR; };

// The basic BSDFs (basic_diffuse / basic_metal / basic_translucent.glsl.inc)
// take their material parameters already fetched (bsdf_material, below):
// SampleSurfaceIntegrand reads them once per hit, in code shared by the
// material types and by the light-sample evaluation and the BSDF sample,
// instead of once in each of those divergent branches.  The expressions are
// the reference's, so the results are the same bits.

// Texture-able material parameters of a basic material (MaterialEvaluateBSDF /
// MaterialSampleBSDF's *_GetParameters): Refl = the base reflectance
// (diffuse / metal), Aux = the metal's specular reflectance or the
// translucent's relative IOR, A / Rough = the GGX alpha of metal and
// translucent materials.
static_assert(PT_BASIC_DIFFUSE_BASE_SPECTRUM == PT_BASIC_METAL_BASE_SPECTRUM, "shared base reflectance word");
struct bsdf_material {
    pt4 Refl, Aux;
    pt2 A;
    bool Rough;
};

PT_DEV bool Diffuse_Evaluate(const bsdf_material& Q, pt3 In, pt4& T, pt4& Pr)
{
    Pr = v4s(In.z / PT_PI);
    T = Pr * Q.Refl;
    return true;
}

PT_DEV bool Metal_Evaluate(const bsdf_material& Q, pt3 In, pt3 Out, pt4& T, pt4& Pr)
{
    const pt2 A = Q.A;
    if (In.z <= 0.0f || Out.z <= 0.0f || !Q.Rough) return false;
    pt3 Half = SafeNormalize(In + Out);
    float Gm = GGXSmithG1(In, A);
    float D = GGXDistribution(Half, A);
    Pr = v4s(Gm * D / (4 * In.z));
    float Gs = GGXSmithG1(Out, A);
    pt4 F = SchlickFresnelMetal(Q.Refl, Q.Aux, dot(In, Half));
    T = Pr * Gs * F;
    return true;
}

PT_DEV bool Metal_Sample(rng& G, const bsdf_material& Q, pt3 In, pt3& Out, pt4& T, pt4& Pr)
{
    const pt2 A = Q.A;
    if (In.z <= 0.0f) return false;
    float U1 = G.R01();
    float U2 = G.R01();
    pt3 N = GGXVisibleNormal(In, A, U1, U2);
    float CosThetaIn = pt_min(dot(N, In), 1.0f);
    Out = 2 * CosThetaIn * N - In;
    if (Out.z <= 0.0f) return false;
    Pr = v4s(1.0f);
    if (Q.Rough) {
        float Gm = GGXSmithG1(In, A);
        float D = GGXDistribution(N, A);
        Pr = Pr * v4s(Gm * D / (4 * In.z));
    }
    float Gs = GGXSmithG1(Out, A);
    pt4 F = SchlickFresnelMetal(Q.Refl, Q.Aux, CosThetaIn);
    T = Pr * Gs * F;
    return true;
}

// Q.Aux = RelativeIOR: Interior / Exterior when In.z < 0, else Exterior /
// Interior (basic_translucent.glsl.inc GetParameters), In the direction
// towards the viewer (Scatter's Out).
PT_DEV bool Translucent_Evaluate(const bsdf_material& Q, pt3 In, pt3 Out, pt4& T, pt4& Pr)
{
    const pt4 RelIOR = Q.Aux;
    const pt2 A = Q.A;
    if (!Q.Rough) { Pr = v4s(0.0f); T = v4s(0.0f); return true; }
    float Gm = GGXSmithG1(In, A);
    if (In.z * Out.z > 0) {
        pt3 Half = SafeNormalize(Out + In);
        float CosThetaIn = dot(Half, In);
        pt4 F = FresnelDielectric(RelIOR, v4s(CosThetaIn));
        float D = GGXDistribution(Half, A);
        Pr = F * Gm * D / (4 * In.z);
    } else {
        pt3 H1 = SafeNormalize(Out + In * RelIOR.x);
        pt3 H2 = SafeNormalize(Out + In * RelIOR.y);
        pt3 H3 = SafeNormalize(Out + In * RelIOR.z);
        pt3 H4 = SafeNormalize(Out + In * RelIOR.w);
        pt4 Ci = v4(dot(In, H1), dot(In, H2), dot(In, H3), dot(In, H4));
        pt4 Co = v4(dot(Out, H1), dot(Out, H2), dot(Out, H3), dot(Out, H4));
        pt4 F = FresnelDielectric(RelIOR, Ci, Co);
        pt4 D = v4s(0.0f);
        if (Ci.x * Co.x < 0.0f) D.x = GGXDistribution(H1, A);
        if (Ci.y * Co.y < 0.0f) D.y = GGXDistribution(H2, A);
        if (Ci.z * Co.z < 0.0f) D.z = GGXDistribution(H3, A);
        if (Ci.w * Co.w < 0.0f) D.w = GGXDistribution(H4, A);
        pt4 Sq = Ci * RelIOR + Co;
        pt4 J = vabs(Co) / (Sq * Sq);
        Pr = D * (1 - F) * Gm * J * vabs(Ci / In.z);
    }
    float Gs = GGXSmithG1(Out, A);
    T = Pr * Gs;
    return true;
}

PT_DEV bool Translucent_Sample(rng& G, const bsdf_material& Q, pt3 In, pt3& Out, pt4& T, pt4& Pr)
{
    const pt4 RelIOR = Q.Aux;
    const pt2 A = Q.A;
    float U1 = G.R01();
    float U2 = G.R01();
    pt3 N = GGXVisibleNormal(In * pt_sign(In.z), A, U1, U2);
    float CosThetaIn = pt_clamp(dot(N, In), -1.0f, +1.0f);
    float CosThetaRefracted = ComputeCosThetaRefracted(RelIOR.x, CosThetaIn);
    float Reflectance = FresnelDielectric(RelIOR.x, CosThetaIn, CosThetaRefracted);
    if (G.R01() < Reflectance) {
        ShadeMark(SM_TRANS_REFLECT);
        Out = 2 * CosThetaIn * N - In;
        if (Out.z * In.z <= 0) return false;
        pt4 F = FresnelDielectric(RelIOR, v4s(CosThetaIn));
        Pr = F;
        if (Q.Rough) {
            float Gm = GGXSmithG1(In, A);
            float D = GGXDistribution(N, A);
            Pr = Pr * (Gm * D / (4 * pt_abs(In.z)));
        }
        float Gs = GGXSmithG1(Out, A);
        T = Pr * Gs;
        return true;
    }
    ShadeMark(SM_TRANS_REFRACT);
    Out = (CosThetaRefracted + RelIOR.x * CosThetaIn) * N - RelIOR.x * In;
    if (Out.z * In.z >= 0) return false;
    if (Q.Rough) {
        pt3 N2 = SafeNormalize(Out + In * RelIOR.y);
        pt3 N3 = SafeNormalize(Out + In * RelIOR.z);
        pt3 N4 = SafeNormalize(Out + In * RelIOR.w);
        pt4 Ci = v4(CosThetaIn, dot(In, N2), dot(In, N3), dot(In, N4));
        pt4 Co = v4(CosThetaRefracted, dot(Out, N2), dot(Out, N3), dot(Out, N4));
        pt4 F = FresnelDielectric(RelIOR, Ci, Co);
        pt4 D = v4s(0.0f);
        D.x = GGXDistribution(N, A);
        if (Ci.y * Co.y < 0.0f) D.y = GGXDistribution(N2, A);
        if (Ci.z * Co.z < 0.0f) D.z = GGXDistribution(N3, A);
        if (Ci.w * Co.w < 0.0f) D.w = GGXDistribution(N4, A);
        float Gm = GGXSmithG1(In, A);
        pt4 Sq = Ci * RelIOR + Co;
        pt4 J = vabs(Co) / (Sq * Sq);
        Pr = D * (1 - F) * Gm * J * vabs(Ci / In.z);
    } else {
        Pr = v4(1 - Reflectance, 0, 0, 0);
    }
    float Gs = GGXSmithG1(Out, A);
    T = Pr * Gs;
    return true;
}

// --- OpenPBR (src/scene/openpbr.glsl.inc) ----------------------------------------
// The reference packs OpenPBR materials but never shades them (its include is
// commented out, scene.glsl.inc:685, and DISPATCH_MATERIAL has no OpenPBR
// case), so by default an OpenPBR hit ends the path as there.  With
// ptSetBasicRendererOpenPBR the layered sampler below is dispatched instead
// (PT_MATS_OPENPBR instantiation): a sampling-only BSDF (HasDirac true, so no
// skybox light sampling), the medium of openpbr.glsl.inc:160-191.  Deviations
// from the uncompiled text: the coat's FresnelDielectric
// arguments are put in signature order; Emission, computed but never read by
// OpenPBR_Sample, is not evaluated; a LayerBounceLimit of 0 leaves In = -Out
// (the reference's out parameter is unassigned).

struct openpbr_parameters {                       // openpbr.glsl.inc:30-47
    uint32_t LayerBounceLimit;
    bool BaseIsMetal, BaseIsTranslucent, CoatIsPresent;
    pt4 BaseReflectance;
    float BaseDiffuseRoughness;
    pt4 CoatRelativeIOR, CoatTransmittance;
    pt2 CoatRoughnessAlpha;
    float SpecularWeight;
    pt4 SpecularRelativeIOR, SpecularReflectance;
    pt2 SpecularRoughnessAlpha;
};

// OpenPBR_Parameters (:66-158): three stochastic layer choices, then the
// spectral parameters at the cluster wavelengths.
PT_DEV openpbr_parameters OpenPBR_Parameters(const dscene& S, rng& G, const bsdf_parameters& P)
{
    const uint32_t M = P.MaterialIndex;
    openpbr_parameters Q;
    Q.CoatIsPresent = G.R01() < MFloat(S, M, PT_OPENPBR_COAT_WEIGHT);
    Q.BaseIsMetal = G.R01() < MFloat(S, M, PT_OPENPBR_BASE_METALNESS);
    Q.BaseIsTranslucent = !Q.BaseIsMetal && G.R01() < MFloat(S, M, PT_OPENPBR_TRANSMISSION_WEIGHT);
    Q.BaseReflectance = MFloat(S, M, PT_OPENPBR_BASE_WEIGHT) *
                        SampleParametricSpectrum(MVec3(S, M, PT_OPENPBR_BASE_SPECTRUM), P.Lambda);
    Q.BaseDiffuseRoughness = MFloat(S, M, PT_OPENPBR_BASE_DIFFUSE_ROUGHNESS);
    uint32_t Tx = MUint(S, M, PT_OPENPBR_BASE_SPECTRUM_TEXTURE_INDEX);
    if (Tx != TEXTURE_INDEX_NONE) {
        pt4 V = SampleTexture(S, Tx, P.TextureUV);
        Q.BaseReflectance = Q.BaseReflectance * SampleParametricSpectrum(v3(V.x, V.y, V.z), P.Lambda);
    }
    const float CoatIOR = MFloat(S, M, PT_OPENPBR_COAT_IOR);
    Q.CoatRelativeIOR = v4s(1.0f); Q.CoatTransmittance = v4s(1.0f); Q.CoatRoughnessAlpha = v2(0.0f, 0.0f);
    if (Q.CoatIsPresent) {
        Q.CoatRelativeIOR = P.ExteriorIOR / CoatIOR;
        Q.CoatTransmittance = SampleParametricSpectrum(MVec3(S, M, PT_OPENPBR_COAT_COLOR_SPECTRUM), P.Lambda);
        Q.CoatRoughnessAlpha = GGXRoughnessAlpha(MFloat(S, M, PT_OPENPBR_COAT_ROUGHNESS),
                                                 MFloat(S, M, PT_OPENPBR_COAT_ROUGHNESS_ANISOTROPY));
    }
    Q.SpecularWeight = MFloat(S, M, PT_OPENPBR_SPECULAR_WEIGHT);
    Q.SpecularReflectance = SampleParametricSpectrum(MVec3(S, M, PT_OPENPBR_SPECULAR_SPECTRUM), P.Lambda);
    pt4 SpecularIOR = CauchyEmpiricalIOR(MFloat(S, M, PT_OPENPBR_SPECULAR_IOR),
                                         MFloat(S, M, PT_OPENPBR_TRANSMISSION_DISPERSION_ABBE_NUMBER), P.Lambda);
    Q.SpecularRelativeIOR = Q.CoatIsPresent ? CoatIOR / SpecularIOR : P.ExteriorIOR / SpecularIOR;
    float SpecularRoughness = MFloat(S, M, PT_OPENPBR_SPECULAR_ROUGHNESS);
    Tx = MUint(S, M, PT_OPENPBR_SPECULAR_ROUGHNESS_TEXTURE_INDEX);
    if (Tx != TEXTURE_INDEX_NONE) SpecularRoughness = SpecularRoughness * SampleTexture(S, Tx, P.TextureUV).x;
    Q.SpecularRoughnessAlpha = GGXRoughnessAlpha(SpecularRoughness, MFloat(S, M, PT_OPENPBR_SPECULAR_ROUGHNESS_ANISOTROPY));
    Q.LayerBounceLimit = MUint(S, M, PT_OPENPBR_LAYER_BOUNCE_LIMIT);
    return Q;
}

// OpenPBR_Medium (:160-191)
PT_DEV void OpenPBR_Medium(const dscene& S, uint32_t M, pt4 Lambda, medium& Md)
{
    Md.IOR = CauchyEmpiricalIOR(MFloat(S, M, PT_OPENPBR_SPECULAR_IOR),
                                MFloat(S, M, PT_OPENPBR_TRANSMISSION_DISPERSION_ABBE_NUMBER), Lambda);
    float TD = MFloat(S, M, PT_OPENPBR_TRANSMISSION_DEPTH);
    if (TD > 0.0f) {
        pt4 Ext = -vlog(SampleParametricSpectrum(MVec3(S, M, PT_OPENPBR_TRANSMISSION_SPECTRUM), Lambda)) / TD;
        pt4 Sc = SampleParametricSpectrum(MVec3(S, M, PT_OPENPBR_TRANSMISSION_SCATTER_SPECTRUM), Lambda) / TD;
        Md.AbsorptionRate = vmax(Ext - Sc, 0.0f);
        Md.ScatteringRate = Sc;
        Md.ScatteringAnisotropy = MFloat(S, M, PT_OPENPBR_TRANSMISSION_SCATTER_ANISOTROPY);
    } else {
        Md.AbsorptionRate = v4s(0.0f);
        Md.ScatteringRate = v4s(0.0f);
        Md.ScatteringAnisotropy = 0.0f;
    }
}

// OpenPBR_CoatSample (:194-283)
PT_DEV void OpenPBR_CoatSample(rng& G, const openpbr_parameters& Q, pt3 Out, pt3& In, pt4& T, pt4& D)
{
    if (!Q.CoatIsPresent) { In = -Out; return; }
    float U1 = G.R01();
    float U2 = G.R01();
    pt3 N = GGXVisibleNormal(Out * pt_sign(Out.z), Q.CoatRoughnessAlpha, U1, U2);
    float Cosine = dot(N, Out);
    pt4 R = Q.CoatRelativeIOR;
    if (Out.z < 0) R = 1.0f / R;
    float RefractedCosineSquared = 1 - R.x * R.x * (1 - Cosine * Cosine);
    float RefractedCosine = -pt_sign(Out.z) * pt_sqrt(pt_max(RefractedCosineSquared, 0.0f));
    float Reflectance = FresnelDielectric(R.x, Cosine, RefractedCosine);
    if (G.R01() < Reflectance) {
        In = 2 * Cosine * N - Out;
        if (In.z * Out.z <= 0) { D = v4s(0.0f); return; }
        T = T * GGXSmithG1(In, Q.CoatRoughnessAlpha);
        if (Out.z < 0) {
            float Exponent = -(0.5f / Out.z + 0.5f / In.z);
            T = T * vpow(Q.CoatTransmittance, Exponent);
        }
    } else {
        In = (R.x * Cosine + RefractedCosine) * N - R.x * Out;
        if (In.z * Out.z > 0) { D = v4s(0.0f); return; }
        T = T * GGXSmithG1(In, Q.CoatRoughnessAlpha);
        if (Out.z < 0) T = T * vpow(Q.CoatTransmittance, -0.5f / Out.z);
        else T = T * vpow(Q.CoatTransmittance, -0.5f / In.z);
    }
}

// OpenPBR_BaseSpecularSample (:286-435)
PT_DEV void OpenPBR_BaseSpecularSample(rng& G, const openpbr_parameters& Q, pt3 Out, pt3& In, pt4& T, pt4& D)
{
    const pt2 A = Q.SpecularRoughnessAlpha;
    float U1 = G.R01();
    float U2 = G.R01();
    pt3 N = GGXVisibleNormal(Out * pt_sign(Out.z), A, U1, U2);
    float Cosine = dot(N, Out);
    if (Q.BaseIsMetal) {
        In = 2 * Cosine * N - Out;
        if (Out.z * In.z <= 0) { D = v4s(0.0f); return; }
        float Shadowing = GGXSmithG1(Out, A);
        pt4 F = Q.SpecularWeight * SchlickFresnelMetal(Q.BaseReflectance, Q.SpecularReflectance, pt_abs(Cosine));
        T = T * (F * Shadowing);
        return;
    }
    pt4 R = Q.SpecularRelativeIOR;
    if (Out.z < 0) R = 1.0f / R;
    if (Q.SpecularWeight < 1.0f) {
        pt4 Rw = pt_sqrt(Q.SpecularWeight) * (1.0f - R) / (1.0f + R);
        R = (1.0f - Rw) / (1.0f + Rw);
    }
    float RefractedCosine = ComputeCosThetaRefracted(R.x, Cosine);
    float Reflectance = FresnelDielectric(R.x, Cosine, RefractedCosine);
    if (G.R01() < Reflectance) {
        In = 2 * Cosine * N - Out;
        if (In.z * Out.z <= 0) { D = v4s(0.0f); return; }
        if (Out.z > 0) T = T * Q.SpecularReflectance;
        T = T * GGXSmithG1(In, A);
        return;
    }
    In = (R.x * Cosine + RefractedCosine) * N - R.x * Out;
    if (In.z * Out.z > 0) { D = v4s(0.0f); return; }
    float Shadowing = GGXSmithG1(In, A);
    if (length(A) > PT_EPSILON) {
        pt4 F = v4s(0.0f);   // the reference's "TODO: This is broken for now!" (:390-391)
        pt3 N2 = SafeNormalize(In + Out * R.y);
        pt3 N3 = SafeNormalize(In + Out * R.z);
        pt3 N4 = SafeNormalize(In + Out * R.w);
        pt4 Dn = v4s(0.0f);
        Dn.x = GGXDistribution(N, A);
        if (dot(In, N2) * dot(Out, N2) < 0.0f) Dn.y = GGXDistribution(N2, A);
        if (dot(In, N3) * dot(Out, N3) < 0.0f) Dn.z = GGXDistribution(N3, A);
        if (dot(In, N4) * dot(Out, N4) < 0.0f) Dn.w = GGXDistribution(N4, A);
        Dn = Dn / pt_max(PT_EPSILON, max4(Dn));
        T = T * (Dn * F * Shadowing);
        D = D * (Dn * F);
    } else {
        T = T * v4(Shadowing, 0, 0, 0);
        D = D * v4(1, 0, 0, 0);
    }
}

// OpenPBR_BaseDiffuseSample (:438-461): Oren-Nayar-weighted cosine sampling.
PT_DEV void OpenPBR_BaseDiffuseSample(rng& G, const openpbr_parameters& Q, pt3 Out, pt3& In, pt4& T)
{
    if (Q.BaseIsTranslucent) { In = -Out; return; }
    In = SafeNormalize(RandomDirection(G) + v3(0, 0, 1));
    float Sv = dot(In, Out) - In.z * Out.z;
    float Tv = Sv > 0 ? pt_max(In.z, Out.z) : 1.0f;
    float SigmaSq = Q.BaseDiffuseRoughness * Q.BaseDiffuseRoughness;
    pt4 A = (1 - 0.5f * SigmaSq / (SigmaSq + 0.33f)) + 0.17f * Q.BaseReflectance * SigmaSq / (SigmaSq + 0.13f);
    float B = 0.45f * SigmaSq / (SigmaSq + 0.09f);
    T = T * (Q.BaseReflectance * (B * Sv / Tv + A));
}

// OpenPBR_Sample (:463-515): a random walk through the layer stack.
PT_DEV bool OpenPBR_Sample(rng& G, const openpbr_parameters& Q, pt3 Out, pt3& In, pt4& T, pt4& D)
{
    enum { EXTERNAL = -1, COAT = 0, BASE_SPECULAR = 1, BASE_DIFFUSE = 2 };
    int Layer = (Out.z > 0 && Q.CoatIsPresent) ? COAT : BASE_SPECULAR;
    T = v4s(1.0f);
    D = v4s(1.0f);
    In = -Out;
    for (uint32_t I = 0; I < Q.LayerBounceLimit; I++) {
        if (Layer == COAT) {
            OpenPBR_CoatSample(G, Q, Out, In, T, D);
            Layer = In.z < 0 ? BASE_SPECULAR : EXTERNAL;
        } else if (Layer == BASE_SPECULAR) {
            OpenPBR_BaseSpecularSample(G, Q, Out, In, T, D);
            Layer = In.z < 0 ? BASE_DIFFUSE : COAT;
        } else if (Layer == BASE_DIFFUSE) {
            OpenPBR_BaseDiffuseSample(G, Q, Out, In, T);
            Layer = In.z < 0 ? EXTERNAL : BASE_SPECULAR;
        } else {
            break;
        }
        if (max4(D) < PT_EPSILON) return false;
        Out = -In;
    }
    return true;
}

// Material-type specialisation of the shade kernel: MATS is a superset of the
// types referenced by the scene's shapes (computed on the host at upload), so
// dispatch branches for absent types are compiled out without changing any
// result.  PT_MATS_SCATTER: some medium can scatter (SceneScatterRate > 0 or
// a translucent / shaded OpenPBR material exists).  PT_MATS_OPENPBR: OpenPBR
// shading is enabled and the scene has OpenPBR shapes.
template <uint32_t MATS>
PT_DEV void LoadMedium(const dscene& S, uint32_t M, pt4 Lambda, medium& Md)
{
    Md.IOR = v4s(1.0f); Md.AbsorptionRate = v4s(0.0f); Md.ScatteringRate = v4s(0.0f); Md.ScatteringAnisotropy = 0.0f;
    if (!(MATS & (PT_MATS_TRANSLUCENT | PT_MATS_OPENPBR))) return;
    uint32_t Type = MUint(S, M, 0);
    if ((MATS & PT_MATS_OPENPBR) && Type == PT_MATERIAL_TYPE_OPENPBR) { OpenPBR_Medium(S, M, Lambda, Md); return; }
    if (!(MATS & PT_MATS_TRANSLUCENT) || Type != PT_MATERIAL_TYPE_BASIC_TRANSLUCENT) return;
    Md.IOR = CauchyEmpiricalIOR(MFloat(S, M, PT_BASIC_TRANSLUCENT_IOR), MFloat(S, M, PT_BASIC_TRANSLUCENT_ABBE_NUMBER), Lambda);
    float TD = MFloat(S, M, PT_BASIC_TRANSLUCENT_TRANSMISSION_DEPTH);
    if (TD > 0.0f) {
        pt4 Ext = -vlog(SampleParametricSpectrum(MVec3(S, M, PT_BASIC_TRANSLUCENT_TRANSMISSION_SPECTRUM), Lambda)) / TD;
        pt4 Sc = SampleParametricSpectrum(MVec3(S, M, PT_BASIC_TRANSLUCENT_SCATTERING_SPECTRUM), Lambda) / TD;
        Md.AbsorptionRate = vmax(Ext - Sc, 0.0f);
        Md.ScatteringRate = Sc;
        Md.ScatteringAnisotropy = MFloat(S, M, PT_BASIC_TRANSLUCENT_SCATTERING_ANISOTROPY);
    }
}

template <uint32_t MATS>
PT_DEV medium ResolveMedium(const dscene& S, uint32_t ShapeIndex, pt4 Lambda)
{
    medium Md;
    if (ShapeIndex == SHAPE_INDEX_NONE) {
        Md.Priority = 0xFFFFFFFFu;
        Md.IOR = v4s(1.0f);
        Md.AbsorptionRate = v4s(0.0f);
        Md.ScatteringRate = v4s(S.g.SceneScatterRate);
        Md.ScatteringAnisotropy = 0.0f;
    } else {
        LoadMedium<MATS>(S, S.shapes[ShapeIndex].MaterialIndex, Lambda, Md);
        Md.Priority = ShapeIndex;
    }
    return Md;
}

// SampleSurfaceIntegrand (basic_scatter.glsl:68-109).  The material's
// parameters are fetched once, in code shared by the types: the metal and
// translucent roughness / anisotropy (HasDirac reads the same roughness
// value) before the light choice, the reflectances after the sampled
// direction is known (a sky sample below the surface ends the path first).
template <uint32_t MATS, uint32_t CLS = 0xFFFFFFFFu>
PT_DEV bool SampleSurfaceIntegrand(const dscene& S, rng& G, pt3 Nrm, pt3 TX, pt3 TY, const bsdf_parameters& P, pt3 Out,
                                   pt3& In, pt4& Throughput, pt4& Probability)
{
    const uint32_t M = P.MaterialIndex;
    const uint32_t Type = MUint(S, M, 0);
    // CLS: the BSDF types this instantiation samples (a class-pure launch
    // compiles only its class's; the medium code still follows MATS).
    constexpr uint32_t B = MATS & CLS;
    const bool diffuse = (B & PT_MATS_DIFFUSE) && Type == PT_MATERIAL_TYPE_BASIC_DIFFUSE;
    const bool metal = (B & PT_MATS_METAL) && Type == PT_MATERIAL_TYPE_BASIC_METAL;
    const bool trans = (B & PT_MATS_TRANSLUCENT) && Type == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT;
    const bool openpbr = (B & PT_MATS_OPENPBR) && Type == PT_MATERIAL_TYPE_OPENPBR;
    bsdf_material Q;
    Q.Rough = false;
    // HasDirac (basic_metal / basic_translucent .glsl.inc: roughness < 1e-3;
    // OpenPBR: sampling only, HasDirac true).
    bool Dirac = openpbr;
    if ((B & (PT_MATS_METAL | PT_MATS_TRANSLUCENT)) && (metal || trans)) {
        const float Roughness = MaterialTexturableValue(
            S, M, metal ? PT_BASIC_METAL_ROUGHNESS : PT_BASIC_TRANSLUCENT_ROUGHNESS, P.TextureUV);
        const float Anisotropy = MaterialTexturableValue(
            S, M, metal ? PT_BASIC_METAL_ROUGHNESS_ANISOTROPY : PT_BASIC_TRANSLUCENT_ROUGHNESS_ANISOTROPY, P.TextureUV);
        Q.A = GGXRoughnessAlpha(Roughness, Anisotropy);
        Q.Rough = Q.A.x * Q.A.y > PT_EPSILON;
        Dirac = Roughness < 1e-3f;
    }
    float LightProbability = Dirac ? 0.0f : S.g.SkyboxSamplingProbability;
    pt4 MaterialPDF = v4s(0.0f);
    pt3 SMD = v3(S.g.SkyboxMeanDirection[0], S.g.SkyboxMeanDirection[1], S.g.SkyboxMeanDirection[2]);
    pt3 Mu = v3(dot(SMD, TX), dot(SMD, TY), dot(SMD, Nrm));
    bool ok;
    // Without PT_MATS_SKY the probability is +-0, so the draw (still made:
    // the RNG sequence is the reference's) never selects the light.
    const float Ul = G.R01();
    const bool light = (MATS & PT_MATS_SKY) && Ul < LightProbability;
    // A diffuse hit draws In by the light choice -- the sky lobe or the
    // material's cosine sample -- and then evaluates the material with the
    // same arguments either way (MaterialEvaluateBSDF / MaterialSampleBSDF of
    // basic_diffuse.glsl.inc), so the evaluation runs once after the join.
    //
    // The sky lobe (RandomVonMisesFisher) and the cosine lobe (RandomDirection
    // + Z) draw the same two numbers into the same spherical construction and
    // differ only in its height Z and its frame, so a wave holding both kinds
    // of lane runs the sqrt, the sine / cosine and the normalization once.
    if (light || diffuse) {
        const float Xi = G.R01();
        float Z;
        pt3 MuX = v3s(0.0f), MuY = v3s(0.0f);
        if (light) {
            ShadeMark(SM_LIGHT);
            Z = 1 + S.vmf_inv_kappa * pt_log(Xi + (1 - Xi) * S.vmf_exp_m2k);
            ComputeCoordinateFrame(Mu, MuX, MuY);
        } else {
            ShadeMark(SM_DIFFUSE_COSINE);
            Z = 2 * Xi - 1;
        }
        const float R = pt_sqrt(1 - Z * Z);
        const float Phi = G.R01() * PT_TAU;
        const pt3 D = v3(R * pt_cos(Phi), R * pt_sin(Phi), Z);
        In = SafeNormalize(light ? D.x * MuX + D.y * MuY + D.z * Mu : D + v3(0, 0, 1));
        if (light && In.z < 0.0f) { ShadeMark(SM_LIGHT_BELOW); return false; }
    }
    // Reflectances: the diffuse and metal base spectrum share a material word
    // (BASE_SPECTRUM = 1), the metal's specular spectrum; the translucent's
    // Cauchy IOR relative to the exterior on Out's side.
    if (diffuse || metal)
        Q.Refl = MaterialTexturableReflectance<MATS == PT_MATS_DIFFUSE>(S, M, PT_BASIC_METAL_BASE_SPECTRUM, P.Lambda,
                                                                        P.TextureUV);
    if (metal) Q.Aux = MaterialTexturableReflectance(S, M, PT_BASIC_METAL_SPECULAR_SPECTRUM, P.Lambda, P.TextureUV);
    if (trans) {
        pt4 Interior = CauchyEmpiricalIOR(MFloat(S, M, PT_BASIC_TRANSLUCENT_IOR),
                                          MFloat(S, M, PT_BASIC_TRANSLUCENT_ABBE_NUMBER), P.Lambda);
        if (Out.z < 0.0f) Q.Aux = Interior / P.ExteriorIOR;
        else Q.Aux = P.ExteriorIOR / Interior;
    }
    if (diffuse) {
        ShadeMark(SM_DIFFUSE_EVAL);
        ok = Diffuse_Evaluate(Q, Out, Throughput, MaterialPDF);
        if (!ok) return false;
    } else if (light) {
        // MaterialEvaluateBSDF(Parameters, Out, In, ...)
        if (metal) {
            ShadeMark(SM_METAL_EVAL);
            ok = Metal_Evaluate(Q, Out, In, Throughput, MaterialPDF);
        } else if (trans) {
            ShadeMark(SM_TRANS_EVAL);
            ok = Translucent_Evaluate(Q, Out, In, Throughput, MaterialPDF);
        } else ok = false;
        if (!ok) return false;
    } else {
        // MaterialSampleBSDF(Parameters, Out, In, ...)
        if (metal) {
            ShadeMark(SM_METAL_SAMPLE);
            ok = Metal_Sample(G, Q, Out, In, Throughput, MaterialPDF);
        } else if (trans) {
            ShadeMark(SM_TRANS_SAMPLE);
            ok = Translucent_Sample(G, Q, Out, In, Throughput, MaterialPDF);
        } else if (openpbr) {
            ShadeMark(SM_OPENPBR);
            openpbr_parameters O = OpenPBR_Parameters(S, G, P);
            ok = OpenPBR_Sample(G, O, Out, In, Throughput, MaterialPDF);
        } else {
            ok = false;
        }
        if (!ok) return false;
    }
    if (!(MATS & PT_MATS_SKY)) {
        // LightProbability = +0 and a finite sky pdf (the host's
        // PT_MATS_SKY rule): +0 * pdf + 1 * MaterialPDF = MaterialPDF + 0.
        Probability = MaterialPDF + v4s(0.0f);
        return true;
    }
    pt4 SkyboxPDF = v4s(VonMisesFisherPDF(S.g.SkyboxConcentration, vmf_consts{S.vmf_inv_kappa, S.vmf_exp_m2k, S.vmf_norm},
                                          Mu, In));
    Probability = LightProbability * SkyboxPDF + (1 - LightProbability) * MaterialPDF;
    return true;
}

}  // namespace ptd
