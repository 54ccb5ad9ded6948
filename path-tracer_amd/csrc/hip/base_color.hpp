// base_color.hpp — a hit's base colour as the preview shows it
// (preview_render.glsl:110-121): MaterialBaseColor observed under D65 and
// taken to linear sRGB.  Shared by the preview kernel (preview.hip) and the
// denoiser's guide kernel (denoise.hip); the observe table is filled by
// pt_launch_observe_table (preview.hip).
#pragma once

#include "pt_device.hpp"
#include "kernels.hpp"

namespace ptd {

// ObserveParametricSpectrumUnderD65 (spectrum.glsl.inc:194-208), 16 samples.
// Everything but the spectrum itself -- each sample's wavelength, D65 weight
// and CIE observer value -- depends on the sample index only, so
// observe_table_kernel (preview.hip) evaluates the 16 samples once per preview
// context or guides object and every observation reads them (uniform index: scalar loads): the same
// functions on the same operands give the same bits, and the 7 exponentials
// of each observer value leave the per-pixel path.
constexpr int OBSERVE_SAMPLES = 16;
struct observe_table {
    float D[OBSERVE_SAMPLES], Lambda[OBSERVE_SAMPLES];
    pt3 Obs[OBSERVE_SAMPLES];
};

static_assert(sizeof(observe_table) == PT_OBSERVE_TABLE_FLOATS * 4, "observe_table size");

PT_DEV pt3 ObserveUnderD65(const observe_table& T, pt4 BetaAndIntensity)
{
    const float DeltaLambda = (PT_CIE_LAMBDA_MAX - PT_CIE_LAMBDA_MIN) / OBSERVE_SAMPLES;
    pt3 Color = v3s(0);
    pt3 Beta = v3(BetaAndIntensity.x, BetaAndIntensity.y, BetaAndIntensity.z);
    for (int I = 0; I < OBSERVE_SAMPLES; I++) {
        float Sp = BetaAndIntensity.w * SampleParametricSpectrum(Beta, T.Lambda[I]);
        Color = Color + Sp * T.D[I] * T.Obs[I] * DeltaLambda;
    }
    return Color;
}

PT_DEV pt3 ObserveUnderD65(const observe_table& T, pt3 Beta) { return ObserveUnderD65(T, v4(Beta.x, Beta.y, Beta.z, 1)); }

// MaterialBaseColor (scene.glsl.inc:254-274,696-701 + *_BaseColor)
PT_DEV pt3 MaterialBaseColor(const dscene& S, const observe_table& Tb, uint32_t M, pt2 UV)
{
    uint32_t Type = MUint(S, M, 0);
    uint32_t A;
    if (Type == PT_MATERIAL_TYPE_BASIC_DIFFUSE) A = PT_BASIC_DIFFUSE_BASE_SPECTRUM;
    else if (Type == PT_MATERIAL_TYPE_BASIC_METAL) A = PT_BASIC_METAL_BASE_SPECTRUM;
    else if (Type == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT) return ObserveUnderD65(Tb, MVec3(S, M, PT_BASIC_TRANSLUCENT_TRANSMISSION_SPECTRUM));
    else return v3s(0);
    pt3 Color = ObserveUnderD65(Tb, MVec3(S, M, A));
    uint32_t TextureIndex = MUint(S, M, A + 3);
    if (TextureIndex != TEXTURE_INDEX_NONE) {
        pt4 T = SampleTexture(S, TextureIndex, UV);
        Color = Color * ObserveUnderD65(Tb, v3(T.x, T.y, T.z));
    }
    return Color;
}

PT_DEV pt3 XYZToSRGB(pt3 V)                                            // CIE_XYZ_TO_SRGB * V (spectrum.glsl.inc:50-55)
{
    return v3(+3.2406f * V.x + -1.5372f * V.y + -0.4986f * V.z,
              -0.9689f * V.x + +1.8758f * V.y + +0.0415f * V.z,
              +0.0557f * V.x + -0.2040f * V.y + +1.0570f * V.z);
}

}  // namespace ptd
