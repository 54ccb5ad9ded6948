/*
 * pt_guides.h — denoise guides that follow perfect mirrors and smooth glass
 * to the surface a pixel shows (definition in DESIGN.md §6 row 13), written
 * once for the device kernel (csrc/hip/denoise.hip, guides_kernel's SPECULAR
 * instantiation) and restated in numpy (tests/specular_guides_restatement.py)
 * under pt_fp.h's convention: IEEE binary32, no contraction, sums left to
 * right, pt_sqrt.  Per-hit arithmetic only: the trace, the hit's attributes,
 * the read of the material's words and the store of the record are the
 * caller's.
 *
 * A pixel's chain starts as ptRenderDenoiseGuides' ray does
 * (pt_reproject_central_ray) with b = 0, tag = 0.  Per hit of shape s at time
 * t along (O, V), with the record's N and TX after their packed round trip:
 *
 *   total  = t at the first hit, total + t after it      (pt_guide_total)
 *   followed iff b < max_bounces and the material is a basic metal or a basic
 *          translucent whose texturable roughness at the hit's UV is < 1e-3,
 *          the integrator's HasDirac                     (pt_guide_followed)
 *   not followed: the record is {N, total, base colour, tag << 16 | s}
 *                                                        (pt_guide_shape_word)
 *   followed: tag = s + 1 if it was 0                    (pt_guide_tag);
 *          W, the direction the surface sends V on       (pt_guide_direction);
 *          O' = (O + t V) + 1e-3 W, V' = unpack(pack(W)) (pt_guide_restart);
 *          b = b + 1.
 *
 * A miss writes the miss record with the sky's colour along the current V and
 * no tag.  The first total is t itself and not 0 + t, so that a hit time of
 * -0 keeps its sign and max_bounces = 0 has ptRenderDenoiseGuides' bits on
 * every input.
 *
 * pt_guide_direction, in this order:
 *   TY  = cross(N, TX)
 *   Out = (-dot(V, TX), -dot(V, TY), -dot(V, N)),  c = Out.z
 *   metal:        In = (-Out.x, -Out.y, Out.z)
 *   translucent:  rel = Out.z < 0 ? eta : 1 / eta   (eta: the Cauchy base
 *                 index, exterior 1, no wavelength)
 *                 k = 1 - (rel * rel) * (1 - c * c)
 *                 !(k > 0): the metal's In (total internal reflection; a NaN
 *                 k, from a NaN normal or index, lands here too)
 *                 else cr = -sign(c) * pt_sqrt(k),
 *                      In = (-rel * Out.x, -rel * Out.y, cr)
 *   W   = (In.x * TX + In.y * TY) + In.z * N
 * The translucent In is the integrator's refracted direction
 * (basic_translucent: (cr + rel c) n - rel Out with the micro-normal
 * n = (0, 0, 1)), without its Fresnel draw: glass always transmits.
 *
 * At c = 0 exactly sign(c) is 0, so cr = 0 and a refracted W is tangential
 * with length rel, not 1; V' is normalised by its packed round trip, and O'
 * moves by 1e-3 rel along the surface.
 *
 * Nothing here traps or leaves the float domain on any input: a zero or NaN
 * normal gives a zero or NaN W, whose packed form is still a defined word
 * (pt_pack_snorm16 clamps through minNum / maxNum, which drop a NaN).
 */
#ifndef PT_GUIDES_H
#define PT_GUIDES_H

#include "pt_fp.h"
#include "pt_glsl.h"
#include "pt_packed.h"
#include "pt_reproject.h"

#ifndef PT_GUIDE_MAX_BOUNCES
#define PT_GUIDE_MAX_BOUNCES 8   /* pt_api.h has it too */
#endif
/* HasDirac's bound (basic_metal / basic_translucent .glsl.inc). */
#define PT_GUIDE_DIRAC_ROUGHNESS 1e-3f
/* basic_scatter.glsl's restart offset along the new direction. */
#define PT_GUIDE_RESTART_OFFSET 1e-3f

/* A material type whose roughness decides: the caller reads the roughness
 * word (pt_guide_roughness_word) only for these. */
PT_HD int pt_guide_candidate(uint32_t type)
{
    return type == PT_MATERIAL_TYPE_BASIC_METAL || type == PT_MATERIAL_TYPE_BASIC_TRANSLUCENT;
}

PT_HD uint32_t pt_guide_roughness_word(uint32_t type)
{
    return type == PT_MATERIAL_TYPE_BASIC_METAL ? PT_BASIC_METAL_ROUGHNESS : PT_BASIC_TRANSLUCENT_ROUGHNESS;
}

/* roughness: MaterialTexturableValue of the roughness word at the hit's UV;
 * not read for a type that is no candidate.  A NaN roughness is not < 1e-3. */
PT_HD int pt_guide_followed(uint32_t type, float roughness, uint32_t b, uint32_t max_bounces)
{
    return b < max_bounces && pt_guide_candidate(type) && roughness < PT_GUIDE_DIRAC_ROUGHNESS;
}

PT_HD float pt_guide_total(float total, float t, uint32_t b) { return b == 0u ? t : total + t; }

/* The first followed shape, + 1; shape indices fit 16 bits (the hit record
 * is shape << 16 | material). */
PT_HD uint32_t pt_guide_tag(uint32_t tag, uint32_t shape) { return tag == 0u ? shape + 1u : tag; }

PT_HD uint32_t pt_guide_shape_word(uint32_t tag, uint32_t shape) { return (tag << 16) | shape; }

/* In, in the hit's frame, for Out = -V in that frame.  eta is read for the
 * translucent type only. */
PT_HD pt3 pt_guide_in(uint32_t type, float eta, pt3 Out)
{
    const pt3 Mirror = v3(-Out.x, -Out.y, Out.z);
    if (type != PT_MATERIAL_TYPE_BASIC_TRANSLUCENT) return Mirror;
    const float c = Out.z;
    const float rel = Out.z < 0.0f ? eta : 1.0f / eta;
    const float k = 1.0f - (rel * rel) * (1.0f - c * c);
    if (!(k > 0.0f)) return Mirror;
    const float cr = -pt_sign(c) * pt_sqrt(k);
    return v3(-rel * Out.x, -rel * Out.y, cr);
}

/* W: the world direction a followed hit sends the ray on. */
PT_HD pt3 pt_guide_direction(uint32_t type, float eta, pt3 N, pt3 TX, pt3 V)
{
    const pt3 TY = cross(N, TX);
    const pt3 Out = v3(-dot(V, TX), -dot(V, TY), -dot(V, N));
    const pt3 In = pt_guide_in(type, eta, Out);
    return (In.x * TX + In.y * TY) + In.z * N;
}

/* basic_scatter.glsl's new ray, with the packed velocity's round trip. */
PT_HD void pt_guide_restart(pt3* O, pt3* V, float t, pt3 W)
{
    const pt3 Pos = *O + t * *V;
    *O = Pos + PT_GUIDE_RESTART_OFFSET * W;
    *V = pt_reproject_unpack_unit(pt_reproject_pack_unit(W));
}

#endif /* PT_GUIDES_H */
