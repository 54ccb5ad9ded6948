/*
 * pt_facetest.h — the two predicates of the lean face test (FaceTest,
 * path-tracer_amd/csrc/hip/traverse.hpp; DESIGN.md §4 "Lean extend").
 *
 * IntersectMeshFace (scene.glsl.inc:304-334) leaves a face by seven early
 * returns; no value depends on which of them fired, so the device evaluates
 * every quantity and forms one miss flag.  This header holds that flag in its
 * folded form and the gate of the fast reciprocal, in plain C++ like pt_fp.h:
 * the device code calls them, and the host library exposes them (ptsFaceTest)
 * so that tests/test_face_predicate.py can hold them against the seven-term
 * form on any operands without a GPU.
 */
#ifndef PT_FACETEST_H
#define PT_FACETEST_H

#include "pt_fp.h"

/* The miss flag of a face test with determinant Det, coordinates U, W and
 * time T against the hit time so far:
 *
 *   |Det| < eps | U < 0 | U > 1 | W < 0 | U + W > 1 | T < 0 | T > Time
 *
 * in four compares.  minNum / maxNum drop a NaN operand, as an ordered compare
 * with a NaN is false: any term below zero makes the minimum negative, and a
 * minimum that is negative is one of the terms; likewise for the maximum
 * against 1.  The zeros' order in the minimum does not matter (neither is
 * below zero).  U + W is the reference's single addition. */
PT_HD int pt_face_miss(float Det, float U, float W, float T, float Time)
{
    const float lo = pt_min(pt_min(U, W), T);
    const float hi = pt_max(U, U + W);
    return (pt_abs(Det) < PT_EPSILON) | (lo < 0.0f) | (hi > 1.0f) | (T > Time);
}

/* The range over which the fast reciprocal (FastRcp, pt_device.hpp: the
 * hardware reciprocal and one Newton step) is the IEEE quotient bit for bit:
 * PT_FAST_RCP_MIN <= |d| < PT_FAST_RCP_MAX.  The one statement of it: the
 * device's exhaustive check (FastRcpRange, ptCheckFastReciprocal) and the gate
 * below both read these. */
#define PT_FAST_RCP_MIN 0x1p-126f
#define PT_FAST_RCP_MAX 0x1p126f

/* Whether 1 / Det has to come from the IEEE division: the fast reciprocal
 * (one hardware reciprocal and one Newton step, FastRcp) equals it bit for
 * bit inside the range above.  Below it |Det| < PT_EPSILON (1e-9 > 2^-126): the
 * face is missed whatever the quotient, which is then never read.  What is
 * left is the huge and the NaN. */
PT_HD int pt_face_needs_division(float Det)
{
    return !(pt_abs(Det) < PT_FAST_RCP_MAX);
}

#endif /* PT_FACETEST_H */
