// cap_unscaled.h — the IEEE division and square root of the arithmetic contract without the scaling steps of hipcc's expansions.  Device code only (gfx950).
//
// hipcc expands a / b into v_div_scale x 2, v_rcp, seven FMAs, v_div_fmas, v_div_fixup (~47 SIMD cycles at the measured class costs,
// docs/experiments.md (60)).  The scale instructions only act on extreme exponents -- a denormal or huge denominator, a numerator
// below 2^-103, a quotient that would be denormal or whose exponents differ by 96 or more (CDNA ISA, V_DIV_SCALE_F32) -- and the
// fix-up only on zeros, infinities and NaNs.  Everywhere else they pass their operands through, and what remains is the sequence
// below: the same instructions on the same operands, so the same bits (29 cycles).  It is therefore ONLY called on operands known to
// be in range -- |a| = 0 or in [2^-80, 2^41], b in [2^-40, 2^41) (a sigma <= 2^38 times a tap length <= sqrt(18): the range the self-test draws from); the reconstruction chain establishes that per tile (post.hip) and
// takes the plain `/` for a tile or wave that fails: the same result by definition.  cap_debug_get(CAP_DEBUG_SELFTEST_DIV) compares both
// forms on the device, bit for bit.  The small-scene shading uses it, div2_unscaled and the square roots below on operands whose range
// follows from the contract's own arithmetic or from a property of the scene established once (cap_shade.h map_to_hemisphere_tame,
// DESIGN.md "fp32 arithmetic contract"); per-vertex range checks with a second copy of the shading body had measured slower
// (docs/experiments.md (70), (97)).
#pragma once

#include "cap_math.h"

namespace cap
{
__device__ __forceinline__ float div_unscaled(float a, float b)
{
    const float r0 = __builtin_amdgcn_rcpf(b);
    const float e0 = fmaf(-b, r0, 1.0f);
    const float r  = fmaf(e0, r0, r0);
    const float q0 = a * r;
    const float e1 = fmaf(-b, q0, a);
    const float q1 = fmaf(e1, r, q0);
    const float e2 = fmaf(-b, q1, a);
    return fmaf(e2, r, q1);
}

// a / k and b / k for one k > 0 (ortho_vector): the reciprocal and its refinement depend on k alone and are computed once; every
// operation and operand of each quotient is div_unscaled's.  That sequence loses the sign of a zero numerator (-0 * r + e = +0),
// which the IEEE quotient keeps, and unit normals out of a mesh file do hold -0: the sign of the numerator is copied onto the
// quotient -- for k > 0 it is the quotient's sign anyway.  Range: k in [2^-40, 2^41), |a| and |b| zero or in [2^-80, 2^41).
__device__ __forceinline__ void div2_unscaled(float a, float b, float k, float& qa, float& qb)
{
    const float r0 = __builtin_amdgcn_rcpf(k);
    const float e0 = fmaf(-k, r0, 1.0f);
    const float r  = fmaf(e0, r0, r0);
    auto        q  = [&](float n) {
        const float q0 = n * r;
        const float e1 = fmaf(-k, q0, n);
        const float q1 = fmaf(e1, r, q0);
        const float e2 = fmaf(-k, q1, n);
        return u2f((f2u(fmaf(e2, r, q1)) & 0x7fffffffu) | (f2u(n) & 0x80000000u));
    };
    qa = q(a), qb = q(b);
}

// sqrtf as hipcc expands it -- v_sqrt_f32, then the candidate one ulp below or above it when the residual x - s * neighbour says so
// (correctly rounded: DESIGN.md "fp32 arithmetic contract") -- without what that expansion puts around it.  The scale-in / scale-out
// pair (x * 2^32 before, * 2^-16 after) acts only for x < 2^-96; the class fix-up passes x itself through for +-0 and +inf.
//   sqrt_pos(x):      neither; x a positive normal number >= 2^-96 (never 0, inf or NaN)
//   sqrt_unscaled(x): the fix-up kept; x = 0, x = +inf or x >= 2^-96
// Inside those ranges: the same instructions on the same operands, so the same bits (cap_debug_get(CAP_DEBUG_SELFTEST_SHADE_UNARY)
// compares every float of them on the device).
__device__ __forceinline__ float sqrt_pos(float x)
{
    const float s  = __builtin_amdgcn_sqrtf(x);
    const float dn = u2f(f2u(s) - 1u), up = u2f(f2u(s) + 1u);
    const float vp = fmaf(-dn, s, x), vs = fmaf(-up, s, x);
    float       r  = vp <= 0.0f ? dn : s;
    r              = vs > 0.0f ? up : r;
    return r;
}
__device__ __forceinline__ float sqrt_unscaled(float x)
{
    const float r = sqrt_pos(x);
    return (x == 0.0f || x == __builtin_inff()) ? x : r;
}
}  // namespace cap
