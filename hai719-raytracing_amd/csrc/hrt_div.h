// Exact fp32 division by a divisor whose reciprocal is already known: a reciprocal and two FMAs instead of an IEEE division.
//
// Plain C++ (no HIP types): the streaming kernels include it as device code, tests/div/div_check.cpp as host code under the
// sanitizers.  Compile with -ffp-contract=off; the FMAs below are explicit.
//
// THE SEQUENCE (Markstein; Brisebarre, Muller, Raina 2004 for a divisor known in advance).  With y = RN(1 / c),
//     q0 = RN(a * y)      r = fma(-q0, c, a)      q = fma(r, y, q0)
// gives q = RN(a / c) in round-to-nearest whenever r is exact and nothing under- or overflows.  The theorem leaves out divisors
// whose significand is all ones; that one significand is checked against `/` for every numerator (tests/test_div_known.py).
//
// THE WINDOW, stated once.  Numerator and divisor must have their magnitude in [2^-60, 2^61) (an exponent window; a numerator may
// also be +-0).  Then
//   y   = RN(1 / c) lies in (2^-61, 2^60]: normal;
//   q0, q lie in (2^-121, 2^121): normal, so neither is rounded twice;
//   r   = a - q0 c is a multiple of ulp(q0) ulp(c) > 2^-48 |a| >= 2^-108, and q0 is within one ulp of a / c (the paper's
//         property 2), so |r| < ulp(q0) |c| < 2^24 ulp(q0) ulp(c): at most 24 significant bits, all above 2^-149 -- the FMA
//         returns it exactly.
// A zero numerator goes through the same three instructions: q0 = a * y is the correctly signed zero, r = +0, and q = +0 * y + q0
// would lose the sign of -0 -- the last step therefore takes the sign of q0, which is the quotient's sign for every input (a
// correctly rounded normal quotient never changes sign).  Everything else -- tiny, huge, infinite, NaN -- is divided by `/`.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define HRT_DIV_FN __host__ __device__ __forceinline__
#else
#define HRT_DIV_FN static inline
#endif

namespace hrtdiv {

#define HRT_DIV_LO 0x1p-60f
#define HRT_DIV_HI 0x1p61f

// |x| in [2^-60, 2^61); false for NaN
HRT_DIV_FN bool in_window(float x) {
    const float ax = __builtin_fabsf(x);
    return ax >= HRT_DIV_LO && ax < HRT_DIV_HI;
}
// ... or +-0: what a numerator may be
HRT_DIV_FN bool num_ok(float a) {
    const float aa = __builtin_fabsf(a);
    return (aa >= HRT_DIV_LO || aa == 0.f) && aa < HRT_DIV_HI;
}

// The three instructions, unguarded: the caller has checked num_ok(a) and in_window(c), and y == 1.f / c.
HRT_DIV_FN float div_known_core(float a, float c, float y) {
    const float q0 = a * y;
    const float r = __builtin_fmaf(-q0, c, a);
    return __builtin_copysignf(__builtin_fmaf(r, y, q0), q0);
}
// ... for a numerator that is not zero: the quotient's sign needs no care
HRT_DIV_FN float div_known_core_nz(float a, float c, float y) {
    const float q0 = a * y;
    return __builtin_fmaf(__builtin_fmaf(-q0, c, a), y, q0);
}

// a / c, bit for bit, given y == 1.f / c (IEEE).  The fallback is rare at wave level: no ray of a frame has a component outside the
// window.  (`&`, not `&&`: one branch, not a chain of them.)
HRT_DIV_FN float div_known(float a, float c, float y) {
    if (!(num_ok(a) & in_window(c))) return a / c;
    return div_known_core(a, c, y);
}

// Guards shared by several quotients: every magnitude in the window, by their smallest and their largest.  A zero fails and is
// left to `/` -- exact zeros are rare among the hot path's numerators.  fmin / fmax skip a NaN, so a NaN beside an ordinary value
// passes: the three instructions then return NaN, as `/` does.
HRT_DIV_FN bool in_window2(float a, float b) {
    const float aa = __builtin_fabsf(a), ab = __builtin_fabsf(b);
    return (__builtin_fminf(aa, ab) >= HRT_DIV_LO) & (__builtin_fmaxf(aa, ab) < HRT_DIV_HI);
}

// a1 / c1 and a2 / c2 under ONE guard (the square's two projections, then its u and v: hrt_kernels.hip quad_t_rcp)
HRT_DIV_FN void div_known_pair(float a1, float c1, float y1, float a2, float c2, float y2, float &o1, float &o2) {
    if (in_window2(a1, a2) & in_window2(c1, c2)) {
        o1 = div_known_core_nz(a1, c1, y1);
        o2 = div_known_core_nz(a2, c2, y2);
    } else {
        o1 = a1 / c1;
        o2 = a2 / c2;
    }
}

// (x, y, z) / L with L = sqrtf(x x + y y + z z) in Vec3.h's order: one IEEE division and three quotients by its result.
// L >= every |component|, so the smallest component bounds everything from below and L everything from above (L is inf or NaN
// when a component is, and then fails its compare).
HRT_DIV_FN void normalize_shared(float x, float y, float z, float &ox, float &oy, float &oz) {
    const float L = __builtin_sqrtf(x * x + y * y + z * z);
    const float m = __builtin_fminf(__builtin_fminf(__builtin_fabsf(x), __builtin_fabsf(y)), __builtin_fabsf(z));
    if ((m >= HRT_DIV_LO) & (L < HRT_DIV_HI)) {
        const float inv = 1.f / L;
        ox = div_known_core_nz(x, L, inv);
        oy = div_known_core_nz(y, L, inv);
        oz = div_known_core_nz(z, L, inv);
    } else {
        ox = x / L; oy = y / L; oz = z / L;
    }
}

}  // namespace hrtdiv
