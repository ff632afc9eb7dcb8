// The octahedral depth map of a probe (include/hrt.h "Probe visibility"): the centre direction of a texel and the texel of a
// vector, as pure functions.
//
// This is the one implementation of both: hrt_probe_depth_kernel (the filter's centres) and hrt_probe_eval_visible_kernel (the
// texel a point is seen through) call it on the device, hrt_probe_depth_direction and hrt_probe_depth_texel on the host, and
// tests/probe_depth/probe_depth_check.cpp in a program of its own under the host sanitizers.  Nothing here touches a device, a
// global or the environment.  All arithmetic is fp32 in the order include/hrt.h writes, without fused multiply-add
// (tests/probe_depth_ref.py states it again in NumPy); only + - * /, sqrtf, floorf, fabsf, fminf and fmaxf are used.
#pragma once

#include "../../include/hrt.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HRT_PD_HD __host__ __device__ __forceinline__
#else
#define HRT_PD_HD inline
#endif

namespace probedepth {

HRT_PD_HD float sg(float v) { return v >= 0.f ? 1.f : -1.f; }

// The fold of the lower hemisphere, from the old pair.
HRT_PD_HD void fold(float &px, float &py) {
#pragma clang fp contract(off)
    const float ox = px, oy = py;
    px = (1.f - fabsf(oy)) * sg(ox);
    py = (1.f - fabsf(ox)) * sg(oy);
}

// The centre direction c_e of texel e = 8 j + i (e < HRT_PROBE_DEPTH_TEXELS): a unit vector.
HRT_PD_HD void direction(uint32_t e, float c[3]) {
#pragma clang fp contract(off)
    const uint32_t i = e % HRT_PROBE_DEPTH_RES, j = e / HRT_PROBE_DEPTH_RES;
    float px = ((float)i + .5f) * .25f - 1.f, py = ((float)j + .5f) * .25f - 1.f;
    const float z = (1.f - fabsf(px)) - fabsf(py);
    if (z < 0.f) fold(px, py);
    const float L = sqrtf((px * px + py * py) + z * z);  // normalize: the trace path's own, divide by the length
    c[0] = px / L;
    c[1] = py / L;
    c[2] = z / L;
}

// One coordinate of the square [-1, 1] as a texel coordinate in 0 .. HRT_PROBE_DEPTH_RES - 1, whatever p holds (a NaN gives 0).
HRT_PD_HD uint32_t coord(float p) {
#pragma clang fp contract(off)
    return (uint32_t)fminf(fmaxf(floorf((p * .5f + .5f) * (float)HRT_PROBE_DEPTH_RES), 0.f), (float)(HRT_PROBE_DEPTH_RES - 1u));
}

// The texel of the vector v != 0, which need not be unit.  Below HRT_PROBE_DEPTH_TEXELS whatever v holds.
HRT_PD_HD uint32_t texel(const float v[3]) {
#pragma clang fp contract(off)
    const float s = (fabsf(v[0]) + fabsf(v[1])) + fabsf(v[2]);
    float px = v[0] / s, py = v[1] / s;
    if (v[2] < 0.f) fold(px, py);
    return HRT_PROBE_DEPTH_RES * coord(py) + coord(px);
}

// Step 3 (b) of the visible look-up for one corner: the Chebyshev weight of a point l away from a probe whose texel towards it
// holds the moments {m1, m2}.
HRT_PD_HD float visibility(float l, float m1, float m2) {
#pragma clang fp contract(off)
    if (!(l > 0.f)) return 1.f;
    if (l <= m1) return 1.f;
    const float var = fmaxf(m2 - m1 * m1, 0.f), q = l - m1;
    const float c = var / (var + q * q);
    return fmaxf((c * c) * c, .001f);
}

}  // namespace probedepth
