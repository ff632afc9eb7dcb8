// The cell of a probe volume (include/hrt.h "Probe volumes", steps 1-3 of THE RULE): for one point record {P, time, N, bias} the
// eight probes round it and their final weights, as a pure function.
//
// This is the one implementation of those steps: hrt_probe_eval_kernel calls it on the device, hrt_probe_volume_weights on the
// host, and tests/probe_volume/probe_volume_check.cpp in a program of its own under the host sanitizers.  Nothing here touches a
// device, a global or the environment.  All arithmetic is fp32 in the order include/hrt.h writes, without fused multiply-add
// (tests/probe_volume_ref.py states it again in NumPy); only + - * /, sqrtf, floorf, fminf and fmaxf are used.
#pragma once

#include "../../include/hrt.h"
#include "hrt_probe_depth_oct.h"

#include <cmath>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define HRT_PV_HD __host__ __device__ __forceinline__
#else
#define HRT_PV_HD inline
#endif

namespace probevol {

// The grid of a volume as the kernels take it, by value: the box, the counts and, per axis, s = (float)n / (hi - lo).
struct Grid {
    float lo[3], hi[3], s[3];
    uint32_t n[3];
};

inline int refuse(std::string &error, const std::string &msg) {
    error = msg;
    return HRT_ERR_INVALID;
}

// The checks of hrt_probe_volume_create on the grid alone, in the header's order, and the Grid they admit.
inline int make_grid(const std::string &who, const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, Grid &g, std::string &error) {
#pragma clang fp contract(off)
    if (!lo) return refuse(error, who + ": lo is NULL");
    if (!hi) return refuse(error, who + ": hi is NULL");
    if (nx == 0u || ny == 0u || nz == 0u) return refuse(error, who + ": nx, ny and nz must be positive");
    // nx * ny <= 2^64 - 2^33 + 1 cannot wrap; the product with nz is compared by division
    if ((uint64_t)nx * ny > (uint64_t)HRT_PROBE_VOLUME_MAX / nz)
        return refuse(error, who + ": nx * ny * nz must be at most HRT_PROBE_VOLUME_MAX = " + std::to_string(HRT_PROBE_VOLUME_MAX));
    const uint32_t count[3] = {nx, ny, nz};
    const char *axis[3] = {"x", "y", "z"};
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a])) return refuse(error, who + ": lo must be finite");
        if (!std::isfinite(hi[a])) return refuse(error, who + ": hi must be finite");
    }
    for (int a = 0; a < 3; ++a) {
        const float e = hi[a] - lo[a];
        g.lo[a] = lo[a];
        g.hi[a] = hi[a];
        g.n[a] = count[a];
        g.s[a] = 0.f;  // not used on an axis with one probe
        if (count[a] == 1u) continue;
        if (e == 0.f) return refuse(error, who + ": lo == hi on axis " + axis[a] + ", which has more than one probe");
        g.s[a] = (float)count[a] / e;
        if (!std::isfinite(g.s[a])) return refuse(error, who + ": the box is too thin on axis " + axis[a] + ": n / (hi - lo) is not finite");
    }
    return HRT_OK;
}

HRT_PV_HD bool finite(float v) { return __builtin_isfinite(v); }

// The rule comes in four pieces, so that the device may hand the corners of a point to different lanes; cell() below composes them
// for one caller, and is what the host and the lane-per-point kernel use.

// The degenerate test and Nn = normalize(N).  false for a degenerate point, whose Nn is 0.
HRT_PV_HD bool normal(const float P[3], const float N[3], float Nn[3]) {
#pragma clang fp contract(off)
    Nn[0] = Nn[1] = Nn[2] = 0.f;
    if (!(finite(P[0]) && finite(P[1]) && finite(P[2]) && finite(N[0]) && finite(N[1]) && finite(N[2]))) return false;
    if (N[0] == 0.f && N[1] == 0.f && N[2] == 0.f) return false;
    const float L = sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);  // normalize: the trace path's own, divide by the length
    const float x = N[0] / L, y = N[1] / L, z = N[2] / L;
    if (!(finite(x) && finite(y) && finite(z))) return false;
    Nn[0] = x;
    Nn[1] = y;
    Nn[2] = z;
    return true;
}

// Step 1: per axis the two probe coordinates and the fraction between them.
struct Axes {
    uint32_t i0[3], i1[3];
    float f[3];
};
HRT_PV_HD void axes(const Grid &g, const float P[3], Axes &ax) {
#pragma clang fp contract(off)
    for (int a = 0; a < 3; ++a) {
        ax.i0[a] = ax.i1[a] = 0u;
        ax.f[a] = 0.f;
        if (g.n[a] == 1u) continue;
        const float top = (float)(g.n[a] - 1u);
        const float x = fminf(fmaxf((P[a] - g.lo[a]) * g.s[a] - .5f, 0.f), top);  // in [0, n - 1] whatever the product is
        ax.i0[a] = (uint32_t)floorf(x);
        if (ax.i0[a] > g.n[a] - 1u) ax.i0[a] = g.n[a] - 1u;  // never taken (x is in range); keeps every index inside the grid by construction
        ax.f[a] = x - (float)ax.i0[a];
        ax.i1[a] = ax.i0[a] + 1u < g.n[a] - 1u ? ax.i0[a] + 1u : g.n[a] - 1u;
    }
}

// Steps 2 and 3 up to the division by W, for corner m (bit 0 of m: x, bit 1: y, bit 2: z): its probe and its weight.
HRT_PV_HD float corner(const Grid &g, const Axes &ax, const float P[3], const float Nn[3], uint32_t flags, uint32_t m, uint32_t &index) {
#pragma clang fp contract(off)
    const uint32_t c[3] = {(m & 1u) ? ax.i1[0] : ax.i0[0], (m & 2u) ? ax.i1[1] : ax.i0[1], (m & 4u) ? ax.i1[2] : ax.i0[2]};
    const float wx = (m & 1u) ? ax.f[0] : 1.f - ax.f[0], wy = (m & 2u) ? ax.f[1] : 1.f - ax.f[1], wz = (m & 4u) ? ax.f[2] : 1.f - ax.f[2];
    index = (c[2] * g.n[1] + c[1]) * g.n[0] + c[0];  // below nx * ny * nz <= HRT_PROBE_VOLUME_MAX
    float w = (wx * wy) * wz;
    if (flags & HRT_PROBE_EVAL_FACING) {
        float v[3];
        for (int a = 0; a < 3; ++a) {
            const float centre = g.lo[a] + (((float)c[a] + .5f) / (float)g.n[a]) * (g.hi[a] - g.lo[a]);
            v[a] = centre - P[a];
        }
        const float l = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        const float cs = l > 0.f ? ((v[0] * Nn[0] + v[1] * Nn[1]) + v[2] * Nn[2]) / l : 0.f;
        const float t = (cs + 1.f) * .5f;
        w = w * (t * t + .2f);
    }
    return w;
}

// Step 3's W: the eight weights added in ascending order.
HRT_PV_HD float total(const float w[8]) {
#pragma clang fp contract(off)
    return ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) + w[7];
}

// Steps 1-3 for the point P with normal N (six floats that may hold anything).  false for a degenerate point: index and weight
// are then zeroed and Nn is 0.  Otherwise index[m] is the probe of corner m, weight[m] its final weight and Nn the normalised
// normal.
HRT_PV_HD bool cell(const Grid &g, const float P[3], const float N[3], uint32_t flags, uint32_t index[8], float weight[8], float Nn[3]) {
#pragma clang fp contract(off)
    for (int m = 0; m < 8; ++m) {
        index[m] = 0u;
        weight[m] = 0.f;
    }
    if (!normal(P, N, Nn)) return false;
    Axes ax;
    axes(g, P, ax);
    for (uint32_t m = 0; m < 8u; ++m) weight[m] = corner(g, ax, P, Nn, flags, m, index[m]);
    if (flags & HRT_PROBE_EVAL_FACING) {
        const float W = total(weight);
        for (int m = 0; m < 8; ++m) weight[m] = weight[m] / W;
    }
    return true;
}

// ---- The visible look-up (include/hrt.h "Probe visibility"): step 3 with the visibility factor.  The pieces again, so that the
// device may hand the corners to different lanes, and cell_visible() that composes them for the host.

// Pb = P + b * Nn.  false when b is not finite: the point is degenerate.
HRT_PV_HD bool biased(const float P[3], const float Nn[3], float b, float Pb[3]) {
#pragma clang fp contract(off)
    for (int a = 0; a < 3; ++a) Pb[a] = P[a] + b * Nn[a];
    return finite(b);
}

// Step 3 (b) up to the load, for corner m: l = |Pb - C_m| and, where l > 0, the texel of the corner's depth map that looks at Pb
// (0 otherwise: it is not read).
HRT_PV_HD float toward(const Grid &g, const Axes &ax, const float Pb[3], uint32_t m, uint32_t &texel) {
#pragma clang fp contract(off)
    const uint32_t c[3] = {(m & 1u) ? ax.i1[0] : ax.i0[0], (m & 2u) ? ax.i1[1] : ax.i0[1], (m & 4u) ? ax.i1[2] : ax.i0[2]};
    float v[3];
    for (int a = 0; a < 3; ++a) {
        const float centre = g.lo[a] + (((float)c[a] + .5f) / (float)g.n[a]) * (g.hi[a] - g.lo[a]);
        v[a] = Pb[a] - centre;
    }
    const float l = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    texel = l > 0.f ? probedepth::texel(v) : 0u;
    return l;
}

// Steps 1-3 of the visible look-up for the record {P, N, b}; `moments` holds HRT_PROBE_DEPTH_TEXELS pairs {m1, m2} per probe.
// false for a degenerate point, as cell().
HRT_PV_HD bool cell_visible(const Grid &g, const float P[3], const float N[3], float b, uint32_t flags, const float *moments, uint32_t index[8],
                            float weight[8], float Nn[3]) {
#pragma clang fp contract(off)
    for (int m = 0; m < 8; ++m) {
        index[m] = 0u;
        weight[m] = 0.f;
    }
    float Pb[3];
    if (!normal(P, N, Nn)) return false;
    if (!biased(P, Nn, b, Pb)) {
        Nn[0] = Nn[1] = Nn[2] = 0.f;
        return false;
    }
    Axes ax;
    axes(g, P, ax);
    for (uint32_t m = 0; m < 8u; ++m) {
        weight[m] = corner(g, ax, P, Nn, flags, m, index[m]);
        uint32_t texel;
        const float l = toward(g, ax, Pb, m, texel);
        const float *mm = moments + 2u * ((size_t)index[m] * HRT_PROBE_DEPTH_TEXELS + texel);
        weight[m] = weight[m] * probedepth::visibility(l, mm[0], mm[1]);
    }
    const float W = total(weight);
    for (int m = 0; m < 8; ++m) weight[m] = weight[m] / W;
    return true;
}

}  // namespace probevol
