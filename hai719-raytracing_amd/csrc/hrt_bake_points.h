// Bake points on the host (include/hrt.h "Baking": hrt_bake_quad_points, hrt_bake_mesh_points): the point records of a
// lightmap over a quad and of the vertices of a triangle mesh, as pure functions.
//
// Nothing here touches a device, a global or the environment: hrt_bake.hip wraps the two functions for the C ABI, and
// tests/bake/bake_check.cpp calls them in a program of its own under the host sanitizers.  All arithmetic is fp32 in the
// order include/hrt.h writes, without fused multiply-add (tests/bake_ref.py states it again in NumPy).
#pragma once

#include "../../include/hrt.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace bakepts {

struct V3 { float x, y, z; };
inline V3 sub(V3 a, V3 b) {
#pragma clang fp contract(off)
    return V3{a.x - b.x, a.y - b.y, a.z - b.z};
}
inline V3 cross(V3 a, V3 b) {
#pragma clang fp contract(off)
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
inline V3 normalize(V3 a) {  // the trace path's: divide by the length, no guard
#pragma clang fp contract(off)
    const float L = std::sqrt((a.x * a.x + a.y * a.y) + a.z * a.z);
    return V3{a.x / L, a.y / L, a.z / L};
}
inline V3 at(const float *p) { return V3{p[0], p[1], p[2]}; }

inline int refuse(std::string &error, const std::string &msg) {
    error = msg;
    return HRT_ERR_INVALID;
}

inline void record(float *r, V3 P, float time, V3 N, float bias) {
    r[0] = P.x; r[1] = P.y; r[2] = P.z; r[3] = time;
    r[4] = N.x; r[5] = N.y; r[6] = N.z; r[7] = bias;
}

// tw x th records, row-major: texel (i, j) at index j * tw + i, at the texel's centre, N = side * the quad's normal.
inline int quad_points(const hrt_quad *q, uint32_t tw, uint32_t th, int32_t side, float time, float bias, float *out, std::string &error) {
#pragma clang fp contract(off)
    const std::string who = "hrt_bake_quad_points";
    if (!q) return refuse(error, who + ": quad is NULL");
    if (!out) return refuse(error, who + ": out_points is NULL");
    if (tw == 0u || th == 0u) return refuse(error, who + ": tw and th must be positive");
    if ((uint64_t)tw * th > 0x7fffffffull)
        return refuse(error, who + ": tw * th must be at most 2^31 - 1 (got " + std::to_string((uint64_t)tw * th) + ")");
    if (side != 1 && side != -1) return refuse(error, who + ": side must be +1 or -1 (got " + std::to_string(side) + ")");
    if (!std::isfinite(time)) return refuse(error, who + ": time must be finite");
    if (!std::isfinite(bias)) return refuse(error, who + ": bias must be finite");
    const V3 v0 = at(q->v0), R = sub(at(q->v1), v0), U = sub(at(q->v3), v0);
    const V3 n = normalize(cross(R, U));
    const float sd = (float)side;
    const V3 N{sd * n.x, sd * n.y, sd * n.z};
    for (uint32_t j = 0; j < th; ++j) {
        const float fv = ((float)j + .5f) / (float)th;
        for (uint32_t i = 0; i < tw; ++i) {
            const float fu = ((float)i + .5f) / (float)tw;
            const V3 P{(v0.x + fu * R.x) + fv * U.x, (v0.y + fu * R.y) + fv * U.y, (v0.z + fu * R.z) + fv * U.z};
            record(out + ((size_t)j * tw + i) * HRT_RAY_FLOATS, P, time, N, bias);
        }
    }
    return HRT_OK;
}

// One record per vertex: N the sum of cross(p1 - p0, p2 - p0) over the triangles that use it, in ascending triangle order,
// left unnormalised; 0 for a vertex no triangle uses.
inline int mesh_points(const float *positions, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, float time, float bias,
                       float *out, std::string &error) {
#pragma clang fp contract(off)
    const std::string who = "hrt_bake_mesh_points";
    if (n_vertices != 0u && !positions) return refuse(error, who + ": positions is NULL");
    if (n_triangles != 0u && !indices) return refuse(error, who + ": indices is NULL");
    if (n_vertices != 0u && !out) return refuse(error, who + ": out_points is NULL");
    if (!std::isfinite(time)) return refuse(error, who + ": time must be finite");
    if (!std::isfinite(bias)) return refuse(error, who + ": bias must be finite");
    for (uint64_t k = 0; k < (uint64_t)n_triangles * 3u; ++k)  // before anything is written or followed
        if (indices[k] >= n_vertices)
            return refuse(error, who + ": triangle " + std::to_string(k / 3u) + " has vertex index " + std::to_string(indices[k]) + " >= n_vertices " +
                                     std::to_string(n_vertices));
    for (uint32_t v = 0; v < n_vertices; ++v) record(out + (size_t)v * HRT_RAY_FLOATS, at(positions + (size_t)v * 3u), time, V3{0.f, 0.f, 0.f}, bias);
    for (uint32_t t = 0; t < n_triangles; ++t) {
        const uint32_t *ix = indices + (size_t)t * 3u;
        const V3 p0 = at(positions + (size_t)ix[0] * 3u), p1 = at(positions + (size_t)ix[1] * 3u), p2 = at(positions + (size_t)ix[2] * 3u);
        const V3 c = cross(sub(p1, p0), sub(p2, p0));
        for (int k = 0; k < 3; ++k) {
            if ((k > 0 && ix[k] == ix[0]) || (k > 1 && ix[k] == ix[1])) continue;  // a triangle counts once for a vertex it names twice
            float *N = out + (size_t)ix[k] * HRT_RAY_FLOATS + 4u;
            N[0] = N[0] + c.x; N[1] = N[1] + c.y; N[2] = N[2] + c.z;
        }
    }
    return HRT_OK;
}

}  // namespace bakepts
