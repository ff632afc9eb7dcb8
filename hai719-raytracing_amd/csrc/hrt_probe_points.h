// Probe positions on the host (include/hrt.h "Light probes": hrt_probe_grid_points): the records of a regular grid of probes
// in a box, as a pure function.
//
// Nothing here touches a device, a global or the environment: hrt_probes.hip wraps the function for the C ABI, and
// tests/probe/probe_check.cpp calls it in a program of its own under the host sanitizers.  All arithmetic is fp32 in the order
// include/hrt.h writes, without fused multiply-add (tests/probe_ref.py states it again in NumPy).
#pragma once

#include "../../include/hrt.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace probepts {

inline int refuse(std::string &error, const std::string &msg) {
    error = msg;
    return HRT_ERR_INVALID;
}

// nx * ny * nz records {P, time}: probe (i, j, k) at index (k * ny + j) * nx + i, at the centre of its cell of the box [lo, hi]
// (lo > hi on an axis runs that axis backwards).
inline int grid_points(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, float time, float *out, std::string &error) {
#pragma clang fp contract(off)
    const std::string who = "hrt_probe_grid_points";
    if (!lo) return refuse(error, who + ": lo is NULL");
    if (!hi) return refuse(error, who + ": hi is NULL");
    if (!out) return refuse(error, who + ": out_probes is NULL");
    if (nx == 0u || ny == 0u || nz == 0u) return refuse(error, who + ": nx, ny and nz must be positive");
    // nx * ny <= 2^64 - 2^33 + 1 cannot wrap; the product with nz is compared by division
    if ((uint64_t)nx * ny > 0x7fffffffull / nz) return refuse(error, who + ": nx * ny * nz must be at most 2^31 - 1");
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a])) return refuse(error, who + ": lo must be finite");
        if (!std::isfinite(hi[a])) return refuse(error, who + ": hi must be finite");
    }
    if (!std::isfinite(time)) return refuse(error, who + ": time must be finite");
    const uint32_t count[3] = {nx, ny, nz};
    for (uint32_t k = 0; k < nz; ++k)
        for (uint32_t j = 0; j < ny; ++j)
            for (uint32_t i = 0; i < nx; ++i) {
                const uint32_t cell[3] = {i, j, k};
                float *r = out + (((size_t)k * ny + j) * nx + i) * HRT_PROBE_FLOATS;
                for (int a = 0; a < 3; ++a) r[a] = lo[a] + (((float)cell[a] + .5f) / (float)count[a]) * (hi[a] - lo[a]);
                r[3] = time;
            }
    return HRT_OK;
}

}  // namespace probepts
