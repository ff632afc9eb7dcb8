// The cell and the weights of a probe volume (csrc/hrt_probe_volume_cell.h) in a program of its own, built with the address and
// undefined-behaviour sanitizers (make probe_volume_check) and run by tests/test_probe_volume_abi.py: no device code, no GPU,
// nothing loaded into another process.
//
//   probe_volume_check    prints one JSON object: per grid the point records it made (u32 bit patterns) and, for flags 0 and
//                         HRT_PROBE_EVAL_FACING, the eight indices and the eight weights (bit patterns) of every point; per
//                         refused grid the return code and the error text
//
// The points: per axis the positions lo + t * (hi - lo) for t below, before, on, between and past the outermost probe centres and
// the faces of the box, in every combination, each with one of a handful of normals; then the degenerate records.  index and
// weight are allocated at exactly eight elements per call, so an element too many is a sanitizer report.
#include "../../hai719-raytracing_amd/csrc/hrt_probe_volume_cell.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static bool g_first = true;

static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

static void list(const char *name, const std::vector<uint32_t> &v) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%u", i ? ", " : "", v[i]);
    std::printf("]");
}

static void grid_case(const char *name, const float (&lo)[3], const float (&hi)[3], uint32_t nx, uint32_t ny, uint32_t nz, int null = 0) {
    probevol::Grid g;
    std::string error;
    const int rc = probevol::make_grid("hrt_probe_volume_create", null == 1 ? nullptr : lo, null == 2 ? nullptr : hi, nx, ny, nz, g, error);
    std::printf("%s\n  \"%s\": {\"rc\": %d, \"error\": \"%s\"", g_first ? "" : ",", name, rc, error.c_str());
    g_first = false;
    if (rc != HRT_OK) {
        std::printf("}");
        return;
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float ts[] = {-0.5f, 0.f, 0.125f, 0.25f, 0.5f, 0.77f, 1.f, 1.5f};
    const float normals[][3] = {{0.f, 0.f, 1.f}, {0.f, -2.f, 0.f}, {0.3f, 0.4f, -0.5f}, {-1e-3f, 2e-3f, 1e-3f}, {5.f, 0.f, 0.f}, {1e18f, -1e18f, 1e18f}};
    std::vector<float> points;
    size_t k = 0;
    for (float tz : ts)
        for (float ty : ts)
            for (float tx : ts) {
                const float t[3] = {tx, ty, tz};
                const float *n = normals[k++ % (sizeof normals / sizeof normals[0])];
                for (int a = 0; a < 3; ++a) points.push_back(lo[a] + t[a] * (hi[a] - lo[a]));
                points.push_back(0.25f);
                for (int a = 0; a < 3; ++a) points.push_back(n[a]);
                points.push_back(1e-4f);
            }
    const float mid[3] = {lo[0] + .4f * (hi[0] - lo[0]), lo[1] + .4f * (hi[1] - lo[1]), lo[2] + .4f * (hi[2] - lo[2])};
    const float degenerate[][8] = {{nan, mid[1], mid[2], 0.f, 0.f, 0.f, 1.f, 0.f},  {mid[0], -inf, mid[2], 0.f, 0.f, 0.f, 1.f, 0.f},
                                   {mid[0], mid[1], mid[2], 0.f, 0.f, inf, 1.f, 0.f}, {mid[0], mid[1], mid[2], 0.f, nan, 0.f, 0.f, 0.f},
                                   {mid[0], mid[1], mid[2], 0.f, 0.f, 0.f, 0.f, 0.f}, {mid[0], mid[1], mid[2], 0.f, -0.f, 0.f, 0.f, 0.f},
                                   {mid[0], mid[1], mid[2], 0.f, 1e-30f, 0.f, 0.f, 0.f},
                                   // not degenerate: time and bias are not read, and huge but finite positions clamp
                                   {mid[0], mid[1], mid[2], nan, 0.f, 1.f, 0.f, inf}, {1e18f, -1e18f, 1e18f, 0.f, 1.f, 1.f, 1.f, 0.f},
                                   {-3e38f, 3e38f, mid[2], 0.f, 0.f, 0.f, -1.f, 0.f}};
    for (const auto &d : degenerate) points.insert(points.end(), d, d + 8);
    std::vector<uint32_t> pbits(points.size());
    for (size_t i = 0; i < points.size(); ++i) pbits[i] = bits(points[i]);
    std::printf(", ");
    list("points", pbits);
    for (uint32_t flags : {0u, (uint32_t)HRT_PROBE_EVAL_FACING}) {
        std::vector<uint32_t> index_all, weight_all;
        for (size_t i = 0; i < points.size() / 8; ++i) {
            std::vector<uint32_t> index(8, 77u);
            std::vector<float> weight(8, 77.f);
            float Nn[3];
            const bool ok = probevol::cell(g, &points[8 * i], &points[8 * i + 4], flags, index.data(), weight.data(), Nn);
            for (int m = 0; m < 8; ++m) {
                if (index[m] >= nx * ny * nz || (!ok && (index[m] != 0u || bits(weight[m]) != 0u))) {
                    std::fprintf(stderr, "%s: point %zu corner %d: index %u, ok %d\n", name, i, m, index[m], (int)ok);
                    std::exit(1);
                }
                index_all.push_back(index[m]);
                weight_all.push_back(bits(weight[m]));
            }
        }
        std::printf(", ");
        list(flags ? "index_facing" : "index", index_all);
        std::printf(", ");
        list(flags ? "weight_facing" : "weight", weight_all);
    }
    std::printf("}");
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the grids of tests/test_gpu_probe_volume.py
    const float lo[3] = {-1.7f, 0.3f, 2.1f}, hi[3] = {2.9f, 1.1f, 7.6f};
    const float back_lo[3] = {-1.f, 2.f, 0.f}, back_hi[3] = {1.f, -0.5f, 3.f};  // lo > hi on y
    std::printf("{");
    grid_case("grid_3x2x4", lo, hi, 3, 2, 4);
    grid_case("grid_1x1x1", lo, hi, 1, 1, 1);
    grid_case("grid_4x1x1", lo, hi, 4, 1, 1);
    grid_case("grid_2x2x2_back", back_lo, back_hi, 2, 2, 2);
    const float flat_hi[3] = {2.9f, 0.3f, 7.6f};  // lo == hi on y: fine where y has one probe
    grid_case("grid_3x1x2_flat", lo, flat_hi, 3, 1, 2);
    grid_case("null_lo", lo, hi, 2, 2, 2, 1);
    grid_case("null_hi", lo, hi, 2, 2, 2, 2);
    grid_case("nx_zero", lo, hi, 0, 2, 2);
    grid_case("ny_zero", lo, hi, 2, 0, 2);
    grid_case("nz_zero", lo, hi, 2, 2, 0);
    grid_case("too_many", lo, hi, 4096u, 4096u, 2u);
    grid_case("too_many_wrapping", lo, hi, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    const float lo_nan[3] = {0.f, nan, 0.f}, hi_inf[3] = {1.f, 1.f, inf};
    grid_case("lo_nan", lo_nan, hi, 2, 2, 2);
    grid_case("hi_inf", lo, hi_inf, 2, 2, 2);
    grid_case("flat_axis", lo, flat_hi, 3, 2, 2);
    const float thin_lo[3] = {0.f, 0.f, 0.f}, thin_hi[3] = {1.f, 1e-44f, 1.f};  // 2 / 1e-44 overflows
    grid_case("thin_axis", thin_lo, thin_hi, 2, 2, 2);
    std::printf("\n}\n");
    return 0;
}
