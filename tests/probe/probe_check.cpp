// The probe grid generator (csrc/hrt_probe_points.h) in a program of its own, built with the address and undefined-behaviour
// sanitizers (make probe_check) and run by tests/test_probe_abi.py: no device code, no GPU, nothing loaded into another process.
//
//   probe_check       prints one JSON object: per case the return code, the error text and the records as u32 bit patterns
//
// Every output buffer is allocated at exactly the size the call may write, so a record too many is a sanitizer report; a refusal
// must come before anything is written, so the sanitizers stay silent on the refused cases too.
#include "../../hai719-raytracing_amd/csrc/hrt_probe_points.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static bool g_first = true;

static void emit(const char *name, int rc, const std::string &error, const std::vector<float> &rec) {
    std::printf("%s\n  \"%s\": {\"rc\": %d, \"error\": \"%s\", \"records\": [", g_first ? "" : ",", name, rc, error.c_str());
    g_first = false;
    for (size_t i = 0; i < rec.size(); ++i) {
        uint32_t u;
        std::memcpy(&u, &rec[i], 4);
        std::printf("%s%u", i ? ", " : "", u);
    }
    std::printf("]}");
}

// null: 1 = lo, 2 = hi, 3 = out
static void grid_case(const char *name, const float (&lo)[3], const float (&hi)[3], uint32_t nx, uint32_t ny, uint32_t nz, float time, int null = 0) {
    const uint64_t n = (uint64_t)nx * ny * (nz ? nz : 1u);
    const bool fits = nx != 0u && ny != 0u && nz != 0u && (uint64_t)nx * ny <= 4096u && n <= 4096u;
    std::vector<float> out(fits ? (size_t)n * HRT_PROBE_FLOATS : 1u);  // a refused grid writes nothing
    std::string error;
    const int rc = probepts::grid_points(null == 1 ? nullptr : lo, null == 2 ? nullptr : hi, nx, ny, nz, time, null == 3 ? nullptr : out.data(), error);
    if (rc != HRT_OK) out.clear();
    emit(name, rc, error, out);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the boxes of tests/test_probe_abi.py: an uneven one, and one that runs backwards on two axes
    const float lo[3] = {-1.7f, 0.3f, 2.1f}, hi[3] = {2.9f, 1.1f, 7.6f};
    const float back_lo[3] = {3.f, -2.f, 5.f}, back_hi[3] = {-1.f, -2.f, 0.5f};
    std::printf("{");
    char name[64];
    const uint32_t sizes[4][3] = {{1, 1, 1}, {3, 2, 2}, {1, 7, 1}, {16, 8, 4}};
    for (const auto &s : sizes) {
        std::snprintf(name, sizeof name, "box_%ux%ux%u", s[0], s[1], s[2]);
        grid_case(name, lo, hi, s[0], s[1], s[2], 0.25f);
        std::snprintf(name, sizeof name, "back_%ux%ux%u", s[0], s[1], s[2]);
        grid_case(name, back_lo, back_hi, s[0], s[1], s[2], 0.f);
    }
    grid_case("null_lo", lo, hi, 2, 2, 2, 0.f, 1);
    grid_case("null_hi", lo, hi, 2, 2, 2, 0.f, 2);
    grid_case("null_out", lo, hi, 2, 2, 2, 0.f, 3);
    grid_case("nx_zero", lo, hi, 0, 2, 2, 0.f);
    grid_case("ny_zero", lo, hi, 2, 0, 2, 0.f);
    grid_case("nz_zero", lo, hi, 2, 2, 0, 0.f);
    grid_case("too_many", lo, hi, 65536u, 32768u, 1u, 0.f);
    grid_case("too_many_wrapping", lo, hi, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.f);
    const float lo_nan[3] = {0.f, nan, 0.f}, hi_inf[3] = {1.f, 1.f, inf};
    grid_case("lo_nan", lo_nan, hi, 2, 2, 2, 0.f);
    grid_case("hi_inf", lo, hi_inf, 2, 2, 2, 0.f);
    grid_case("time_nan", lo, hi, 2, 2, 2, nan);
    grid_case("time_inf", lo, hi, 2, 2, 2, -inf);
    std::printf("\n}\n");
    return 0;
}
