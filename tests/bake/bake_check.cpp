// The bake point generators (csrc/hrt_bake_points.h) in a program of their own, built with the address and undefined-behaviour
// sanitizers (make bake_check) and run by tests/test_bake_abi.py: no device code, no GPU, nothing loaded into another process.
//
//   bake_check        prints one JSON object: per case the return code, the error text and the records as u32 bit patterns
//
// Every output buffer is allocated at exactly the size the call may write, so a record too many is a sanitizer report; a refusal
// must come before a bad index is followed, so the sanitizers stay silent on the refused cases too.
#include "../../hai719-raytracing_amd/csrc/hrt_bake_points.h"

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

static hrt_quad make_quad(const float (&v0)[3], const float (&v1)[3], const float (&v3)[3]) {
    hrt_quad q{};
    std::memcpy(q.v0, v0, 12); std::memcpy(q.v1, v1, 12); std::memcpy(q.v3, v3, 12);
    return q;
}

static void quad_case(const char *name, const hrt_quad *q, uint32_t tw, uint32_t th, int32_t side, float time, float bias, bool null_out = false) {
    const uint64_t n = (uint64_t)tw * th;
    std::vector<float> out(n != 0u && n <= 4096u ? (size_t)n * HRT_RAY_FLOATS : 1u);  // a refused frame writes nothing
    std::string error;
    const int rc = bakepts::quad_points(q, tw, th, side, time, bias, null_out ? nullptr : out.data(), error);
    if (rc != HRT_OK) out.clear();
    emit(name, rc, error, out);
}

static void mesh_case(const char *name, const std::vector<float> &pos, const std::vector<uint32_t> &idx, float time, float bias, int null_which = 0) {
    const uint32_t nv = (uint32_t)(pos.size() / 3u), nt = (uint32_t)(idx.size() / 3u);
    std::vector<float> out((size_t)nv * HRT_RAY_FLOATS);
    std::string error;
    const int rc = bakepts::mesh_points(null_which == 1 ? nullptr : pos.data(), nv, null_which == 2 ? nullptr : idx.data(), nt, time, bias,
                                        null_which == 3 ? nullptr : out.data(), error);
    if (rc != HRT_OK) out.clear();
    emit(name, rc, error, out);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the tilted quad and the floor-like quad of tests/test_bake_abi.py
    const hrt_quad tilted = make_quad({0.3f, -1.7f, 2.1f}, {2.9f, -1.1f, 2.6f}, {-0.2f, 0.8f, 3.3f});
    const hrt_quad floor_ = make_quad({-2.f, -2.f, 2.f}, {2.f, -2.f, 2.f}, {-2.f, -2.f, -2.f});
    std::printf("{");
    char name[64];
    const uint32_t sizes[3] = {1u, 3u, 8u};
    for (uint32_t tw : sizes)
        for (uint32_t th : sizes)
            for (int32_t side : {1, -1}) {
                std::snprintf(name, sizeof name, "tilted_%ux%u_%s", tw, th, side > 0 ? "front" : "back");
                quad_case(name, &tilted, tw, th, side, 0.25f, 1e-4f);
                std::snprintf(name, sizeof name, "floor_%ux%u_%s", tw, th, side > 0 ? "front" : "back");
                quad_case(name, &floor_, tw, th, side, 0.f, 0.f);
            }
    quad_case("quad_null", nullptr, 2, 2, 1, 0.f, 0.f);
    quad_case("quad_null_out", &tilted, 2, 2, 1, 0.f, 0.f, true);
    quad_case("quad_tw_zero", &tilted, 0, 2, 1, 0.f, 0.f);
    quad_case("quad_th_zero", &tilted, 2, 0, 1, 0.f, 0.f);
    quad_case("quad_too_many", &tilted, 65536u, 32768u, 1, 0.f, 0.f);
    quad_case("quad_side_zero", &tilted, 2, 2, 0, 0.f, 0.f);
    quad_case("quad_side_two", &tilted, 2, 2, 2, 0.f, 0.f);
    quad_case("quad_time_nan", &tilted, 2, 2, 1, nan, 0.f);
    quad_case("quad_bias_inf", &tilted, 2, 2, 1, 0.f, inf);

    // a fan of three triangles round vertex 0 (shared), vertex 5 unused, one triangle naming vertex 4 twice
    const std::vector<float> pos = {0.f, 0.f, 0.f, 1.f, 0.1f, 0.f, 0.2f, 1.f, 0.3f, -1.f, 0.4f, 0.5f, 0.3f, -1.f, 0.25f, 7.f, 8.f, 9.f};
    const std::vector<uint32_t> idx = {0, 1, 2, 0, 2, 3, 0, 3, 4, 4, 4, 1};
    mesh_case("mesh_fan", pos, idx, 0.5f, 1e-3f);
    mesh_case("mesh_no_triangles", pos, {}, 0.f, 0.f);
    mesh_case("mesh_empty", {}, {}, 0.f, 0.f);
    mesh_case("mesh_bad_index", pos, {0, 1, 2, 0, 6, 1}, 0.f, 0.f);
    mesh_case("mesh_huge_index", pos, {0, 1, 0xFFFFFFFFu}, 0.f, 0.f);
    mesh_case("mesh_null_positions", pos, idx, 0.f, 0.f, 1);
    mesh_case("mesh_null_indices", pos, idx, 0.f, 0.f, 2);
    mesh_case("mesh_null_out", pos, idx, 0.f, 0.f, 3);
    mesh_case("mesh_time_inf", pos, idx, -inf, 0.f);
    mesh_case("mesh_bias_nan", pos, idx, 0.f, nan);
    std::printf("\n}\n");
    return 0;
}
