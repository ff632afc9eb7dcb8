// The look-up of a lit ray's tail (include/hrt.h "Lit rays", step 5) in a program of its own: the shared cell header
// (csrc/hrt_probe_volume_cell.h: cell, cell_visible) on the point records {p = o + t * d, time, n, bias} a lit kernel makes of its
// hits, built with the address and undefined-behaviour sanitizers (make probe_lit_check) and run by tests/test_probe_lit_abi.py: no
// device code, no GPU, nothing loaded into another process.
//
//   probe_lit_check    prints one JSON object: the point records it made (u32 bit patterns) -- hits of rays from inside and outside
//                      the grid's box with unit normals, then the degenerate ones a kernel can meet: a hit point that overflowed, a
//                      NaN one, a zero normal, a normal with a NaN --, the moments, and for eval_flags 0, FACING, VISIBLE and
//                      FACING | VISIBLE the eight indices and the eight weights of every record
//
// index and weight are allocated at exactly eight elements per call and the moments at exactly 64 pairs per probe, so an element
// or a texel too many is a sanitizer report.
#include "../../hai719-raytracing_amd/csrc/hrt_probe_volume_cell.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

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

static uint32_t g_state = 2024u;
static float uniform() {  // in [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.f / 16777216.f);
}

int main() {
#pragma clang fp contract(off)
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float lo[3] = {-1.7f, 0.3f, 2.1f}, hi[3] = {2.9f, 1.1f, 7.6f};  // the 3 x 2 x 2 grid of tests/test_gpu_probe_depth.py
    const uint32_t nx = 3, ny = 2, nz = 2, count = nx * ny * nz;
    const float bias = 1e-3f, time = 0.25f;
    probevol::Grid g;
    std::string error;
    if (probevol::make_grid("probe_lit_check", lo, hi, nx, ny, nz, g, error) != HRT_OK) return 1;
    std::vector<float> moments((size_t)count * HRT_PROBE_DEPTH_TEXELS * 2u);
    for (size_t i = 0; i < moments.size() / 2; ++i) {
        const float u = uniform(), m1 = .2f + 3.f * uniform();
        moments[2 * i] = u < .15f ? inf : m1;
        moments[2 * i + 1] = u < .15f ? 0.f : u < .3f ? m1 * m1 : u < .45f ? .5f * (m1 * m1) : m1 * m1 + .3f * uniform();
    }
    std::vector<float> points;
    auto record = [&](const float o[3], const float d[3], float t, const float n[3]) {
        for (int a = 0; a < 3; ++a) points.push_back(o[a] + t * d[a]);  // Surface::p of the hit
        points.push_back(time);
        for (int a = 0; a < 3; ++a) points.push_back(n[a]);
        points.push_back(bias);
    };
    for (int k = 0; k < 600; ++k) {
        float o[3], d[3], n[3];
        const float reach = k % 3 == 0 ? 3.f : 1.f;  // origins inside the box, and up to a box length outside it
        for (int a = 0; a < 3; ++a) o[a] = lo[a] + ((uniform() - .5f) * reach + .5f) * (hi[a] - lo[a]);
        for (float *v : {d, n}) {
            float L = 0.f;
            while (!(L > 1e-3f)) {
                for (int a = 0; a < 3; ++a) v[a] = uniform() * 2.f - 1.f;
                L = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            }
            for (int a = 0; a < 3; ++a) v[a] = v[a] / L;
        }
        record(o, d, uniform() * 4.f, n);
    }
    {
        const float o[3] = {0.f, .5f, 3.f}, z[3] = {0.f, 0.f, 1.f}, zero[3] = {0.f, 0.f, 0.f}, bad[3] = {0.f, nan, 1.f};
        const float far[3] = {1e18f, -1e18f, 1e18f}, huge[3] = {3e38f, -3e38f, 3e38f};
        record(far, z, 1e18f, z);       // finite and far outside: clamps to the outermost probes
        record(huge, huge, 3e38f, z);   // o + t * d overflows: a hit point that is not finite
        record(o, z, nan, z);
        record(o, z, 1.f, zero);
        record(o, z, 1.f, bad);
        record(o, z, inf, z);
    }
    std::vector<uint32_t> pbits, mbits;
    for (float x : points) pbits.push_back(bits(x));
    for (float x : moments) mbits.push_back(bits(x));
    std::printf("{\n  ");
    list("points", pbits);
    std::printf(",\n  ");
    list("moments", mbits);
    const uint32_t VISIBLE = HRT_LIT_VISIBLE;
    for (uint32_t eval_flags : {0u, (uint32_t)HRT_PROBE_EVAL_FACING, VISIBLE, (uint32_t)HRT_PROBE_EVAL_FACING | VISIBLE}) {
        std::vector<uint32_t> index_all, weight_all;
        for (size_t i = 0; i < points.size() / 8; ++i) {
            std::vector<uint32_t> index(8, 77u);
            std::vector<float> weight(8, 77.f);
            float Nn[3];
            const float *P = &points[8 * i], *N = &points[8 * i + 4];
            const uint32_t facing = eval_flags & HRT_PROBE_EVAL_FACING;  // what a lit kernel hands on
            const bool ok = (eval_flags & VISIBLE) ? probevol::cell_visible(g, P, N, points[8 * i + 7], facing, moments.data(), index.data(), weight.data(), Nn)
                                                   : probevol::cell(g, P, N, facing, index.data(), weight.data(), Nn);
            for (int m = 0; m < 8; ++m) {
                if (index[m] >= count || (!ok && (index[m] != 0u || bits(weight[m]) != 0u))) {
                    std::fprintf(stderr, "point %zu corner %d: index %u, ok %d\n", i, m, index[m], (int)ok);
                    return 1;
                }
                index_all.push_back(index[m]);
                weight_all.push_back(bits(weight[m]));
            }
        }
        char name[32];
        std::printf(",\n  ");
        std::snprintf(name, sizeof name, "index_%u", eval_flags);
        list(name, index_all);
        std::printf(",\n  ");
        std::snprintf(name, sizeof name, "weight_%u", eval_flags);
        list(name, weight_all);
    }
    std::printf("\n}\n");
    return 0;
}
