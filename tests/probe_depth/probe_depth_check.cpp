// The octahedral depth map (csrc/hrt_probe_depth_oct.h) and the visibility piece of the cell header (csrc/hrt_probe_volume_cell.h:
// biased, toward, cell_visible) in a program of its own, built with the address and undefined-behaviour sanitizers (make
// probe_depth_check) and run by tests/test_probe_depth_abi.py: no device code, no GPU, nothing loaded into another process.
//
//   probe_depth_check    prints one JSON object: the 64 centre directions (u32 bit patterns) and the texel each maps back to; a
//                        list of vectors (bit patterns) -- texel edges and diagonals, the axes, z = +-0, NaN and infinite
//                        components, random ones of wildly different lengths -- and their texels; and for one grid the point
//                        records and moments it made and, for flags 0 and HRT_PROBE_EVAL_FACING, the eight indices and the eight
//                        weights of the visible look-up of every point
//
// The moments are allocated at exactly 64 pairs per probe and index and weight at exactly eight elements per call, so a texel or
// an element too many is a sanitizer report.
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

static uint32_t g_state = 12345u;
static float uniform() {  // in [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.f / 16777216.f);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::printf("{\n  ");
    {
        std::vector<uint32_t> dir, back;
        for (uint32_t e = 0; e < HRT_PROBE_DEPTH_TEXELS; ++e) {
            std::vector<float> c(3, 77.f);
            probedepth::direction(e, c.data());
            for (float x : c) dir.push_back(bits(x));
            back.push_back(probedepth::texel(c.data()));
        }
        list("direction", dir);
        std::printf(",\n  ");
        list("centre_texel", back);
    }
    {
        std::vector<float> v;
        auto add = [&](float x, float y, float z) { v.push_back(x); v.push_back(y); v.push_back(z); };
        for (int i = 0; i <= 8; ++i)  // texel edges and corners of the square, unfolded onto both hemispheres
            for (int j = 0; j <= 8; ++j) {
                const float px = (float)i * .25f - 1.f, py = (float)j * .25f - 1.f, z = (1.f - std::fabs(px)) - std::fabs(py);
                if (z >= 0.f) { add(px, py, z); add(3.f * px, 3.f * py, -3.f * z); }
            }
        for (float a : {1.f, -1.f}) { add(a, 0.f, 0.f); add(0.f, a, 0.f); add(0.f, 0.f, a); }                   // the six axes
        for (float a : {1.f, -1.f}) for (float b : {1.f, -1.f}) for (float c : {1.f, -1.f}) add(a, b, c);    // the diagonals
        for (float a : {1.f, -1.f}) for (float b : {1.f, -1.f}) { add(a, b, 0.f); add(a, b, -0.f); add(a, 0.f, b); add(0.f, a, b); }
        add(0.5f, 0.25f, 0.f); add(0.5f, 0.25f, -0.f); add(-1e-30f, 1e-30f, -0.f); add(1e-42f, 0.f, 0.f); add(3e38f, 3e38f, 3e38f);
        add(nan, 1.f, 1.f); add(1.f, nan, -1.f); add(inf, 1.f, 1.f); add(1.f, 1.f, -inf); add(0.f, 0.f, 0.f);  // whatever comes in: a texel below 64
        for (int k = 0; k < 4000; ++k) {
            float scale = 1.f;
            for (int s = (int)(uniform() * 60.f) - 30; s != 0; s += s < 0 ? 1 : -1) scale *= s < 0 ? .1f : 10.f;
            add((uniform() - .5f) * scale, (uniform() - .5f) * scale, (uniform() - .5f) * scale);
        }
        std::vector<uint32_t> vb, tx;
        for (float x : v) vb.push_back(bits(x));
        for (size_t i = 0; i < v.size() / 3; ++i) {
            const std::vector<float> one(v.begin() + 3 * i, v.begin() + 3 * i + 3);
            const uint32_t e = probedepth::texel(one.data());
            if (e >= HRT_PROBE_DEPTH_TEXELS) {
                std::fprintf(stderr, "vector %zu: texel %u\n", i, e);
                return 1;
            }
            tx.push_back(e);
        }
        std::printf(",\n  ");
        list("vectors", vb);
        std::printf(",\n  ");
        list("texel", tx);
    }
    {   // the visible look-up on the 3 x 2 x 2 grid of tests/test_gpu_probe_depth.py
        const float lo[3] = {-1.7f, 0.3f, 2.1f}, hi[3] = {2.9f, 1.1f, 7.6f};
        const uint32_t nx = 3, ny = 2, nz = 2, count = nx * ny * nz;
        probevol::Grid g;
        std::string error;
        if (probevol::make_grid("probe_depth_check", lo, hi, nx, ny, nz, g, error) != HRT_OK) return 1;
        std::vector<float> moments((size_t)count * HRT_PROBE_DEPTH_TEXELS * 2u);
        for (size_t i = 0; i < moments.size() / 2; ++i) {
            const float u = uniform(), m1 = .2f + 3.f * uniform();
            moments[2 * i] = u < .15f ? inf : m1;
            moments[2 * i + 1] = u < .15f ? 0.f : u < .3f ? m1 * m1 : u < .45f ? .5f * (m1 * m1) : m1 * m1 + .3f * uniform();
        }
        const float ts[] = {-0.5f, 0.f, 0.125f, 0.25f, 0.5f, 0.77f, 1.f, 1.5f};
        const float normals[][3] = {{0.f, 0.f, 1.f}, {0.f, -2.f, 0.f}, {0.3f, 0.4f, -0.5f}, {-1e-3f, 2e-3f, 1e-3f}, {5.f, 0.f, 0.f}, {1e18f, -1e18f, 1e18f}};
        const float biases[] = {0.f, 1e-4f, -0.3f, 0.5f, 2.f};
        std::vector<float> points;
        size_t k = 0;
        for (float tz : ts)
            for (float ty : ts)
                for (float tx : ts) {
                    const float t[3] = {tx, ty, tz};
                    const float *n = normals[k % (sizeof normals / sizeof normals[0])];
                    for (int a = 0; a < 3; ++a) points.push_back(lo[a] + t[a] * (hi[a] - lo[a]));
                    points.push_back(0.25f);
                    for (int a = 0; a < 3; ++a) points.push_back(n[a]);
                    points.push_back(biases[k % (sizeof biases / sizeof biases[0])]);
                    ++k;
                }
        const float mid[3] = {lo[0] + .4f * (hi[0] - lo[0]), lo[1] + .4f * (hi[1] - lo[1]), lo[2] + .4f * (hi[2] - lo[2])};
        const float c0[3] = {lo[0] + (.5f / 3.f) * (hi[0] - lo[0]), lo[1] + (.5f / 2.f) * (hi[1] - lo[1]), lo[2] + (.5f / 2.f) * (hi[2] - lo[2])};  // probe 0
        const float special[][8] = {{nan, mid[1], mid[2], 0.f, 0.f, 0.f, 1.f, 0.f},  {mid[0], mid[1], mid[2], 0.f, 0.f, inf, 1.f, 0.f},
                                    {mid[0], mid[1], mid[2], 0.f, 0.f, 0.f, 0.f, 0.f}, {mid[0], mid[1], mid[2], 0.f, 1e-30f, 0.f, 0.f, 0.f},
                                    {mid[0], mid[1], mid[2], 0.f, 0.f, 1.f, 0.f, inf}, {mid[0], mid[1], mid[2], 0.f, 0.f, 1.f, 0.f, nan},  // the bias
                                    {mid[0], mid[1], mid[2], 0.f, 0.f, 1.f, 0.f, -inf},
                                    // not degenerate: a point at a probe centre (l == 0), huge but finite positions and biases
                                    {c0[0], c0[1], c0[2], nan, 0.f, 1.f, 0.f, 0.f}, {1e18f, -1e18f, 1e18f, 0.f, 1.f, 1.f, 1.f, 1e18f},
                                    {-3e38f, 3e38f, mid[2], 0.f, 0.f, 0.f, -1.f, 3e38f}};
        for (const auto &d : special) points.insert(points.end(), d, d + 8);
        std::vector<uint32_t> pbits, mbits;
        for (float x : points) pbits.push_back(bits(x));
        for (float x : moments) mbits.push_back(bits(x));
        std::printf(",\n  ");
        list("points", pbits);
        std::printf(",\n  ");
        list("moments", mbits);
        for (uint32_t flags : {0u, (uint32_t)HRT_PROBE_EVAL_FACING}) {
            std::vector<uint32_t> index_all, weight_all;
            for (size_t i = 0; i < points.size() / 8; ++i) {
                std::vector<uint32_t> index(8, 77u);
                std::vector<float> weight(8, 77.f);
                float Nn[3];
                const bool ok = probevol::cell_visible(g, &points[8 * i], &points[8 * i + 4], points[8 * i + 7], flags, moments.data(), index.data(),
                                                       weight.data(), Nn);
                for (int m = 0; m < 8; ++m) {
                    if (index[m] >= count || (!ok && (index[m] != 0u || bits(weight[m]) != 0u))) {
                        std::fprintf(stderr, "point %zu corner %d: index %u, ok %d\n", i, m, index[m], (int)ok);
                        return 1;
                    }
                    index_all.push_back(index[m]);
                    weight_all.push_back(bits(weight[m]));
                }
            }
            std::printf(",\n  ");
            list(flags ? "index_facing" : "index", index_all);
            std::printf(",\n  ");
            list(flags ? "weight_facing" : "weight", weight_all);
        }
    }
    std::printf("\n}\n");
    return 0;
}
