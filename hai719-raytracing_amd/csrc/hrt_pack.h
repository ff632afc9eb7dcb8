// Scene packing: hrt_scene_desc -> the host arrays and header of hrt_device.h, as a pure function.
//
// pack_scene touches no device and reads no global or environment: hrt_scene_create (hrt_api.hip) calls it and uploads
// what it returns, and tests/pack/pack_check.cpp calls it on a machine without a GPU, under the host sanitizers.  It is
// also the library's whole defence against a malformed description: every index the kernels will follow is checked
// here, before it is followed.  tests/golden/pack_hashes.json pins the packed bytes and the refusal texts.
#pragma once

#include "hrt_device.h"

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {

// What hrt_scene_create uploads.  The header carries every scalar the packing decides; its device pointers are null.
struct PackedScene {
    std::vector<float4> tabs;  // squares | materials | spheres | mesh records | sphere pair-filter rows (| short exception lists)
    std::vector<float4> qfilter;
    std::vector<uint4> units;
    std::vector<float4> tris, planes, colors;
    std::vector<uint4> vids;
    std::vector<DImage> images;
    std::vector<uint32_t> texels;
    std::vector<float4> lights, exceptions;
    DScene header{};        // prune_ok as the fp64 bound alone decides it
    float bound = 0.f;      // largest distance of any scene point from the origin (filter margins)
    uint32_t max_leaf = 0;  // most triangles in one KD leaf
};

// The tables that end up side by side in PackedScene::tabs (layout_tabs).
struct PackTables {
    std::vector<float4> quads, mats, spheres, sfilter;
    std::vector<DMesh> meshes;
};

int refuse(std::string &error, const std::string &msg) {
    error = msg;
    return HRT_ERR_INVALID;
}

float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct H3 { float x, y, z; };
// host fp32 helpers in the reference's evaluation order (no contraction): these fold the
// per-quad constants exactly as Square::intersect would compute them per call.
H3 h_sub(H3 a, H3 b) {
#pragma clang fp contract(off)
    return H3{a.x - b.x, a.y - b.y, a.z - b.z};
}
H3 h_cross(H3 a, H3 b) {
#pragma clang fp contract(off)
    return H3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
float h_dot(H3 a, H3 b) {
#pragma clang fp contract(off)
    return a.x * b.x + a.y * b.y + a.z * b.z;
}
float h_len(H3 a) { return (float)std::sqrt((double)h_dot(a, a)); }
H3 h_normalize(H3 a) {
    float L = h_len(a);
    return H3{a.x / L, a.y / L, a.z / L};
}

// Square::intersect's per-call constants (Square.h:66-72: edges, normal, |R|, |U|, D0), computed once in the same fp32
// arithmetic -> the 7 float4 rows of hrt_device.h.
void fold_quad(const hrt_quad &q, const hrt_material &m, std::vector<float4> &quads) {
    const H3 v0{q.v0[0], q.v0[1], q.v0[2]}, v1{q.v1[0], q.v1[1], q.v1[2]}, v3{q.v3[0], q.v3[1], q.v3[2]};
    const H3 R = h_sub(v1, v0), U = h_sub(v3, v0);
    const H3 n = h_normalize(h_cross(R, U));
    uint32_t flags = 0;
    if (m.type == HRT_MAT_GLASS) flags |= HRT_QUAD_FLAG_GLASS;
    if (m.motion[0] != 0.f || m.motion[1] != 0.f || m.motion[2] != 0.f) flags |= HRT_QUAD_FLAG_MOVING;
    quads.push_back(make_float4(v0.x, v0.y, v0.z, h_dot(v0, n)));
    quads.push_back(make_float4(n.x, n.y, n.z, as_float(flags)));
    quads.push_back(make_float4(R.x, R.y, R.z, h_len(R)));
    quads.push_back(make_float4(U.x, U.y, U.z, h_len(U)));
    quads.push_back(make_float4(m.motion[0], m.motion[1], m.motion[2], as_float((uint32_t)q.material)));
    quads.push_back(make_float4(q.tangent[0], q.tangent[1], q.tangent[2], 0.f));
    quads.push_back(make_float4(q.bitangent[0], q.bitangent[1], q.bitangent[2], 0.f));
}

// The rows of the squares' no-division filter (hrt_device.h DScene::qfilter; hrt_kernels.hip quad_filter), from the folded
// rows: sections for static squares lying (nearly) in an axis plane, by normal axis, then all others.  The constants of
// the axis form and the error analysis behind them are stated at quad_filter_axis.
void build_quad_filter(const std::vector<float4> &quads, uint32_t nq, std::vector<float4> &qf, uint32_t count[4]) {
    std::vector<float4> sec[4];
    for (int k = 0; k < 4; ++k) count[k] = 0;
    for (uint32_t i = 0; i < nq; ++i) {
        const float4 *q = &quads[(size_t)HRT_QUAD_ROWS * i];
        const double p0[3] = {q[0].x, q[0].y, q[0].z}, n[3] = {q[1].x, q[1].y, q[1].z}, R[3] = {q[2].x, q[2].y, q[2].z}, U[3] = {q[3].x, q[3].y, q[3].z};
        const double lenR = q[2].w, lenU = q[3].w;
        uint32_t flags;
        std::memcpy(&flags, &q[1].w, 4);
        int K = -1;   // normal axis
        double eps_n = 0.0, eps_e = 0.0;
        if (!(flags & HRT_QUAD_FLAG_MOVING) && lenR > 0.0 && lenU > 0.0) {
            int k = 0;
            for (int c = 1; c < 3; ++c) if (std::fabs(n[c]) > std::fabs(n[k])) k = c;
            const int a = (k + 1) % 3, b = (k + 2) % 3;
            eps_n = std::fabs(n[a]) + std::fabs(n[b]) + std::fabs(1.0 - std::fabs(n[k]));
            const double dev_ab = (std::fabs(R[k]) + std::fabs(R[b])) / lenR + (std::fabs(U[k]) + std::fabs(U[a])) / lenU;  // R along a, U along b
            const double dev_ba = (std::fabs(R[k]) + std::fabs(R[a])) / lenR + (std::fabs(U[k]) + std::fabs(U[b])) / lenU;  // or the other way round
            eps_e = std::min(dev_ab, dev_ba);
            if (eps_n <= 1e-4 && eps_e <= 1e-4 && std::isfinite(eps_n) && std::isfinite(eps_e)) K = k;
        }
        if (K >= 0) {
            const int a = (K + 1) % 3, b = (K + 2) % 3;
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int c = 0; c < 4; ++c)      // the four corners p0, p0 + R, p0 + U, p0 + R + U
                for (int x = 0; x < 3; ++x) {
                    const double v = p0[x] + ((c & 1) ? R[x] : 0.0) + ((c & 2) ? U[x] : 0.0);
                    lo[x] = std::min(lo[x], v); hi[x] = std::max(hi[x], v);
                }
            const double widen = (2.0 * eps_e + 2e-6) * (lenR + lenU);  // proj = qq.R / |R| against qq_a, and its own rounding
            auto centre = [&](int x) { return (float)(0.5 * (lo[x] + hi[x])); };
            auto half = [&](int x) { return std::nextafter((float)(0.5 * (hi[x] - lo[x]) + widen + 2.4e-7 * (std::fabs(lo[x]) + std::fabs(hi[x]))), INFINITY); };
            const float sgn = n[K] < 0.0 ? -1.f : 1.f;
            const float par = (float)(8.0 * (eps_n + 4e-7));
            const float cq = (float)(2.5e6 * (eps_n + 3e-7));
            const uint32_t bits = ((flags & HRT_QUAD_FLAG_GLASS) ? 1u : 0u) | (sgn < 0.f ? 2u : 0u) | (i << 8);
            sec[K].push_back(make_float4(sgn * q[0].w, centre(a), centre(b), half(a)));
            sec[K].push_back(make_float4(half(b), as_float(bits), par, cq));
            ++count[K];
        } else {
            sec[3].push_back(make_float4(q[0].x, q[0].y, q[0].z, q[0].w));
            sec[3].push_back(make_float4(q[1].y, q[1].z, q[1].x, as_float(flags | (i << 8))));
            sec[3].push_back(make_float4(q[2].x, q[3].x, q[2].y, q[3].y));
            sec[3].push_back(make_float4(q[2].z, q[3].z, q[2].w, q[3].w));
            ++count[3];
        }
    }
    qf.clear();
    for (int k = 0; k < 4; ++k) qf.insert(qf.end(), sec[k].begin(), sec[k].end());
}

// Triangle(c0,c1,c2) + computeBarycentricCoordinates constants (Triangle.h:26-37, 62-70) -> the plane and the 4 rows of hrt_device.h.
// The barycentric denominator fl(fl(d00 * d11) - fl(d01 * d01)) is not stored: the kernels recompute it from the rows, in the
// same two roundings (tri_inside).
void fold_triangle(const H3 c[3], uint32_t id, std::vector<float4> &tris, std::vector<float4> &planes) {
    const H3 e1 = h_sub(c[1], c[0]), e2 = h_sub(c[2], c[0]);
    const H3 nn = h_cross(e1, e2);
    const float norm = h_len(nn);
    const H3 n{nn.x / norm, nn.y / norm, nn.z / norm};
    const float d00 = h_dot(e1, e1), d01 = h_dot(e1, e2), d11 = h_dot(e2, e2);
    planes.push_back(make_float4(n.x, n.y, n.z, h_dot(c[0], n)));
    tris.push_back(make_float4(c[0].x, c[0].y, c[0].z, d11));
    tris.push_back(make_float4(e1.x, e1.y, e1.z, d00));
    tris.push_back(make_float4(e2.x, e2.y, e2.z, d01));
    tris.push_back(make_float4(as_float(id), 0.f, 0.f, 0.f));  // read only when the triangle is shaded
}

// Triangle t of mesh M, scaled as the reference scales it (KDTree.cpp:38-40), folded onto the end of the soup.
void push_triangle(const hrt_mesh &M, uint32_t t, std::vector<float4> &tris, std::vector<float4> &planes) {
    H3 c[3];
    for (int j = 0; j < 3; ++j) {
        const float *p = M.positions + 3 * (size_t)M.indices[3 * (size_t)t + j];
        c[j] = H3{p[0] * HRT_TRIANGLE_SCALING, p[1] * HRT_TRIANGLE_SCALING, p[2] * HRT_TRIANGLE_SCALING};
    }
    fold_triangle(c, t, tris, planes);
}

// ---- the checks that need no packing: every scene-level index and count
int check_desc(const hrt_scene_desc &D, std::string &error) {
    for (uint32_t i = 0; i < D.n_materials; ++i) {
        const hrt_material &m = D.materials[i];
        if (m.image >= (int32_t)D.n_images || m.normal_map >= (int32_t)D.n_images)
            return refuse(error, "material references an image that does not exist");
        if (m.type < 0 || m.type > 2 || m.texture_type < 0 || m.texture_type > 2)
            return refuse(error, "material type / texture type out of range");
        if (m.normal_map >= 0 && (D.images[m.normal_map].w < 1 || D.images[m.normal_map].h < 1))
            return refuse(error, "normal map image is empty");
    }
    for (uint32_t i = 0; i < D.n_spheres; ++i)
        if (D.spheres[i].material < 0 || (uint32_t)D.spheres[i].material >= D.n_materials)
            return refuse(error, "sphere material out of range");
    for (uint32_t i = 0; i < D.n_quads; ++i)
        if (D.quads[i].material < 0 || (uint32_t)D.quads[i].material >= D.n_materials)
            return refuse(error, "quad material out of range");
    if (D.skybox_image >= (int32_t)D.n_images) return refuse(error, "skybox image out of range");
    if (D.n_lights && !D.lights) return refuse(error, "lights missing");
    if (D.n_meshes > 32u) return refuse(error, "more than 32 meshes in one scene (the parked-mesh mask is 32 bits)");
    // the soup of all meshes: a path record names a triangle by soup slot in 25 bits (hrt_stream.hip sp_hit_word).  By the counts alone,
    // before any array is read: an irregular triangle takes one row, and there are at most min(n_exceptions, n_triangles) of them
    uint64_t rows = 0;
    for (uint32_t mi = 0; mi < D.n_meshes; ++mi) rows += (uint64_t)D.meshes[mi].n_leaf_tris + std::min(D.meshes[mi].n_exceptions, D.meshes[mi].n_triangles);
    if (rows > (uint64_t)HRT_MAX_SOUP_SLOTS)
        return refuse(error, "triangle soup of " + std::to_string(rows) + " rows (leaf triangles + irregular triangles of all meshes): more than HRT_MAX_SOUP_SLOTS = " +
                                 std::to_string(HRT_MAX_SOUP_SLOTS) + " (a path record keeps 25 bits of soup slot)");
    return HRT_OK;
}

// ---- scene extent: an upper bound on |point| for every point a ray can start from or hit
float scene_bound(const hrt_scene_desc &D) {
    double b = 0.0;
    auto grow = [&](double x, double y, double z, double extra) { b = std::max(b, std::sqrt(x * x + y * y + z * z) + extra); };
    auto mlen = [&](const hrt_material &m) { return std::sqrt((double)m.motion[0] * m.motion[0] + (double)m.motion[1] * m.motion[1] + (double)m.motion[2] * m.motion[2]); };
    for (uint32_t i = 0; i < D.n_spheres; ++i) {
        const hrt_sphere &sp = D.spheres[i];
        grow(sp.center[0], sp.center[1], sp.center[2], std::fabs((double)sp.radius) + mlen(D.materials[sp.material]));
    }
    for (uint32_t i = 0; i < D.n_quads; ++i) {
        const hrt_quad &q = D.quads[i];
        const double ml = mlen(D.materials[q.material]);
        grow(q.v0[0], q.v0[1], q.v0[2], ml);
        grow(q.v1[0], q.v1[1], q.v1[2], ml);
        grow(q.v3[0], q.v3[1], q.v3[2], ml);
        grow((double)q.v1[0] + q.v3[0] - q.v0[0], (double)q.v1[1] + q.v3[1] - q.v0[1], (double)q.v1[2] + q.v3[2] - q.v0[2], ml);
    }
    for (uint32_t mi = 0; mi < D.n_meshes; ++mi)
        for (uint32_t v = 0; v < D.meshes[mi].n_vertices; ++v) {
            const float *p = D.meshes[mi].positions + 3 * (size_t)v;
            grow(p[0] * 1.00001, p[1] * 1.00001, p[2] * 1.00001, 0.0);
        }
    for (uint32_t i = 0; i < D.n_lights; ++i) grow(D.lights[i].pos[0], D.lights[i].pos[1], D.lights[i].pos[2], std::fabs((double)D.lights[i].radius));
    return (float)b;
}

// ---- spheres / quads (with their filter) / sphere pair filter / lights / materials
void pack_primitives(const hrt_scene_desc &D, PackTables &T, PackedScene &P) {
    for (uint32_t i = 0; i < D.n_spheres; ++i) {
        const hrt_sphere &sp = D.spheres[i];
        const hrt_material &m = D.materials[sp.material];
        T.spheres.push_back(make_float4(sp.center[0], sp.center[1], sp.center[2], sp.radius));
        T.spheres.push_back(make_float4(m.motion[0], m.motion[1], m.motion[2], as_float((uint32_t)sp.material)));
    }
    for (uint32_t i = 0; i < D.n_quads; ++i) fold_quad(D.quads[i], D.materials[D.quads[i].material], T.quads);
    build_quad_filter(T.quads, D.n_quads, P.qfilter, P.header.qf_n);
    {   // hrt_device.h DScene::tab_sfilter; hrt_kernels.hip sphere_filter
        const uint32_t ns = D.n_spheres, pairs = (ns + 1u) / 2u;
        for (uint32_t p = 0; p < pairs; ++p) {
            const uint32_t a = 2u * p, b = std::min(2u * p + 1u, ns - 1u);
            const float4 a0 = T.spheres[2u * a], a1 = T.spheres[2u * a + 1u], b0 = T.spheres[2u * b], b1 = T.spheres[2u * b + 1u];
            T.sfilter.push_back(make_float4(a0.x, b0.x, a0.y, b0.y));
            T.sfilter.push_back(make_float4(a0.z, b0.z, a0.w * a0.w, b0.w * b0.w));
            T.sfilter.push_back(make_float4(a1.x, b1.x, a1.y, b1.y));
            T.sfilter.push_back(make_float4(a1.z, b1.z, std::fabs(a0.w), std::fabs(b0.w)));
        }
        P.header.sf_pairs = pairs;
        P.header.sf_psize = std::max(1u, (pairs + 63u) / 64u);
    }
    for (uint32_t i = 0; i < D.n_lights; ++i) {
        const hrt_light &l = D.lights[i];
        P.lights.push_back(make_float4(l.pos[0], l.pos[1], l.pos[2], l.radius));
        P.lights.push_back(make_float4(l.color[0], l.color[1], l.color[2], 0.f));
    }
    for (uint32_t i = 0; i < D.n_materials; ++i) {
        const hrt_material &m = D.materials[i];
        T.mats.push_back(make_float4(m.albedo[0], m.albedo[1], m.albedo[2], m.transparency));
        T.mats.push_back(make_float4(m.index_medium, as_float((uint32_t)m.type), as_float((uint32_t)m.texture_type),
                                     as_float((uint32_t)(m.emissive ? 1 : 0))));
        T.mats.push_back(make_float4(m.checker1[0], m.checker1[1], m.checker1[2], m.tex_scale_x));
        T.mats.push_back(make_float4(m.checker2[0], m.checker2[1], m.checker2[2], m.tex_scale_y));
        T.mats.push_back(make_float4(m.light_color[0], m.light_color[1], m.light_color[2], m.light_intensity));
        T.mats.push_back(make_float4(as_float((uint32_t)m.image), as_float((uint32_t)m.normal_map), 0.f, 0.f));
        T.mats.push_back(make_float4(0.f, 0.f, 0.f, 0.f));  // rows 6, 7: geometry of the texture / the normal map, filled in by pack_images
        T.mats.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// ---- images -> RGBA8 words, and the {texel offset, w, h} of each material's images (rows 6, 7), so that a lane need not
// chase the image table
int pack_images(const hrt_scene_desc &D, std::vector<float4> &mats, PackedScene &P, std::string &error) {
    for (uint32_t i = 0; i < D.n_images; ++i) {
        const hrt_image &im = D.images[i];
        DImage di;
        di.offset = (uint32_t)P.texels.size();
        di.w = im.w; di.h = im.h; di.pad = 0;
        if (im.w >= 1 && im.h >= 1) {
            if (!im.rgb) return refuse(error, "image without pixels");
            const size_t n = (size_t)im.w * im.h;
            for (size_t p = 0; p < n; ++p)
                P.texels.push_back((uint32_t)im.rgb[3 * p] | ((uint32_t)im.rgb[3 * p + 1] << 8) | ((uint32_t)im.rgb[3 * p + 2] << 16));
        }
        P.images.push_back(di);
    }
    auto geometry = [&](int32_t image) { return make_float4(as_float(P.images[image].offset), as_float((uint32_t)P.images[image].w), as_float((uint32_t)P.images[image].h), 0.f); };
    for (uint32_t i = 0; i < D.n_materials; ++i) {
        const hrt_material &m = D.materials[i];
        if (m.image >= 0) mats[(size_t)HRT_MAT_ROWS * i + 6] = geometry(m.image);
        if (m.normal_map >= 0) mats[(size_t)HRT_MAT_ROWS * i + 7] = geometry(m.normal_map);
    }
    return HRT_OK;
}

// ---- per mesh: what is checked before any of its arrays is followed
int check_mesh(const hrt_scene_desc &D, const hrt_mesh &M, std::string &error) {
    if (M.material < 0 || (uint32_t)M.material >= D.n_materials) return refuse(error, "mesh material out of range");
    for (uint32_t k = 0; k < 3 * M.n_triangles; ++k)
        if (M.indices[k] >= M.n_vertices) return refuse(error, "mesh vertex index out of range");
    if (M.n_leaf_tris && (M.kd_root == HRT_KD_NIL || !M.kd_units || !M.n_kd_units))
        return refuse(error, "mesh has triangles but no flattened KD-tree");
    if (M.n_exceptions && !M.exceptions) return refuse(error, "mesh exceptions missing");
    return HRT_OK;
}

// A ref of M's tree names units inside kd_units (HRT_KD_NIL names none).
bool kd_in_range(const hrt_mesh &M, uint32_t ref) {
    if (ref == HRT_KD_NIL) return true;
    const uint32_t idx = ref & ~HRT_KD_LEAF;
    return (uint64_t)idx + ((ref & HRT_KD_LEAF) ? 4u : 1u) <= M.n_kd_units;
}

// The child links must form a TREE: a nodelet reached twice (a shared subtree, or a cycle -- on which a walk would descend
// forever) is refused.  reached[unit]: 1 = an inner nodelet of the tree, 2 = a leaf of the tree.
int kd_reach(const hrt_mesh &M, std::vector<uint8_t> &reached, std::string &error) {
    reached.assign(M.n_kd_units, 0);
    std::vector<uint32_t> stack{M.kd_root};
    reached[M.kd_root & ~HRT_KD_LEAF] = (M.kd_root & HRT_KD_LEAF) ? 2 : 1;
    while (!stack.empty()) {
        const uint32_t ref = stack.back();
        stack.pop_back();
        if (ref & HRT_KD_LEAF) continue;
        const hrt_kdunit &u = M.kd_units[ref];
        for (int c = 2; c < 4; ++c) {
            const uint32_t child = u.w[c];
            if (child == HRT_KD_NIL || !kd_in_range(M, child) || reached[child & ~HRT_KD_LEAF]) return refuse(error, "malformed flattened KD-tree (a nodelet is reached twice through child links)");
            reached[child & ~HRT_KD_LEAF] = (child & HRT_KD_LEAF) ? 2 : 1;
            stack.push_back(child);
        }
    }
    return HRT_OK;
}

// ---- per mesh: the KD-tree, re-laid for the walk behind the trees of the meshes before it; root = its rebased ref.
// The caller's tree (include/hrt.h: 16-byte inner nodelets, 64-byte leaves, any numbering) becomes:
//   inner nodes: TREELETS of two levels in 32 bytes  {split, left child's split, right child's split, axes}
//   {refs of the four grandchildren}  (axes: 2 bits per node; 3 = the child is a leaf, both exits of its pair hold its ref),
//   one for the root, one for every grandchild that is an inner node and one for every inner node a rope points at --
//   a walk then descends two levels per round trip (csrc/hrt_kernels.hip kd_descend);
//   leaves keep their four units {lo, first} {hi, count} {ropes -x +x -y +y} {ropes -z +z}, refs translated, on 64-byte lines.
// Numbering is breadth-first from the root, so a prefix of the array is the top of the tree (what the kernels stage in LDS).
// Only well-formed nodelets the ROOT reaches through child links are accepted, as what they are: a rope, too, may only name
// such a nodelet, with its own kind (an inner unit named as a leaf would be read as four units from a two-unit slot).
int relay_kd(const hrt_mesh &M, std::vector<uint4> &units, uint32_t &root, uint32_t &max_leaf, std::string &error) {
    units.resize((units.size() + 3u) & ~(size_t)3u, make_uint4(0, 0, 0, 0));  // every mesh's nodelets start on a 64-byte line (the host aligns clusters and leaves)
    const uint32_t unit_base = (uint32_t)units.size();
    root = HRT_KD_NIL;
    if (!M.n_leaf_tris) return HRT_OK;
    if (M.kd_root == HRT_KD_NIL || !kd_in_range(M, M.kd_root)) return refuse(error, "malformed flattened KD-tree");
    std::vector<uint8_t> reached;
    if (const int rc = kd_reach(M, reached, error)) return rc;
    std::vector<uint32_t> new_of(M.n_kd_units, 0xFFFFFFFFu);  // caller's unit index -> unit index in this mesh's new list
    std::vector<uint32_t> order;                               // caller's refs in the order they are laid out
    uint32_t cur = 0;
    bool ok = true;
    auto want = [&](uint32_t ref) {
        if (ref == HRT_KD_NIL) return;
        if (!kd_in_range(M, ref)) { ok = false; return; }
        const uint32_t idx = ref & ~HRT_KD_LEAF;
        if (reached[idx] != ((ref & HRT_KD_LEAF) ? 2 : 1)) { ok = false; return; }  // (ropes: child links were checked by kd_reach)
        if (new_of[idx] != 0xFFFFFFFFu) return;
        const uint32_t size = (ref & HRT_KD_LEAF) ? 4u : 2u;
        cur = (cur + size - 1u) & ~(size - 1u);
        new_of[idx] = cur;
        cur += size;
        order.push_back(ref);
    };
    auto inner_ok = [&](const hrt_kdunit &u) { return u.w[1] <= 2u && u.w[2] != HRT_KD_NIL && u.w[3] != HRT_KD_NIL && kd_in_range(M, u.w[2]) && kd_in_range(M, u.w[3]); };
    want(M.kd_root);
    for (size_t q = 0; ok && q < order.size(); ++q) {
        const uint32_t ref = order[q], idx = ref & ~HRT_KD_LEAF;
        const hrt_kdunit *u = M.kd_units + idx;
        if (ref & HRT_KD_LEAF) {
            if ((uint64_t)u[0].w[3] + u[1].w[3] > M.n_leaf_tris) { ok = false; break; }
            if (u[1].w[3] >= 0xFFFFu) return refuse(error, "KD leaf with 65535 or more triangles (the resumable walk keeps a 16-bit leaf cursor): build the tree with a smaller leaf_max");
            max_leaf = std::max(max_leaf, u[1].w[3]);
            for (int f = 0; f < 4; ++f) want(u[2].w[f]);
            want(u[3].w[0]);
            want(u[3].w[1]);
        } else {
            if (!inner_ok(*u)) { ok = false; break; }
            for (int c = 0; c < 2 && ok; ++c) {
                const uint32_t child = u->w[2 + c];
                if (child & HRT_KD_LEAF) { want(child); continue; }
                const hrt_kdunit &y = M.kd_units[child];
                if (!inner_ok(y)) { ok = false; break; }
                want(y.w[2]);
                want(y.w[3]);
            }
        }
    }
    if (!ok) return refuse(error, "malformed flattened KD-tree (a link or rope names a unit that is not a nodelet of this tree, or not of that kind)");
    auto tr = [&](uint32_t ref) -> uint32_t { return ref == HRT_KD_NIL ? ref : ((new_of[ref & ~HRT_KD_LEAF] + unit_base) | (ref & HRT_KD_LEAF)); };
    units.resize(unit_base + ((cur + 3u) & ~3u), make_uint4(0, 0, 0, 0));
    for (uint32_t ref : order) {
        const uint32_t idx = ref & ~HRT_KD_LEAF;
        const hrt_kdunit *u = M.kd_units + idx;
        uint4 *o = &units[unit_base + new_of[idx]];
        if (ref & HRT_KD_LEAF) {
            o[0] = make_uint4(u[0].w[0], u[0].w[1], u[0].w[2], u[0].w[3]);
            o[1] = make_uint4(u[1].w[0], u[1].w[1], u[1].w[2], u[1].w[3]);
            o[2] = make_uint4(tr(u[2].w[0]), tr(u[2].w[1]), tr(u[2].w[2]), tr(u[2].w[3]));
            o[3] = make_uint4(tr(u[3].w[0]), tr(u[3].w[1]), 0, 0);
        } else {
            uint32_t split[2] = {0, 0}, axis[2] = {3, 3}, exits[4];
            for (int c = 0; c < 2; ++c) {
                const uint32_t child = u->w[2 + c];
                if (child & HRT_KD_LEAF) {
                    exits[2 * c] = exits[2 * c + 1] = tr(child);
                } else {
                    const hrt_kdunit &y = M.kd_units[child];
                    split[c] = y.w[0]; axis[c] = y.w[1];
                    exits[2 * c] = tr(y.w[2]); exits[2 * c + 1] = tr(y.w[3]);
                }
            }
            o[0] = make_uint4(u->w[0], split[0], split[1], u->w[1] | (axis[0] << 2) | (axis[1] << 4));
            o[1] = make_uint4(exits[0], exits[1], exits[2], exits[3]);
        }
    }
    root = tr(M.kd_root);
    return HRT_OK;
}

// ---- per mesh: the triangle soup in leaf order
int pack_soup(const hrt_mesh &M, std::vector<float4> &tris, std::vector<float4> &planes, std::string &error) {
    for (uint32_t k = 0; k < M.n_leaf_tris; ++k) {
        const uint32_t t = M.leaf_tris[k];
        if (t >= M.n_triangles) return refuse(error, "leaf triangle id out of range");
        push_triangle(M, t, tris, planes);
    }
    return HRT_OK;
}

// ---- per mesh: irregular triangles (include/hrt.h hrt_tri_exception), grouped by TRIANGLE.  The reference tests such a
// triangle when the ray passes a leaf box that holds it (KDTree.cpp:32-46), and the outcome of the triangle test does not
// depend on which box that was: so each irregular triangle is folded once (its rows sit behind the mesh's leaf-ordered soup)
// and tested at most once per ray, and only a ray that HITS it closer than the best so far goes through the list of its
// reference boxes (exact AABB.h:48-65 arithmetic) to learn whether the reference would have tested it at all.
// Entries, 2 rows each, threaded depth-first:
//   inner   {lo', HRT_EXC_INNER} {hi', skip}     padded bounds of a subtree: only culls
//   leaf    {cull lo, soup slot} {cull hi, nb}   then nb box entries {box lo, last} {box hi, 0} the walk jumps over; the boxes of one
//           reference leaf follow each other (`last` = 1 on the final one) and must ALL be passed for that leaf to count
// The cull box of a well-conditioned triangle is its own padded bounds (an accepted hit point lies in the triangle up to
// the rounding of the barycentric solve, ~1e-7 / sin^2); a sliver's barycentric test accepts points anywhere in its
// plane, so its cull box is the padded union of its reference boxes (a ray that passes none of them is not tested).
struct ExcGroup { float lo[3], hi[3]; uint32_t tri; std::vector<std::array<float, 7>> boxes; };  // cull box; box: lo, hi, 1.f on the last box of its leaf

// One group per irregular triangle: its distinct boxes by reference leaf, and its cull box.
int group_exceptions(const hrt_mesh &M, std::vector<ExcGroup> &groups, std::string &error) {
    std::vector<uint32_t> order(M.n_exceptions);
    for (uint32_t k = 0; k < M.n_exceptions; ++k) {
        if (M.exceptions[k].triangle >= M.n_triangles) return refuse(error, "exception triangle id out of range");
        order[k] = k;
    }
    static_assert(offsetof(hrt_tri_exception, box_max) == offsetof(hrt_tri_exception, box_min) + 12, "box_min and box_max are contiguous");
    auto box_cmp = [&](uint32_t x, uint32_t y) { return std::memcmp(M.exceptions[x].box_min, M.exceptions[y].box_min, 24); };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {   // by triangle, then by reference leaf (the caller's order inside a leaf)
        const hrt_tri_exception &ex = M.exceptions[x], &ey = M.exceptions[y];
        return ex.triangle < ey.triangle || (ex.triangle == ey.triangle && ex.group < ey.group);
    });
    for (size_t q = 0; q < order.size(); ++q) {
        const hrt_tri_exception &e = M.exceptions[order[q]];
        const bool same_tri = !groups.empty() && groups.back().tri == e.triangle;
        const bool same_leaf = same_tri && q > 0 && M.exceptions[order[q - 1]].group == e.group;
        if (!same_tri) {
            groups.emplace_back();
            groups.back().tri = e.triangle;
        }
        if (same_leaf && box_cmp(order[q - 1], order[q]) == 0) continue;  // the same box twice
        if (!same_leaf && !groups.back().boxes.empty()) groups.back().boxes.back()[6] = 1.f;  // the previous leaf's boxes end here
        std::array<float, 7> bx;
        std::memcpy(bx.data(), e.box_min, 24);
        bx[6] = 0.f;
        groups.back().boxes.push_back(bx);
    }
    for (ExcGroup &g : groups) g.boxes.back()[6] = 1.f;
    for (ExcGroup &g : groups) {
        double c[3][3];
        for (int j = 0; j < 3; ++j) {
            const float *pp = M.positions + 3 * (size_t)M.indices[3 * (size_t)g.tri + j];
            for (int a = 0; a < 3; ++a) c[j][a] = (double)(pp[a] * HRT_TRIANGLE_SCALING);
        }
        double e1[3], e2[3], cr[3];
        for (int a = 0; a < 3; ++a) { e1[a] = c[1][a] - c[0][a]; e2[a] = c[2][a] - c[0][a]; }
        cr[0] = e1[1] * e2[2] - e1[2] * e2[1]; cr[1] = e1[2] * e2[0] - e1[0] * e2[2]; cr[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const double l1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], l2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
        const double sin2 = (cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) / (l1 * l2);
        const bool own_bounds = std::isfinite(sin2) && sin2 >= 1e-2;  // NaN (zero edge): the union of the boxes
        for (int a = 0; a < 3; ++a) {
            double lo = INFINITY, hi = -INFINITY;
            if (own_bounds) {
                for (int j = 0; j < 3; ++j) { lo = std::min(lo, c[j][a]); hi = std::max(hi, c[j][a]); }
            } else {
                for (const auto &bx : g.boxes) {  // (AABB::intersects reads a box's faces in either order: a cut outside its node leaves one)
                    lo = std::min(lo, (double)std::min(bx[a], bx[3 + a])); hi = std::max(hi, (double)std::max(bx[a], bx[3 + a]));
                }
            }
            double ext = 0.0;
            for (int x = 0; x < 3; ++x) ext = std::max(ext, std::max(std::fabs(e1[x]), std::fabs(e2[x])));
            const double pad = (own_bounds ? 1e-3 * ext : 0.0) + 1e-4 * std::max(1.0, std::max(std::fabs(lo), std::fabs(hi)));
            g.lo[a] = (float)(lo - pad); g.hi[a] = (float)(hi + pad);
        }
    }
    return HRT_OK;
}

// The entries of groups [lo, hi), depth-first: one group is a leaf entry with its boxes (its triangle folded behind the soup);
// more are split at the median of their centres along the widest axis, under an inner entry.
void emit_exceptions(const hrt_mesh &M, std::vector<ExcGroup> &g, size_t lo, size_t hi, size_t first_entry, std::vector<float4> &tris,
                     std::vector<float4> &planes, std::vector<float4> &out) {
    if (hi - lo == 1) {
        const ExcGroup &b = g[lo];
        const uint32_t slot = (uint32_t)(tris.size() / HRT_TRI_ROWS);
        push_triangle(M, b.tri, tris, planes);
        out.push_back(make_float4(b.lo[0], b.lo[1], b.lo[2], as_float(slot)));
        out.push_back(make_float4(b.hi[0], b.hi[1], b.hi[2], as_float((uint32_t)b.boxes.size())));
        for (const auto &bx : b.boxes) {
            out.push_back(make_float4(bx[0], bx[1], bx[2], as_float(bx[6] != 0.f ? 1u : 0u)));  // .w: 1 = the last box of its reference leaf
            out.push_back(make_float4(bx[3], bx[4], bx[5], 0.f));
        }
        return;
    }
    float bmin[3] = {INFINITY, INFINITY, INFINITY}, bmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    float cmin[3] = {INFINITY, INFINITY, INFINITY}, cmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = lo; i < hi; ++i)
        for (int a = 0; a < 3; ++a) {
            bmin[a] = std::min(bmin[a], g[i].lo[a]); bmax[a] = std::max(bmax[a], g[i].hi[a]);
            const float c = 0.5f * (g[i].lo[a] + g[i].hi[a]);
            cmin[a] = std::min(cmin[a], c); cmax[a] = std::max(cmax[a], c);
        }
    int axis = 0;
    for (int a = 1; a < 3; ++a) if (cmax[a] - cmin[a] > cmax[axis] - cmin[axis]) axis = a;
    const size_t mid = lo + (hi - lo) / 2;
    std::nth_element(g.begin() + lo, g.begin() + mid, g.begin() + hi, [axis](const ExcGroup &x, const ExcGroup &y) {
        const float cx = x.lo[axis] + x.hi[axis], cy = y.lo[axis] + y.hi[axis];
        return cx < cy || (cx == cy && x.tri < y.tri);
    });
    const size_t self = out.size();
    float pmin[3], pmax[3];
    for (int a = 0; a < 3; ++a) {
        const float pad = 1e-4f * std::max(1.f, std::max(std::fabs(bmin[a]), std::fabs(bmax[a])));
        pmin[a] = bmin[a] - pad; pmax[a] = bmax[a] + pad;
    }
    out.push_back(make_float4(pmin[0], pmin[1], pmin[2], as_float(HRT_EXC_INNER)));
    out.push_back(make_float4(pmax[0], pmax[1], pmax[2], 0.f));
    emit_exceptions(M, g, lo, mid, first_entry, tris, planes, out);
    emit_exceptions(M, g, mid, hi, first_entry, tris, planes, out);
    out[self + 1].w = as_float((uint32_t)(out.size() / 2 - first_entry));  // skip: first entry behind this subtree, relative to the mesh's list
}

// Appends M's threaded list to `exceptions`; n_exc = its entries.
int thread_exceptions(const hrt_mesh &M, std::vector<float4> &tris, std::vector<float4> &planes, std::vector<float4> &exceptions, uint32_t &n_exc,
                      std::string &error) {
    n_exc = 0;
    if (!M.n_exceptions) return HRT_OK;
    std::vector<ExcGroup> groups;
    if (const int rc = group_exceptions(M, groups, error)) return rc;
    const size_t first_entry = exceptions.size() / 2;
    emit_exceptions(M, groups, 0, groups.size(), first_entry, tris, planes, exceptions);
    n_exc = (uint32_t)(exceptions.size() / 2 - first_entry);
    return HRT_OK;
}

// ---- per mesh: face colours, or vertex colours with the triangles' vertex ids
void pack_colors(const hrt_mesh &M, DMesh &dm, std::vector<float4> &colors, std::vector<uint4> &vids) {
    dm.color_type = HRT_COLOR_NONE;
    if (M.color_type == HRT_COLOR_FACE && M.face_colors) {
        dm.color_type = HRT_COLOR_FACE;
        dm.color_base = (uint32_t)colors.size();
        for (uint32_t t = 0; t < M.n_triangles; ++t)
            colors.push_back(make_float4(M.face_colors[3 * t], M.face_colors[3 * t + 1], M.face_colors[3 * t + 2], 0.f));
    } else if (M.color_type == HRT_COLOR_VERTEX && M.vert_colors) {
        dm.color_type = HRT_COLOR_VERTEX;
        dm.vcolor_base = (uint32_t)colors.size();
        for (uint32_t v = 0; v < M.n_vertices; ++v)
            colors.push_back(make_float4(M.vert_colors[3 * v], M.vert_colors[3 * v + 1], M.vert_colors[3 * v + 2], 0.f));
        dm.color_base = (uint32_t)vids.size();
        for (uint32_t t = 0; t < M.n_triangles; ++t)
            vids.push_back(make_uint4(M.indices[3 * t], M.indices[3 * t + 1], M.indices[3 * t + 2], 0));
    }
}

// ---- one mesh: its record, with its nodelets (refs rebased), leaf-ordered soup, exception list and colours behind those of
// the meshes before it
int pack_mesh(const hrt_scene_desc &D, const hrt_mesh &M, PackedScene &P, std::vector<DMesh> &meshes, std::string &error) {
    if (const int rc = check_mesh(D, M, error)) return rc;
    DMesh dm;
    std::memset(&dm, 0, sizeof(dm));
    for (int a = 0; a < 3; ++a) {
        dm.aabb_lo[a] = M.aabb_min[a]; dm.aabb_hi[a] = M.aabb_max[a];
        dm.kd_lo[a] = M.kd_min[a]; dm.kd_hi[a] = M.kd_max[a];
    }
    if (const int rc = relay_kd(M, P.units, dm.root, P.max_leaf, error)) return rc;
    dm.tri_base = (uint32_t)(P.tris.size() / HRT_TRI_ROWS);
    dm.n_soup = M.n_leaf_tris;
    if (const int rc = pack_soup(M, P.tris, P.planes, error)) return rc;
    dm.exc_base = (uint32_t)(P.exceptions.size() / 2);
    if (const int rc = thread_exceptions(M, P.tris, P.planes, P.exceptions, dm.n_exc, error)) return rc;
    dm.material = (uint32_t)M.material;
    pack_colors(M, dm, P.colors, P.vids);
    meshes.push_back(dm);
    return HRT_OK;
}

// ---- squares | materials | spheres | mesh records | sphere pair filter (| short exception lists) in one array, and its offsets
void layout_tabs(const PackTables &T, PackedScene &P) {
    static_assert(sizeof(DMesh) % sizeof(float4) == 0, "mesh records are whole rows");
    std::vector<float4> &tabs = P.tabs;
    DScene &d = P.header;
    d.tab_quads = 0;
    tabs.insert(tabs.end(), T.quads.begin(), T.quads.end());
    d.tab_mats = (uint32_t)tabs.size();
    tabs.insert(tabs.end(), T.mats.begin(), T.mats.end());
    d.tab_spheres = (uint32_t)tabs.size();
    tabs.insert(tabs.end(), T.spheres.begin(), T.spheres.end());
    d.tab_meshes = (uint32_t)tabs.size();
    tabs.resize(tabs.size() + T.meshes.size() * (sizeof(DMesh) / sizeof(float4)));
    if (!T.meshes.empty()) std::memcpy(&tabs[d.tab_meshes], T.meshes.data(), T.meshes.size() * sizeof(DMesh));
    d.tab_sfilter = (uint32_t)tabs.size();
    tabs.insert(tabs.end(), T.sfilter.begin(), T.sfilter.end());
    d.tab_exc = (uint32_t)tabs.size();
    d.exc_in_tabs = P.exceptions.size() <= 1536u ? 1u : 0u;  // short exception lists ride along (24 KB at most)
    if (d.exc_in_tabs) tabs.insert(tabs.end(), P.exceptions.begin(), P.exceptions.end());
    d.tab_rows = (uint32_t)tabs.size();
}

// ---- exact path pruning needs 0 x value == 0 for every value a zero throughput meets, and a finite throughput wherever a
// pruned term is dropped (hrt_device.h DScene::prune_ok).  Bounded in fp64: the throughput is a product of at most
// HRT_MAXBOUNCES albedo-like colours (albedos, checkers, mesh colours; texels are bytes <= 1), and what it multiplies is
// an emission (light colour or checker x intensity), the direct-light sum (lights x light colour x albedo x |1 - t|)
// or the sky (<= HRT_MAXBOUNCES + 1).  Below FLT_MAX / 2 (room for fp32 rounding) no term of a path can overflow.
uint32_t prune_bound(const hrt_scene_desc &D, const std::vector<float4> &colors) {
    bool finite = true;
    auto mag = [&](float v) { finite = finite && std::isfinite(v); return std::fabs((double)v); };
    auto mag3 = [&](const float *v) { return std::max(mag(v[0]), std::max(mag(v[1]), mag(v[2]))); };
    double albedo = 1.0, emit = 0.0, transmit = 1.0, light = 0.0;
    for (uint32_t i = 0; i < D.n_materials; ++i) {
        const hrt_material &m = D.materials[i];
        const double checker = std::max(mag3(m.checker1), mag3(m.checker2));
        albedo = std::max(albedo, std::max(mag3(m.albedo), checker));
        const double e = std::max(1.0, std::max(mag3(m.light_color), checker)) * mag(m.light_intensity);
        if (m.emissive) emit = std::max(emit, e);
        transmit = std::max(transmit, std::fabs(1.0 - (double)m.transparency));
        finite = finite && std::isfinite(m.transparency);
    }
    for (uint32_t i = 0; i < D.n_lights; ++i) light = std::max(light, mag3(D.lights[i].color));
    for (const float4 &c : colors) albedo = std::max(albedo, std::max(mag(c.x), std::max(mag(c.y), mag(c.z))));
    const double term = std::max(std::max(emit, (double)HRT_MAXBOUNCES + 1.0), (double)D.n_lights * light * albedo * transmit);
    const double bound = std::pow(albedo, (double)HRT_MAXBOUNCES) * term;
    return (finite && bound < 0.5 * (double)FLT_MAX) ? 1u : 0u;
}

// The stages in order.  The order of the refusals is behaviour: a description with two defects is refused for the first
// one met here.  Returns HRT_OK, or HRT_ERR_INVALID with the reason in `error`.
int pack_scene(const hrt_scene_desc &D, PackedScene &P, std::string &error) {
    P = PackedScene{};
    PackTables T;
    if (const int rc = check_desc(D, error)) return rc;
    P.bound = scene_bound(D);
    pack_primitives(D, T, P);
    if (const int rc = pack_images(D, T.mats, P, error)) return rc;
    for (uint32_t mi = 0; mi < D.n_meshes; ++mi)
        if (const int rc = pack_mesh(D, D.meshes[mi], P, T.meshes, error)) return rc;
    layout_tabs(T, P);
    DScene &d = P.header;
    d.n_spheres = D.n_spheres; d.n_quads = D.n_quads; d.n_meshes = D.n_meshes; d.n_lights = D.n_lights;
    d.n_images = D.n_images;
    d.n_kd_units = (uint32_t)P.units.size();
    d.dark_sky = D.dark_sky;
    d.prune_ok = prune_bound(D, P.colors);
    d.any_motion = 0u;  // (time x 0 == 0 whatever the time: with no motion anywhere a ray's time is never looked at)
    for (uint32_t i = 0; i < D.n_materials; ++i)
        if (!(D.materials[i].motion[0] == 0.f && D.materials[i].motion[1] == 0.f && D.materials[i].motion[2] == 0.f)) d.any_motion = 1u;
    d.skybox_image = (D.skybox_image >= 0 && D.images[D.skybox_image].w >= 1 && D.images[D.skybox_image].h >= 1) ? D.skybox_image : -1;
    return HRT_OK;
}

}  // namespace
