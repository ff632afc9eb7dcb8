// The descriptions pack_check packs, and its two modes.  A case is either one of the host layer's named scenes or built
// by hand here, small, so that every branch of the packing (csrc/hrt_pack.h) is reached; the refusal cases corrupt one
// valid hand-built description in one place each (a few in two, to pin which refusal comes first).
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hrt_host.h"

// Packs a description; with dump, prints the packed scene (pack_dump.h) to stdout when it is accepted.
typedef int (*PackFn)(const hrt_scene_desc &desc, bool dump, std::string &error);

inline uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct MeshStore {
    std::vector<float> pos, fcol, vcol;
    std::vector<uint32_t> idx, leaf_tris;
    std::vector<hrt_kdunit> units;
    std::vector<hrt_tri_exception> exc;
};

struct Case {
    std::vector<hrt_material> materials;
    std::vector<hrt_sphere> spheres;
    std::vector<hrt_quad> quads;
    std::vector<hrt_light> lights;
    std::vector<hrt_image> images;
    std::deque<std::vector<uint8_t>> pixels;
    std::vector<hrt_mesh> meshes, alt_meshes;
    std::deque<MeshStore> stores;
    int32_t dark_sky = 0, skybox = -1;
    hrt_host_scene *host = nullptr;          // a named scene: the host layer owns the description
    const hrt_scene_desc *host_desc = nullptr;
    Case() = default;
    Case(const Case &) = delete;
    ~Case() { if (host) hrt_host_scene_free(host); }

    hrt_scene_desc desc() const {
        if (host_desc) return *host_desc;
        hrt_scene_desc d;
        std::memset(&d, 0, sizeof(d));
        d.n_materials = (uint32_t)materials.size(); d.materials = materials.data();
        d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
        d.n_quads = (uint32_t)quads.size(); d.quads = quads.data();
        d.n_meshes = (uint32_t)meshes.size(); d.meshes = meshes.data();
        d.n_lights = (uint32_t)lights.size(); d.lights = lights.data();
        d.n_images = (uint32_t)images.size(); d.images = images.data();
        d.dark_sky = dark_sky;
        d.skybox_image = skybox;
        return d;
    }
    int32_t add_material(int32_t type = HRT_MAT_DIFFUSE, float mx = 0.f, float my = 0.f, float mz = 0.f) {
        hrt_material m;
        std::memset(&m, 0, sizeof(m));
        m.albedo[0] = 0.5f; m.albedo[1] = 0.6f; m.albedo[2] = 0.7f;
        m.index_medium = 1.4f;
        m.type = type;
        m.checker1[0] = m.checker1[1] = m.checker1[2] = 0.1f;
        m.checker2[0] = m.checker2[1] = m.checker2[2] = 0.9f;
        m.tex_scale_x = 2.f; m.tex_scale_y = 3.f;
        m.light_color[0] = m.light_color[1] = m.light_color[2] = 1.f;
        m.image = m.normal_map = -1;
        m.motion[0] = mx; m.motion[1] = my; m.motion[2] = mz;
        materials.push_back(m);
        return (int32_t)materials.size() - 1;
    }
    int32_t add_image(int32_t w, int32_t h) {
        pixels.emplace_back((size_t)(w > 0 && h > 0 ? 3 * w * h : 0));
        for (size_t i = 0; i < pixels.back().size(); ++i) pixels.back()[i] = (uint8_t)((i * 31u + 7u) % 256u);
        images.push_back(hrt_image{w, h, pixels.back().empty() ? nullptr : pixels.back().data()});
        return (int32_t)images.size() - 1;
    }
    void add_sphere(float x, float y, float z, float r, int32_t material) { spheres.push_back(hrt_sphere{{x, y, z}, r, material}); }
    void add_quad(const float v0[3], const float r[3], const float u[3], int32_t material) {
        hrt_quad q;
        for (int a = 0; a < 3; ++a) {
            q.v0[a] = v0[a]; q.v1[a] = v0[a] + r[a]; q.v3[a] = v0[a] + u[a];
            q.tangent[a] = r[a]; q.bitangent[a] = u[a];
        }
        q.material = material;
        quads.push_back(q);
    }
    void add_light(float x, float y, float z, float r) { lights.push_back(hrt_light{{x, y, z}, r, {1.f, 0.9f, 0.8f}}); }
    void add_exception(MeshStore &S, uint32_t tri, uint32_t group, float lx, float ly, float lz, float hx, float hy, float hz) {
        S.exc.push_back(hrt_tri_exception{tri, {lx, ly, lz}, {hx, hy, hz}, group});
    }
    // points the last mesh at its store's arrays again (after one of them was resized)
    void rebind(hrt_mesh &M, MeshStore &S) {
        M.n_vertices = (uint32_t)(S.pos.size() / 3); M.positions = S.pos.data();
        M.n_triangles = (uint32_t)(S.idx.size() / 3); M.indices = S.idx.data();
        M.vert_colors = S.vcol.empty() ? nullptr : S.vcol.data();
        M.face_colors = S.fcol.empty() ? nullptr : S.fcol.data();
        M.n_kd_units = (uint32_t)S.units.size(); M.kd_units = S.units.data();
        M.n_leaf_tris = (uint32_t)S.leaf_tris.size(); M.leaf_tris = S.leaf_tris.data();
        M.n_exceptions = (uint32_t)S.exc.size(); M.exceptions = S.exc.empty() ? nullptr : S.exc.data();
    }
    MeshStore &add_grid_mesh(uint32_t n, int32_t material, float ox, const std::vector<std::array<float, 9>> &extra_tris = {},
                             const std::vector<uint32_t> &out_of_tree = {});
};

// The hand-laid tree of add_grid_mesh, in the caller's numbering (on purpose not the breadth-first one the packing lays):
// unit 0 is padding, the root at 1 splits x with the inner node 2 (which splits y into the leaves A at 8 and B at 4) on its
// left and the leaf C at 12 on its right.  A and B rope to C and to each other, C ropes back to the inner node 2.
enum : uint32_t { KD_ROOT = 1, KD_LEFT = 2, KD_LEAF_B = 4, KD_LEAF_A = 8, KD_LEAF_C = 12, KD_UNITS = 16 };

// An n x n grid of squares (2 n^2 triangles) at a bumpy height, plus extra triangles given by their corners, under the tree
// above.  The triangles not listed in out_of_tree are dealt to the leaves in thirds; B's last is also C's first.
inline MeshStore &Case::add_grid_mesh(uint32_t n, int32_t material, float ox, const std::vector<std::array<float, 9>> &extra_tris,
                                      const std::vector<uint32_t> &out_of_tree) {
    stores.emplace_back();
    MeshStore &S = stores.back();
    for (uint32_t j = 0; j <= n; ++j)
        for (uint32_t i = 0; i <= n; ++i) {
            S.pos.push_back(ox + (float)i); S.pos.push_back((float)j); S.pos.push_back(0.05f * (float)((i * 7u + j * 3u) % 5u));
        }
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t a = j * (n + 1) + i, b = a + 1, c = a + n + 1, d = c + 1;
            for (uint32_t v : {a, b, d, a, d, c}) S.idx.push_back(v);
        }
    for (const auto &t : extra_tris)
        for (int v = 0; v < 3; ++v) {
            S.idx.push_back((uint32_t)(S.pos.size() / 3));
            for (int a = 0; a < 3; ++a) S.pos.push_back(t[3 * v + a]);
        }
    const uint32_t n_tris = (uint32_t)(S.idx.size() / 3);
    for (uint32_t t = 0; t < n_tris; ++t) {
        bool out = false;
        for (uint32_t o : out_of_tree) out = out || o == t;
        if (!out) S.leaf_tris.push_back(t);
    }
    hrt_mesh M;
    std::memset(&M, 0, sizeof(M));
    M.color_type = HRT_COLOR_NONE;
    M.material = material;
    for (int a = 0; a < 3; ++a) { M.aabb_min[a] = INFINITY; M.aabb_max[a] = -INFINITY; }
    for (size_t v = 0; v < S.pos.size(); ++v) {
        M.aabb_min[v % 3] = std::fmin(M.aabb_min[v % 3], S.pos[v]); M.aabb_max[v % 3] = std::fmax(M.aabb_max[v % 3], S.pos[v]);
    }
    for (int a = 0; a < 3; ++a) { M.kd_min[a] = M.aabb_min[a] - 0.01f; M.kd_max[a] = M.aabb_max[a] + 0.01f; }
    const float midx = ox + 0.5f * (float)n, midy = 0.5f * (float)n;
    const uint32_t third = (uint32_t)S.leaf_tris.size() / 3u, L = HRT_KD_LEAF, NIL = HRT_KD_NIL;
    S.units.assign(KD_UNITS, hrt_kdunit{{0, 0, 0, 0}});
    S.units[KD_ROOT] = hrt_kdunit{{fbits(midx), 0u, KD_LEFT, KD_LEAF_C | L}};
    S.units[KD_LEFT] = hrt_kdunit{{fbits(midy), 1u, KD_LEAF_A | L, KD_LEAF_B | L}};
    auto leaf = [&](uint32_t at, float lx, float ly, float hx, float hy, uint32_t first, uint32_t count, std::array<uint32_t, 6> ropes) {
        S.units[at] = hrt_kdunit{{fbits(lx), fbits(ly), fbits(M.kd_min[2]), first}};
        S.units[at + 1] = hrt_kdunit{{fbits(hx), fbits(hy), fbits(M.kd_max[2]), count}};
        S.units[at + 2] = hrt_kdunit{{ropes[0], ropes[1], ropes[2], ropes[3]}};
        S.units[at + 3] = hrt_kdunit{{ropes[4], ropes[5], 0u, 0u}};
    };
    leaf(KD_LEAF_A, M.kd_min[0], M.kd_min[1], midx, midy, 0u, third, {NIL, KD_LEAF_C | L, NIL, KD_LEAF_B | L, NIL, NIL});
    leaf(KD_LEAF_B, M.kd_min[0], midy, midx, M.kd_max[1], third, third, {NIL, KD_LEAF_C | L, KD_LEAF_A | L, NIL, NIL, NIL});
    leaf(KD_LEAF_C, midx, M.kd_min[1], M.kd_max[0], M.kd_max[1], 2u * third - 1u, (uint32_t)S.leaf_tris.size() - (2u * third - 1u), {KD_LEFT, NIL, NIL, NIL, NIL, NIL});
    M.kd_root = KD_ROOT;
    rebind(M, S);
    meshes.push_back(M);
    return S;
}

inline void add_colors(Case &c, MeshStore &S, hrt_mesh &M, int32_t color_type) {
    for (size_t k = 0; k < S.idx.size(); ++k) S.fcol.push_back((float)((k * 37u) % 256u) / 255.f);
    for (size_t k = 0; k < S.pos.size(); ++k) S.vcol.push_back((float)((k * 91u + 5u) % 256u) / 255.f);
    c.rebind(M, S);
    M.color_type = color_type;
}

const char *const k_named_scenes[] = {"cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool"};
const char *const k_hash_cases[] = {"cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool", "empty", "spheres_odd", "quads",
                                    "light_skybox", "skybox_empty", "prune_off", "mesh_colors", "mesh_irregular", "mesh_exc_long"};

inline std::unique_ptr<Case> make_hash_case(const std::string &name, const char *assets) {
    std::unique_ptr<Case> c(new Case());
    for (const char *scene : k_named_scenes)
        if (name == scene) {   // the five named scenes at seed 1
            if (hrt_host_scene_new(assets, &c->host) || hrt_host_scene_setup(c->host, scene, 16.f / 9.f, 1) ||
                hrt_host_scene_flatten(c->host, &c->host_desc)) {
                std::fprintf(stderr, "pack_check: %s: %s\n", scene, hrt_host_last_error());
                return nullptr;
            }
            return c;
        }
    if (name == "empty") {
    } else if (name == "spheres_odd") {   // an odd count (the last pairs with itself), one moving, one of negative radius
        const int32_t still = c->add_material(), moving = c->add_material(HRT_MAT_DIFFUSE, 0.f, 0.25f, 0.f);
        c->add_sphere(0.f, 0.f, -3.f, 1.f, still);
        c->add_sphere(2.f, 0.5f, -4.f, 0.5f, moving);
        c->add_sphere(-2.f, -0.5f, -5.f, -0.75f, still);
    } else if (name == "quads") {   // tilted; one in each axis plane (one of them facing backwards); glass; moving; one without extent
        const int32_t wall = c->add_material(), glass = c->add_material(HRT_MAT_GLASS), moving = c->add_material(HRT_MAT_DIFFUSE, 0.1f, 0.f, 0.f);
        const float o[3] = {0.f, 0.f, 0.f}, p[3] = {-1.f, 2.f, -3.f}, x[3] = {2.f, 0.f, 0.f}, y[3] = {0.f, 1.5f, 0.f}, z[3] = {0.f, 0.f, 3.f};
        const float tr[3] = {1.f, 0.3f, 0.2f}, tu[3] = {-0.2f, 1.f, 0.4f}, none[3] = {0.f, 0.f, 0.f};
        c->add_quad(o, tr, tu, wall);
        c->add_quad(p, x, y, wall);
        c->add_quad(p, y, z, wall);
        c->add_quad(p, z, x, wall);
        c->add_quad(o, y, x, wall);
        c->add_quad(p, x, z, glass);
        c->add_quad(o, x, y, moving);
        c->add_quad(o, none, y, wall);
    } else if (name == "light_skybox" || name == "skybox_empty") {   // a light, textures on a material, a skybox (with and without pixels)
        const int32_t tex = c->add_image(4, 3), nmap = c->add_image(2, 2), sky = name == "skybox_empty" ? c->add_image(0, 0) : c->add_image(8, 4);
        const int32_t m = c->add_material();
        c->materials[m].texture_type = HRT_TEX_IMAGE; c->materials[m].image = tex; c->materials[m].normal_map = nmap;
        const int32_t lamp = c->add_material();
        c->materials[lamp].emissive = 1; c->materials[lamp].light_intensity = 5.f;
        c->add_sphere(0.f, 0.f, -3.f, 1.f, m);
        c->add_sphere(0.f, 3.f, -3.f, 0.5f, lamp);
        c->add_light(1.f, 4.f, 2.f, 0.3f);
        c->skybox = sky;
        c->dark_sky = 1;
    } else if (name == "prune_off") {   // an albedo whose sixth power leaves fp32
        const int32_t m = c->add_material();
        c->materials[m].albedo[1] = 1e30f;
        c->add_sphere(0.f, 0.f, -3.f, 1.f, m);
    } else if (name == "mesh_colors") {   // face colours, vertex colours, and a mesh with nothing in its tree
        const int32_t m = c->add_material();
        MeshStore &faces = c->add_grid_mesh(3, m, 0.f);
        add_colors(*c, faces, c->meshes.back(), HRT_COLOR_FACE);
        MeshStore &verts = c->add_grid_mesh(2, m, 5.f);
        add_colors(*c, verts, c->meshes.back(), HRT_COLOR_VERTEX);
        MeshStore &S = c->add_grid_mesh(1, m, 9.f);
        S.leaf_tris.clear();
        c->rebind(c->meshes.back(), S);
        c->meshes.back().kd_root = HRT_KD_NIL;
    } else if (name == "mesh_irregular") {
        // triangle 18 is a sliver, 19 has a zero edge; 2, 5 and 7 are well-conditioned.  Five groups (inner entries and skips),
        // given out of order: 18 sits in two reference leaves, 19 has one box twice and a second box in the same leaf, one box
        // of 5 has its faces the other way round.
        const int32_t m = c->add_material();
        MeshStore &S = c->add_grid_mesh(3, m, 0.f, {{0.f, 0.f, 1.f, 2.f, 0.f, 1.f, 1.f, 1e-5f, 1.f}, {0.f, 0.f, 2.f, 0.f, 0.f, 2.f, 1.f, 0.f, 2.f}}, {2, 5, 7, 18, 19});
        c->add_exception(S, 19, 0, -0.1f, -0.1f, 1.9f, 1.1f, 0.1f, 2.1f);
        c->add_exception(S, 7, 0, 0.f, 1.f, -0.1f, 1.5f, 2.f, 0.3f);
        c->add_exception(S, 18, 1, 1.f, -0.5f, 0.5f, 2.5f, 0.5f, 1.5f);
        c->add_exception(S, 19, 0, -0.1f, -0.1f, 1.9f, 1.1f, 0.1f, 2.1f);
        c->add_exception(S, 2, 0, 0.5f, -0.2f, -0.1f, 2.2f, 1.2f, 0.4f);
        c->add_exception(S, 18, 0, -0.5f, -0.5f, 0.5f, 1.f, 0.5f, 1.5f);
        c->add_exception(S, 19, 0, -0.3f, -0.2f, 1.5f, 0.5f, 0.2f, 2.5f);
        c->add_exception(S, 5, 3, 3.1f, 2.f, 0.4f, 1.9f, 0.9f, -0.1f);
        c->rebind(c->meshes.back(), S);
    } else if (name == "mesh_exc_long") {   // 300 irregular triangles of two boxes each: more than 1536 rows, so the list stays out of `tabs`
        const int32_t m = c->add_material();
        MeshStore &S = c->add_grid_mesh(13, m, 0.f);
        for (uint32_t t = 0; t < 300; ++t)
            for (uint32_t g = 0; g < 2; ++g) {
                const float x = (float)(t % 26u) * 0.5f, y = (float)(t / 26u);
                c->add_exception(S, t, g, x - 0.6f + (float)g, y - 0.1f, -0.1f, x + 0.6f + (float)g, y + 1.1f, 0.4f);
            }
        c->rebind(c->meshes.back(), S);
    } else {
        std::fprintf(stderr, "pack_check: no hash case '%s'\n", name.c_str());
        return nullptr;
    }
    return c;
}

// The valid description every refusal case starts from: two images, three materials (one textured), a sphere, a square, a light,
// a skybox and a grid mesh with two irregular triangles.
inline void make_refuse_base(Case &c) {
    c.add_image(4, 3);
    c.add_image(2, 2);
    const int32_t m = c.add_material();
    const int32_t tex = c.add_material();
    c.materials[tex].image = 0; c.materials[tex].normal_map = 1;
    c.add_material(HRT_MAT_GLASS);
    c.add_sphere(0.f, 0.f, -3.f, 1.f, tex);
    const float o[3] = {0.f, 0.f, 0.f}, x[3] = {2.f, 0.f, 0.f}, y[3] = {0.f, 1.5f, 0.f};
    c.add_quad(o, x, y, m);
    c.add_light(1.f, 4.f, 2.f, 0.3f);
    c.skybox = 0;
    MeshStore &S = c.add_grid_mesh(3, m, 0.f, {}, {2, 5});
    c.add_exception(S, 2, 0, 0.5f, -0.2f, -0.1f, 2.2f, 1.2f, 0.4f);
    c.add_exception(S, 5, 0, 1.9f, 0.9f, -0.1f, 3.1f, 2.f, 0.4f);
    c.rebind(c.meshes.back(), S);
}

struct RefuseCase {
    const char *name;
    std::function<hrt_scene_desc(Case &)> corrupt;  // corrupts the base in place and returns its description
};

inline hrt_scene_desc with_meshes(Case &c) {
    hrt_scene_desc d = c.desc();
    d.n_meshes = (uint32_t)c.alt_meshes.size(); d.meshes = c.alt_meshes.data();
    return d;
}
inline hrt_mesh huge_soup_mesh() {   // counts alone, every array pointer null
    hrt_mesh M;
    std::memset(&M, 0, sizeof(M));
    M.n_leaf_tris = HRT_MAX_SOUP_SLOTS; M.n_exceptions = 5; M.n_triangles = 1; M.n_vertices = 3;
    return M;
}

inline std::vector<RefuseCase> refuse_cases() {
    const uint32_t L = HRT_KD_LEAF;
#define MESH c.meshes[0]
#define STORE c.stores[0]
#define CASE(name, ...) {name, [=](Case &c) -> hrt_scene_desc { __VA_ARGS__; return c.desc(); }}
    return {
        CASE("material_image_range", c.materials[0].image = 2),
        CASE("material_normal_map_range", c.materials[0].normal_map = 2),
        CASE("material_type_low", c.materials[0].type = -1),
        CASE("material_type_high", c.materials[0].type = 3),
        CASE("texture_type_low", c.materials[0].texture_type = -1),
        CASE("texture_type_high", c.materials[0].texture_type = 3),
        CASE("normal_map_empty_w", c.images[1].w = 0),
        CASE("normal_map_empty_h", c.images[1].h = 0),
        CASE("sphere_material_low", c.spheres[0].material = -1),
        CASE("sphere_material_high", c.spheres[0].material = 3),
        CASE("quad_material_low", c.quads[0].material = -1),
        CASE("quad_material_high", c.quads[0].material = 3),
        CASE("mesh_material_low", MESH.material = -1),
        CASE("mesh_material_high", MESH.material = 3),
        CASE("skybox_range", c.skybox = 2),
        {"lights_missing", [](Case &c) { hrt_scene_desc d = c.desc(); d.lights = nullptr; return d; }},
        {"meshes_33", [](Case &c) { c.alt_meshes.assign(33, c.meshes[0]); return with_meshes(c); }},
        {"soup_limit", [](Case &c) { c.alt_meshes.assign(1, huge_soup_mesh()); return with_meshes(c); }},
        CASE("image_without_pixels", c.images[0].rgb = nullptr),
        CASE("vertex_index_range", STORE.idx[4] = MESH.n_vertices),
        CASE("no_tree_root_nil", MESH.kd_root = HRT_KD_NIL),
        CASE("no_tree_units_null", MESH.kd_units = nullptr),
        CASE("no_tree_no_units", MESH.n_kd_units = 0),
        CASE("exceptions_missing", MESH.exceptions = nullptr),
        CASE("kd_root_range_inner", MESH.kd_root = KD_UNITS),
        CASE("kd_root_range_leaf", MESH.kd_root = (KD_UNITS - 3u) | L),
        CASE("child_nil", STORE.units[KD_ROOT].w[2] = HRT_KD_NIL),
        CASE("child_range", STORE.units[KD_ROOT].w[3] = (KD_UNITS - 2u) | L),
        CASE("child_shared_subtree", STORE.units[KD_LEFT].w[3] = KD_LEAF_C | L),
        CASE("child_cycle_to_root", STORE.units[KD_LEFT].w[2] = KD_ROOT),
        CASE("rope_inner_as_leaf", STORE.units[KD_LEAF_A + 2].w[0] = KD_LEFT | L),
        CASE("rope_leaf_as_inner", STORE.units[KD_LEAF_A + 2].w[0] = KD_LEAF_B),
        CASE("rope_unreached", STORE.units[KD_LEAF_A + 2].w[0] = 0u),
        CASE("rope_range", STORE.units[KD_LEAF_A + 3].w[1] = (KD_UNITS - 1u) | L),
        CASE("inner_axis_root", STORE.units[KD_ROOT].w[1] = 3u),
        CASE("inner_axis_child", STORE.units[KD_LEFT].w[1] = 3u),
        CASE("leaf_range", STORE.units[KD_LEAF_C + 1].w[3] += 1u),
        CASE("leaf_count_65535", STORE.leaf_tris.resize(70000u, 0u); c.rebind(MESH, STORE); STORE.units[KD_LEAF_C + 1].w[3] = 65535u),
        CASE("leaf_triangle_range", STORE.leaf_tris[1] = MESH.n_triangles),
        CASE("exception_triangle_range", STORE.exc[1].triangle = MESH.n_triangles),
        // two defects: the first one met in the order of the packing is the one named
        CASE("first_sphere_then_meshes", c.spheres[0].material = 3; MESH.material = 3),
        CASE("first_image_then_mesh", c.images[0].rgb = nullptr; MESH.material = 3),
        CASE("first_vertex_then_root", STORE.idx[4] = MESH.n_vertices; MESH.kd_root = KD_UNITS),
        CASE("first_tree_then_leaf_triangle", STORE.units[KD_ROOT].w[1] = 3u; STORE.leaf_tris[1] = MESH.n_triangles),
        CASE("first_leaf_triangle_then_exception", STORE.leaf_tris[1] = MESH.n_triangles; STORE.exc[1].triangle = MESH.n_triangles),
        {"first_mesh0_leaf_triangle_then_mesh1_material", [](Case &c) {
             c.stores[0].leaf_tris[1] = c.meshes[0].n_triangles;
             c.alt_meshes = {c.meshes[0], c.meshes[0]};
             c.alt_meshes[1].material = 3;
             return with_meshes(c);
         }},
    };
#undef CASE
#undef STORE
#undef MESH
}

inline std::string json_string(const std::string &s) {
    std::string out = "\"";
    for (char ch : s) {
        if (ch == '"' || ch == '\\') out += '\\';
        out += ch;
    }
    return out + "\"";
}

// pack_check <asset root> hash <case | all>      the packed scene of each case
// pack_check <asset root> refuse <case | all>    {"base_rc", "rc", "error"} of each corruption and of the description it corrupts
// Exit status 0 when every case ran (a refusal is a result, not a failure); 2 for a case that could not be built or a hash
// case that was refused.
inline int pack_check_main(int argc, char **argv, PackFn pack) {
    if (argc != 4 || (std::strcmp(argv[2], "hash") && std::strcmp(argv[2], "refuse"))) {
        std::fprintf(stderr, "usage: %s <asset root> hash|refuse <case|all>\n", argv[0]);
        return 2;
    }
    const bool hash = !std::strcmp(argv[2], "hash");
    const std::string which = argv[3];
    int status = 0, n = 0;
    std::string error;
    std::printf("{");
    if (hash) {
        for (const char *name : k_hash_cases) {
            if (which != "all" && which != name) continue;
            std::unique_ptr<Case> c = make_hash_case(name, argv[1]);
            if (!c) return 2;
            std::printf("%s\n\"%s\":", n++ ? "," : "", name);
            const int rc = pack(c->desc(), true, error);
            if (rc) {
                std::printf("{\"rc\":%d,\"error\":%s}", rc, json_string(error).c_str());
                status = 2;
            }
        }
    } else {
        for (const RefuseCase &r : refuse_cases()) {
            if (which != "all" && which != r.name) continue;
            Case base, bad;
            make_refuse_base(base);
            make_refuse_base(bad);
            const int base_rc = pack(base.desc(), false, error);
            error.clear();
            const int rc = pack(r.corrupt(bad), false, error);
            std::printf("%s\n\"%s\":{\"base_rc\":%d,\"rc\":%d,\"error\":%s}", n++ ? "," : "", r.name, base_rc, rc, json_string(error).c_str());
        }
    }
    std::printf("\n}\n");
    if (!n) {
        std::fprintf(stderr, "pack_check: no case '%s'\n", which.c_str());
        return 2;
    }
    return status;
}
