// What pack_check prints of a packed scene: per array the element count and the 64-bit FNV-1a of its bytes, then the
// header's scalars, the bound (as its bits) and max_leaf -- one JSON object.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>

inline uint64_t pack_fnv1a(const void *p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
    return h;
}

struct PackDump {
    FILE *f;
    bool first = true;
    explicit PackDump(FILE *out) : f(out) { std::fprintf(f, "{\"vectors\":{"); }
    void vec(const char *name, const void *p, size_t count, size_t elem) {
        std::fprintf(f, "%s\"%s\":[%zu,\"%016llx\"]", first ? "" : ",", name, count, (unsigned long long)pack_fnv1a(p, count * elem));
        first = false;
    }
    template <class Scene>  // DScene (csrc/hrt_device.h)
    void header(const Scene &d, float bound, uint32_t max_leaf) {
        uint32_t bits;
        std::memcpy(&bits, &bound, 4);
        std::fprintf(f, "},\"header\":{\"tab_quads\":%u,\"tab_mats\":%u,\"tab_spheres\":%u,\"tab_meshes\":%u,\"tab_sfilter\":%u,\"tab_exc\":%u,\"tab_rows\":%u,"
                        "\"exc_in_tabs\":%u,\"qf_n\":[%u,%u,%u,%u],\"sf_pairs\":%u,\"sf_psize\":%u,\"n_spheres\":%u,\"n_quads\":%u,\"n_meshes\":%u,"
                        "\"n_lights\":%u,\"n_images\":%u,\"n_kd_units\":%u,\"dark_sky\":%d,\"skybox_image\":%d,\"any_motion\":%u,\"prune_ok\":%u},"
                        "\"bound\":\"%08x\",\"max_leaf\":%u}",
                     d.tab_quads, d.tab_mats, d.tab_spheres, d.tab_meshes, d.tab_sfilter, d.tab_exc, d.tab_rows, d.exc_in_tabs, d.qf_n[0], d.qf_n[1],
                     d.qf_n[2], d.qf_n[3], d.sf_pairs, d.sf_psize, d.n_spheres, d.n_quads, d.n_meshes, d.n_lights, d.n_images, d.n_kd_units,
                     d.dark_sky, d.skybox_image, d.any_motion, d.prune_ok, bits, max_leaf);
    }
};
