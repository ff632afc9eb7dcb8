// Adaptive lit frames (include/hrt.h "Adaptive lit frames": hrt_render_lit_adaptive_device, hrt_render_lit_adaptive): the per-tile
// sample counts of hrt_adaptive.hip for a lens frame whose paths END in a probe volume.  Included by hrt_api.hip inside its
// extern "C" block, after hrt_lens_adaptive.hip (lens_adaptive_check, lens_adaptive_frame, lens_adaptive_host: the rounds' host
// side, parameterised by the launch) and hrt_bake_lit.hip.
//
// There is no new device function in this file, only instantiations over the tile-list source of hrt_lens.hip:
//   LensTileRays x lit_sample   hrt_lens_tiles_lit_kernel         lit_body: item i is lane i & 63 of active tile i >> 6
//   LensTileRays x VolumeTail   hrt_lens_tiles_lit_paths_kernel   radiance_body, as hrt_lens_tiles_kernel with the volume tail
// The rounds, the sums (la_tiles), the lists and keep words (ad_compact / ad_words), the reader ordering, the events and the count
// map are hrt_lens_adaptive.hip's, lens_tiles_launch included: this client only gives it the lit record and tables.  Every launch passes
// HRT_RADIANCE_ACCUMULATE, and a sample depends only on (seed, pixel, sample), so every tile ends with the bits of hrt_render_lit
// at its count.  An item outside the image makes no traced sample: its three floats are read and written back as they were.

// The launch record: that of the tile-list lens kernel with the volume and K.
using DLensTilesLit = Lit<DLensTilesRadiance>;

// Waves per SIMD: INHERITED from the single-frame lit kernels (hrt_lit_frames.hip: 5 and 4), not measured for this source.
#ifndef HRT_LENS_TILES_LIT_MIN_WAVES
#define HRT_LENS_TILES_LIT_MIN_WAVES HRT_LENS_LIT_MIN_WAVES
#endif
#ifndef HRT_LENS_TILES_LIT_PATHS_MIN_WAVES
#define HRT_LENS_TILES_LIT_PATHS_MIN_WAVES HRT_LENS_LIT_PATHS_MIN_WAVES
#endif

HRT_LIT_FAMILY(hrt_lens_tiles_lit_kernel, LensTileRays, DLensTilesLit, HRT_LENS_TILES_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_tiles_lit_paths_kernel, LensTileRays, DLensTilesLit, VolumeTail, HRT_LENS_TILES_LIT_PATHS_MIN_WAVES)

// The launch of a call's rounds (the scene entered): lens_tiles_launch with the lit record and the table tail_after chooses.
static auto lit_tiles_launch_of(hrt_scene *s, const LitRule &R, const DLens &L, uint32_t w, uint32_t h, uint64_t seed, uint32_t flags, hipStream_t stream) {
    return [=](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, hipEvent_t e0, hipEvent_t e1) -> int {
        DLensTilesLit Q;
        R.fill(Q);
        return lens_tiles_launch(R.tail_after ? hrt_lens_tiles_lit_paths_kernel_builds : hrt_lens_tiles_lit_kernel_builds, Q, s, L, w, h, list, n, first,
                                 add, seed, flags, sums, stream, e0, e1);
    };
}

// The checks of both entry points, in the header's order: lens_adaptive_check's, tail_after, "Lit rays"' volume checks, the scene.
static int lit_adaptive_check(const std::string &who, hrt_scene *s, const LitRule &R, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *p,
                              uint32_t flags, const float *out, const char *out_name, const uint32_t *spp, const char *spp_name, DLens &L) {
    int rc = lens_adaptive_check(who, lens, w, h, p, flags, out, out_name, spp, spp_name, L);
    if (rc == HRT_OK) rc = R.check(who);
    if (rc == HRT_OK) rc = R.enter(who, s);
    return rc;
}

int hrt_render_lit_adaptive_device(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params,
                                   uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_frame,
                                   uint32_t *d_tile_spp, void *stream) {
    const LitRule R{v, eval_flags, bias, tail_after};
    DLens L;
    const int rc = lit_adaptive_check("hrt_render_lit_adaptive_device", s, R, lens, w, h, params, flags, d_frame, "d_frame", d_tile_spp, "d_tile_spp", L);
    if (rc != HRT_OK) return rc;
    double ms = 0.0;
    return lens_adaptive_frame(s, w, h, params, flags, d_frame, d_tile_spp, (hipStream_t)stream, &ms,
                               lit_tiles_launch_of(s, R, L, w, h, seed, flags, (hipStream_t)stream));
}

// Blocking, into host memory, on the null stream.
int hrt_render_lit_adaptive(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params,
                            uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb, uint32_t *out_tile_spp,
                            hrt_stats *stats) {
    const LitRule R{v, eval_flags, bias, tail_after};
    DLens L;
    const int rc = lit_adaptive_check("hrt_render_lit_adaptive", s, R, lens, w, h, params, flags, out_rgb, "out_rgb", out_tile_spp, "out_tile_spp", L);
    if (rc != HRT_OK) return rc;
    return lens_adaptive_host(s, w, h, params, flags, out_rgb, out_tile_spp, stats, lit_tiles_launch_of(s, R, L, w, h, seed, flags, nullptr));
}
