// Adaptive lit frames (include/hrt.h "Adaptive lit frames": hrt_render_lit_adaptive_device, hrt_render_lit_adaptive): the per-tile
// sample counts of hrt_adaptive.hip for a lens frame whose paths END in a probe volume.  Included by hrt_api.hip inside its
// extern "C" block, after hrt_lens_adaptive.hip (lens_adaptive_check, lens_adaptive_frame, lens_adaptive_host: the rounds' host
// side, parameterised by the launch) and hrt_bake_lit.hip.
//
// There is no new device function in this file, only instantiations over the tile-list source of hrt_lens.hip:
//   LensTileRays x lit_sample   hrt_lens_tiles_lit_kernel         lit_body: item i is lane i & 63 of active tile i >> 6
//   LensTileRays x VolumeTail   hrt_lens_tiles_lit_paths_kernel   radiance_body, as hrt_lens_tiles_kernel with the volume tail
// The rounds, the sums (la_tiles), the lists and keep words (ad_compact / ad_words), the reader ordering, the events and the count
// map are hrt_lens_adaptive.hip's: this client only puts a lit launch in place of lens_tiles_launch.  Every launch passes
// HRT_RADIANCE_ACCUMULATE, and a sample depends only on (seed, pixel, sample), so every tile ends with the bits of hrt_render_lit
// at its count.  An item outside the image makes no traced sample: its three floats are read and written back as they were.

// The launch record: that of the tile-list lens kernel with the volume and K.
struct DLensTilesLit : DLensTilesRadiance {
    DLitVolume vol;
    uint32_t tail_after;
};

// Waves per SIMD: INHERITED from the single-frame lit kernels (hrt_lit_frames.hip: 5 and 4), not measured for this source.
#ifndef HRT_LENS_TILES_LIT_MIN_WAVES
#define HRT_LENS_TILES_LIT_MIN_WAVES HRT_LENS_LIT_MIN_WAVES
#endif
#ifndef HRT_LENS_TILES_LIT_PATHS_MIN_WAVES
#define HRT_LENS_TILES_LIT_PATHS_MIN_WAVES HRT_LENS_LIT_PATHS_MIN_WAVES
#endif

HRT_LIT_FRAME_FAMILY(hrt_lens_tiles_lit_kernel, LensTileRays, DLensTilesLit, HRT_LENS_TILES_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_tiles_lit_paths_kernel, LensTileRays, DLensTilesLit, VolumeTail, HRT_LENS_TILES_LIT_PATHS_MIN_WAVES)

// What a call's launches share.
struct LitTiles {
    hrt_scene *s;
    const hrt_probe_volume *v;
    DLens L;
    uint32_t w, h;
    uint64_t seed;
    uint32_t flags, eval_flags;
    float bias;
    uint32_t tail_after;
    hipStream_t stream;
};

// One launch of a tile-list lit kernel (the scene entered): lens_tiles_launch with the volume.
static int lit_tiles_launch(const LitTiles &T, const uint32_t *list, uint32_t n_active, uint32_t first, uint32_t add, float *sums, hipEvent_t e0,
                            hipEvent_t e1) {
    DLensTilesLit Q;
    Q.w = T.w;
    Q.h = T.h;
    Q.tiles_x = (T.w + HRT_TILE - 1u) / HRT_TILE;
    Q.list = list;
    Q.lens = T.L;
    Q.vol = lit_volume(T.v, T.eval_flags, T.bias);
    Q.tail_after = T.tail_after;
    HIP_TRY(hipEventRecord(e0, T.stream));
    // n_active <= the frame's tiles, which the entry points hold to (2^31 - 1) / 64
    const int rc = radiance_launch(T.tail_after ? hrt_lens_tiles_lit_paths_kernel_builds : hrt_lens_tiles_lit_kernel_builds, Q, T.s, first, add, T.seed,
                                   (T.flags & (HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE)) | HRT_RADIANCE_ACCUMULATE, sums,
                                   n_active * 64u, T.stream);  // refuses a launch HIP refused
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipEventRecord(e1, T.stream));
    return HRT_OK;
}

// The checks of both entry points, in the header's order: lens_adaptive_check's, tail_after, "Lit rays"' volume checks, the scene.
static int lit_adaptive_check(const std::string &who, hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h,
                              const hrt_adaptive *p, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, const float *out,
                              const char *out_name, const uint32_t *spp, const char *spp_name, DLens &L) {
    int rc = lens_adaptive_check(who, lens, w, h, p, flags, out, out_name, spp, spp_name, L);
    if (rc == HRT_OK) rc = lit_frame_tail_check(who, tail_after);
    if (rc == HRT_OK) rc = lit_volume_check(who, v, eval_flags, bias);
    if (rc == HRT_OK) rc = lit_enter(who, s, v);
    return rc;
}

int hrt_render_lit_adaptive_device(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params,
                                   uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_frame,
                                   uint32_t *d_tile_spp, void *stream) {
    LitTiles T{s, v, {}, w, h, seed, flags, eval_flags, bias, tail_after, (hipStream_t)stream};
    const int rc = lit_adaptive_check("hrt_render_lit_adaptive_device", s, v, lens, w, h, params, flags, eval_flags, bias, tail_after, d_frame, "d_frame",
                                      d_tile_spp, "d_tile_spp", T.L);
    if (rc != HRT_OK) return rc;
    double ms = 0.0;
    return lens_adaptive_frame(s, w, h, params, flags, d_frame, d_tile_spp, T.stream, &ms,
                               [&](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, hipEvent_t e0, hipEvent_t e1) -> int {
                                   return lit_tiles_launch(T, list, n, first, add, sums, e0, e1);
                               });
}

// Blocking, into host memory, on the null stream.
int hrt_render_lit_adaptive(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params,
                            uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb, uint32_t *out_tile_spp,
                            hrt_stats *stats) {
    LitTiles T{s, v, {}, w, h, seed, flags, eval_flags, bias, tail_after, nullptr};
    const int rc = lit_adaptive_check("hrt_render_lit_adaptive", s, v, lens, w, h, params, flags, eval_flags, bias, tail_after, out_rgb, "out_rgb",
                                      out_tile_spp, "out_tile_spp", T.L);
    if (rc != HRT_OK) return rc;
    return lens_adaptive_host(s, w, h, params, flags, out_rgb, out_tile_spp, stats,
                              [&](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, hipEvent_t e0, hipEvent_t e1) -> int {
                                  return lit_tiles_launch(T, list, n, first, add, sums, e0, e1);
                              });
}
