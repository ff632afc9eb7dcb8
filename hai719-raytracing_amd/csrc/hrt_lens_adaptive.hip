// Adaptive lens frames (include/hrt.h hrt_render_lens_adaptive*): the per-tile sample counts of hrt_adaptive.hip under any lens.
// Included by hrt_api.hip inside its extern "C" block, after hrt_adaptive.hip (the rounds' kernels and parameter checks) and
// hrt_lens.hip (the tile-list lens kernel and the lens checks).
//
// The rounds are adaptive_rounds' (hrt_adaptive.hip) with the fused lens kernel, hrt_lens_tiles_kernel, in place of the trace
// kernels.  The gather, judge, compact and finalize kernels run unchanged, with rank 0 of world 1: the lens kernel's item i is lane
// i & 63 of active tile i >> 6, which is exactly the compact buffer they read and write, so nothing is scattered.  Every lens launch
// passes HRT_RADIANCE_ACCUMULATE: a round continues the stored sums in sample order, and since a sample depends only on (seed,
// pixel, sample) every tile ends with the bits of hrt_render_lens at its count.
//
// The lens travels as a kernel argument, the lists and keep words are ad_compact / ad_words (shared with hrt_render_adaptive: the
// two may not overlap on one scene), the sums are la_tiles; the work-queue head, the path pool, the camera blocks and the trace
// launches' events are not touched.
//
// The host side of the rounds -- lens_adaptive_run, lens_adaptive_frame, lens_adaptive_host -- takes the launch of the tile-list
// kernel as a callable: lens_tiles_launch with the plain record and table here, with the lit ones in hrt_lit_adaptive.hip
// (hrt_render_lit_adaptive*), which shares everything else with this file.

// One launch of a tile-list lens kernel (the scene entered): samples [first, first + add) of the n_active tiles of `list` (NULL:
// every tile) onto the running sums at `sums`, between events e0 and e1 on `stream`.  Q and its builds: DLensTilesRadiance and
// hrt_lens_tiles_kernel_builds, or the record and a table of an adaptive lit frame (hrt_lit_adaptive.hip) with the rule filled in.
extern "C++" {
template <class QT>
static int lens_tiles_launch(void (*const *builds)(const QT), QT &Q, hrt_scene *s, const DLens &L, uint32_t w, uint32_t h, const uint32_t *list,
                             uint32_t n_active, uint32_t first, uint32_t add, uint64_t seed, uint32_t flags, float *sums, hipStream_t stream,
                             hipEvent_t e0, hipEvent_t e1) {
    Q.w = w;
    Q.h = h;
    Q.tiles_x = (w + HRT_TILE - 1u) / HRT_TILE;
    Q.list = list;
    Q.lens = L;
    HIP_TRY(hipEventRecord(e0, stream));
    // n_active <= the frame's tiles, which the entry points hold to (2^31 - 1) / 64
    const int rc = radiance_launch(builds, Q, s, first, add, seed,
                                   (flags & (HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE)) | HRT_RADIANCE_ACCUMULATE, sums,
                                   n_active * 64u, stream);  // refuses a launch HIP refused
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipEventRecord(e1, stream));
    return HRT_OK;
}
}  // extern "C++"

// The rounds (adaptive_rounds, hrt_adaptive.hip) over all tiles of the frame with a tile-list kernel: d_sums (tile-major, every
// tile) ends with the means, d_counts with each tile's count (NULL: the scene's own count map).
//   launch(list, n, first, add, sums, e0, e1)   one launch of the tile-list kernel between the events: lens_tiles_launch with the
//                                               client's record and table -- the one thing the two clients do not share
// ev: two pairs of timing events, the call's own: pair 0 around round 0's launch, pair 1 around every later one.  The stream is
// synchronised once per round from round 1 on, and the times are read after it; a fault of a round's kernels ends the call there,
// before the length of the next list is believed.
extern "C++" {
template <class Launch>
static int lens_adaptive_run(hrt_scene *s, uint32_t w, uint32_t h, const hrt_adaptive *p, uint32_t flags, float *d_sums, uint32_t *d_counts,
                             hipStream_t stream, const Event ev[4], double *kernel_ms, Launch launch) {
    *kernel_ms = 0.0;
    auto add_time = [&](hipEvent_t e0, hipEvent_t e1) -> int {  // after the synchronisation that covers e1
        float f = 0.f;
        HIP_TRY(hipEventElapsedTime(&f, e0, e1));
        *kernel_ms += (double)f;
        return HRT_OK;
    };
    return adaptive_rounds(
        s, AdFrame{w, h, (w + HRT_TILE - 1u) / HRT_TILE, hrt_tiles_total(w, h), 0u, 1u}, p, (flags & HRT_FLAG_GAMMA) != 0u, d_sums, d_counts, stream,
        [&](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, uint32_t round) -> int {
            const Event *const e = ev + (round == 0u ? 0 : 2);
            return launch(list, n, first, add, sums, (hipEvent_t)e[0], (hipEvent_t)e[1]);
        },
        [&](uint32_t round) -> int {
            const int rc = round == 1u ? add_time(ev[0], ev[1]) : HRT_OK;
            return rc != HRT_OK ? rc : add_time(ev[2], ev[3]);
        });
}
}  // extern "C++"

// The checks of both entry points, in the header's order (all before the scene and the library state); fills L.
static int lens_adaptive_check(const std::string &who, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *p, uint32_t flags,
                               const float *out, const char *out_name, const uint32_t *spp, const char *spp_name, DLens &L) {
    if (flags & HRT_RADIANCE_ACCUMULATE)
        return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE: the rounds keep the running sums themselves, the result is the means");
    { const int frc = lens_flags_check(who, flags); if (frc != HRT_OK) return frc; }
    { const int prc = adaptive_params_check(who, p); if (prc != HRT_OK) return prc; }
    { const int lrc = lens_check(who, lens, L); if (lrc != HRT_OK) return lrc; }
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    const uint64_t tiles = (uint64_t)((w + HRT_TILE - 1u) / HRT_TILE) * ((h + HRT_TILE - 1u) / HRT_TILE);
    if (tiles * 64u > k_max_pixels)
        return fail(HRT_ERR_INVALID, who + ": frame too large: tiles * 64 is " + std::to_string(tiles * 64u) + ", above the " + std::to_string(k_max_pixels) + " items one launch indexes");
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is not 4-byte aligned");
    if ((uintptr_t)spp % sizeof(uint32_t)) return fail(HRT_ERR_INVALID, who + ": " + spp_name + " is not 4-byte aligned");
    return HRT_OK;
}

// The rounds into la_tiles on `stream`, then the row-major frame into d_frame (the scene entered).  The sums buffer is read by the
// previous call's assemble launch: one on another stream is waited for on `stream`.
extern "C++" {
template <class Launch>
static int lens_adaptive_frame(hrt_scene *s, uint32_t w, uint32_t h, const hrt_adaptive *p, uint32_t flags, float *d_frame, uint32_t *d_counts,
                               hipStream_t stream, double *kernel_ms, Launch launch) {
    const uint32_t tiles = hrt_tiles_total(w, h);
    const size_t tile_bytes = (size_t)tiles * 192u * sizeof(float);
    int rc = s->la_tiles.cap < tile_bytes ? s->la_reader.sync() : HRT_OK;  // the old sums are freed: their last reader is done
    if (rc == HRT_OK) rc = s->la_tiles.grow(tile_bytes);
    if (rc == HRT_OK) rc = s->la_reader.wait_on(stream);
    if (rc != HRT_OK) return rc;
    Event ev[4];
    for (Event &e : ev)
        if ((rc = e.ready()) != HRT_OK) return rc;
    if ((rc = lens_adaptive_run(s, w, h, p, flags, s->la_tiles.as<float>(), d_counts, stream, ev, kernel_ms, launch)) != HRT_OK) return rc;
    if ((rc = hrt_assemble_frame(s->la_tiles.as<float>(), tiles, w, h, 1, d_frame, stream)) != HRT_OK) return rc;
    return s->la_reader.mark(stream);
}

// The blocking form (the scene entered), into host memory on the null stream.  The count map is the scene's (ad_words), as
// hrt_render_adaptive's.
template <class Launch>
static int lens_adaptive_host(hrt_scene *s, uint32_t w, uint32_t h, const hrt_adaptive *p, uint32_t flags, float *out_rgb, uint32_t *out_tile_spp,
                              hrt_stats *stats, Launch launch) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t frame_bytes = (size_t)w * h * 3u * sizeof(float);
    int rc;
    if ((rc = s->la_frame.grow(frame_bytes)) != HRT_OK) return rc;
    double ms = 0.0;
    if ((rc = lens_adaptive_frame(s, w, h, p, flags, s->la_frame.as<float>(), nullptr, nullptr, &ms, launch)) != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->la_frame.p, frame_bytes, hipMemcpyDeviceToHost));
    uint64_t samples = 0;  // degenerate samples count: every in-image pixel has its tile's count
    if ((rc = adaptive_counts_to_host(s, w, h, out_tile_spp, stats ? &samples : nullptr)) != HRT_OK) return rc;
    if (stats) {
        fill_stats(s, stats, t0, ms, samples);
        stats->lds_bytes = 0u;  // the tree is read from global memory
        stats->waves_launched = 0u;
    }
    return HRT_OK;
}
}  // extern "C++"

int hrt_render_lens_adaptive_device(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params, uint64_t seed,
                                    uint32_t flags, float *d_frame, uint32_t *d_tile_spp, void *stream) {
    const std::string who = "hrt_render_lens_adaptive_device";
    DLens L;
    int rc = lens_adaptive_check(who, lens, w, h, params, flags, d_frame, "d_frame", d_tile_spp, "d_tile_spp", L);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    double ms = 0.0;
    return lens_adaptive_frame(s, w, h, params, flags, d_frame, d_tile_spp, (hipStream_t)stream, &ms,
                               [&](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, hipEvent_t e0, hipEvent_t e1) -> int {
                                   DLensTilesRadiance Q;
                                   return lens_tiles_launch(hrt_lens_tiles_kernel_builds, Q, s, L, w, h, list, n, first, add, seed, flags, sums,
                                                            (hipStream_t)stream, e0, e1);
                               });
}

// Blocking, into host memory, on the null stream.
int hrt_render_lens_adaptive(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, const hrt_adaptive *params, uint64_t seed,
                             uint32_t flags, float *out_rgb, uint32_t *out_tile_spp, hrt_stats *stats) {
    const std::string who = "hrt_render_lens_adaptive";
    DLens L;
    int rc = lens_adaptive_check(who, lens, w, h, params, flags, out_rgb, "out_rgb", out_tile_spp, "out_tile_spp", L);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    return lens_adaptive_host(s, w, h, params, flags, out_rgb, out_tile_spp, stats,
                              [&](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, hipEvent_t e0, hipEvent_t e1) -> int {
                                  DLensTilesRadiance Q;
                                  return lens_tiles_launch(hrt_lens_tiles_kernel_builds, Q, s, L, w, h, list, n, first, add, seed, flags, sums, nullptr, e0,
                                                           e1);
                              });
}
