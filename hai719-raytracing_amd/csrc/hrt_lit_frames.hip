// Lit frames (include/hrt.h "Lit frames": hrt_render_lit_device, hrt_render_lit, hrt_render_lit_views_device, hrt_render_lit_views):
// the frame of a lens camera whose paths END in a probe volume -- the product of the lens sources (hrt_lens.hip: LensRays,
// LensViewRays) and the two rules that end a path in a volume (hrt_probe_lit.hip: lit_sample, one segment; hrt_lit_paths.hip:
// VolumeTail, the K-th diffuse hit).  Included by hrt_api.hip inside its extern "C" block, after hrt_lit_paths.hip.
//
// There is no new device function in this file, only instantiations.  Sources x rules:
//   LensRays     x lit_sample   hrt_lens_lit_kernel              lit_body with a per-sample source: lane i is pixel i
//   LensRays     x VolumeTail   hrt_lens_lit_paths_kernel        radiance_body, as hrt_lens_kernel with hrt_lit_paths_kernel's tail
//   LensViewRays x lit_sample   hrt_lens_views_lit_kernel        item i is pixel i % npix of view i / npix
//   LensViewRays x VolumeTail   hrt_lens_views_lit_paths_kernel
// A lane makes the ray of every sample in registers (lens_sample), so a frame needs no w*h*32-byte ray buffer and one launch
// instead of two per sample.  In a batch a lane reads its view's lens and seed from the table where it uses them: a wave straddles
// views whenever w*h is no multiple of 64.  A sample the lens rule does not trace (outside a fisheye's circle, a thin lens with
// c <= 0) adds nothing and still counts in the divisor.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

// The launch records: those of the lens frames with the volume and K (radiance_launch, query_launch, radiance_body and lit_body reach
// the fields they share by name; the one-segment kernels do not read tail_after).
struct DLensLit : DLensRadiance {
    DLitVolume vol;
    uint32_t tail_after;
};
struct DLensViewsLit : DLensViewsRadiance {
    DLitVolume vol;
    uint32_t tail_after;
};

extern "C++" {
static void radiance_seed(DLensViewsLit &, uint64_t) {}  // as DLensViewsRadiance: every view has its own
}

// Waves per SIMD the plain and lights builds of each family leave registers for (the proof builds: 2, as everywhere), chosen by
// the A/B of tools/lit_frame_bench.py over -D builds of these (profiles/lit_frame_waves_ab.json, DESIGN.md section 5 "Lit
// frames").  Measured on MI355X, cornell_mesh, 2 / 3 / 4 / 5 waves: a 1080p frame of 16 samples takes 3.98 / 3.73 / 3.44 / 3.41 ms
// with one segment, 16.2 / 12.1 / 11.4 / 9.8 ms with tail_after = 1 and 23.9 / 20.6 / 18.8 / 24.1 ms with tail_after = 2 (four
// waves also win both tails at one sample); 64 views of 128 x 128 x 16 take 4.51 / 3.79 / 3.45 / 3.44 ms with one segment and
// 18.6 / 13.0 / 12.7 / 10.2 ms with tail_after = 1.  The record-ray siblings sit at 2 (hrt_lit_kernel, by register count) and 3.
#ifndef HRT_LENS_LIT_MIN_WAVES
#define HRT_LENS_LIT_MIN_WAVES 5
#endif
#ifndef HRT_LENS_LIT_PATHS_MIN_WAVES
#define HRT_LENS_LIT_PATHS_MIN_WAVES 4
#endif
#ifndef HRT_LENS_VIEWS_LIT_MIN_WAVES
#define HRT_LENS_VIEWS_LIT_MIN_WAVES 5
#endif
#ifndef HRT_LENS_VIEWS_LIT_PATHS_MIN_WAVES
#define HRT_LENS_VIEWS_LIT_PATHS_MIN_WAVES 5
#endif

// The four builds of lit_body over a per-sample source, and their table, indexed lights | exact << 1 as radiance_launch indexes it.
#define HRT_LIT_FRAME_FAMILY(base, SRC, QT, WAVES)                                                                                              \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, WAVES) base(const QT Q) { lit_body<false, false, SRC, QT>(Q); }               \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, WAVES) base##_lights(const QT Q) { lit_body<true, false, SRC, QT>(Q); }       \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) base##_exact(const QT Q) { lit_body<false, true, SRC, QT>(Q); }            \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) base##_lights_exact(const QT Q) { lit_body<true, true, SRC, QT>(Q); }      \
    static void (*const base##_builds[4])(const QT) = {base, base##_lights, base##_exact, base##_lights_exact};

HRT_LIT_FRAME_FAMILY(hrt_lens_lit_kernel, LensRays, DLensLit, HRT_LENS_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_lit_paths_kernel, LensRays, DLensLit, VolumeTail, HRT_LENS_LIT_PATHS_MIN_WAVES)
HRT_LIT_FRAME_FAMILY(hrt_lens_views_lit_kernel, LensViewRays, DLensViewsLit, HRT_LENS_VIEWS_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_views_lit_paths_kernel, LensViewRays, DLensViewsLit, VolumeTail, HRT_LENS_VIEWS_LIT_PATHS_MIN_WAVES)

// tail_after of a lit frame: 0 is the one-segment rule, 1 .. HRT_MAXBOUNCES lit_tail_check's.
static int lit_frame_tail_check(const std::string &who, uint32_t tail_after) { return tail_after == 0u ? HRT_OK : lit_tail_check(who, tail_after); }

// The fused launch into d_frame on `stream` (the scene entered), then the gamma: lens_launch with the volume.
static int lit_frame_launch(hrt_scene *s, const hrt_probe_volume *v, const DLens &L, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                            uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_frame, hipStream_t stream) {
    DLensLit Q;
    Q.w = w;
    Q.h = h;
    Q.lens = L;
    Q.vol = lit_volume(v, eval_flags, bias);
    Q.tail_after = tail_after;
    const int rc = radiance_launch(tail_after ? hrt_lens_lit_paths_kernel_builds : hrt_lens_lit_kernel_builds, Q, s, first_sample, n_samples, seed,
                                   flags & ~(uint32_t)HRT_FLAG_GAMMA, d_frame, w * h, stream);
    if (rc != HRT_OK || !(flags & HRT_FLAG_GAMMA)) return rc;
    return lens_gamma(d_frame, (uint64_t)Q.n * 3u, stream);
}

// The fused launch over all views into d_frames on `stream` (the scene entered), then the gamma: lens_views_launch with the volume.
static int lit_views_launch(hrt_scene *s, const hrt_probe_volume *v, std::vector<DLensView> &blocks, uint32_t w, uint32_t h, uint32_t first_sample,
                            uint32_t n_samples, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_frames,
                            hipStream_t stream) {
    DLensViewsLit Q;
    { const int src = lens_views_stage(s, blocks, stream, &Q.views); if (src != HRT_OK) return src; }
    Q.w = w;
    Q.h = h;
    Q.npix = w * h;
    Q.vol = lit_volume(v, eval_flags, bias);
    Q.tail_after = tail_after;
    int rc = radiance_launch(tail_after ? hrt_lens_views_lit_paths_kernel_builds : hrt_lens_views_lit_kernel_builds, Q, s, first_sample, n_samples, 0u,
                             flags & ~(uint32_t)HRT_FLAG_GAMMA, d_frames, (uint32_t)blocks.size() * Q.npix, stream);
    if (rc == HRT_OK) rc = s->lens_views.staged(stream);
    if (rc != HRT_OK || !(flags & HRT_FLAG_GAMMA)) return rc;
    return lens_gamma(d_frames, (uint64_t)Q.n * 3u, stream);
}

// Checked in the header's order: hrt_render_lens_device's checks, tail_after, "Lit rays"' volume checks, then the scene.
int hrt_render_lit_device(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample,
                          uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_frame,
                          void *stream) {
    const std::string who = "hrt_render_lit_device";
    DLens L;
    int rc = lens_render_check(who, lens, w, h, first_sample, n_samples, flags, d_frame, "d_frame", L);
    if (rc == HRT_OK) rc = lit_frame_tail_check(who, tail_after);
    if (rc == HRT_OK) rc = lit_volume_check(who, v, eval_flags, bias);
    if (rc == HRT_OK) rc = lit_enter(who, s, v);
    if (rc != HRT_OK) return rc;
    return lit_frame_launch(s, v, L, w, h, first_sample, n_samples, seed, flags, eval_flags, bias, tail_after, d_frame, (hipStream_t)stream);
}

// Blocking, into host memory (BlockingCall).
int hrt_render_lit(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags,
                   uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb, hrt_stats *stats) {
    const std::string who = "hrt_render_lit";
    DLens L;
    if (flags & HRT_RADIANCE_ACCUMULATE) return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (hrt_render_lit_device)");
    int rc = lens_render_check(who, lens, w, h, 0u, spp, flags, out_rgb, "out_rgb", L);
    if (rc == HRT_OK) rc = lit_frame_tail_check(who, tail_after);
    if (rc == HRT_OK) rc = lit_volume_check(who, v, eval_flags, bias);
    if (rc == HRT_OK) rc = lit_enter(who, s, v);
    if (rc != HRT_OK) return rc;
    BlockingCall call;
    return call.run(s, (size_t)w * h * 3u * sizeof(float), out_rgb, (uint64_t)w * h * spp, stats, [&](float *d_frame) {
        return lit_frame_launch(s, v, L, w, h, 0u, spp, seed, flags, eval_flags, bias, tail_after, d_frame, nullptr);
    });
}

// Checked in the header's order: hrt_render_lens_views_device's checks (an empty batch skips all but the flags), tail_after, (an
// empty batch returns,) "Lit rays"' volume checks, then the scene.
int hrt_render_lit_views_device(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                uint32_t first_sample, uint32_t n_samples, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after,
                                float *d_frames, void *stream) {
    const std::string who = "hrt_render_lit_views_device";
    std::vector<DLensView> blocks;
    int rc = lens_views_check(who, views, n_views, w, h, first_sample, n_samples, flags, d_frames, "d_frames", blocks);
    if (rc == HRT_OK) rc = lit_frame_tail_check(who, tail_after);
    if (rc != HRT_OK || n_views == 0u) return rc;
    if ((rc = lit_volume_check(who, v, eval_flags, bias)) != HRT_OK) return rc;
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    return lit_views_launch(s, v, blocks, w, h, first_sample, n_samples, flags, eval_flags, bias, tail_after, d_frames, (hipStream_t)stream);
}

// Blocking, into host memory (BlockingCall).
int hrt_render_lit_views(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t spp,
                         uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb, hrt_stats *stats) {
    const std::string who = "hrt_render_lit_views";
    std::vector<DLensView> blocks;
    if (flags & HRT_RADIANCE_ACCUMULATE) return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (hrt_render_lit_views_device)");
    int rc = lens_views_check(who, views, n_views, w, h, 0u, spp, flags, out_rgb, "out_rgb", blocks);
    if (rc == HRT_OK) rc = lit_frame_tail_check(who, tail_after);
    if (rc != HRT_OK) return rc;
    if (n_views == 0u) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return HRT_OK;
    }
    if ((rc = lit_volume_check(who, v, eval_flags, bias)) != HRT_OK) return rc;
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    BlockingCall call;
    return call.run(s, (size_t)n_views * w * h * 3u * sizeof(float), out_rgb, (uint64_t)n_views * w * h * spp, stats, [&](float *d_frames) {
        return lit_views_launch(s, v, blocks, w, h, 0u, spp, flags, eval_flags, bias, tail_after, d_frames, nullptr);
    });
}
