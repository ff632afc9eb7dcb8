// Lit frames (include/hrt.h "Lit frames": hrt_render_lit_device, hrt_render_lit, hrt_render_lit_views_device, hrt_render_lit_views):
// the frame of a lens camera whose paths END in a probe volume -- the product of the lens sources (hrt_lens.hip: LensRays,
// LensViewRays) and the two rules that end a path in a volume (hrt_probe_lit.hip: lit_sample, one segment; hrt_lit_paths.hip:
// VolumeTail, the K-th diffuse hit).  Included by hrt_api.hip inside its extern "C" block, after hrt_lit_paths.hip.  The host side
// is hrt_lens.hip's (lens_frame_call, lens_launch, lens_views_call, lens_views_launch) with a LitRule and the records below.
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

// The launch records: those of the lens frames with the volume and K.  The views record has no launch seed, as its base.
using DLensLit = Lit<DLensRadiance>;
using DLensViewsLit = Lit<DLensViewsRadiance>;

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

HRT_LIT_FAMILY(hrt_lens_lit_kernel, LensRays, DLensLit, HRT_LENS_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_lit_paths_kernel, LensRays, DLensLit, VolumeTail, HRT_LENS_LIT_PATHS_MIN_WAVES)
HRT_LIT_FAMILY(hrt_lens_views_lit_kernel, LensViewRays, DLensViewsLit, HRT_LENS_VIEWS_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_views_lit_paths_kernel, LensViewRays, DLensViewsLit, VolumeTail, HRT_LENS_VIEWS_LIT_PATHS_MIN_WAVES)

// Checked in the header's order: hrt_render_lens_device's checks, tail_after, "Lit rays"' volume checks, then the scene.
static int lit_frame(const std::string &who, bool dev, hrt_scene *s, const LitRule &R, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample,
                     uint32_t n_samples, uint64_t seed, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return lens_frame_call(who, dev, s, R, lens, w, h, first_sample, n_samples, flags, out, stream, stats,
                           [&](const DLens &L, float *d_frame, hipStream_t st) {
                               DLensLit Q;
                               R.fill(Q);
                               return lens_launch(R.tail_after ? hrt_lens_lit_paths_kernel_builds : hrt_lens_lit_kernel_builds, Q, s, L, w, h, first_sample,
                                                  n_samples, seed, flags, d_frame, st);
                           });
}

int hrt_render_lit_device(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample,
                          uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_frame,
                          void *stream) {
    return lit_frame("hrt_render_lit_device", true, s, LitRule{v, eval_flags, bias, tail_after}, lens, w, h, first_sample, n_samples, seed, flags, d_frame,
                     stream, nullptr);
}

// Blocking, into host memory.
int hrt_render_lit(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags,
                   uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb, hrt_stats *stats) {
    return lit_frame("hrt_render_lit", false, s, LitRule{v, eval_flags, bias, tail_after}, lens, w, h, 0u, spp, seed, flags, out_rgb, nullptr, stats);
}

// Checked in the header's order: hrt_render_lens_views_device's checks (an empty batch skips all but the flags), tail_after, (an
// empty batch returns,) "Lit rays"' volume checks, then the scene.
static int lit_views(const std::string &who, bool dev, hrt_scene *s, const LitRule &R, const hrt_lens_view *views, uint32_t n_views, uint32_t w,
                     uint32_t h, uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return lens_views_call(who, dev, s, R, views, n_views, w, h, first_sample, n_samples, flags, out, stream, stats,
                           [&](std::vector<DLensView> &blocks, float *d_frames, hipStream_t st) {
                               DLensViewsLit Q;
                               R.fill(Q);
                               return lens_views_launch(R.tail_after ? hrt_lens_views_lit_paths_kernel_builds : hrt_lens_views_lit_kernel_builds, Q, s,
                                                        blocks, w, h, first_sample, n_samples, flags, d_frames, st);
                           });
}

int hrt_render_lit_views_device(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                                uint32_t first_sample, uint32_t n_samples, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after,
                                float *d_frames, void *stream) {
    return lit_views("hrt_render_lit_views_device", true, s, LitRule{v, eval_flags, bias, tail_after}, views, n_views, w, h, first_sample, n_samples, flags,
                     d_frames, stream, nullptr);
}

// Blocking, into host memory.
int hrt_render_lit_views(hrt_scene *s, const hrt_probe_volume *v, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t spp,
                         uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out_rgb, hrt_stats *stats) {
    return lit_views("hrt_render_lit_views", false, s, LitRule{v, eval_flags, bias, tail_after}, views, n_views, w, h, 0u, spp, flags, out_rgb, nullptr,
                     stats);
}
