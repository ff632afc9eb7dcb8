// Lit bakes (include/hrt.h "Lit bakes": hrt_bake_lit_device, hrt_bake_lit): the final gather of a baked-lighting pipeline -- the
// cosine-weighted rays of bake points (hrt_bake.hip: BakeRays) whose paths END in a probe volume, by either of the two rules that
// end a path there (hrt_probe_lit.hip: lit_sample, one segment; hrt_lit_paths.hip: VolumeTail, the K-th diffuse hit).  Included by
// hrt_api.hip inside its extern "C" block, after hrt_lit_frames.hip.  The host side is hrt_bake.hip's (bake_call, bake_launch) with
// a LitRule and the record below.
//
// There is no new device function in this file, only instantiations.  Source x rules:
//   BakeRays x lit_sample   hrt_bake_lit_kernel         lit_body with a per-sample source: lane i is point i
//   BakeRays x VolumeTail   hrt_bake_lit_paths_kernel   radiance_body, as hrt_bake_kernel with hrt_lit_paths_kernel's tail
// A lane reads its point record again at every sample and makes the ray in registers (bake_sample), so a lit bake needs no
// n * 32-byte ray buffer and one launch instead of two per sample.  A sample bake_sample refuses adds nothing and still counts in
// the divisor.  The look-up's bias (DLitVolume::bias) is applied at the HIT; the point record's own bias float moves the ray's
// origin inside bake_sample: the two never meet.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

// The launch record: that of a bake with the volume and K.
using DBakeLit = Lit<DBake>;

// Waves per SIMD the plain and lights builds leave registers for (the proof builds: 2, as everywhere), chosen by the A/B of
// tools/bake_lit_bench.py over -D builds of these (profiles/bake_lit_waves_ab.json, DESIGN.md section 5 "Lit bakes"); they
// started at the single-frame lens-lit siblings' 5 and 4.  Measured on MI355X, cornell_mesh, the floor at 512 x 512 x 256 samples,
// 2 / 3 / 4 / 5 waves: 19.5 / 18.5 / 15.4 / 15.5 ms with one segment (at 16 samples 1.29 / 1.25 / 1.03 / 1.07), 25.0 / 25.1 /
// 23.4 / 25.2 ms with tail_after = 1 and 42.6 / 43.7 / 40.0 / 43.4 ms with tail_after = 2: four waves win every row of the path
// family and, narrowly, of the one-segment family.
#ifndef HRT_BAKE_LIT_MIN_WAVES
#define HRT_BAKE_LIT_MIN_WAVES 4
#endif
#ifndef HRT_BAKE_LIT_PATHS_MIN_WAVES
#define HRT_BAKE_LIT_PATHS_MIN_WAVES 4
#endif

HRT_LIT_FAMILY(hrt_bake_lit_kernel, BakeRays, DBakeLit, HRT_BAKE_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_bake_lit_paths_kernel, BakeRays, DBakeLit, VolumeTail, HRT_BAKE_LIT_PATHS_MIN_WAVES)

// Checked in the header's order: hrt_bake_device's checks, tail_after, "Lit rays"' volume checks, then the scene.
static int bake_lit(const std::string &who, bool dev, hrt_scene *s, const LitRule &R, const float *points, const uint32_t *keys, uint32_t n,
                    uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return bake_call(who, dev, s, R, points, keys, n, first_sample, n_samples, flags, out, stream, stats,
                     [&](const float *d_points, const uint32_t *d_keys, float *d_out, hipStream_t st) {
                         DBakeLit Q;
                         R.fill(Q);
                         return bake_launch(R.tail_after ? hrt_bake_lit_paths_kernel_builds : hrt_bake_lit_kernel_builds, Q, s, d_points, d_keys, n,
                                            first_sample, n_samples, seed, flags, d_out, st);
                     });
}

int hrt_bake_lit_device(hrt_scene *s, const hrt_probe_volume *v, const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                        uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                        void *stream) {
    return bake_lit("hrt_bake_lit_device", true, s, LitRule{v, eval_flags, bias, tail_after}, d_points, d_keys, n, first_sample, n_samples, seed, flags,
                    d_out, stream, nullptr);
}

// Blocking, from and into host memory.
int hrt_bake_lit(hrt_scene *s, const hrt_probe_volume *v, const float *points, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed,
                 uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out, hrt_stats *stats) {
    return bake_lit("hrt_bake_lit", false, s, LitRule{v, eval_flags, bias, tail_after}, points, keys, n, 0u, spp, seed, flags, out, nullptr, stats);
}
