// Lit bakes (include/hrt.h "Lit bakes": hrt_bake_lit_device, hrt_bake_lit): the final gather of a baked-lighting pipeline -- the
// cosine-weighted rays of bake points (hrt_bake.hip: BakeRays) whose paths END in a probe volume, by either of the two rules that
// end a path there (hrt_probe_lit.hip: lit_sample, one segment; hrt_lit_paths.hip: VolumeTail, the K-th diffuse hit).  Included by
// hrt_api.hip inside its extern "C" block, after hrt_lit_frames.hip (HRT_LIT_FRAME_FAMILY, lit_frame_tail_check).
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

// The launch record: that of a bake with the volume and K (radiance_launch, query_launch, radiance_body and lit_body reach the
// fields they share by name; the one-segment kernels do not read tail_after).
struct DBakeLit : DBake {
    DLitVolume vol;
    uint32_t tail_after;
};

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

HRT_LIT_FRAME_FAMILY(hrt_bake_lit_kernel, BakeRays, DBakeLit, HRT_BAKE_LIT_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_bake_lit_paths_kernel, BakeRays, DBakeLit, VolumeTail, HRT_BAKE_LIT_PATHS_MIN_WAVES)

// The fused launch into d_out on `stream` (the scene entered): bake_launch with the volume.
static int bake_lit_launch(hrt_scene *s, const hrt_probe_volume *v, const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                           uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                           hipStream_t stream) {
    DBakeLit Q;
    Q.points = (const float4 *)d_points;
    Q.keys = d_keys;
    Q.vol = lit_volume(v, eval_flags, bias);
    Q.tail_after = tail_after;
    return radiance_launch(tail_after ? hrt_bake_lit_paths_kernel_builds : hrt_bake_lit_kernel_builds, Q, s, first_sample, n_samples, seed, flags, d_out, n,
                           stream);
}

// Checked in the header's order: hrt_bake_device's checks, tail_after, "Lit rays"' volume checks, then the scene.
int hrt_bake_lit_device(hrt_scene *s, const hrt_probe_volume *v, const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                        uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                        void *stream) {
    const std::string who = "hrt_bake_lit_device";
    int rc = bake_flags_check(who, flags);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = bake_points_check(who, d_points, d_keys, n, true)) != HRT_OK) return rc;
    if ((rc = samples_out_check(who, first_sample, n_samples, d_out, "d_out")) != HRT_OK) return rc;
    if ((rc = lit_frame_tail_check(who, tail_after)) != HRT_OK) return rc;
    if ((rc = lit_volume_check(who, v, eval_flags, bias)) != HRT_OK) return rc;
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    return bake_lit_launch(s, v, d_points, d_keys, n, first_sample, n_samples, seed, flags, eval_flags, bias, tail_after, d_out, (hipStream_t)stream);
}

// Blocking, from and into host memory (BlockingCall; the points and keys are device buffers of the call's, too).
int hrt_bake_lit(hrt_scene *s, const hrt_probe_volume *v, const float *points, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed,
                 uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out, hrt_stats *stats) {
    const std::string who = "hrt_bake_lit";
    if (flags & HRT_RADIANCE_ACCUMULATE) return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (hrt_bake_lit_device)");
    int rc = bake_flags_check(who, flags);
    if (rc != HRT_OK) return rc;
    if (n == 0u) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return HRT_OK;
    }
    if ((rc = bake_points_check(who, points, keys, n, false)) != HRT_OK) return rc;
    if ((rc = samples_out_check(who, 0u, spp, out, "out")) != HRT_OK) return rc;
    if ((rc = lit_frame_tail_check(who, tail_after)) != HRT_OK) return rc;
    if ((rc = lit_volume_check(who, v, eval_flags, bias)) != HRT_OK) return rc;
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    BlockingCall call;
    Scratch d_points, d_keys;
    if ((rc = d_points.from_host(points, (size_t)n * HRT_RAY_FLOATS * sizeof(float))) != HRT_OK) return rc;
    if (keys && (rc = d_keys.from_host(keys, (size_t)n * sizeof(uint32_t))) != HRT_OK) return rc;
    return call.run(s, (size_t)n * 3u * sizeof(float), out, (uint64_t)n * spp, stats, [&](float *d_out) {
        return bake_lit_launch(s, v, d_points.as<float>(), d_keys.as<uint32_t>(), n, 0u, spp, seed, flags, eval_flags, bias, tail_after, d_out, nullptr);
    });
}
