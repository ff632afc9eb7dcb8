// Path features (include/hrt.h "Path features": hrt_path_features, hrt_render_path_features, hrt_render_lens_path_features,
// hrt_render_lens_views_path_features): the denoisers' feature record taken at the FIRST DIFFUSE hit of the integrator's own path
// instead of at the first hit -- mirror and glass are followed, the albedo is the throughput there, the depth the length of the
// chain.  Included by hrt_api.hip inside its extern "C" block, after hrt_lit_paths.hip (HRT_TAIL_FAMILY) and hrt_lens.hip (the lens
// sources and checks).
//
// There is no path loop in this file: the kernels are radiance_body (hrt_radiance.hip) with the FeatureTail policy, "Lit paths"
// with K = 1 and a feature record where hrt_path_tails writes a tail record.  Sources:
//   RecordRays    hrt_path_features_kernel             one lane per ray, ONE sample: the record itself, stored
//   LensRays      hrt_lens_path_features_kernel        lane i is pixel i: the records of its samples summed in its output, then divided
//   LensViewRays  hrt_lens_views_path_features_kernel  item i is pixel i % npix of view i / npix
// The sums of a pixel live in its output record: one lane owns the item, its samples run in ascending order, and it reads back
// what it wrote itself.  Twelve floats of registers would cost the path more than twelve loads and stores per sample do.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

extern "C++" {
namespace hrtk {

// The feature record of a path, or (FOLD: a per-sample source) its sum over the samples of item i, in Q.out + 12 i; i < Q.n.
struct FeatureTail {
    static constexpr int kind = 3;
    template <class QT>
    __device__ static __forceinline__ float *record(const QT &Q, uint32_t i) { return Q.out + (size_t)i * HRT_FEATURE_FLOATS; }
    template <class QT>
    __device__ static __forceinline__ void begin(const QT &Q, uint32_t i) {  // the sums start from +0
        float *o = record(Q, i);
        for (uint32_t k = 0; k < HRT_FEATURE_FLOATS; ++k) o[k] = 0.f;
    }
    template <bool FOLD, class QT>
    __device__ static __forceinline__ void reached(const QT &Q, uint32_t i, const f3 &thr, const f3 &n, const f3 &E, float depth) {
        float *o = record(Q, i);
        const float r[11] = {thr.x, thr.y, thr.z, n.x, n.y, n.z, E.x, E.y, E.z, depth, 1.f};
        if constexpr (FOLD) {
            for (uint32_t k = 0; k < 11u; ++k) o[k] = o[k] + r[k];
        } else {
            for (uint32_t k = 0; k < 11u; ++k) o[k] = r[k];
            o[11] = 0.f;
        }
    }
    template <bool FOLD, class QT>
    __device__ static __forceinline__ void unreached(const QT &Q, uint32_t i, const f3 &E) {  // the emitters seen on the way stay
        float *o = record(Q, i);
        if constexpr (FOLD) {
            o[6] = o[6] + E.x; o[7] = o[7] + E.y; o[8] = o[8] + E.z;
        } else {
            for (uint32_t k = 0; k < HRT_FEATURE_FLOATS; ++k) o[k] = 0.f;
            o[6] = E.x; o[7] = E.y; o[8] = E.z;
        }
    }
    template <class QT>
    __device__ static __forceinline__ void degenerate(const QT &Q, uint32_t i) { begin(Q, i); }
    template <class QT>
    __device__ static __forceinline__ void finish(const QT &Q, uint32_t i) {  // the means, as features_body divides
        float *o = record(Q, i);
        const float c = (float)Q.n_samples;
        for (uint32_t k = 0; k < 11u; ++k) o[k] = o[k] / c;
        o[11] = 0.f;
    }
};

}  // namespace hrtk
}  // extern "C++"

// Waves per SIMD the plain and lights builds leave registers for (the proof builds: 2, as everywhere), chosen by the A/B of
// tools/path_guides_bench.py --waves-ab over -D builds of these (profiles/path_features_waves_ab.json, DESIGN.md section 5 "Path
// features"), starting from the bounds of the lit path families over the same sources (5, 4 and 5).  Measured on MI355X, 2 / 3 / 4 / 5
// waves, cornell_mesh and random_spheres (lights): one sample of 1080p record rays 0.234 / 0.181 / 0.182 / 0.163 and 1.13 / 0.962 /
// 0.934 / 0.876 ms, a 1080p frame of 16 samples 7.64 / 5.49 / 4.31 / 3.41 and 16.6 / 14.1 / 13.4 / 11.6 ms, 64 views of 128 x 128 x 16
// 10.95 / 7.61 / 6.19 / 5.79 and 35.4 / 26.0 / 22.1 / 20.9 ms.  Five wins all six: the tail has no look-up to hold registers for, so
// the frame family leaves the four of hrt_lens_lit_paths_kernel.
#ifndef HRT_PATH_FEATURES_MIN_WAVES
#define HRT_PATH_FEATURES_MIN_WAVES HRT_RADIANCE_MIN_WAVES
#endif
#ifndef HRT_LENS_PATH_FEATURES_MIN_WAVES
#define HRT_LENS_PATH_FEATURES_MIN_WAVES 5
#endif
#ifndef HRT_LENS_VIEWS_PATH_FEATURES_MIN_WAVES
#define HRT_LENS_VIEWS_PATH_FEATURES_MIN_WAVES 5
#endif

HRT_TAIL_FAMILY(hrt_path_features_kernel, RecordRays, DRadiance, FeatureTail, HRT_PATH_FEATURES_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_path_features_kernel, LensRays, DLensRadiance, FeatureTail, HRT_LENS_PATH_FEATURES_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_lens_views_path_features_kernel, LensViewRays, DLensViewsRadiance, FeatureTail, HRT_LENS_VIEWS_PATH_FEATURES_MIN_WAVES)

// Checked in the header's order: hrt_path_tails' checks without tail_after and bias (d_out: 4-byte aligned, the record is 48 bytes).
int hrt_path_features(hrt_scene *s, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, uint32_t flags,
                      float *d_out, void *stream) {
    const std::string who = "hrt_path_features";
    int rc = query_check(who, flags, 0u, nullptr, nullptr, nullptr, 4u, 0u);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = query_check(who, flags, 0u, d_rays, d_keys, d_out, 4u, n)) != HRT_OK) return rc;
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    DRadiance Q;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    return radiance_launch(hrt_path_features_kernel_builds, Q, s, sample, 1u, seed, flags, d_out, n, stream);
}

// What the frame forms check after the lens and the frame, in the header's order.
static int path_features_samples_check(const std::string &who, uint32_t first_sample, uint32_t n_samples, const float *d_features) {
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive (a pixel-centre path has no stream)");
    if ((uint64_t)first_sample + n_samples > 0xffffffffull) return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples overflows 32 bits");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if ((uintptr_t)d_features % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": d_features is not 4-byte aligned");
    return HRT_OK;
}

// The fused launch of one frame's path features on `stream` (the lens checked, the scene entered).
static int lens_path_features_launch(hrt_scene *s, const DLens &L, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                                     float *d_features, hipStream_t stream) {
    DLensRadiance Q;
    return lens_launch(hrt_lens_path_features_kernel_builds, Q, s, L, w, h, first_sample, n_samples, seed, 0u, d_features, stream);
}

int hrt_render_lens_path_features(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                                  float *d_features, void *stream) {
    const std::string who = "hrt_render_lens_path_features";
    DLens L;
    int rc = lens_check(who, lens, L);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc == HRT_OK) rc = path_features_samples_check(who, first_sample, n_samples, d_features);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    return lens_path_features_launch(s, L, w, h, first_sample, n_samples, seed, d_features, (hipStream_t)stream);
}

// The pinhole lens of a camera hrt_render accepts.
static hrt_lens pinhole_lens(const hrt_camera *cam) {
    hrt_lens lens;
    std::memset(&lens, 0, sizeof(lens));
    lens.cam = *cam;
    lens.projection = HRT_LENS_PERSPECTIVE;
    return lens;
}

int hrt_render_path_features(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                             float *d_features, void *stream) {
    const std::string who = "hrt_render_path_features";
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    const hrt_lens lens = pinhole_lens(cam);
    DLens L;
    int rc = check_frame(who, w, h, k_max_records);
    if (rc == HRT_OK) rc = path_features_samples_check(who, first_sample, n_samples, d_features);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc == HRT_OK) rc = lens_check(who, &lens, L);  // the camera, refused as hrt_render_features refuses it: after the scene
    if (rc != HRT_OK) return rc;
    return lens_path_features_launch(s, L, w, h, first_sample, n_samples, seed, d_features, (hipStream_t)stream);
}

// dn_render's feature launch under HRT_GUIDES_FIRST_DIFFUSE (hrt_denoise.hip declares it): the scene entered, n_samples >= 1.
static int path_features_frame(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                               float *d_features, hipStream_t stream) {
    const hrt_lens lens = pinhole_lens(cam);
    DLens L;
    const int rc = lens_check("hrt_render_path_features", &lens, L);
    return rc != HRT_OK ? rc : lens_path_features_launch(s, L, w, h, first_sample, n_samples, seed, d_features, stream);
}

int hrt_render_lens_views_path_features(hrt_scene *s, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t first_sample,
                                        uint32_t n_samples, float *d_features, void *stream) {
    const std::string who = "hrt_render_lens_views_path_features";
    std::vector<DLensView> blocks;
    if (n_views == 0u) return HRT_OK;
    int rc = lens_views_blocks(who, views, n_views, blocks);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc == HRT_OK) rc = path_features_samples_check(who, first_sample, n_samples, d_features);
    if (rc == HRT_OK) rc = lens_views_limit(who, n_views, w, h, k_max_records);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    DLensViewsRadiance Q;
    return lens_views_launch(hrt_lens_views_path_features_kernel_builds, Q, s, blocks, w, h, first_sample, n_samples, 0u, d_features, (hipStream_t)stream);
}
