// Lit paths (include/hrt.h "Lit paths": hrt_trace_lit_paths, hrt_path_tails, hrt_probes_lit_paths_device, hrt_probes_lit_paths): a
// path of the integrator that ENDS in a probe volume at its K-th diffuse hit -- mirror and glass are followed, and K - 1 real diffuse
// bounces are traced before the volume takes over.  Included by hrt_api.hip inside its extern "C" block, after hrt_probe_lit.hip
// (DLit, DProbeLit, lit_lookup and the host checks, which carry tail_after for the entry points here).
//
// There is no path loop in this file: the kernels are radiance_body (hrt_radiance.hip) with a TAIL policy -- bounce loop, mesh
// parking, direct light and sky are the integrator's own, and the policy is the one hook in stage C, between `thr = thr * albedo`
// and `scatter`.  Sources x tails:
//   RecordRays x VolumeTail  hrt_lit_paths_kernel         one lane per ray, the samples of a ray in ascending order
//   RecordRays x RecordTail  hrt_path_tails_kernel        one lane per ray, ONE sample: the path's end as 16 floats instead of a colour
//   ProbeRays  x VolumeTail  hrt_probes_lit_paths_kernel  one wave per (probe, block) item, ProbeRays' sums
// A path with a tail is not pruned (radiance_body turns `prune` off for it): the last-segment prune would drop a hit at which the
// tail fires, and a tail record counts segments by the unpruned rule.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

// The launch records: those of the one-segment forms with K, and DRadiance with K and the bias a tail record carries.
struct DLitPaths : DLit {
    uint32_t tail_after;
};
struct DProbeLitPaths : DProbeLit {
    uint32_t tail_after;
};
struct DPathTails : DRadiance {  // out: HRT_TAIL_FLOATS floats per ray
    uint32_t tail_after;
    float bias;
};

extern "C++" {
namespace hrtk {

// G at the tail: the look-up of {p, time, n, bias} in the launch's volume, as a lit ray's.
struct VolumeTail {
    static constexpr int kind = 1;
    template <class QT>
    __device__ static __forceinline__ f3 gather(const QT &Q, const f3 &p, const f3 &n) { return lit_lookup(Q.vol, p, n); }
};

// The path's end, written out: four 16-byte stores per lane into record i.
struct RecordTail {
    static constexpr int kind = 2;
    __device__ static __forceinline__ void store(const DPathTails &Q, uint32_t i, const float4 &a, const float4 &b, const float4 &c, const float4 &d) {
        float4 *o = (float4 *)Q.out + (size_t)i * (HRT_TAIL_FLOATS / 4u);  // i < Q.n
        o[0] = a; o[1] = b; o[2] = c; o[3] = d;
    }
    __device__ static __forceinline__ void reached(const DPathTails &Q, uint32_t i, const f3 &p, float time, const f3 &n, const f3 &thr, uint32_t segments,
                                                   const f3 &rad) {
        store(Q, i, make_float4(p.x, p.y, p.z, time), make_float4(n.x, n.y, n.z, Q.bias),
              make_float4(thr.x, thr.y, thr.z, __uint_as_float(segments | HRT_TAIL_REACHED)), make_float4(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f, 0.f));
    }
    __device__ static __forceinline__ void unreached(const DPathTails &Q, uint32_t i, uint32_t segments, const f3 &rad) {
        store(Q, i, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, __uint_as_float(segments)),
              make_float4(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f, 0.f));
    }
    __device__ static __forceinline__ void degenerate(const DPathTails &Q, uint32_t i) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        store(Q, i, z, z, z, z);
    }
};

}  // namespace hrtk
}  // extern "C++"

// The four builds of a radiance_body family with a tail.  WAVES: the waves per SIMD the plain and lights builds leave registers for.
// The volume tail's look-up holds 28 accumulators and eight weights on top of the path's state: at two waves (the one-segment lit
// kernels' bound) nothing spills, and it is the slowest form.  Measured on MI355X, cornell_mesh (DESIGN.md section 5 "Lit paths";
// -DHRT_LIT_PATHS_MIN_WAVES / -DHRT_PROBES_LIT_PATHS_MIN_WAVES: the A/B builds), 2 / 3 / 4 / 5 waves: a 16^3 x 1024 probe update
// with tail_after = 1 takes 2.32 / 2.10 / 1.84 / 1.80 ms, a 1080p sample of the lit frame 0.387 / 0.326 / 0.373 / 0.350 ms.
#define HRT_TAIL_FAMILY(base, SRC, QT, TAIL, WAVES)                                                                                                   \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, WAVES) base(const QT Q) { radiance_body<false, false, SRC, QT, TAIL>(Q); }          \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, WAVES) base##_lights(const QT Q) { radiance_body<true, false, SRC, QT, TAIL>(Q); }  \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) base##_exact(const QT Q) { radiance_body<false, true, SRC, QT, TAIL>(Q); }       \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) base##_lights_exact(const QT Q) { radiance_body<true, true, SRC, QT, TAIL>(Q); } \
    static void (*const base##_builds[4])(const QT) = {base, base##_lights, base##_exact, base##_lights_exact};

#ifndef HRT_LIT_PATHS_MIN_WAVES
#define HRT_LIT_PATHS_MIN_WAVES 3
#endif
#ifndef HRT_PROBES_LIT_PATHS_MIN_WAVES
#define HRT_PROBES_LIT_PATHS_MIN_WAVES 5
#endif
HRT_TAIL_FAMILY(hrt_lit_paths_kernel, RecordRays, DLitPaths, VolumeTail, HRT_LIT_PATHS_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_path_tails_kernel, RecordRays, DPathTails, RecordTail, HRT_RADIANCE_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_probes_lit_paths_kernel, ProbeRays, DProbeLitPaths, VolumeTail, HRT_PROBES_LIT_PATHS_MIN_WAVES)

static int lit_tail_check(const std::string &who, uint32_t tail_after) {
    if (tail_after < 1u || tail_after > HRT_MAXBOUNCES)
        return fail(HRT_ERR_INVALID, who + ": tail_after must be in 1 .. HRT_MAXBOUNCES = " + std::to_string(HRT_MAXBOUNCES) + " (got " + std::to_string(tail_after) + ")");
    return HRT_OK;
}

static int lit_paths_launch(hrt_scene *s, const DLitVolume &vol, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                            uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t tail_after, float *d_out, void *stream) {
    DLitPaths Q;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    Q.vol = vol;
    Q.tail_after = tail_after;
    return radiance_launch(hrt_lit_paths_kernel_builds, Q, s, first_sample, n_samples, seed, flags, d_out, n, stream);
}

// The trace launch of a fused update with a tail: Q0 is the record probes_lit_launch has filled for the one-segment kernel.
static int probes_lit_paths_trace(hrt_scene *s, const DProbeLit &Q0, uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags,
                                  uint32_t tail_after, uint32_t items, hipStream_t stream) {
    DProbeLitPaths Q;
    static_cast<DProbeLit &>(Q) = Q0;
    Q.tail_after = tail_after;
    return radiance_launch(hrt_probes_lit_paths_kernel_builds, Q, s, first_sample, n_samples, seed, flags, s->pl_blocks.as<float>(), items * 64u, stream);
}

int hrt_trace_lit_paths(hrt_scene *s, const hrt_probe_volume *v, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                        uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                        void *stream) {
    return lit_trace("hrt_trace_lit_paths", true, s, v, d_rays, d_keys, n, first_sample, n_samples, seed, flags, eval_flags, bias, tail_after, d_out, stream);
}

int hrt_probes_lit_paths_device(hrt_scene *s, const hrt_probe_volume *v, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                                uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                                void *stream) {
    return probes_lit_device("hrt_probes_lit_paths_device", true, s, v, d_probes, d_keys, n, first_sample, n_samples, seed, flags, eval_flags, bias,
                             tail_after, d_out, stream);
}

int hrt_probes_lit_paths(hrt_scene *s, const hrt_probe_volume *v, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed,
                         uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out, hrt_stats *stats) {
    return probes_lit_host("hrt_probes_lit_paths", true, s, v, probes, keys, n, spp, seed, flags, eval_flags, bias, tail_after, out, stats);
}

// Checked in the header's order: flags, tail_after, bias, (an empty batch,) the pointers, n, then the scene and the library state.
int hrt_path_tails(hrt_scene *s, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, uint32_t flags, float bias,
                   uint32_t tail_after, float *d_out, void *stream) {
    const std::string who = "hrt_path_tails";
    int rc = query_check(who, flags, 0u, nullptr, nullptr, nullptr, 16u, 0u);
    if (rc == HRT_OK) rc = lit_tail_check(who, tail_after);
    if (rc != HRT_OK) return rc;
    if (!std::isfinite(bias)) return fail(HRT_ERR_INVALID, who + ": bias must be finite (got " + std::to_string(bias) + ")");
    if (n == 0u) return HRT_OK;
    if ((rc = query_check(who, flags, 0u, d_rays, d_keys, d_out, 16u, n)) != HRT_OK) return rc;
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    DPathTails Q;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    Q.tail_after = tail_after;
    Q.bias = bias;
    return radiance_launch(hrt_path_tails_kernel_builds, Q, s, sample, 1u, seed, flags, d_out, n, stream);
}
