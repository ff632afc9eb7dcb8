// Lit paths (include/hrt.h "Lit paths": hrt_trace_lit_paths, hrt_path_tails, hrt_probes_lit_paths_device, hrt_probes_lit_paths): a
// path of the integrator that ENDS in a probe volume at its K-th diffuse hit -- mirror and glass are followed, and K - 1 real diffuse
// bounces are traced before the volume takes over -- and, since each shares one body with its "Lit paths" form, the entry points of
// "Lit rays" (hrt_trace_lit, hrt_probes_lit_device, hrt_probes_lit).  Included by hrt_api.hip inside its extern "C" block, after
// hrt_probe_lit.hip (Lit<Base>, lit_lookup, the one-segment kernels and LitRule) and hrt_probes.hip (probe_call, probe_launch).
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

// The launch record of a tail record's kernel: DRadiance with K and the bias the record carries (no volume: not a Lit<Base>).
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
#define HRT_TAIL_FAMILY(base, SRC, QT, TAIL, WAVES) \
    HRT_KERNEL_FAMILY(base, QT, (HRT_RADIANCE_WG, WAVES), (HRT_RADIANCE_WG, 2), radiance_body, SRC, QT, TAIL)

#ifndef HRT_LIT_PATHS_MIN_WAVES
#define HRT_LIT_PATHS_MIN_WAVES 3
#endif
#ifndef HRT_PROBES_LIT_PATHS_MIN_WAVES
#define HRT_PROBES_LIT_PATHS_MIN_WAVES 5
#endif
HRT_TAIL_FAMILY(hrt_lit_paths_kernel, RecordRays, DLit, VolumeTail, HRT_LIT_PATHS_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_path_tails_kernel, RecordRays, DPathTails, RecordTail, HRT_RADIANCE_MIN_WAVES)
HRT_TAIL_FAMILY(hrt_probes_lit_paths_kernel, ProbeRays, DProbeLit, VolumeTail, HRT_PROBES_LIT_PATHS_MIN_WAVES)

// hrt_trace_lit and hrt_trace_lit_paths, checked in the header's order.
static int lit_trace(const std::string &who, hrt_scene *s, const LitRule &R, const float *d_rays, const uint32_t *d_keys, uint32_t n,
                     uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_out, void *stream) {
    {  // the flags alone first (query_check with an empty batch), then the rule, then the rest of query_check
        const int frc = query_check(who, flags, HRT_RADIANCE_ACCUMULATE, nullptr, nullptr, nullptr, 4u, 0u);
        if (frc != HRT_OK) return frc;
    }
    int rc = R.check(who);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = query_check(who, flags, HRT_RADIANCE_ACCUMULATE, d_rays, d_keys, d_out, 4u, n)) != HRT_OK) return rc;
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    if ((rc = R.enter(who, s)) != HRT_OK) return rc;
    DLit Q;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    R.fill(Q);
    if (R.tail_after) return radiance_launch(hrt_lit_paths_kernel_builds, Q, s, first_sample, n_samples, seed, flags, d_out, n, stream);
    return radiance_launch(hrt_lit_kernel_builds, static_cast<LitOne<DRadiance> &>(Q), s, first_sample, n_samples, seed, flags, d_out, n, stream);
}

int hrt_trace_lit(hrt_scene *s, const hrt_probe_volume *v, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                  uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, float *d_out, void *stream) {
    return lit_trace("hrt_trace_lit", s, LitRule{v, eval_flags, bias, 0u}, d_rays, d_keys, n, first_sample, n_samples, seed, flags, d_out, stream);
}

int hrt_trace_lit_paths(hrt_scene *s, const hrt_probe_volume *v, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                        uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                        void *stream) {
    return lit_trace("hrt_trace_lit_paths", s, LitRule{v, eval_flags, bias, tail_after, 1u}, d_rays, d_keys, n, first_sample, n_samples, seed, flags, d_out,
                     stream);
}

// The four lit probe entry points: probe_call with the rule, probe_launch with the lit record (all of it, or its one-segment head),
// the table tail_after chooses and block values of their own (pl_blocks: a lit probe launch may overlap a plain one).
static int probes_lit(const std::string &who, bool dev, hrt_scene *s, const LitRule &R, const float *probes, const uint32_t *keys,
                      uint32_t n, uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return probe_call(who, dev, s, R, "a lit probe launch has one kernel form", probes, keys, n, first_sample, n_samples, flags, out, stream, stats,
                      [&](const float *d_probes, const uint32_t *d_keys, float *d_out, hipStream_t st) {
                          DProbeLit Q;
                          R.fill(Q);
                          if (R.tail_after)
                              return probe_launch(hrt_probes_lit_paths_kernel_builds, Q, s, s->pl_blocks, d_probes, d_keys, n, first_sample, n_samples, seed,
                                                  flags, d_out, st);
                          return probe_launch(hrt_probes_lit_kernel_builds, static_cast<LitOne<DProbe> &>(Q), s, s->pl_blocks, d_probes, d_keys, n,
                                              first_sample, n_samples, seed, flags, d_out, st);
                      });
}

int hrt_probes_lit_device(hrt_scene *s, const hrt_probe_volume *v, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                          uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, float *d_out, void *stream) {
    return probes_lit("hrt_probes_lit_device", true, s, LitRule{v, eval_flags, bias, 0u}, d_probes, d_keys, n, first_sample, n_samples, seed, flags,
                      d_out, stream, nullptr);
}

int hrt_probes_lit(hrt_scene *s, const hrt_probe_volume *v, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed,
                   uint32_t flags, uint32_t eval_flags, float bias, float *out, hrt_stats *stats) {
    return probes_lit("hrt_probes_lit", false, s, LitRule{v, eval_flags, bias, 0u}, probes, keys, n, 0u, spp, seed, flags, out, nullptr, stats);
}

int hrt_probes_lit_paths_device(hrt_scene *s, const hrt_probe_volume *v, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                                uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                                void *stream) {
    return probes_lit("hrt_probes_lit_paths_device", true, s, LitRule{v, eval_flags, bias, tail_after, 1u}, d_probes, d_keys, n, first_sample, n_samples,
                      seed, flags, d_out, stream, nullptr);
}

int hrt_probes_lit_paths(hrt_scene *s, const hrt_probe_volume *v, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed,
                         uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out, hrt_stats *stats) {
    return probes_lit("hrt_probes_lit_paths", false, s, LitRule{v, eval_flags, bias, tail_after, 1u}, probes, keys, n, 0u, spp, seed, flags, out, nullptr,
                      stats);
}

// Checked in the header's order: flags, tail_after, bias, (an empty batch,) the pointers, n, then the scene and the library state.
int hrt_path_tails(hrt_scene *s, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, uint32_t flags, float bias,
                   uint32_t tail_after, float *d_out, void *stream) {
    const std::string who = "hrt_path_tails";
    int rc = query_check(who, flags, 0u, nullptr, nullptr, nullptr, 16u, 0u);
    if (rc == HRT_OK) rc = lit_tail_check(who, tail_after, 1u);
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
