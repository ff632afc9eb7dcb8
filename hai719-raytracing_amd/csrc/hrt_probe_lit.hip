// Lit rays and probe relighting (include/hrt.h "Lit rays": hrt_trace_lit, hrt_probes_lit_device, hrt_probes_lit and the hysteresis
// update hrt_probe_volume_blend*): the radiance of a ray whose path ENDS in a probe volume at its first hit -- one closest hit, the
// hit shaded with the integrator's own device functions, and everything beyond it taken from the volume as it stands.  Included by
// hrt_api.hip inside its extern "C" block, after hrt_probes.hip (probe_sample, ProbeRays' sum, the record checks), hrt_rays.hip
// (query_context, query_margin, query_ray) and hrt_probe_volume.hip (the volume, pv_fold_corner, pv_basis, pv_channel).
//
// Two shapes of one per-sample body (lit_sample):
//   hrt_lit_kernel builds: one lane per ray by grid stride, the samples of a ray in ascending order -- the probe-lit frame;
//   hrt_probes_lit_kernel builds: one WAVE per (probe, block of HRT_PROBE_BLOCK samples) item, as hrt_probe_kernel maps them, but
//     with a body of its own: a sample is ONE segment, so none of radiance_body's stages is needed -- no bounce loop, no mesh
//     parking.  A lane makes its sample's direction (probe_sample), traces, shades, gathers, and adds value x basis onto its 27
//     partial sums with ProbeRays::add; the wave closes the item with ProbeRays::finish and hrt_probe_fold_kernel adds a probe's
//     blocks.  The sum is therefore "Light probes"' sum, addition for addition.
// The look-up inside both is a LANE TO A POINT: every lane has a hit of its own, so it runs probevol::cell / cell_visible
// (hrt_probe_volume_cell.h) and reads its eight records whole, as the lane-per-point build of hrt_probe_eval_kernel does.  The
// cooperative form (eight lanes serving one hit's corners in eight passes through LDS) was not built.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

// What a lit launch reads of the volume, by value inside the launch record.
struct DLitVolume {
    probevol::Grid grid;
    const float4 *packed;   // count records of HRT_PROBE_RECORD_FLOATS floats
    const float2 *moments;  // count x HRT_PROBE_DEPTH_TEXELS pairs; NULL without HRT_LIT_VISIBLE
    uint32_t eval_flags;    // HRT_PROBE_EVAL_FACING or 0
    float bias;
};

// The launch records: DRadiance and DProbe (query_launch and radiance_launch reach their fields by name) with the volume.
struct DLit : DRadiance {
    DLitVolume vol;
};
struct DProbeLit : DProbe {
    DLitVolume vol;
};

extern "C++" {
namespace hrtk {

// G: the look-up of the point record {p, time, n, bias}, steps 1-6 of "Probe volumes" (irradiance form) or of "Probe visibility".
__device__ __forceinline__ f3 lit_lookup(const DLitVolume &V, const f3 &p, const f3 &n) {
    const float P[3] = {p.x, p.y, p.z}, N[3] = {n.x, n.y, n.z};
    uint32_t index[8];
    float weight[8], Nn[3];
    const bool ok = V.moments ? probevol::cell_visible(V.grid, P, N, V.bias, V.eval_flags, (const float *)V.moments, index, weight, Nn)
                              : probevol::cell(V.grid, P, N, V.eval_flags, index, weight, Nn);
    if (!ok) return mk(0.f, 0.f, 0.f);  // a degenerate point record
    float a[HRT_PV_PIECES][4];
#pragma unroll
    for (uint32_t q = 0; q < HRT_PV_PIECES; ++q) a[q][0] = a[q][1] = a[q][2] = a[q][3] = 0.f;
#pragma unroll
    for (uint32_t m = 0; m < 8u; ++m) {
        const float4 *rec = V.packed + (size_t)index[m] * HRT_PV_PIECES;  // an index < nx * ny * nz
#pragma unroll
        for (uint32_t q = 0; q < HRT_PV_PIECES; ++q) pv_fold_corner(a[q], weight[m], rec[q]);
    }
    float Y[HRT_PROBE_COEFFS], g[3];
    pv_basis(Nn[0], Nn[1], Nn[2], Y);
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        float mine[HRT_PROBE_COEFFS];
#pragma unroll
        for (uint32_t k = 0; k < HRT_PROBE_COEFFS; ++k) mine[k] = a[(3u * k + ch) >> 2][(3u * k + ch) & 3u];
        g[ch] = pv_channel(mine, Y, false);
    }
    return mk(g[0], g[1], g[2]);
}

// Steps 2-5 of the rule for one sample: `ray` with its margin and first-segment flags in cx, rng at draw 3 of the sample's stream.
template <bool LIGHTS, class CX>
__device__ __forceinline__ f3 lit_sample(const CX &cx, const DLitVolume &V, const Ray &ray, Rng &rng) {
    f3 thr = mk(1.f, 1.f, 1.f), rad = mk(0.f, 0.f, 0.f);
    const Hit h = closest_hit(cx, ray);
    if (h.kind == 0u) {
        rad = rad + thr * sky(cx, ray.d, 6);  // radiance_body's miss on a path's first segment
        return mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f);
    }
    const Surface sf = shade(cx, ray, h);
    f3 direct = mk(0.f, 0.f, 0.f);
    if (LIGHTS) direct = direct_light(cx, sf, ray, rng);
    rad = rad + thr * (direct + sf.emission);
    thr = thr * sf.albedo;
    f3 G = mk(0.f, 0.f, 0.f);
    if (sf.type == 0u) G = lit_lookup(V, sf.p, sf.n);  // diffuse; mirror and glass are not followed
    return mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f) + thr * G;
}

// One lane per ray by grid stride; hrt_trace_radiance's handling of a degenerate ray, of the keys and of the running sums.
// SRC is radiance_body's source policy: RecordRays reads record i once, with Q.keys and the launch's seed; a per-sample source
// (LensRays, LensViewRays: the lit frames of hrt_lit_frames.hip) makes the ray, the margin, the key and the seed of every sample,
// and a sample it does not trace adds nothing.
template <bool LIGHTS, bool EXACT, class SRC = RecordRays, class QT = DLit>
__device__ __forceinline__ void lit_body(const QT &Q) {
    CtxT<EXACT, false, false, true> cx;
    unsigned long long stamps_local[17] = {0};
    query_context(cx, Q.scene, Q.lds_units, Q.flags, stamps_local);
    const bool accumulate = (Q.flags & HRT_RADIANCE_ACCUMULATE) != 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const float far = query_far(Q.bound);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < Q.n; i += stride) {
        float *o = Q.out + (size_t)i * 3u;
        Ray ray;
        [[maybe_unused]] float tmax;  // not read: a path's first segment has no far end
        if constexpr (!SRC::per_sample) {
            if (!query_ray(Q, i, ray, tmax)) {  // adds nothing
                if (!accumulate) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
                continue;
            }
        }
        uint32_t key;
        if constexpr (SRC::per_sample) key = SRC::key(Q, i);
        else key = Q.keys ? Q.keys[i] : i;
        if constexpr (!SRC::per_sample) query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, cx.flags);
        f3 sum = mk(0.f, 0.f, 0.f);
        if (accumulate) sum = mk(o[0], o[1], o[2]);
        for (uint32_t s = 0; s < Q.n_samples; ++s) {
            Rng rng;
            if constexpr (SRC::per_sample) {  // this sample's own ray, and the margin and far-origin flag of that ray
                if (!SRC::sample(Q, i, Q.first_sample + s, ray)) continue;  // a degenerate sample adds nothing
                query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, cx.flags);
                uint32_t seed_lo, seed_hi;
                SRC::seed(Q, i, seed_lo, seed_hi);
                rng.start(seed_lo, seed_hi, key, Q.first_sample + s);
            } else {
                rng.start(Q.seed_lo, Q.seed_hi, key, Q.first_sample + s);
            }
            rng.i = 3u;  // draws 0..2 are the camera's u, v, time
            sum = sum + lit_sample<LIGHTS>(cx, Q.vol, ray, rng);
        }
        const float ns = accumulate ? 1.f : (float)Q.n_samples;  // x / 1.f is exact
        o[0] = sum.x / ns; o[1] = sum.y / ns; o[2] = sum.z / ns;
    }
}

// One wave per (probe, block) item by a wave-granular grid stride: Q.n counts lanes, 64 per item, and is a multiple of 64, as is
// the stride, so a whole wave takes an item or none.  ProbeRays keeps the item's four words and the lanes' partial sums in LDS; a
// wave touches only its own columns and words, so nothing here needs a barrier.
template <bool LIGHTS, bool EXACT>
__device__ __forceinline__ void probes_lit_body(const DProbeLit &Q) {
    CtxT<EXACT, false, false, true> cx;
    unsigned long long stamps_local[17] = {0};
    query_context(cx, Q.scene, Q.lds_units, Q.flags, stamps_local);
    const uint32_t stride = gridDim.x * blockDim.x;
    const float far = query_far(Q.bound);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < Q.n; i += stride) {
        ProbeRays::begin(Q, i);
        const uint32_t key = ProbeRays::key(Q, i), end = ProbeRays::end(Q, i);
        for (uint32_t s = ProbeRays::first(Q, i); s < end; s += 64u) {  // one pass while HRT_PROBE_BLOCK is 64
            Ray ray;
            if (!ProbeRays::sample(Q, i, Q.first_sample + s, ray)) continue;  // a degenerate sample adds nothing
            query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, cx.flags);
            Rng rng;
            rng.start(Q.seed_lo, Q.seed_hi, key, Q.first_sample + s);
            rng.i = 3u;
            const f3 v = lit_sample<LIGHTS>(cx, Q.vol, ray, rng);
            ProbeRays::add(Q, i, Q.first_sample + s, mk(0.f, 0.f, 0.f) + v);  // what a one-sample hrt_trace_lit stores
        }
        ProbeRays::finish(Q, i);  // all 64 lanes
    }
}

}  // namespace hrtk
}  // extern "C++"

// The four builds of a lit body -- plain, lights, and the two proof builds of HRT_FLAG_EXACT_ONLY -- and their table, indexed
// lights | exact << 1 as radiance_launch indexes it.
#define HRT_LIT_FAMILY(base, body, QT)                                                                                     \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG) base(const QT Q) { body<false, false>(Q); }              \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG) base##_lights(const QT Q) { body<true, false>(Q); }      \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG) base##_exact(const QT Q) { body<false, true>(Q); }       \
    extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG) base##_lights_exact(const QT Q) { body<true, true>(Q); } \
    static void (*const base##_builds[4])(const QT) = {base, base##_lights, base##_exact, base##_lights_exact};

HRT_LIT_FAMILY(hrt_lit_kernel, lit_body, DLit)
HRT_LIT_FAMILY(hrt_probes_lit_kernel, probes_lit_body, DProbeLit)

// One lane per 16-byte piece of a packed record: p = (keep * p) + ((1.f - keep) * c) for the probe's 27 floats, zeros past them.
extern "C" __global__ void __launch_bounds__(HRT_PV_WG) hrt_probe_blend_kernel(const float *__restrict__ coeffs, uint32_t n_pieces, float keep,
                                                                                float4 *__restrict__ packed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // n_pieces <= 2^27
    if (i >= n_pieces) return;
    const uint32_t probe = i / HRT_PV_PIECES, q = i - probe * HRT_PV_PIECES;
    const float *src = coeffs + (size_t)probe * (3u * HRT_PROBE_COEFFS);
    const float4 old = packed[i];
    const float p[4] = {old.x, old.y, old.z, old.w};
    float v[4];
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) v[c] = 4u * q + c < 3u * HRT_PROBE_COEFFS ? (keep * p[c]) + ((1.f - keep) * src[4u * q + c]) : 0.f;
    packed[i] = make_float4(v[0], v[1], v[2], v[3]);
}

// Checks 2..6 of the header's order: eval_flags, the volume, bias.
static int lit_volume_check(const std::string &who, const hrt_probe_volume *v, uint32_t eval_flags, float bias) {
    if (eval_flags & HRT_PROBE_EVAL_RADIANCE)
        return fail(HRT_ERR_INVALID, who + ": eval_flags: HRT_PROBE_EVAL_RADIANCE: the tail of a lit ray is the irradiance about the hit's normal");
    const uint32_t known = HRT_PROBE_EVAL_FACING | HRT_LIT_VISIBLE;
    if (eval_flags & ~known) return fail(HRT_ERR_INVALID, who + ": eval_flags: unknown bits " + std::to_string(eval_flags & ~known));
    if (!v) return fail(HRT_ERR_INVALID, who + ": volume is NULL");
    if (!v->loaded) return fail(HRT_ERR_INVALID, who + ": the volume has no coefficients yet (hrt_probe_volume_update)");
    if ((eval_flags & HRT_LIT_VISIBLE) && !v->has_depth)
        return fail(HRT_ERR_INVALID, who + ": eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet (hrt_probe_volume_update_depth)");
    if (!std::isfinite(bias)) return fail(HRT_ERR_INVALID, who + ": bias must be finite (got " + std::to_string(bias) + ")");
    return HRT_OK;
}

// The last checks: the scene, a volume of another device than the scene's, then the library state.
static int lit_enter(const std::string &who, hrt_scene *s, const hrt_probe_volume *v) {
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    if (v->device != s->device)
        return fail(HRT_ERR_INVALID, who + ": the volume lives on device " + std::to_string(v->device) + ", the scene on device " + std::to_string(s->device));
    return enter_scene(who, s);
}

static DLitVolume lit_volume(const hrt_probe_volume *v, uint32_t eval_flags, float bias) {
    DLitVolume V;
    V.grid = v->grid;
    V.packed = v->packed.as<float4>();
    V.moments = (eval_flags & HRT_LIT_VISIBLE) ? v->depth.as<float2>() : nullptr;
    V.eval_flags = eval_flags & HRT_PROBE_EVAL_FACING;
    V.bias = bias;
    return V;
}

// "Lit paths" (hrt_lit_paths.hip, which comes after this file): the same entry points with a tail after `tail_after` diffuse hits.
// Here tail_after == 0 stands for the one-segment forms of this file; theirs check it right after the flags.
static int lit_tail_check(const std::string &who, uint32_t tail_after);
static int lit_paths_launch(hrt_scene *s, const DLitVolume &vol, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                            uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t tail_after, float *d_out, void *stream);
static int probes_lit_paths_trace(hrt_scene *s, const DProbeLit &Q0, uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags,
                                  uint32_t tail_after, uint32_t items, hipStream_t stream);

static int lit_trace(const std::string &who, bool paths, hrt_scene *s, const hrt_probe_volume *v, const float *d_rays, const uint32_t *d_keys, uint32_t n,
                     uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after,
                     float *d_out, void *stream) {
    {  // the flags alone first (query_check with an empty batch), then the volume, then the rest of query_check
        const int frc = query_check(who, flags, HRT_RADIANCE_ACCUMULATE, nullptr, nullptr, nullptr, 4u, 0u);
        if (frc != HRT_OK) return frc;
    }
    if (paths) { const int trc = lit_tail_check(who, tail_after); if (trc != HRT_OK) return trc; }
    int rc = lit_volume_check(who, v, eval_flags, bias);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = query_check(who, flags, HRT_RADIANCE_ACCUMULATE, d_rays, d_keys, d_out, 4u, n)) != HRT_OK) return rc;
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    if (paths) return lit_paths_launch(s, lit_volume(v, eval_flags, bias), d_rays, d_keys, n, first_sample, n_samples, seed, flags, tail_after, d_out, stream);
    DLit Q;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    Q.vol = lit_volume(v, eval_flags, bias);
    return radiance_launch(hrt_lit_kernel_builds, Q, s, first_sample, n_samples, seed, flags, d_out, n, stream);
}

int hrt_trace_lit(hrt_scene *s, const hrt_probe_volume *v, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                  uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, float *d_out, void *stream) {
    return lit_trace("hrt_trace_lit", false, s, v, d_rays, d_keys, n, first_sample, n_samples, seed, flags, eval_flags, bias, 0u, d_out, stream);
}

// The flags of a lit probe launch: a probe launch's.
static int probes_lit_flags_check(const std::string &who, uint32_t flags) {
    return fused_flags_check(who, flags, "a lit probe launch has one kernel form", "a probe has no direction to normalise",
                             "probes are linear radiance, not a frame");
}

// The fused launch into d_out on `stream` (the scene entered, the limit checked): the trace launch into the scene's block values,
// then hrt_probe_fold_kernel, also when a probe has one block.
static int probes_lit_launch(hrt_scene *s, const hrt_probe_volume *v, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                             uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *d_out,
                             hipStream_t stream) {
    const uint32_t nblocks = (uint32_t)(((uint64_t)n_samples + HRT_PROBE_BLOCK - 1u) / HRT_PROBE_BLOCK);
    const uint32_t items = n * nblocks;  // <= HRT_PROBE_MAX_BLOCKS
    if (const int rc = s->pl_blocks.grow((size_t)items * HRT_PROBE_SUMS * sizeof(float))) return rc;
    DProbeLit Q;
    Q.probes = (const float4 *)d_probes;
    Q.keys = d_keys;
    Q.nblocks = nblocks;
    Q.vol = lit_volume(v, eval_flags, bias);
    if (const int rc = tail_after ? probes_lit_paths_trace(s, Q, first_sample, n_samples, seed, flags, tail_after, items, stream)
                                  : radiance_launch(hrt_probes_lit_kernel_builds, Q, s, first_sample, n_samples, seed, flags, s->pl_blocks.as<float>(),
                                                    items * 64u, stream))
        return rc;
    const uint32_t n_sums = n * HRT_PROBE_SUMS;
    hipLaunchKernelGGL(hrt_probe_fold_kernel, dim3((n_sums + 255u) / 256u), dim3(256), 0, stream, s->pl_blocks.as<float>(), n_sums, nblocks, n_samples,
                       (flags & HRT_RADIANCE_ACCUMULATE) ? 1u : 0u, d_out);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

static int probes_lit_device(const std::string &who, bool paths, hrt_scene *s, const hrt_probe_volume *v, const float *d_probes, const uint32_t *d_keys,
                             uint32_t n, uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias,
                             uint32_t tail_after, float *d_out, void *stream) {
    int rc = probes_lit_flags_check(who, flags);
    if (rc == HRT_OK && paths) rc = lit_tail_check(who, tail_after);
    if (rc == HRT_OK) rc = lit_volume_check(who, v, eval_flags, bias);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = probe_records_check(who, d_probes, d_keys, n, true)) != HRT_OK) return rc;
    if ((rc = probe_samples_out_check(who, n, first_sample, n_samples, d_out, "d_out")) != HRT_OK) return rc;
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    return probes_lit_launch(s, v, d_probes, d_keys, n, first_sample, n_samples, seed, flags, eval_flags, bias, tail_after, d_out, (hipStream_t)stream);
}

int hrt_probes_lit_device(hrt_scene *s, const hrt_probe_volume *v, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample,
                          uint32_t n_samples, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, float *d_out, void *stream) {
    return probes_lit_device("hrt_probes_lit_device", false, s, v, d_probes, d_keys, n, first_sample, n_samples, seed, flags, eval_flags, bias, 0u, d_out,
                             stream);
}

// Blocking, from and into host memory (BlockingCall; the probes and keys are device buffers of the call's, too).
static int probes_lit_host(const std::string &who, bool paths, hrt_scene *s, const hrt_probe_volume *v, const float *probes, const uint32_t *keys, uint32_t n,
                           uint32_t spp, uint64_t seed, uint32_t flags, uint32_t eval_flags, float bias, uint32_t tail_after, float *out, hrt_stats *stats) {
    if (flags & HRT_RADIANCE_ACCUMULATE)
        return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (" + who + "_device)");
    int rc = probes_lit_flags_check(who, flags);
    if (rc == HRT_OK && paths) rc = lit_tail_check(who, tail_after);
    if (rc == HRT_OK) rc = lit_volume_check(who, v, eval_flags, bias);
    if (rc != HRT_OK) return rc;
    if (n == 0u) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return HRT_OK;
    }
    if ((rc = probe_records_check(who, probes, keys, n, false)) != HRT_OK) return rc;
    if ((rc = probe_samples_out_check(who, n, 0u, spp, out, "out")) != HRT_OK) return rc;
    if ((rc = lit_enter(who, s, v)) != HRT_OK) return rc;
    BlockingCall call;
    Scratch d_probes, d_keys;
    if ((rc = d_probes.from_host(probes, (size_t)n * HRT_PROBE_FLOATS * sizeof(float))) != HRT_OK) return rc;
    if (keys && (rc = d_keys.from_host(keys, (size_t)n * sizeof(uint32_t))) != HRT_OK) return rc;
    return call.run(s, (size_t)n * HRT_PROBE_SUMS * sizeof(float), out, (uint64_t)n * spp, stats, [&](float *d_out) {
        return probes_lit_launch(s, v, d_probes.as<float>(), d_keys.as<uint32_t>(), n, 0u, spp, seed, flags, eval_flags, bias, tail_after, d_out, nullptr);
    });
}

int hrt_probes_lit(hrt_scene *s, const hrt_probe_volume *v, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed,
                   uint32_t flags, uint32_t eval_flags, float bias, float *out, hrt_stats *stats) {
    return probes_lit_host("hrt_probes_lit", false, s, v, probes, keys, n, spp, seed, flags, eval_flags, bias, 0u, out, stats);
}

// ---- The hysteresis update of a volume's packed records.

static int pv_blend_check(const std::string &who, const hrt_probe_volume *v, const float *coeffs, const char *name, float keep) {
    if (!v) return fail(HRT_ERR_INVALID, who + ": volume is NULL");
    if (!coeffs) return fail(HRT_ERR_INVALID, who + ": " + name + " is NULL");
    if ((uintptr_t)coeffs % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + name + " is not 4-byte aligned");
    if (!(keep >= 0.f && keep < 1.f)) return fail(HRT_ERR_INVALID, who + ": keep must be in [0, 1) (got " + std::to_string(keep) + ")");
    if (!v->loaded) return fail(HRT_ERR_INVALID, who + ": the volume has no coefficients yet (hrt_probe_volume_update)");
    return pv_enter(who, v);
}

static int pv_blend(hrt_probe_volume *v, const float *d_coeffs, float keep, hipStream_t stream) {
    const uint32_t pieces = v->count * HRT_PV_PIECES;  // <= 2^27
    hipLaunchKernelGGL(hrt_probe_blend_kernel, dim3((pieces + HRT_PV_WG - 1u) / HRT_PV_WG), dim3(HRT_PV_WG), 0, stream, d_coeffs, pieces, keep,
                       v->packed.as<float4>());
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

int hrt_probe_volume_blend_device(hrt_probe_volume *v, const float *d_coeffs, float keep, void *stream) {
    if (const int rc = pv_blend_check("hrt_probe_volume_blend_device", v, d_coeffs, "d_coeffs", keep)) return rc;
    return pv_blend(v, d_coeffs, keep, (hipStream_t)stream);
}

int hrt_probe_volume_blend(hrt_probe_volume *v, const float *coeffs, float keep) {
    if (const int rc = pv_blend_check("hrt_probe_volume_blend", v, coeffs, "coeffs", keep)) return rc;
    Scratch d_coeffs;
    if (const int rc = d_coeffs.from_host(coeffs, (size_t)v->count * 3u * HRT_PROBE_COEFFS * sizeof(float))) return rc;
    if (const int rc = pv_blend(v, d_coeffs.as<float>(), keep, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));  // before the staging copy goes
    return HRT_OK;
}
