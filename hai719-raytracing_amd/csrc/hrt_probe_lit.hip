// Lit rays and probe relighting (include/hrt.h "Lit rays" and the hysteresis update hrt_probe_volume_blend*): the radiance of a ray
// whose path ENDS in a probe volume at its first hit -- one closest hit, the hit shaded with the integrator's own device functions,
// and everything beyond it taken from the volume as it stands.  Included by hrt_api.hip inside its extern "C" block, after
// hrt_probes.hip (probe_sample, ProbeRays' sum), hrt_rays.hip (query_context, query_margin, query_ray) and hrt_probe_volume.hip
// (the volume, pv_fold_corner, pv_basis, pv_channel).
//
// This file states the rule "a path ends in the volume" ONCE for every lit source: on the device DLitVolume, the record template
// Lit<Base> and lit_lookup; on the host LitRule, the value an entry point makes of its four rule parameters, with the rule's
// checks and the record's filling.  The entry points of "Lit rays" are in hrt_lit_paths.hip, next to their "Lit paths" forms.
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

// The launch record of a lit source: its plain sibling's (query_launch, radiance_launch and the sibling's own launch reach their
// fields by name) with the volume and K = tail_after.  The one-segment kernels do not read tail_after; those over record rays and
// probes (hrt_lit_kernel, hrt_probes_lit_kernel) take the record WITHOUT that word, LitOne<Base>, the head of a Lit<Base>.  With
// the word their kernel arguments would grow by eight bytes, the hidden arguments behind them would move, and one s_add_u32 in
// each of the eight kernels would change: they are kept instruction for instruction instead.
extern "C++" {
template <class Base>
struct LitOne : Base {
    DLitVolume vol;
};
template <class Base>
struct Lit : LitOne<Base> {
    uint32_t tail_after;  // 0: one segment
};
}
using DLit = Lit<DRadiance>;
using DProbeLit = Lit<DProbe>;

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
template <bool LIGHTS, bool EXACT, class SRC, class QT>
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
template <bool LIGHTS, bool EXACT, class QT>
__device__ __forceinline__ void probes_lit_body(const QT &Q) {
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

// The families of the two bodies over record rays and probes, without a register bound; over a per-sample source (the lit
// frames and bakes of the later files) a family of lit_body names the waves per SIMD of its plain and lights builds.
#define HRT_LIT_FAMILY(base, SRC, QT, WAVES) HRT_KERNEL_FAMILY(base, QT, (HRT_RADIANCE_WG, WAVES), (HRT_RADIANCE_WG, 2), lit_body, SRC, QT)

HRT_KERNEL_FAMILY(hrt_lit_kernel, LitOne<DRadiance>, (HRT_RADIANCE_WG), (HRT_RADIANCE_WG), lit_body, RecordRays, LitOne<DRadiance>)
HRT_KERNEL_FAMILY(hrt_probes_lit_kernel, LitOne<DProbe>, (HRT_RADIANCE_WG), (HRT_RADIANCE_WG), probes_lit_body, LitOne<DProbe>)

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

// tail_after: 0 is the one-segment rule where the entry point accepts it (least == 0), else 1 .. HRT_MAXBOUNCES (hrt_path_tails has
// a tail_after and no volume, so no LitRule).
static int lit_tail_check(const std::string &who, uint32_t tail_after, uint32_t least) {
    if (tail_after < least || tail_after > HRT_MAXBOUNCES)
        return fail(HRT_ERR_INVALID, who + ": tail_after must be in 1 .. HRT_MAXBOUNCES = " + std::to_string(HRT_MAXBOUNCES) + " (got " + std::to_string(tail_after) + ")");
    return HRT_OK;
}

// THE RULE on the host: what an entry point makes of (volume, eval_flags, bias, tail_after), once, and passes on as one value.  A
// one-segment entry point of "Lit rays" has tail_after 0, a *_paths entry point the least tail_after 1.  A plain entry point has
// NoRule (hrt_radiance.hip) in its place.
extern "C++" {
struct LitRule {
    const hrt_probe_volume *v;
    uint32_t eval_flags;
    float bias;
    uint32_t tail_after;
    uint32_t least = 0u;  // the smallest tail_after the entry point accepts: 1 for the *_paths entry points

    int check_tail(const std::string &who) const { return lit_tail_check(who, tail_after, least); }
    // "Lit rays"' checks 2..6 of the header's order: eval_flags, the volume, bias.
    int check_volume(const std::string &who) const {
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
    // Both, where nothing comes between them (a batch of views returns for no views there).
    int check(const std::string &who) const {
        const int rc = check_tail(who);
        return rc != HRT_OK ? rc : check_volume(who);
    }
    // The last checks: the scene, a volume of another device than the scene's, then the library state.
    int enter(const std::string &who, hrt_scene *s) const {
        if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
        if (v->device != s->device)
            return fail(HRT_ERR_INVALID, who + ": the volume lives on device " + std::to_string(v->device) + ", the scene on device " + std::to_string(s->device));
        return enter_scene(who, s);
    }
    // The rule's part of a launch record (the checks passed).
    template <class Base>
    void fill(Lit<Base> &Q) const {
        Q.vol.grid = v->grid;
        Q.vol.packed = v->packed.as<float4>();
        Q.vol.moments = (eval_flags & HRT_LIT_VISIBLE) ? v->depth.as<float2>() : nullptr;
        Q.vol.eval_flags = eval_flags & HRT_PROBE_EVAL_FACING;
        Q.vol.bias = bias;
        Q.tail_after = tail_after;
    }
};
}  // extern "C++"

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
