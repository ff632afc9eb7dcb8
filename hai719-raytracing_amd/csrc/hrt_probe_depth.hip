// Probe depth (include/hrt.h "Probe visibility": hrt_probe_depth_device, hrt_probe_depth and the two host-only functions of the
// octahedral map): per probe and per texel of an 8 x 8 octahedral map the filtered sums of the distance and the squared distance
// to the scene, over the directions the SH coefficients of "Light probes" saw.  Included by hrt_api.hip inside its extern "C"
// block, after hrt_probes.hip (probe_sample, the record checks) and hrt_rays.hip (query_context, query_margin, closest_hit's
// callers).
//
// As for the probes, one WAVE is one work item, a (probe, block) pair of up to 64 samples.  The wave has two roles in turn.  First
// a lane is a sample: it makes its direction by the rule, traces the closest hit as hrt_rays_closest_kernel does for the record
// hrt_probe_rays writes, and leaves {d, r} in the wave's 64 slots of LDS.  Then a lane is a texel: lane e keeps c_e in registers,
// walks the slots in ascending sample order -- every lane reads the same slot, a broadcast -- and stores its {W, A, B}.
// hrt_probe_depth_fold_kernel adds a probe's block values in ascending order.  The order of every addition is the header's and
// does not depend on how the device schedules the waves.  (The slots could be read through read-lane instead of LDS; the bits do
// not depend on that choice.)
//
// The two roles of a wave are ordered by the LDS queue of the wave itself: its ds_write and ds_read instructions complete in
// order, and the fences below keep the compiler from moving either across the role change.  No workgroup barrier: waves of one
// workgroup take different numbers of items.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

static_assert(HRT_PROBE_DEPTH_TEXELS == 64u && HRT_PROBE_DEPTH_FLOATS == 3u * HRT_PROBE_DEPTH_TEXELS, "a wave's lane is a texel");
#define HRT_PD_BLOCK 64u  // samples per block of the sum: a wave

// The launch record (query_launch reaches scene, bound, lds_units, flags and n by name).  n counts LANES, 64 per (probe, block)
// item; out is the block values, HRT_PROBE_DEPTH_FLOATS floats per item.
struct DProbeDepth {
    const DScene *scene;
    const float4 *probes;  // 1 float4 per probe: {P, time}
    const uint32_t *keys;  // RNG key of probe i (NULL: i)
    float *out;            // the block values
    uint32_t n;
    uint32_t flags;
    uint32_t first_sample, n_samples;
    uint32_t seed_lo, seed_hi;
    uint32_t lds_units;
    float bound;
    uint32_t nblocks;      // blocks per probe: ceil(n_samples / 64)
    float r_max;
};

extern "C++" {
namespace hrtk {

__device__ __forceinline__ void pd_wave_sync() {  // between the two roles of a wave: see the head of the file
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool EXACT>
__device__ __forceinline__ void probe_depth_body(const DProbeDepth &Q) {
    __shared__ float4 s_slot[HRT_RAYS_WG];  // {d, r} of the wave's 64 samples
    CtxT<EXACT, false, false, true> cx;
    unsigned long long stamps_local[17] = {0};
    query_context(cx, Q.scene, Q.lds_units, Q.flags, stamps_local);
    const float far = query_far(Q.bound);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t items = Q.n >> 6, stride = gridDim.x * (HRT_RAYS_WG / 64u);
    float4 *slot = s_slot + 64u * wave;
    float c[3];
    probedepth::direction(lane, c);
    for (uint32_t item = blockIdx.x * (HRT_RAYS_WG / 64u) + wave; item < items; item += stride) {  // the same item for a whole wave
        const uint32_t probe = item / Q.nblocks, block = item - probe * Q.nblocks;
        const uint32_t key = Q.keys ? Q.keys[probe] : probe;
        const uint32_t count = min(HRT_PD_BLOCK, Q.n_samples - block * HRT_PD_BLOCK);  // >= 1
        // a lane is a sample
        Ray ray;
        ray.o = ray.d = mk(0.f, 0.f, 0.f);  // a lane past the block's end holds a slot nobody reads
        ray.time = 0.f;
        const float4 a = ld((gf4)Q.probes, probe);
        const bool ok = lane < count && probe_sample(a, Q.seed_lo, Q.seed_hi, key, Q.first_sample + block * HRT_PD_BLOCK + lane, ray);
        float r = Q.r_max;
        if (ok) {
            query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, cx.flags);
            const Hit h = closest_hit(cx, ray);
            if (h.kind && h.t < __builtin_inff()) r = fminf(h.t, Q.r_max);  // the record's tmax is +inf: hrt_trace_rays' own test
        }
        const uint64_t live = __ballot(ok);
        slot[lane] = make_float4(ray.d.x, ray.d.y, ray.d.z, r);
        pd_wave_sync();
        // a lane is a texel
        float W = 0.f, A = 0.f, B = 0.f;
        for (uint32_t j = 0; j < count; ++j) {
            if (!((live >> j) & 1ull)) continue;  // a degenerate sample adds nothing
            const float4 s = slot[j];
            float w = fmaxf(0.f, (c[0] * s.x + c[1] * s.y) + c[2] * s.z);
            w = w * w; w = w * w; w = w * w; w = w * w; w = w * w;
            W = W + w;
            A = A + w * s.w;
            B = B + w * (s.w * s.w);
        }
        float *o = Q.out + (size_t)item * HRT_PROBE_DEPTH_FLOATS + 3u * lane;
        o[0] = W; o[1] = A; o[2] = B;
        pd_wave_sync();  // the slots are free for the wave's next item
    }
}

}  // namespace hrtk
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_probe_depth_kernel(const DProbeDepth Q) { probe_depth_body<false>(Q); }
// HRT_FLAG_EXACT_ONLY: the proof build (no filters, no v_rcp_f32; see CtxT)
extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_probe_depth_exact_kernel(const DProbeDepth Q) { probe_depth_body<true>(Q); }

// One lane per (probe, texel, sum): the block values in ascending order, then the sums or the running sums.
extern "C" __global__ void __launch_bounds__(256) hrt_probe_depth_fold_kernel(const float *__restrict__ blocks, uint32_t n_sums, uint32_t nblocks,
                                                                              uint32_t accumulate, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // n_sums <= 2^20 * 192
    if (i >= n_sums) return;
    const uint32_t probe = i / HRT_PROBE_DEPTH_FLOATS, k = i - probe * HRT_PROBE_DEPTH_FLOATS;
    const float *b = blocks + (size_t)probe * nblocks * HRT_PROBE_DEPTH_FLOATS + k;
    float t = 0.f;
    for (uint32_t j = 0; j < nblocks; ++j) t = t + b[(size_t)j * HRT_PROBE_DEPTH_FLOATS];
    out[i] = accumulate ? out[i] + t : t;
}

// The flags of a depth launch: a probe launch's without the frame's; every other bit is refused by name.
static int probe_depth_flags_check(const std::string &who, uint32_t flags) {
    return fused_flags_check(who, flags, "a depth launch has one kernel form", "a probe has no direction to normalise",
                             "depth is a distance, not a frame");
}

// Checks 4..6 of the header's order: the counts and the limit, r_max, the output.
static int probe_depth_counts_out_check(const std::string &who, uint32_t n, uint32_t first_sample, uint32_t n_samples, float r_max, const float *out,
                                        const char *out_name) {
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    const uint64_t items = (uint64_t)n * (((uint64_t)n_samples + HRT_PD_BLOCK - 1u) / HRT_PD_BLOCK);
    if (items > HRT_PROBE_DEPTH_MAX_BLOCKS)
        return fail(HRT_ERR_INVALID, who + ": n * ceil(n_samples / 64) must be at most HRT_PROBE_DEPTH_MAX_BLOCKS = " +
                                         std::to_string(HRT_PROBE_DEPTH_MAX_BLOCKS) + " (got " + std::to_string(items) + ")");
    if (!(std::isfinite(r_max) && r_max > 0.f)) return fail(HRT_ERR_INVALID, who + ": r_max must be finite and positive (got " + std::to_string(r_max) + ")");
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is not 4-byte aligned");
    return HRT_OK;
}

// The launch into d_out on `stream` (the scene entered, the limit checked): the trace launch into the scene's block values, then
// the fold, also when a probe has one block.
static int probe_depth_launch(hrt_scene *s, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample, uint32_t n_samples,
                              uint64_t seed, float r_max, uint32_t flags, float *d_out, hipStream_t stream) {
    const uint32_t nblocks = (uint32_t)(((uint64_t)n_samples + HRT_PD_BLOCK - 1u) / HRT_PD_BLOCK);
    const uint32_t items = n * nblocks;  // <= HRT_PROBE_DEPTH_MAX_BLOCKS
    if (const int rc = s->pd_blocks.grow((size_t)items * HRT_PROBE_DEPTH_FLOATS * sizeof(float))) return rc;
    DProbeDepth Q;
    Q.probes = (const float4 *)d_probes;
    Q.keys = d_keys;
    Q.out = s->pd_blocks.as<float>();
    Q.n = items * 64u;  // <= 2^26
    Q.flags = flags;
    Q.first_sample = first_sample;
    Q.n_samples = n_samples;
    Q.seed_lo = (uint32_t)seed;
    Q.seed_hi = (uint32_t)(seed >> 32);
    Q.nblocks = nblocks;
    Q.r_max = r_max;
    if (const int rc = query_launch((flags & HRT_FLAG_EXACT_ONLY) ? hrt_probe_depth_exact_kernel : hrt_probe_depth_kernel, Q, s, false, HRT_RAYS_WG, stream))
        return rc;
    const uint32_t n_sums = n * HRT_PROBE_DEPTH_FLOATS;
    hipLaunchKernelGGL(hrt_probe_depth_fold_kernel, dim3((n_sums + 255u) / 256u), dim3(256), 0, stream, s->pd_blocks.as<float>(), n_sums, nblocks,
                       (flags & HRT_RADIANCE_ACCUMULATE) ? 1u : 0u, d_out);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// Both forms, checked in the header's order; the blocking one runs the launch on device copies of the probes and keys.
static int probe_depth_entry(const std::string &who, bool dev, hrt_scene *s, const float *probes, const uint32_t *keys, uint32_t n,
                             uint32_t first_sample, uint32_t n_samples, uint64_t seed, float r_max, uint32_t flags, float *out, void *stream,
                             hrt_stats *stats) {
    int rc = dev ? HRT_OK : blocking_accumulate_check(who, flags);
    if (rc == HRT_OK) rc = probe_depth_flags_check(who, flags);
    if (rc != HRT_OK) return rc;
    if (n == 0u) return empty_batch(stats);
    if ((rc = probe_records_check(who, probes, keys, n, dev)) != HRT_OK) return rc;
    if ((rc = probe_depth_counts_out_check(who, n, first_sample, n_samples, r_max, out, dev ? "d_out" : "out")) != HRT_OK) return rc;
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    const auto launch = [&](const float *d_probes, const uint32_t *d_keys, float *d_out, hipStream_t st) {
        return probe_depth_launch(s, d_probes, d_keys, n, first_sample, n_samples, seed, r_max, flags, d_out, st);
    };
    if (dev) return launch(probes, keys, out, (hipStream_t)stream);
    BlockingCall call;
    return call.run_batch(s, probes, HRT_PROBE_FLOATS * sizeof(float), keys, n, (size_t)n * HRT_PROBE_DEPTH_FLOATS * sizeof(float), out,
                          (uint64_t)n * n_samples, stats, launch);
}

int hrt_probe_depth_device(hrt_scene *s, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample, uint32_t n_samples,
                           uint64_t seed, float r_max, uint32_t flags, float *d_out, void *stream) {
    return probe_depth_entry("hrt_probe_depth_device", true, s, d_probes, d_keys, n, first_sample, n_samples, seed, r_max, flags, d_out, stream, nullptr);
}

// Blocking, from and into host memory.
int hrt_probe_depth(hrt_scene *s, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed, float r_max, uint32_t flags,
                    float *out, hrt_stats *stats) {
    return probe_depth_entry("hrt_probe_depth", false, s, probes, keys, n, 0u, spp, seed, r_max, flags, out, nullptr, stats);
}

int hrt_probe_depth_texel(const float v[3], uint32_t *texel) {
    const std::string who = "hrt_probe_depth_texel";
    if (!v) return fail(HRT_ERR_INVALID, who + ": v is NULL");
    if (!texel) return fail(HRT_ERR_INVALID, who + ": texel is NULL");
    *texel = probedepth::texel(v);
    return HRT_OK;
}

int hrt_probe_depth_direction(uint32_t texel, float out[3]) {
    const std::string who = "hrt_probe_depth_direction";
    if (texel >= HRT_PROBE_DEPTH_TEXELS)
        return fail(HRT_ERR_INVALID, who + ": texel must be below HRT_PROBE_DEPTH_TEXELS = " + std::to_string(HRT_PROBE_DEPTH_TEXELS) + " (got " + std::to_string(texel) + ")");
    if (!out) return fail(HRT_ERR_INVALID, who + ": out is NULL");
    probedepth::direction(texel, out);
    return HRT_OK;
}
