// Light probes (include/hrt.h "Light probes": hrt_probe_rays, hrt_probes_device, hrt_probes and the host grid generator): the
// radiance arriving at caller-supplied points from every direction, projected onto 9 spherical-harmonic coefficients per colour
// channel, through the unchanged integrator.  Included by hrt_api.hip inside its extern "C" block, after hrt_bake.hip.
//
// probe_dir / probe_sample are the one implementation of the direction rule of include/hrt.h.  Two kernels call them:
// hrt_probe_rays_kernel writes the rays as records (the sibling of hrt_bake_rays_kernel); the hrt_probe_kernel builds are
// radiance_body with the ProbeRays source.  A probe batch is few items with many samples each, the opposite of every other
// family, so here one WAVE is one work item -- a (probe, block) pair of up to HRT_PROBE_BLOCK samples -- and the wave's lane is the
// rule's lane: lane l traces samples l, l + 64, ... of the block and adds each, times the nine basis values of its direction, to
// its own 27 partial sums.  When no lane has a sample left the wave folds the 64 partials by halving and lane 0 stores the block
// value; hrt_probe_fold_kernel then adds a probe's block values in ascending order.  The order of every addition is the header's
// and does not depend on how the device schedules the waves.
//
// The 27 partial sums of a lane live in LDS (coefficient-major, so that the 64 lanes of a wave touch 64 consecutive words), not
// in registers: the radiance kernels already sit at the register cap of HRT_RADIANCE_MIN_WAVES waves per SIMD.  A finished sample
// makes its direction again from the counter-based generator instead of holding it across the path.  No call here touches the
// per-launch state of a scene; the block values are a scratch buffer of the scene's own.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

static_assert(HRT_PROBE_BLOCK % 64u == 0u && HRT_PROBE_BLOCK >= 64u, "HRT_PROBE_BLOCK is a whole number of waves");
#define HRT_PROBE_SUMS (3u * HRT_PROBE_COEFFS)  // floats per probe, per block value and per lane: 9 coefficients x 3 channels

// The launch record of the hrt_probe_kernel builds: DRadiance with the probe records in place of the rays (radiance_launch,
// query_launch and radiance_body reach the fields they share by name).  n counts LANES, 64 per (probe, block) item; out is the
// block values, HRT_PROBE_SUMS floats per item.
struct DProbe {
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
    uint32_t nblocks;      // blocks per probe: ceil(n_samples / HRT_PROBE_BLOCK)
};

extern "C++" {
namespace hrtk {

// The direction of sample `sample` of the probe with key `key`: uniform on the sphere.
__device__ __forceinline__ f3 probe_dir(uint32_t seed_lo, uint32_t seed_hi, uint32_t key, uint32_t sample) {
    Rng rng;
    rng.start(seed_lo, seed_hi, key, sample);
    const float b0 = rng.next(), b1 = rng.next();  // draws 0 and 1: the slots a bake uses; a radiance path starts at draw 3
    const float z = 1.f - 2.f * b0, r = sqrtf(fmaxf(0.f, 1.f - z * z)), phi = 6.2831855f * b1;
    return normalize(mk(r * cosf(phi), r * sinf(phi), z));
}

// THE RULE for the probe record a = {P, time}, key and sample; false for a degenerate sample, whose ray is {P, 0, time}.
__device__ __forceinline__ bool probe_sample(const float4 &a, uint32_t seed_lo, uint32_t seed_hi, uint32_t key, uint32_t sample, Ray &ray) {
    ray.o = mk(a.x, a.y, a.z);
    ray.d = mk(0.f, 0.f, 0.f);
    ray.time = a.w;
    if (!(rays_finite(a.x) && rays_finite(a.y) && rays_finite(a.z) && rays_finite(a.w))) return false;
    const f3 d = probe_dir(seed_lo, seed_hi, key, sample);
    if (!(rays_finite(d.x) && rays_finite(d.y) && rays_finite(d.z)) || (d.x == 0.f && d.y == 0.f && d.z == 0.f)) return false;
    ray.d = d;
    return true;
}

// radiance_body's source for probes, with wave_items: lane i works for item i / 64 = probe * nblocks + block, as lane i % 64 of
// the rule.  What the item's lanes share -- probe, block, key -- is worked out once per item (begin) and kept in four words of LDS
// per wave; the lane's sink is column threadIdx.x of s_sink.
struct ProbeRays {
    static constexpr bool per_sample = true;
    static constexpr bool wave_items = true;
    struct Shared {
        float sink[HRT_PROBE_SUMS][HRT_RADIANCE_WG];
        uint32_t item[HRT_RADIANCE_WG / 64u][4];  // probe, block, key, samples in the block
    };
    __device__ static __forceinline__ Shared &shared() {
        __shared__ Shared s_probe;
        return s_probe;
    }
    __device__ static __forceinline__ const uint32_t *item(uint32_t) { return shared().item[threadIdx.x >> 6]; }

    __device__ static __forceinline__ void begin(const DProbe &Q, uint32_t i) {
        Shared &sh = shared();
        const uint32_t it = i >> 6, probe = it / Q.nblocks, block = it - probe * Q.nblocks;
        uint32_t *w = sh.item[threadIdx.x >> 6];  // every lane of the wave writes the same four words
        w[0] = probe;
        w[1] = block;
        w[2] = Q.keys ? Q.keys[probe] : probe;
        w[3] = min((uint32_t)HRT_PROBE_BLOCK, Q.n_samples - block * HRT_PROBE_BLOCK);
        for (uint32_t k = 0; k < HRT_PROBE_SUMS; ++k) sh.sink[k][threadIdx.x] = 0.f;
    }
    __device__ static __forceinline__ uint32_t key(const DProbe &, uint32_t i) { return item(i)[2]; }
    __device__ static __forceinline__ void seed(const DProbe &Q, uint32_t, uint32_t &lo, uint32_t &hi) { lo = Q.seed_lo; hi = Q.seed_hi; }
    // lane l has the block's samples l, l + 64, ..., as indices from first_sample: from first() in steps of 64 below end()
    __device__ static __forceinline__ uint32_t first(const DProbe &, uint32_t i) { return item(i)[1] * HRT_PROBE_BLOCK + (i & 63u); }
    __device__ static __forceinline__ uint32_t end(const DProbe &, uint32_t i) { return item(i)[1] * HRT_PROBE_BLOCK + item(i)[3]; }
    __device__ static __forceinline__ bool sample(const DProbe &Q, uint32_t i, uint32_t sample, Ray &ray) {
        const uint32_t *w = item(i);
        const float4 a = ld((gf4)Q.probes, w[0]);
        return probe_sample(a, Q.seed_lo, Q.seed_hi, w[2], sample, ray);  // every float of the ray is finite and d != 0: lens_traced's checks
    }
    // A finished sample: v times the nine basis values of its direction onto the lane's partial sums, one multiply and one add
    // per term.
    __device__ static __forceinline__ void add(const DProbe &Q, uint32_t i, uint32_t sample, const f3 &v) {
        Shared &sh = shared();
        const f3 d = probe_dir(Q.seed_lo, Q.seed_hi, item(i)[2], sample);
        const float x = d.x, y = d.y, z = d.z;
        const float Y[HRT_PROBE_COEFFS] = {0.2820948f,
                                           0.48860251f * y, 0.48860251f * z, 0.48860251f * x,
                                           1.0925485f * (x * y), 1.0925485f * (y * z),
                                           0.31539157f * (3.f * (z * z) - 1.f),
                                           1.0925485f * (x * z), 0.54627422f * (x * x - y * y)};
        const float c[3] = {v.x, v.y, v.z};
#pragma unroll
        for (uint32_t k = 0; k < HRT_PROBE_COEFFS; ++k)
#pragma unroll
            for (uint32_t ch = 0; ch < 3u; ++ch) {
                float &a = sh.sink[3u * k + ch][threadIdx.x];
                a = a + Y[k] * c[ch];
            }
    }
    // The item boundary, all 64 lanes: the halving over the lane partials, then lane 0 stores the block value.
    __device__ static __forceinline__ void finish(const DProbe &Q, uint32_t i) {
        Shared &sh = shared();
        float *o = Q.out + (size_t)(i >> 6) * HRT_PROBE_SUMS;
#pragma unroll 1
        for (uint32_t k = 0; k < HRT_PROBE_SUMS; ++k) {
            float a = sh.sink[k][threadIdx.x];
#pragma unroll
            for (uint32_t m = 32u; m != 0u; m >>= 1) a = a + __shfl_down(a, m, 64);  // lanes >= m hold what nobody reads
            if ((i & 63u) == 0u) o[k] = a;
        }
    }
};

}  // namespace hrtk
}  // extern "C++"

// hrt_probe_rays: the ray of sample `sample` of every probe as a {P, time} {d, +inf} record; a degenerate sample is {P, time} {0, +inf}.
extern "C" __global__ void __launch_bounds__(256) hrt_probe_rays_kernel(const float4 *__restrict__ probes, const uint32_t *__restrict__ keys,
                                                                        uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi,
                                                                        float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = probes[i];
    Ray r;
    if (!probe_sample(a, seed_lo, seed_hi, keys ? keys[i] : i, sample, r)) r.d = mk(0.f, 0.f, 0.f);
    out[2u * i] = a;
    out[2u * i + 1u] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_inff());
}

// The fused probes: radiance_body over (probe, block) items, one wave each.
HRT_RADIANCE_FAMILY(hrt_probe_kernel, ProbeRays, DProbe)

// One lane per (probe, coefficient, channel): the block values in ascending order, then the mean or the running sum.
extern "C" __global__ void __launch_bounds__(256) hrt_probe_fold_kernel(const float *__restrict__ blocks, uint32_t n_sums, uint32_t nblocks,
                                                                        uint32_t n_samples, uint32_t accumulate, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sums) return;
    const uint32_t probe = i / HRT_PROBE_SUMS, kc = i - probe * HRT_PROBE_SUMS;
    const float *b = blocks + (size_t)probe * nblocks * HRT_PROBE_SUMS + kc;
    float t = 0.f;
    for (uint32_t k = 0; k < nblocks; ++k) t = t + b[(size_t)k * HRT_PROBE_SUMS];
    out[i] = accumulate ? out[i] + t : t / (float)n_samples;
}

// The flags of a probe launch; one_form: why the kernel-form flags are refused, which names the plain or the lit launch.
static int probe_flags_check(const std::string &who, uint32_t flags, const char *one_form) {
    return fused_flags_check(who, flags, one_form, "a probe has no direction to normalise", "probes are linear radiance, not a frame");
}

// Checks 3..5 of the header's order: the probe records, the keys, the count.  `dev`: device pointers (d_ names, 16-byte records).
static int probe_records_check(const std::string &who, const void *probes, const void *keys, uint32_t n, bool dev) {
    const std::string pn = dev ? "d_probes" : "probes", kn = dev ? "d_keys" : "keys";
    const uintptr_t align = dev ? 16u : 4u;
    if (!probes) return fail(HRT_ERR_INVALID, who + ": " + pn + " is NULL");
    if ((uintptr_t)probes % align) return fail(HRT_ERR_INVALID, who + ": " + pn + " is not " + std::to_string(align) + "-byte aligned");
    if ((uintptr_t)keys % 4u) return fail(HRT_ERR_INVALID, who + ": " + kn + " is not 4-byte aligned");
    if (n > 0x7fffffffu) return fail(HRT_ERR_INVALID, who + ": n must be at most 2^31 - 1 (got " + std::to_string(n) + ")");
    return HRT_OK;
}

// Checks 6..9: the samples, the limit on (probe, block) items, the output.
static int probe_samples_out_check(const std::string &who, uint32_t n, uint32_t first_sample, uint32_t n_samples, const float *out,
                                   const char *out_name) {
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    const uint64_t items = (uint64_t)n * (((uint64_t)n_samples + HRT_PROBE_BLOCK - 1u) / HRT_PROBE_BLOCK);
    if (items > HRT_PROBE_MAX_BLOCKS)
        return fail(HRT_ERR_INVALID, who + ": n * ceil(n_samples / HRT_PROBE_BLOCK) must be at most HRT_PROBE_MAX_BLOCKS = " +
                                         std::to_string(HRT_PROBE_MAX_BLOCKS) + " (got " + std::to_string(items) + ")");
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is not 4-byte aligned");
    return HRT_OK;
}

int hrt_probe_rays(const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, float *d_rays, void *stream) {
    const std::string who = "hrt_probe_rays";
    if (n == 0u) return HRT_OK;
    { const int prc = probe_records_check(who, d_probes, d_keys, n, true); if (prc != HRT_OK) return prc; }
    { const int rrc = rays_out_check(who, d_rays); if (rrc != HRT_OK) return rrc; }
    hipLaunchKernelGGL(hrt_probe_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, (const float4 *)d_probes, d_keys, n, sample,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (float4 *)d_rays);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// The fused launch into d_out on `stream` (the scene entered, the limit checked): the trace launch into `blocks`, a scratch buffer
// of the scene's that this family alone uses, then the fold, also when a probe has one block.  Q, its builds and its blocks: DProbe,
// hrt_probe_kernel_builds and pr_blocks, or those of a lit probe launch (hrt_lit_paths.hip) with the rule filled in and pl_blocks.
extern "C++" {
template <class QT>
static int probe_launch(void (*const *builds)(const QT), QT &Q, hrt_scene *s, Scratch &blocks, const float *d_probes, const uint32_t *d_keys,
                        uint32_t n, uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_out, hipStream_t stream) {
    const uint32_t nblocks = (uint32_t)(((uint64_t)n_samples + HRT_PROBE_BLOCK - 1u) / HRT_PROBE_BLOCK);
    const uint32_t items = n * nblocks;  // <= HRT_PROBE_MAX_BLOCKS
    if (const int rc = blocks.grow((size_t)items * HRT_PROBE_SUMS * sizeof(float))) return rc;
    Q.probes = (const float4 *)d_probes;
    Q.keys = d_keys;
    Q.nblocks = nblocks;
    if (const int rc = radiance_launch(builds, Q, s, first_sample, n_samples, seed, flags, blocks.as<float>(), items * 64u, stream)) return rc;
    const uint32_t n_sums = n * HRT_PROBE_SUMS;
    hipLaunchKernelGGL(hrt_probe_fold_kernel, dim3((n_sums + 255u) / 256u), dim3(256), 0, stream, blocks.as<float>(), n_sums, nblocks, n_samples,
                       (flags & HRT_RADIANCE_ACCUMULATE) ? 1u : 0u, d_out);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// Both forms of a probe launch, plain (NoRule) or lit (LitRule), checked in the header's
// order: the flags, the rule's, (an empty batch,) the records, the samples and the output, then the scene.
// launch(d_probes, d_keys, d_out, stream) is the fused launch; the blocking form runs it on device copies of the probes and keys.
template <class Rule, class Launch>
static int probe_call(const std::string &who, bool dev, hrt_scene *s, const Rule &R, const char *one_form, const float *probes,
                      const uint32_t *keys, uint32_t n, uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *out, void *stream,
                      hrt_stats *stats, Launch launch) {
    int rc = dev ? HRT_OK : blocking_accumulate_check(who, flags);
    if (rc == HRT_OK) rc = probe_flags_check(who, flags, one_form);
    if (rc == HRT_OK) rc = R.check(who);
    if (rc != HRT_OK) return rc;
    if (n == 0u) return empty_batch(stats);
    if ((rc = probe_records_check(who, probes, keys, n, dev)) != HRT_OK) return rc;
    if ((rc = probe_samples_out_check(who, n, first_sample, n_samples, out, dev ? "d_out" : "out")) != HRT_OK) return rc;
    if ((rc = R.enter(who, s)) != HRT_OK) return rc;
    if (dev) return launch(probes, keys, out, (hipStream_t)stream);
    BlockingCall call;
    return call.run_batch(s, probes, HRT_PROBE_FLOATS * sizeof(float), keys, n, (size_t)n * HRT_PROBE_SUMS * sizeof(float), out,
                          (uint64_t)n * n_samples, stats, launch);
}
}  // extern "C++"

static int probes_entry(const std::string &who, bool dev, hrt_scene *s, const float *probes, const uint32_t *keys, uint32_t n, uint32_t first_sample,
                        uint32_t n_samples, uint64_t seed, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return probe_call(who, dev, s, NoRule{}, "a probe launch has one kernel form", probes, keys, n, first_sample, n_samples, flags, out, stream, stats,
                      [&](const float *d_probes, const uint32_t *d_keys, float *d_out, hipStream_t st) {
                          DProbe Q;
                          return probe_launch(hrt_probe_kernel_builds, Q, s, s->pr_blocks, d_probes, d_keys, n, first_sample, n_samples, seed, flags, d_out, st);
                      });
}

int hrt_probes_device(hrt_scene *s, const float *d_probes, const uint32_t *d_keys, uint32_t n, uint32_t first_sample, uint32_t n_samples,
                      uint64_t seed, uint32_t flags, float *d_out, void *stream) {
    return probes_entry("hrt_probes_device", true, s, d_probes, d_keys, n, first_sample, n_samples, seed, flags, d_out, stream, nullptr);
}

// Blocking, from and into host memory.
int hrt_probes(hrt_scene *s, const float *probes, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed, uint32_t flags, float *out,
               hrt_stats *stats) {
    return probes_entry("hrt_probes", false, s, probes, keys, n, 0u, spp, seed, flags, out, nullptr, stats);
}

int hrt_probe_grid_points(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, float time, float *out_probes) {
    std::string error;
    const int rc = probepts::grid_points(lo, hi, nx, ny, nz, time, out_probes, error);
    return rc == HRT_OK ? rc : fail(rc, error);
}
