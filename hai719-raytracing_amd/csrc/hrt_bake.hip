// Baking (include/hrt.h "Baking": hrt_bake_rays, hrt_bake_device, hrt_bake and the two host point generators): the radiance
// arriving at caller-supplied surface points, cosine-weighted about their normals, through the unchanged integrator.  Included by
// hrt_api.hip inside its extern "C" block, after hrt_lens.hip (radiance_body, the query helpers, lens_traced).
//
// bake_sample is the one implementation of THE RULE of include/hrt.h: the ray of sample `sample` of a point record.  Two kernels
// call it: hrt_bake_rays_kernel writes the rays as records (the sibling of hrt_camera_rays_kernel and hrt_lens_rays_kernel); the
// hrt_bake_kernel builds are radiance_body with the BakeRays source -- lane i is point i, and at the start of every sample the
// point record is read again (two coalesced 16-byte loads, as RecordRays re-reads its ray) and the ray made in registers, so a bake
// needs no n * 32-byte ray buffer and one launch instead of two per sample.  Nothing of the point lives past sample(): a bake
// source holds no state of its own across a path.  No call here touches the per-launch state of a scene.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

// The launch record of the hrt_bake_kernel builds: DRadiance with the point records in place of the rays (radiance_launch,
// query_launch and radiance_body reach the fields they share by name).
struct DBake {
    const DScene *scene;
    const float4 *points;  // 2 float4 per point: {P, time} {N, bias}
    const uint32_t *keys;  // RNG key of point i (NULL: i)
    float *out;            // 3 floats per point
    uint32_t n;
    uint32_t flags;
    uint32_t first_sample, n_samples;
    uint32_t seed_lo, seed_hi;
    uint32_t lds_units;
    float bound;
};

extern "C++" {
namespace hrtk {

// THE RULE for the point record {a, b} = {P, time} {N, bias}, key and sample; false for a degenerate sample, whose ray is
// {P, 0, time}.  Straight-line code but for the early return of a degenerate point, which draws nothing.
__device__ __forceinline__ bool bake_sample(const float4 &a, const float4 &b, uint32_t seed_lo, uint32_t seed_hi, uint32_t key, uint32_t sample,
                                            Ray &ray) {
    const f3 P = mk(a.x, a.y, a.z), N = mk(b.x, b.y, b.z);
    const float bias = b.w;
    ray.o = P;
    ray.d = mk(0.f, 0.f, 0.f);
    ray.time = a.w;
    if (!(rays_finite(a.x) && rays_finite(a.y) && rays_finite(a.z) && rays_finite(a.w) && rays_finite(b.x) && rays_finite(b.y) &&
          rays_finite(b.z) && rays_finite(b.w)) || bias < 0.f || (N.x == 0.f && N.y == 0.f && N.z == 0.f))
        return false;
    const f3 Nn = normalize(N);
    if (!(rays_finite(Nn.x) && rays_finite(Nn.y) && rays_finite(Nn.z)) || (Nn.x == 0.f && Nn.y == 0.f && Nn.z == 0.f)) return false;
    Rng rng;
    rng.start(seed_lo, seed_hi, key, sample);
    const float b0 = rng.next(), b1 = rng.next();  // draws 0 and 1: the camera's u, v slots; a radiance path starts at draw 3
    const float r = sqrtf(b0), phi = 6.2831855f * b1;
    const float x = r * cosf(phi), y = r * sinf(phi), z = sqrtf(1.f - b0);  // cosine-weighted about +z
    const float sg = copysignf(1.f, Nn.z), fa = -1.f / (sg + Nn.z), fb = (Nn.x * Nn.y) * fa;  // branch-free frame, no pole
    const f3 T = mk(1.f + (sg * (Nn.x * Nn.x)) * fa, sg * fb, (-sg) * Nn.x);
    const f3 B = mk(fb, sg + (Nn.y * Nn.y) * fa, -Nn.y);
    const f3 d = normalize((x * T + y * B) + z * Nn);
    const f3 O = P + bias * Nn;
    if (!(rays_finite(O.x) && rays_finite(O.y) && rays_finite(O.z) && rays_finite(d.x) && rays_finite(d.y) && rays_finite(d.z)) ||
        (d.x == 0.f && d.y == 0.f && d.z == 0.f))
        return false;
    ray.o = O;
    ray.d = d;
    return true;
}

// radiance_body's source for bake points: item i is point i, keyed by Q.keys with the launch's seed.  The record is read where it
// is used, by the lane that uses it.
struct BakeRays {
    static constexpr bool per_sample = true;
    __device__ static __forceinline__ uint32_t key(const DBake &Q, uint32_t i) { return Q.keys ? Q.keys[i] : i; }
    __device__ static __forceinline__ void seed(const DBake &Q, uint32_t, uint32_t &lo, uint32_t &hi) { lo = Q.seed_lo; hi = Q.seed_hi; }
    __device__ static __forceinline__ bool sample(const DBake &Q, uint32_t i, uint32_t sample, Ray &ray) {
        const gf4 pts = (gf4)Q.points;
        const float4 a = ld(pts, 2u * i), b = ld(pts, 2u * i + 1u);
        return bake_sample(a, b, Q.seed_lo, Q.seed_hi, key(Q, i), sample, ray) && lens_traced(ray);
    }
};

}  // namespace hrtk
}  // extern "C++"

// hrt_bake_rays: the ray of sample `sample` of every point as a {O, time} {d, +inf} record; a degenerate sample is {P, time} {0, +inf}.
extern "C" __global__ void __launch_bounds__(256) hrt_bake_rays_kernel(const float4 *__restrict__ points, const uint32_t *__restrict__ keys,
                                                                       uint32_t n, uint32_t sample, uint32_t seed_lo, uint32_t seed_hi,
                                                                       float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = points[2u * i], b = points[2u * i + 1u];
    Ray r;
    if (!bake_sample(a, b, seed_lo, seed_hi, keys ? keys[i] : i, sample, r)) {
        r.o = mk(a.x, a.y, a.z);
        r.d = mk(0.f, 0.f, 0.f);
    }
    out[2u * i] = make_float4(r.o.x, r.o.y, r.o.z, a.w);
    out[2u * i + 1u] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_inff());
}

// The fused bake: radiance_body over points.
HRT_RADIANCE_FAMILY(hrt_bake_kernel, BakeRays, DBake)

// The flags of a bake.
static int bake_flags_check(const std::string &who, uint32_t flags) {
    return fused_flags_check(who, flags, "a bake has one kernel form", "the normal of a bake point is always normalised",
                             "a bake is linear radiance, not a frame");
}

// Checks 3..5 of the header's order: the point records, the keys, the count.  `dev`: device pointers (d_ names, 16-byte records).
static int bake_points_check(const std::string &who, const void *points, const void *keys, uint32_t n, bool dev) {
    const std::string pn = dev ? "d_points" : "points", kn = dev ? "d_keys" : "keys";
    const uintptr_t align = dev ? 16u : 4u;
    if (!points) return fail(HRT_ERR_INVALID, who + ": " + pn + " is NULL");
    if ((uintptr_t)points % align) return fail(HRT_ERR_INVALID, who + ": " + pn + " is not " + std::to_string(align) + "-byte aligned");
    if ((uintptr_t)keys % 4u) return fail(HRT_ERR_INVALID, who + ": " + kn + " is not 4-byte aligned");
    if (n > 0x7fffffffu) return fail(HRT_ERR_INVALID, who + ": n must be at most 2^31 - 1 (got " + std::to_string(n) + ")");
    return HRT_OK;
}

int hrt_bake_rays(const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t sample, uint64_t seed, float *d_rays, void *stream) {
    const std::string who = "hrt_bake_rays";
    if (n == 0u) return HRT_OK;
    { const int prc = bake_points_check(who, d_points, d_keys, n, true); if (prc != HRT_OK) return prc; }
    { const int rrc = rays_out_check(who, d_rays); if (rrc != HRT_OK) return rrc; }
    hipLaunchKernelGGL(hrt_bake_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, (const float4 *)d_points, d_keys, n, sample,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (float4 *)d_rays);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// The fused launch into d_out on `stream` (the scene entered).  Q and its builds: DBake and hrt_bake_kernel_builds, or the record
// and a table of a lit bake (hrt_bake_lit.hip) with the rule filled in.
extern "C++" {
template <class QT>
static int bake_launch(void (*const *builds)(const QT), QT &Q, hrt_scene *s, const float *d_points, const uint32_t *d_keys, uint32_t n,
                       uint32_t first_sample, uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_out, hipStream_t stream) {
    Q.points = (const float4 *)d_points;
    Q.keys = d_keys;
    return radiance_launch(builds, Q, s, first_sample, n_samples, seed, flags, d_out, n, stream);
}

// Both forms of a bake, plain (NoRule) or lit (LitRule), checked in the header's order: the flags, (an empty batch,) the points,
// the samples and the output, the rule's, then the scene.  launch(d_points, d_keys, d_out, stream) is the fused launch; the blocking
// form runs it on device copies of the points and keys (BlockingCall::run_batch).
template <class Rule, class Launch>
static int bake_call(const std::string &who, bool dev, hrt_scene *s, const Rule &R, const float *points, const uint32_t *keys, uint32_t n,
                     uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *out, void *stream, hrt_stats *stats, Launch launch) {
    int rc = dev ? HRT_OK : blocking_accumulate_check(who, flags);
    if (rc == HRT_OK) rc = bake_flags_check(who, flags);
    if (rc != HRT_OK) return rc;
    if (n == 0u) return empty_batch(stats);
    if ((rc = bake_points_check(who, points, keys, n, dev)) != HRT_OK) return rc;
    if ((rc = samples_out_check(who, first_sample, n_samples, out, dev ? "d_out" : "out")) != HRT_OK) return rc;
    if ((rc = R.check(who)) != HRT_OK) return rc;
    if ((rc = R.enter(who, s)) != HRT_OK) return rc;
    if (dev) return launch(points, keys, out, (hipStream_t)stream);
    BlockingCall call;
    return call.run_batch(s, points, HRT_RAY_FLOATS * sizeof(float), keys, n, (size_t)n * 3u * sizeof(float), out, (uint64_t)n * n_samples, stats, launch);
}
}  // extern "C++"

static int bake_entry(const std::string &who, bool dev, hrt_scene *s, const float *points, const uint32_t *keys, uint32_t n, uint32_t first_sample,
                      uint32_t n_samples, uint64_t seed, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return bake_call(who, dev, s, NoRule{}, points, keys, n, first_sample, n_samples, flags, out, stream, stats,
                     [&](const float *d_points, const uint32_t *d_keys, float *d_out, hipStream_t st) {
                         DBake Q;
                         return bake_launch(hrt_bake_kernel_builds, Q, s, d_points, d_keys, n, first_sample, n_samples, seed, flags, d_out, st);
                     });
}

int hrt_bake_device(hrt_scene *s, const float *d_points, const uint32_t *d_keys, uint32_t n, uint32_t first_sample, uint32_t n_samples,
                    uint64_t seed, uint32_t flags, float *d_out, void *stream) {
    return bake_entry("hrt_bake_device", true, s, d_points, d_keys, n, first_sample, n_samples, seed, flags, d_out, stream, nullptr);
}

// Blocking, from and into host memory.
int hrt_bake(hrt_scene *s, const float *points, const uint32_t *keys, uint32_t n, uint32_t spp, uint64_t seed, uint32_t flags, float *out,
             hrt_stats *stats) {
    return bake_entry("hrt_bake", false, s, points, keys, n, 0u, spp, seed, flags, out, nullptr, stats);
}

int hrt_bake_quad_points(const hrt_quad *quad, uint32_t tw, uint32_t th, int32_t side, float time, float bias, float *out_points) {
    std::string error;
    const int rc = bakepts::quad_points(quad, tw, th, side, time, bias, out_points, error);
    return rc == HRT_OK ? rc : fail(rc, error);
}

int hrt_bake_mesh_points(const float *positions, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, float time, float bias,
                         float *out_points) {
    std::string error;
    const int rc = bakepts::mesh_points(positions, n_vertices, indices, n_triangles, time, bias, out_points, error);
    return rc == HRT_OK ? rc : fail(rc, error);
}
