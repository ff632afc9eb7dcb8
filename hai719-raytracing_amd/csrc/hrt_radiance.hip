// Radiance queries on caller rays (include/hrt.h hrt_trace_radiance) and the camera rays of a frame (hrt_camera_rays).
// Included by hrt_api.hip inside its extern "C" block, after hrt_rays.hip (DRays' constants and rays_finite).
//
// hrt_radiance_kernel is trace_body (hrt_kernels.hip) with the camera taken out: one lane per ray, and per sample one path whose
// first segment is the caller's ray, then the same stages -- A (spheres, squares, mesh gates), B (mesh walks, deferred until
// HRT_MESH_BATCH lanes of the wave are parked or nobody else can move), C (shade, direct light, scatter, sky) -- with the same
// pruning and the same sum.  A lane that finishes the last sample of its ray stores it and takes its next ray by a grid stride
// at once, without waiting for the rest of the wave; work is assigned by lane index alone, so no scene state is touched (the
// call may overlap a render of the same scene).  The ray record is read again at the start of every sample (two 16-byte loads)
// instead of being kept in registers across the path.
//
// Filter margin and far origins as in rays_body (hrt_rays.hip, DESIGN.md section 5 "Ray queries"): err_abs = 2e-6 (bound + |o| + 1)
// for a unit direction, +inf otherwise, for the whole path (bounce origins lie within `bound`); a first segment from farther than
// HRT_RAYS_FAR (bound + 1) tests every triangle of a gated mesh (mesh_brute), bounce segments are walked.

#define HRT_RADIANCE_WG 256u
#ifndef HRT_RADIANCE_MIN_WAVES
#define HRT_RADIANCE_MIN_WAVES 5  // waves per SIMD the register allocator leaves room for; A/B on MI355X, 1080p x 16 samples, tree from
                                  // global memory: 4 -> 5 is +20 % on Cornell+mesh, +14 % on the pool, +15 % on random_spheres (DESIGN.md
                                  // section 5 "Radiance queries")
#endif

struct DRadiance {
    const DScene *scene;
    const float4 *rays;    // 2 float4 per ray: {o, time} {d, tmax}
    const uint32_t *keys;  // RNG key of ray i (NULL: i)
    float *out;            // 3 floats per ray
    uint32_t n;
    uint32_t flags;
    uint32_t first_sample, n_samples;
    uint32_t seed_lo, seed_hi;
    uint32_t lds_units;    // leading kd units each workgroup stages into LDS (0: every nodelet from global memory)
    float bound;           // hrt_scene::bound
};

extern "C++" {
namespace hrtk {

// The record of ray i as the first segment of a path: false if it is degenerate (include/hrt.h hrt_trace_radiance).
__device__ __forceinline__ bool radiance_ray(const DRadiance &Q, uint32_t i, Ray &ray) {
    const gf4 rays = (gf4)Q.rays;
    const float4 a = ld(rays, 2u * i), b = ld(rays, 2u * i + 1u);
    ray.o = mk(a.x, a.y, a.z);
    ray.time = a.w;
    ray.d = mk(b.x, b.y, b.z);
    bool ok = rays_finite(a.x) && rays_finite(a.y) && rays_finite(a.z) && rays_finite(a.w) && rays_finite(b.x) &&
              rays_finite(b.y) && rays_finite(b.z) && !(b.x == 0.f && b.y == 0.f && b.z == 0.f);
    if (ok && (Q.flags & HRT_RAYS_NORMALIZE)) {  // the Ray constructor (Line.h:13-16); a length that under- or overflows is degenerate
        ray.d = normalize(ray.d);
        ok = rays_finite(ray.d.x) && rays_finite(ray.d.y) && rays_finite(ray.d.z) && !(ray.d.x == 0.f && ray.d.y == 0.f && ray.d.z == 0.f);
    }
    return ok;
}

template <bool LIGHTS, bool EXACT>
__device__ __forceinline__ void radiance_body(const DRadiance &Q) {
    extern __shared__ uint4 s_units[];
    CtxT<EXACT, false, false, true> cx;
    cx.S = (cscene)Q.scene;
    cx.set_tables((gf4)cx.S->tabs, (gf1)c_u8_lut, cx.S);
    cx.lds = (lu4)s_units;
    cx.lds_n = Q.lds_units;
    cx.flags = Q.flags;
    cx.err_abs = 0.f;
    unsigned long long stamps_local[17] = {0};
    cx.st = stamps_local;
    {
        gu4 g_units = (gu4)cx.S->kd_units;
        for (uint32_t i = threadIdx.x; i < cx.lds_n; i += blockDim.x) s_units[i] = ld(g_units, i);
    }
    __syncthreads();
    const bool has_mesh = cx.S->n_meshes != 0u;
    const bool prune = !EXACT && cx.S->prune_ok != 0u;  // as trace_body
    const bool sky_is_zero = cx.S->skybox_image < 0 && cx.S->dark_sky != 0;
    const bool accumulate = (Q.flags & HRT_RADIANCE_ACCUMULATE) != 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const float far2 = HRT_RAYS_FAR * (Q.bound + 1.f);

    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // this lane's ray
    uint32_t key = 0;        // its RNG key
    uint32_t first_flags = Q.flags;  // cx.flags of its first segments (+ MESH_BRUTE for a far origin)
    f3 sum = mk(0.f, 0.f, 0.f);
    uint32_t s = 0;          // next sample of this lane's ray
    int remaining = 0;       // bounces left on the current path; 0 = needs a new path
    Ray ray;
    ray.o = mk(0.f, 0.f, 0.f); ray.d = mk(0.f, 0.f, 1.f); ray.time = 0.f;
    f3 thr = mk(1.f, 1.f, 1.f), rad = mk(0.f, 0.f, 0.f);
    Rng rng;
    rng.k0 = rng.k1 = rng.i = 0;
    Hit h;
    h.kind = 0; h.index = 0; h.t = HRT_FLT_MAX; h.tri = 0; h.a0 = 0.f; h.a1 = 0.f;
    uint32_t parked = 0;     // meshes whose box this lane's ray enters and that are still to be walked
    uint32_t stage = 0;      // 0: needs stage A   1: parked for stage B   2: ready for stage C   3: pruned
    bool live = false;

    // The lane's next ray from i on that is not degenerate: its key, margin, flags and starting sum.  A degenerate ray adds
    // nothing: 0 in mean mode, its sums left as they are under HRT_RADIANCE_ACCUMULATE.
    auto next_ray = [&]() {
        live = false;
        for (; i < Q.n; i += stride) {
            if (radiance_ray(Q, i, ray)) {
                live = true;
                break;
            }
            if (!accumulate) { float *o_ = Q.out + (size_t)i * 3u; o_[0] = 0.f; o_[1] = 0.f; o_[2] = 0.f; }
        }
        if (live) {
            key = Q.keys ? Q.keys[i] : i;
            const float olen = length(ray.o);
            cx.err_abs = fabsf(dot(ray.d, ray.d) - 1.f) <= 1e-5f ? 2e-6f * (Q.bound + olen + 1.f) : __builtin_inff();
            first_flags = olen > far2 ? (Q.flags | HRT_FLAG_MESH_BRUTE) : Q.flags;
            sum = mk(0.f, 0.f, 0.f);
            if (accumulate) { const float *a_ = Q.out + (size_t)i * 3u; sum = mk(a_[0], a_[1], a_[2]); }
            s = 0;
        }
    };

    next_ray();
    while (__ballot(live) != 0ull) {
        // ---- stage A: (re)start a path, spheres + squares, mesh gates
        if (live && stage == 0u) {
            if (remaining == 0) {  // sample first_sample + s of ray i: the caller's ray, RNG stream (seed, key, sample) from draw 3
                (void)radiance_ray(Q, i, ray);
                rng.start(Q.seed_lo, Q.seed_hi, key, Q.first_sample + s);
                rng.i = 3u;  // draws 0..2 are the camera's u, v, time
                cx.flags = first_flags;
                thr = mk(1.f, 1.f, 1.f);
                rad = mk(0.f, 0.f, 0.f);
                remaining = 6;  // MAXBOUNCES
            }
            h = prims_hit(cx, ray);
            parked = has_mesh ? mesh_gates(cx, ray) : 0u;
            stage = parked ? 1u : 2u;
            if (!LIGHTS && prune && remaining == 1) {  // the path's last segment: only an emitting closest hit can still reach the sample
                bool dead;
                if (h.kind == 0u) {
                    dead = sky_is_zero;
                } else {
                    const uint32_t mat = h.kind == 1u ? __float_as_uint(ld(cx.ts, HRT_SPHERE_ROWS * h.index + 1u).w)
                                                      : __float_as_uint(ld(cx.tq, HRT_QUAD_ROWS * h.index + 4u).w);
                    dead = __float_as_uint(ld(cx.tm, HRT_MAT_ROWS * mat + 1u).w) == 0u;
                }
                if (dead) { h.kind = 0u; parked = 0u; stage = 3u; }  // ends below with the radiance it has
            }
        }
        // ---- stage B: walk the meshes for the parked lanes once enough of them have gathered
        if (has_mesh) {
            const uint64_t waiting = __ballot(live && stage == 1u);
            const uint64_t ready = __ballot(live && stage >= 2u);
            if (waiting != 0ull && (__popcll(waiting) >= HRT_MESH_BATCH || ready == 0ull)) {
                if (live && stage == 1u) {
                    meshes_hit(cx, ray, parked, h);
                    stage = 2u;
                }
            }
        }
        // ---- stage C: shade, scatter, end of path; end of ray
        if (live && stage >= 2u) {
            bool ended;
            if (stage == 3u) {
                ended = true;  // pruned on its last segment (stage A): nothing is added
            } else if (h.kind == 0u) {
                rad = rad + thr * sky(cx, ray.d, remaining);
                ended = true;
            } else {
                const Surface sf = shade(cx, ray, h);
                f3 direct = mk(0.f, 0.f, 0.f);
                if (LIGHTS) direct = direct_light(cx, sf, ray, rng);
                rad = rad + thr * (direct + sf.emission);
                thr = thr * sf.albedo;
                scatter(sf, ray, rng);
                cx.flags = Q.flags;  // bounce segments are walked
                --remaining;
                ended = (remaining == 0) || (prune && thr.x == 0.f && thr.y == 0.f && thr.z == 0.f);
            }
            if (ended) {
                sum = sum + mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f);  // Scene.h:348
                remaining = 0;
                if (++s == Q.n_samples) {  // the ray is done: its mean (or running sum), then the lane's next ray
                    const float ns = accumulate ? 1.f : (float)Q.n_samples;  // x / 1.f is exact
                    float *o = Q.out + (size_t)i * 3u;
                    o[0] = sum.x / ns; o[1] = sum.y / ns; o[2] = sum.z / ns;
                    i += stride;
                    next_ray();
                }
            }
            stage = 0u;
        }
    }
}

}  // namespace hrtk
}  // extern "C++"

// hrt_camera_rays: the camera ray of sample `sample` of every pixel, as trace_body makes it (draws 0..2 of stream (seed, pixel,
// sample)), as a {o, time} {d, +inf} record.
extern "C" __global__ void __launch_bounds__(256) hrt_camera_rays_kernel(const DCamera C, uint32_t w, uint32_t h, uint32_t sample,
                                                                         uint32_t seed_lo, uint32_t seed_hi, float4 *__restrict__ out) {
    const uint32_t pixel = blockIdx.x * blockDim.x + threadIdx.x;
    if (pixel >= w * h) return;
    const uint32_t px = pixel % w, py = pixel / w;
    Rng rng;
    rng.start(seed_lo, seed_hi, pixel, sample);
    const float u = ((float)px + rng.next()) / (float)w;
    const float v = ((float)py + rng.next()) / (float)h;
    const float tm = rng.next();
    const Ray r = camera_ray<false>(&C, u, v, tm);
    out[2u * pixel] = make_float4(r.o.x, r.o.y, r.o.z, r.time);
    out[2u * pixel + 1u] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_inff());
}

extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, HRT_RADIANCE_MIN_WAVES) hrt_radiance_kernel(const DRadiance Q) { radiance_body<false, false>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, HRT_RADIANCE_MIN_WAVES) hrt_radiance_kernel_lights(const DRadiance Q) { radiance_body<true, false>(Q); }
// HRT_FLAG_EXACT_ONLY: the proof builds (no filters, no v_rcp_f32; see CtxT).  Not tuned: 2 waves per SIMD, as trace_body's
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) hrt_radiance_kernel_exact(const DRadiance Q) { radiance_body<false, true>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) hrt_radiance_kernel_lights_exact(const DRadiance Q) { radiance_body<true, true>(Q); }

int hrt_trace_radiance(hrt_scene *s, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample, uint32_t n_samples,
                       uint64_t seed, uint32_t flags, float *d_out, void *stream) {
    const std::string who = "hrt_trace_radiance";
    const uint32_t known = HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE | HRT_RAYS_NORMALIZE | HRT_RADIANCE_ACCUMULATE;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": unknown flags bits " + std::to_string(flags & ~known));
    if ((flags & HRT_FLAG_MESH_BRUTE) && !(flags & HRT_FLAG_EXACT_ONLY)) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY");
    if (n > 0u) {
        if (!d_rays) return fail(HRT_ERR_INVALID, who + ": d_rays is NULL");
        if ((uintptr_t)d_rays % 16u) return fail(HRT_ERR_INVALID, who + ": d_rays is not 16-byte aligned");
        if (d_keys && (uintptr_t)d_keys % 4u) return fail(HRT_ERR_INVALID, who + ": d_keys is not 4-byte aligned");
        if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
        if ((uintptr_t)d_out % 4u) return fail(HRT_ERR_INVALID, who + ": d_out is not 4-byte aligned");
    }
    if (n > 0x7fffffffu) return fail(HRT_ERR_INVALID, who + ": n must be at most 2^31 - 1 (got " + std::to_string(n) + ")");
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    if (n == 0u) return HRT_OK;
    { const int drc = use_device(s->device); if (drc != HRT_OK) return drc; }
    DRadiance Q;
    Q.scene = s->d_scene;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    Q.out = d_out;
    Q.n = n;
    Q.flags = flags;
    Q.first_sample = first_sample;
    Q.n_samples = n_samples;
    Q.seed_lo = (uint32_t)seed;
    Q.seed_hi = (uint32_t)(seed >> 32);
    // The tree prefix is NOT staged by default: measured on MI355X (DESIGN.md section 5 "Radiance queries"), its 36 KiB per workgroup
    // cost a fifth of the resident waves at 5 waves per SIMD and -12..-16 % on the mesh scenes.  HRT_RADIANCE_STAGE_TREE builds keep
    // the staged form for A/B runs (HRT_FLAG_NO_LDS_TREE turns it off there).  <= 64 KiB: no attribute to raise.
#ifdef HRT_RADIANCE_STAGE_TREE
    Q.lds_units = (flags & HRT_FLAG_NO_LDS_TREE) ? 0u : std::min<uint32_t>(s->lds_units, 4096u);
#else
    Q.lds_units = 0u;
#endif
    Q.bound = s->bound;
    const bool exact = (flags & HRT_FLAG_EXACT_ONLY) != 0u;
    const bool lights = s->d.n_lights != 0u;
    void (*const k)(const DRadiance) = exact ? (lights ? hrt_radiance_kernel_lights_exact : hrt_radiance_kernel_exact)
                                             : (lights ? hrt_radiance_kernel_lights : hrt_radiance_kernel);
    const size_t lds_bytes = (size_t)Q.lds_units * 16u;
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k, (int)HRT_RADIANCE_WG, lds_bytes));
    const uint64_t resident = (uint64_t)std::max(per_cu, 1) * (uint64_t)std::max(g_rt.cus, 1);
    const uint64_t needed = ((uint64_t)n + HRT_RADIANCE_WG - 1u) / HRT_RADIANCE_WG;
    const uint32_t grid = (uint32_t)std::min(resident, needed);
    hipLaunchKernelGGL(k, dim3(grid), dim3(HRT_RADIANCE_WG), lds_bytes, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

int hrt_camera_rays(const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, float *d_rays, void *stream) {
    const std::string who = "hrt_camera_rays";
    if (!cam) return fail(HRT_ERR_INVALID, who + ": cam is NULL");
    DCamera C;
    { const int crc = make_camera(cam, C); if (crc != HRT_OK) return crc; }  // refused as hrt_render refuses it
    if (!w || !h) return fail(HRT_ERR_INVALID, who + ": w and h must be positive");
    if ((uint64_t)w * h > 0x7fffffffull) return fail(HRT_ERR_INVALID, who + ": w * h must be at most 2^31 - 1");
    if (!d_rays) return fail(HRT_ERR_INVALID, who + ": d_rays is NULL");
    if ((uintptr_t)d_rays % 16u) return fail(HRT_ERR_INVALID, who + ": d_rays is not 16-byte aligned");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_camera_rays_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, C, w, h, sample,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (float4 *)d_rays);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}
