// Lens cameras (include/hrt.h hrt_lens_rays, hrt_render_lens*): thin-lens depth of field, orthographic, equirectangular and
// equidistant fisheye projections in front of the unchanged integrator.  Included by hrt_api.hip inside its extern "C" block, after
// hrt_radiance.hip (radiance_body and the query helpers) and hrt_denoise.hip (features_body).
//
// lens_sample is the one implementation of THE RULE of include/hrt.h: the ray of sample `sample` of pixel `pixel`.  Three kernels
// call it: hrt_lens_rays_kernel writes the rays as records (the sibling of hrt_camera_rays_kernel); the hrt_lens_kernel builds are
// radiance_body with the LensRays source -- lane i is pixel i, and at the start of every sample the ray is made in registers instead
// of being read from a record, so a frame needs no w*h*32-byte buffer and one launch instead of two per sample; and
// hrt_lens_features_kernel is features_body with the lens in place of the camera.  The lens travels as a kernel argument: no call
// here touches the per-launch state of a scene.
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

// hrt_lens -> what lens_sample reads.  R, U, F, E are the camera's vectors as the caller gave them; `cam` is camera_ray's block.
struct DLens {
    DCamera cam;
    float eye[3];
    uint32_t projection;  // HRT_LENS_*
    float right[3];
    float aperture;       // aperture_radius
    float up[3];
    float focus;          // focus_distance
    float forward[3];
    float extent;
    float aspect;
    uint32_t pad[3];
};

// The launch record of the hrt_lens_kernel builds: DRadiance with the lens and the frame in place of the ray and key arrays
// (query_launch and radiance_body read the fields they share by name).
struct DLensRadiance {
    const DScene *scene;
    float *out;            // 3 floats per pixel
    uint32_t n;            // w * h
    uint32_t flags;
    uint32_t first_sample, n_samples;
    uint32_t seed_lo, seed_hi;
    uint32_t lds_units;
    float bound;
    uint32_t w, h;
    DLens lens;
};

extern "C++" {
namespace hrtk {

// A ray the query layer traces (query_ray's rule without HRT_RAYS_NORMALIZE): every component finite, d != 0.
__device__ __forceinline__ bool lens_traced(const Ray &r) {
    return rays_finite(r.o.x) && rays_finite(r.o.y) && rays_finite(r.o.z) && rays_finite(r.time) && rays_finite(r.d.x) &&
           rays_finite(r.d.y) && rays_finite(r.d.z) && !(r.d.x == 0.f && r.d.y == 0.f && r.d.z == 0.f);
}

// THE RULE for film position (u, v), time and lens draws (l0, l1); false for a degenerate sample, whose ray is {E, 0, time}.
// The projection is the same for every lane: one branch on it, each arm straight-line code.
__device__ __forceinline__ bool lens_project(const DLens &L, float u, float v, float time, float l0, float l1, Ray &ray) {
    const f3 R = mk(L.right[0], L.right[1], L.right[2]), U = mk(L.up[0], L.up[1], L.up[2]), F = mk(L.forward[0], L.forward[1], L.forward[2]);
    const f3 E = mk(L.eye[0], L.eye[1], L.eye[2]);
    ray.o = E;
    ray.d = mk(0.f, 0.f, 0.f);
    ray.time = time;
    switch (L.projection) {
    case HRT_LENS_PERSPECTIVE: {
        const Ray r = camera_ray<false>(&L.cam, u, v, time);
        if (L.aperture == 0.f) {  // the pinhole: hrt_camera_rays' ray, untouched
            ray = r;
            return true;
        }
        const float rad = L.aperture * sqrtf(l0), phi = 6.2831855f * l1;
        const float a = rad * cosf(phi), b = rad * sinf(phi);
        const float c = dot(r.d, F);  // (d0 F0 + d1 F1) + d2 F2
        if (!(c > 0.f)) return false;
        const float tf = L.focus / c;
        const f3 P = r.o + tf * r.d;
        const f3 O = r.o + (a * R + b * U);
        ray.o = O;
        ray.d = normalize(P - O);
        return true;
    }
    case HRT_LENS_ORTHOGRAPHIC: {
        const float sx = (2.f * u - 1.f) * ((0.5f * L.extent) * L.aspect), sy = (1.f - 2.f * v) * (0.5f * L.extent);
        ray.o = E + (sx * R + sy * U);
        ray.d = normalize(F);
        return true;
    }
    case HRT_LENS_EQUIRECT: {
        const float phi = (2.f * u - 1.f) * 3.1415927f, th = (0.5f - v) * 3.1415927f;
        const float ct = cosf(th), st = sinf(th);
        ray.d = normalize(((ct * sinf(phi)) * R + st * U) + (ct * cosf(phi)) * F);
        return true;
    }
    default: {  // HRT_LENS_FISHEYE
        const float qx = (2.f * u - 1.f) * L.aspect, qy = 1.f - 2.f * v;
        const float rr = sqrtf(qx * qx + qy * qy);
        if (rr > 1.f) return false;
        const float th = rr * (L.extent * 0.5f * (3.1415927f / 180.f));
        if (rr == 0.f) {
            ray.d = normalize(F);
        } else {
            const float k = sinf(th) / rr;
            ray.d = normalize(((k * qx) * R + (k * qy) * U) + cosf(th) * F);
        }
        return true;
    }
    }
}

// Sample `sample` of pixel `pixel` of a w x h frame: u, v, time from draws 0..2 of stream (seed, pixel, sample) as camera_sample
// draws them, the thin lens' l0, l1 from draws HRT_LENS_DRAW and HRT_LENS_DRAW + 1 of the same stream (only a thin lens draws them).
__device__ __forceinline__ bool lens_sample(const DLens &L, uint32_t seed_lo, uint32_t seed_hi, uint32_t w, uint32_t h, uint32_t pixel,
                                            uint32_t sample, Ray &ray) {
    const uint32_t x = pixel % w, y = pixel / w;
    Rng rng;
    rng.start(seed_lo, seed_hi, pixel, sample);
    const float u = ((float)x + rng.next()) / (float)w;
    const float v = ((float)y + rng.next()) / (float)h;
    const float tm = rng.next();
    float l0 = 0.f, l1 = 0.f;
    if (L.projection == HRT_LENS_PERSPECTIVE && L.aperture != 0.f) {
        rng.i = HRT_LENS_DRAW;
        l0 = rng.next();
        l1 = rng.next();
    }
    return lens_project(L, u, v, tm, l0, l1, ray);
}

// radiance_body's source for a lens: the ray of (pixel, sample), traced if the rule makes one and the query layer accepts it.
struct LensRays {
    static constexpr bool per_sample = true;
    __device__ static __forceinline__ bool sample(const DLensRadiance &Q, uint32_t pixel, uint32_t sample, Ray &ray) {
        return lens_sample(Q.lens, Q.seed_lo, Q.seed_hi, Q.w, Q.h, pixel, sample, ray) && lens_traced(ray);
    }
};

// features_body's source for a lens.  A pinhole keeps the render's margin (R.err_abs, R.flags), so that its features are
// hrt_render_features' bit for bit; every other lens moves the origin or the direction per sample and takes the margin and the
// far-origin rule of that sample's ray, as hrt_trace_rays does for the same record.
struct LensFeatureRays {
    const DLens &L;
    float bound;  // hrt_scene::bound
    template <class CX>
    __device__ __forceinline__ bool operator()(CX &cx, const DRender &R, uint32_t n, uint32_t idx, uint32_t k, Ray &ray) const {
        bool ok;
        if (n == 0u) {
            const uint32_t x = idx % R.w, y = idx / R.w;
            ok = lens_project(L, ((float)x + 0.5f) / (float)R.w, ((float)y + 0.5f) / (float)R.h, 0.f, 0.f, 0.f, ray);
        } else {
            ok = lens_sample(L, R.seed_lo, R.seed_hi, R.w, R.h, idx, R.s0 + k, ray);
        }
        if (!(L.projection == HRT_LENS_PERSPECTIVE && L.aperture == 0.f)) {
            query_margin(ray, bound, query_far(bound), R.flags, cx.err_abs, cx.flags);
        }
        return ok && lens_traced(ray);
    }
};

}  // namespace hrtk
}  // extern "C++"

// hrt_lens_rays: the lens ray of sample `sample` of every pixel as a {o, time} {d, +inf} record; a degenerate sample is {E, time} {0, +inf}.
extern "C" __global__ void __launch_bounds__(256) hrt_lens_rays_kernel(const DLens L, uint32_t w, uint32_t h, uint32_t sample, uint32_t seed_lo,
                                                                       uint32_t seed_hi, float4 *__restrict__ out) {
    const uint32_t pixel = blockIdx.x * blockDim.x + threadIdx.x;
    if (pixel >= w * h) return;
    Ray r;
    if (!lens_sample(L, seed_lo, seed_hi, w, h, pixel, sample, r)) {
        r.o = mk(L.eye[0], L.eye[1], L.eye[2]);
        r.d = mk(0.f, 0.f, 0.f);
    }
    out[2u * pixel] = make_float4(r.o.x, r.o.y, r.o.z, r.time);
    out[2u * pixel + 1u] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_inff());
}

// The fused frame: radiance_body over pixels.  Launch bounds and shape are hrt_radiance_kernel's.
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, HRT_RADIANCE_MIN_WAVES) hrt_lens_kernel(const DLensRadiance Q) { radiance_body<false, false, LensRays>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, HRT_RADIANCE_MIN_WAVES) hrt_lens_kernel_lights(const DLensRadiance Q) { radiance_body<true, false, LensRays>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) hrt_lens_kernel_exact(const DLensRadiance Q) { radiance_body<false, true, LensRays>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RADIANCE_WG, 2) hrt_lens_kernel_lights_exact(const DLensRadiance Q) { radiance_body<true, true, LensRays>(Q); }

// hrt_render_lens_features: hrt_features_kernel with the lens as a kernel argument in place of the scene's camera block.
extern "C" __global__ void __launch_bounds__(256) hrt_lens_features_kernel(const DRender R, const DLens L, float bound, uint32_t n,
                                                                           float *__restrict__ out) {
    features_body<CtxT<false, false, false, true>>(R, n, out, LensFeatureRays{L, bound});
}

// The lens checks, in the header's order; fills L.  `who` names the entry point in every message but the camera's own.
static int lens_check(const std::string &who, const hrt_lens *lens, DLens &L) {
    if (!lens) return fail(HRT_ERR_INVALID, who + ": lens is NULL");
    std::memset(&L, 0, sizeof(L));
    { const int crc = make_camera(&lens->cam, L.cam); if (crc != HRT_OK) return crc; }  // refused as hrt_render refuses it
    const uint32_t p = lens->projection;
    if (p > HRT_LENS_FISHEYE)
        return fail(HRT_ERR_INVALID, who + ": projection must be HRT_LENS_PERSPECTIVE, _ORTHOGRAPHIC, _EQUIRECT or _FISHEYE (got " + std::to_string(p) + ")");
    const float a = lens->aperture_radius, f = lens->focus_distance, e = lens->extent;
    if (!std::isfinite(a) || a < 0.f) return fail(HRT_ERR_INVALID, who + ": aperture_radius must be finite and >= 0");
    if (a != 0.f && p != HRT_LENS_PERSPECTIVE) return fail(HRT_ERR_INVALID, who + ": aperture_radius must be 0 unless the projection is HRT_LENS_PERSPECTIVE");
    if (a > 0.f && (!std::isfinite(f) || !(f > 0.f))) return fail(HRT_ERR_INVALID, who + ": focus_distance must be finite and > 0 when aperture_radius > 0");
    if (p == HRT_LENS_ORTHOGRAPHIC) {
        if (!std::isfinite(e) || !(e > 0.f)) return fail(HRT_ERR_INVALID, who + ": extent must be finite and > 0 (HRT_LENS_ORTHOGRAPHIC: the height of the view volume)");
    } else if (p == HRT_LENS_FISHEYE) {
        if (!(e > 0.f && e <= 360.f)) return fail(HRT_ERR_INVALID, who + ": extent must be in (0, 360] (HRT_LENS_FISHEYE: the field of view in degrees)");
    } else if (!(e == 0.f)) {
        return fail(HRT_ERR_INVALID, who + ": extent must be 0 unless the projection is HRT_LENS_ORTHOGRAPHIC or HRT_LENS_FISHEYE");
    }
    for (int k = 0; k < 3; ++k) {
        L.eye[k] = lens->cam.eye[k]; L.right[k] = lens->cam.right[k]; L.up[k] = lens->cam.up[k]; L.forward[k] = lens->cam.forward[k];
    }
    L.projection = p;
    L.aperture = a;
    L.focus = a > 0.f ? f : 0.f;
    L.extent = e;
    L.aspect = lens->cam.aspect;
    return HRT_OK;
}

int hrt_lens_rays(const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, float *d_rays, void *stream) {
    const std::string who = "hrt_lens_rays";
    DLens L;
    { const int lrc = lens_check(who, lens, L); if (lrc != HRT_OK) return lrc; }
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    if (!d_rays) return fail(HRT_ERR_INVALID, who + ": d_rays is NULL");
    if ((uintptr_t)d_rays % 16u) return fail(HRT_ERR_INVALID, who + ": d_rays is not 16-byte aligned");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_lens_rays_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, L, w, h, sample, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (float4 *)d_rays);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// The checks hrt_render_lens_device and hrt_render_lens share, in the header's order (all before the scene); fills L.
static int lens_render_check(const std::string &who, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                             uint32_t flags, const float *out, const char *out_name, DLens &L) {
    static const struct { uint32_t bit; const char *name; } no_form[] = {
        {HRT_FLAG_WAVE_KERNEL, "HRT_FLAG_WAVE_KERNEL"}, {HRT_FLAG_STREAM_KERNEL, "HRT_FLAG_STREAM_KERNEL"}, {HRT_FLAG_DUAL_KERNEL, "HRT_FLAG_DUAL_KERNEL"}};
    for (const auto &f : no_form)
        if (flags & f.bit) return fail(HRT_ERR_INVALID, who + ": flags: " + f.name + ": a lens frame has one kernel form");
    if (flags & HRT_FLAG_NO_SHADOW_CULL) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_NO_SHADOW_CULL: the query kernels have no such build");
    if (flags & HRT_RAYS_NORMALIZE) return fail(HRT_ERR_INVALID, who + ": flags: HRT_RAYS_NORMALIZE: a lens ray is made by the rule, not given");
    const uint32_t known = HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE | HRT_RADIANCE_ACCUMULATE | HRT_FLAG_GAMMA;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": flags: unknown bits " + std::to_string(flags & ~known));
    { const int brc = check_mesh_brute(who, flags); if (brc != HRT_OK) return brc; }
    if ((flags & HRT_FLAG_GAMMA) && (flags & HRT_RADIANCE_ACCUMULATE))
        return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_GAMMA cannot be combined with HRT_RADIANCE_ACCUMULATE (running sums are linear)");
    { const int lrc = lens_check(who, lens, L); if (lrc != HRT_OK) return lrc; }
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is not 4-byte aligned");
    return HRT_OK;
}

// The fused launch into d_frame on `stream` (the scene entered), then the gamma: hrt_gamma_kernel, the in-place kernel of the
// one-shot render (hrt_finalize_kernel's expression after its division), over the means, in pieces its 32-bit index can address.
static int lens_launch(hrt_scene *s, const DLens &L, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                       uint32_t flags, float *d_frame, hipStream_t stream) {
    DLensRadiance Q;
    Q.out = d_frame;
    Q.n = w * h;
    Q.flags = flags & ~(uint32_t)HRT_FLAG_GAMMA;
    Q.first_sample = first_sample;
    Q.n_samples = n_samples;
    Q.seed_lo = (uint32_t)seed;
    Q.seed_hi = (uint32_t)(seed >> 32);
    Q.w = w;
    Q.h = h;
    Q.lens = L;
    const bool exact = (flags & HRT_FLAG_EXACT_ONLY) != 0u;
    const bool lights = s->d.n_lights != 0u;
    void (*const k)(const DLensRadiance) = exact ? (lights ? hrt_lens_kernel_lights_exact : hrt_lens_kernel_exact)
                                                 : (lights ? hrt_lens_kernel_lights : hrt_lens_kernel);
    const int rc = query_launch(k, Q, s, HRT_RADIANCE_STAGE_TREE, HRT_RADIANCE_WG, stream);  // the tree from global memory, as hrt_trace_radiance
    if (rc != HRT_OK || !(flags & HRT_FLAG_GAMMA)) return rc;
    const uint64_t total = (uint64_t)Q.n * 3u, piece = 1ull << 30;
    for (uint64_t at = 0; at < total; at += piece) {
        const uint32_t n = (uint32_t)std::min(piece, total - at);
        hipLaunchKernelGGL(hrt_gamma_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_frame + at, n);
        HIP_TRY(hipGetLastError());
    }
    return HRT_OK;
}

int hrt_render_lens_device(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                           uint32_t flags, float *d_frame, void *stream) {
    const std::string who = "hrt_render_lens_device";
    DLens L;
    int rc = lens_render_check(who, lens, w, h, first_sample, n_samples, flags, d_frame, "d_frame", L);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    return lens_launch(s, L, w, h, first_sample, n_samples, seed, flags, d_frame, (hipStream_t)stream);
}

// Blocking, into host memory.  The device frame and the two events are the call's own, so that this form, too, leaves the scene's
// state alone.
int hrt_render_lens(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags, float *out_rgb,
                    hrt_stats *stats) {
    const std::string who = "hrt_render_lens";
    DLens L;
    if (flags & HRT_RADIANCE_ACCUMULATE) return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (hrt_render_lens_device)");
    int rc = lens_render_check(who, lens, w, h, 0u, spp, flags, out_rgb, "out_rgb", L);
    if (rc == HRT_OK) rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t bytes = (size_t)w * h * 3u * sizeof(float);
    float *d_frame = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float ms = 0.f;
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc((void **)&d_frame, bytes));
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, nullptr));
        const int lrc = lens_launch(s, L, w, h, 0u, spp, seed, flags, d_frame, nullptr);
        if (lrc != HRT_OK) return lrc;
        HIP_TRY(hipEventRecord(ev1, nullptr));
        HIP_TRY(hipMemcpy(out_rgb, d_frame, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        return HRT_OK;
    };
    rc = run();
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (d_frame) (void)hipFree(d_frame);
    if (rc != HRT_OK) return rc;
    if (stats) {
        fill_stats(s, stats, t0, (double)ms, (uint64_t)w * h * spp);
        stats->lds_bytes = 0u;  // the tree is read from global memory
        stats->waves_launched = 0u;
    }
    return HRT_OK;
}

int hrt_render_lens_features(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                             float *d_features, void *stream) {
    const std::string who = "hrt_render_lens_features";
    DLens L;
    { const int lrc = lens_check(who, lens, L); if (lrc != HRT_OK) return lrc; }
    int rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if ((uint64_t)first_sample + n_samples > 0xffffffffull) return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples overflows 32 bits");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    DRender R;
    DCamera C;
    if ((rc = fill_render(s, &lens->cam, w, h, 1, seed, 0, 0, 1, R, C)) != HRT_OK) return rc;
    R.cam = nullptr;  // the lens is a kernel argument
    R.s0 = first_sample;
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_lens_features_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, R, L, s->bound, n_samples, d_features);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}
