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
// Batched lens views (hrt_render_lens_views*): N lens frames of one scene as ONE dense index space of N * w * h items, item i being
// pixel i % (w*h) of view i / (w*h).  The hrt_lens_views_kernel builds are radiance_body with the LensViewRays source, whose lane
// takes the lens and the seed of its item's view from a table in device memory (DLensView) at the point of use -- per LANE: a wave
// straddles views whenever w*h is no multiple of 64, and lanes take their next item by grid stride on their own, so the view is
// never wave-uniform.  The item-major store is the view-major, row-major layout of the frames.  hrt_lens_views_features_kernel is
// features_body over the same items.  The table is the scene's (a StagedTable, hrt_api.hip, as the view blocks of
// hrt_views.hip); nothing of the trace launches' state is touched.
//
// Adaptive lens frames (hrt_render_lens_adaptive*, the rounds are in hrt_lens_adaptive.hip): the lens kernel over a LIST OF TILES.  The
// hrt_lens_tiles_kernel builds are radiance_body with the LensTileRays source over n_active * 64 items, item i being lane i & 63 of
// active tile i >> 6 -- the tile-major layout the adaptive rounds' judge reads, so the launch adds its samples straight onto the
// compact sums buffer (HRT_RADIANCE_ACCUMULATE), with no scatter.  An item outside the image makes no traced sample.
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

// One view of a batched lens launch: the lens, the seed of its frame and, for the features of a pinhole view, the render's margin
// for its eye (what a one-lens launch keeps in DRender::err_abs).  240 bytes, read per lane with vector loads.
struct DLensView {
    DLens lens;
    uint32_t seed_lo, seed_hi;
    float err_abs;
    uint32_t pad;
};

// The launch record of the hrt_lens_kernel builds: DRadiance with the lens and the frame in place of the ray and key arrays
// (radiance_launch, query_launch and radiance_body reach the fields they share by name).
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

// The launch record of the hrt_lens_views_kernel builds: the table of views in place of the one lens and the launch's seed.
struct DLensViewsRadiance {
    const DScene *scene;
    float *out;            // 3 floats per item: view-major, each view row-major
    uint32_t n;            // n_views * w * h
    uint32_t flags;
    uint32_t first_sample, n_samples;
    uint32_t lds_units;
    float bound;
    uint32_t w, h, npix;   // npix = w * h
    const DLensView *views;
};

// The launch record of the hrt_lens_tiles_kernel builds: DLensRadiance over a list of 8 x 8 tiles.  out + 3 * i is the compact
// tile-major sums buffer of the adaptive rounds (hrt_adaptive.hip): 64 items per active tile, item lane = (y & 7) * 8 + (x & 7).
struct DLensTilesRadiance {
    const DScene *scene;
    float *out;            // 3 floats per item: 64 items per active tile, in list order
    uint32_t n;            // n_active * 64
    uint32_t flags;
    uint32_t first_sample, n_samples;
    uint32_t seed_lo, seed_hi;
    uint32_t lds_units;
    float bound;
    uint32_t w, h, tiles_x;
    const uint32_t *list;  // the active tiles, n_active of them (NULL: tile k is k, every tile of the frame)
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
// One branch on the projection, each arm straight-line code: the same arm for every lane of a one-lens launch; in a batch the
// lanes of a wave may hold different views, and the arms their lenses name run one after the other.
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
    __device__ static __forceinline__ uint32_t key(const DLensRadiance &, uint32_t pixel) { return pixel; }
    __device__ static __forceinline__ void seed(const DLensRadiance &Q, uint32_t, uint32_t &lo, uint32_t &hi) { lo = Q.seed_lo; hi = Q.seed_hi; }
    __device__ static __forceinline__ bool sample(const DLensRadiance &Q, uint32_t pixel, uint32_t sample, Ray &ray) {
        return lens_sample(Q.lens, Q.seed_lo, Q.seed_hi, Q.w, Q.h, pixel, sample, ray) && lens_traced(ray);
    }
};

// radiance_body's source for a batch of lens views: item i is pixel i % npix of view i / npix, keyed by that pixel and its view's
// seed.  The lens is NOT wave-uniform (see the head of this file): lens_sample reads the view's block through a reference into
// the table, so every field is loaded by the lane that uses it where it uses it, and no lens is held in registers across the path.
// i < Q.n = n_views * npix, so the view is inside the table.
struct LensViewRays {
    static constexpr bool per_sample = true;
    __device__ static __forceinline__ uint32_t key(const DLensViewsRadiance &Q, uint32_t i) { return i % Q.npix; }
    __device__ static __forceinline__ void seed(const DLensViewsRadiance &Q, uint32_t i, uint32_t &lo, uint32_t &hi) {
        const DLensView &V = Q.views[i / Q.npix];
        lo = V.seed_lo; hi = V.seed_hi;
    }
    __device__ static __forceinline__ bool sample(const DLensViewsRadiance &Q, uint32_t i, uint32_t sample, Ray &ray) {
        const uint32_t view = i / Q.npix;
        const DLensView &V = Q.views[view];
        return lens_sample(V.lens, V.seed_lo, V.seed_hi, Q.w, Q.h, i - view * Q.npix, sample, ray) && lens_traced(ray);
    }
};

// radiance_body's source for a list of tiles of one lens frame: item i is lane i & 63 of active tile k = i >> 6, whose tile is
// list[k] (k itself without a list); the lane's pixel is x = (tile % tiles_x) * 8 + (lane & 7), y = (tile / tiles_x) * 8 + (lane >> 3)
// -- hrt_ad_judge_kernel's layout for rank 0 of world 1 -- keyed y * w + x with the launch's seed, so a sample is LensRays' sample of
// that pixel bit for bit.  An item outside the image makes no traced sample: under HRT_RADIANCE_ACCUMULATE, which every such
// launch passes, its three floats are read and written back as they were.  i < Q.n = n_active * 64, so k is inside the list.
// The workgroup is 256 lanes and the stride a multiple of 64, so the lanes of a wave walk the same tiles; but a lane takes its
// next item the moment its own is done (radiance_body), so at any one time they may stand at different tiles: the slot is
// loaded by the lane that needs it (4 bytes, shared by the tile's 64 lanes in the cache) and never broadcast.
struct LensTileRays {
    static constexpr bool per_sample = true;
    // The pixel of item i; false outside the image.
    __device__ static __forceinline__ bool pixel(const DLensTilesRadiance &Q, uint32_t i, uint32_t &p) {
        const uint32_t k = i >> 6, lane = i & 63u;
        const uint32_t tile = Q.list ? Q.list[k] : k;
        const uint32_t x = (tile % Q.tiles_x) * 8u + (lane & 7u), y = (tile / Q.tiles_x) * 8u + (lane >> 3);
        p = y * Q.w + x;
        return x < Q.w && y < Q.h;
    }
    __device__ static __forceinline__ uint32_t key(const DLensTilesRadiance &Q, uint32_t i) {
        uint32_t p;
        (void)pixel(Q, i, p);
        return p;
    }
    __device__ static __forceinline__ void seed(const DLensTilesRadiance &Q, uint32_t, uint32_t &lo, uint32_t &hi) { lo = Q.seed_lo; hi = Q.seed_hi; }
    __device__ static __forceinline__ bool sample(const DLensTilesRadiance &Q, uint32_t i, uint32_t sample, Ray &ray) {
        uint32_t p;
        return pixel(Q, i, p) && lens_sample(Q.lens, Q.seed_lo, Q.seed_hi, Q.w, Q.h, p, sample, ray) && lens_traced(ray);
    }
};

// features_body's source for a lens.  A pinhole keeps the render's margin (R.err_abs, R.flags), so that its features are
// hrt_render_features' bit for bit; every other lens moves the origin or the direction per sample and takes the margin and the
// far-origin rule of that sample's ray, as hrt_trace_rays does for the same record.
struct LensFeatureRays {
    const DLens &L;
    float bound;  // hrt_scene::bound
    __device__ __forceinline__ uint32_t items(const DRender &R) const { return R.w * R.h; }
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

// features_body's source for a batch of lens views: item idx is pixel idx % (w*h) of view idx / (w*h), with that view's lens and
// seed; R.w x R.h is one view's frame.  What LensFeatureRays does for its one lens, per lane: a pinhole view takes the render's
// margin for its own eye from its block.
struct LensViewFeatureRays {
    const DLensView *views;
    float bound;  // hrt_scene::bound
    uint32_t n_items;
    __device__ __forceinline__ uint32_t items(const DRender &) const { return n_items; }
    template <class CX>
    __device__ __forceinline__ bool operator()(CX &cx, const DRender &R, uint32_t n, uint32_t idx, uint32_t k, Ray &ray) const {
        const uint32_t npix = R.w * R.h, view = idx / npix, pixel = idx - view * npix;
        const DLensView &V = views[view];
        const DLens &L = V.lens;
        bool ok;
        if (n == 0u) {
            const uint32_t x = pixel % R.w, y = pixel / R.w;
            ok = lens_project(L, ((float)x + 0.5f) / (float)R.w, ((float)y + 0.5f) / (float)R.h, 0.f, 0.f, 0.f, ray);
        } else {
            ok = lens_sample(L, V.seed_lo, V.seed_hi, R.w, R.h, pixel, R.s0 + k, ray);
        }
        if (L.projection == HRT_LENS_PERSPECTIVE && L.aperture == 0.f) {
            cx.err_abs = V.err_abs;
            cx.flags = R.flags;
        } else {
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

// The fused frame: radiance_body over pixels.
HRT_RADIANCE_FAMILY(hrt_lens_kernel, LensRays, DLensRadiance)

// The fused frames of a batch: radiance_body over the items of all views.
HRT_RADIANCE_FAMILY(hrt_lens_views_kernel, LensViewRays, DLensViewsRadiance)

// The fused frame over a list of tiles: radiance_body over the 64 items of every active tile.
HRT_RADIANCE_FAMILY(hrt_lens_tiles_kernel, LensTileRays, DLensTilesRadiance)

// hrt_render_lens_features: hrt_features_kernel with the lens as a kernel argument in place of the scene's camera block.
extern "C" __global__ void __launch_bounds__(256) hrt_lens_features_kernel(const DRender R, const DLens L, float bound, uint32_t n,
                                                                           float *__restrict__ out) {
    features_body<CtxT<false, false, false, true>>(R, n, out, LensFeatureRays{L, bound});
}

// hrt_render_lens_views_features: the same over the n_items = n_views * w * h items of a batch, the lenses from the table.
extern "C" __global__ void __launch_bounds__(256) hrt_lens_views_features_kernel(const DRender R, const DLensView *__restrict__ views, float bound,
                                                                                 uint32_t n_items, uint32_t n, float *__restrict__ out) {
    features_body<CtxT<false, false, false, true>>(R, n, out, LensViewFeatureRays{views, bound, n_items});
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
    { const int rrc = rays_out_check(who, d_rays); if (rrc != HRT_OK) return rrc; }
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_lens_rays_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, L, w, h, sample, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (float4 *)d_rays);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// The flags of a fused lens launch, one frame or a batch.
static int lens_flags_check(const std::string &who, uint32_t flags) {
    return fused_flags_check(who, flags, "a lens frame has one kernel form", "a lens ray is made by the rule, not given", nullptr);
}

// The checks hrt_render_lens_device and hrt_render_lens share, in the header's order (all before the scene); fills L.
static int lens_render_check(const std::string &who, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                             uint32_t flags, const float *out, const char *out_name, DLens &L) {
    { const int frc = lens_flags_check(who, flags); if (frc != HRT_OK) return frc; }
    { const int lrc = lens_check(who, lens, L); if (lrc != HRT_OK) return lrc; }
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    return samples_out_check(who, first_sample, n_samples, out, out_name);
}

// HRT_FLAG_GAMMA of a fused lens launch: hrt_gamma_kernel, the in-place kernel of the one-shot render (hrt_finalize_kernel's
// expression after its division), over the `total` floats of the means, in pieces its 32-bit index can address.
static int lens_gamma(float *d_frame, uint64_t total, hipStream_t stream) {
    const uint64_t piece = 1ull << 30;
    for (uint64_t at = 0; at < total; at += piece) {
        const uint32_t n = (uint32_t)std::min(piece, total - at);
        hipLaunchKernelGGL(hrt_gamma_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_frame + at, n);
        HIP_TRY(hipGetLastError());
    }
    return HRT_OK;
}

// The fused launch into d_frame on `stream` (the scene entered), then the gamma.  Q and its builds: DLensRadiance and
// hrt_lens_kernel_builds, or the record and a table of a lit frame (hrt_lit_frames.hip) with the rule filled in.
extern "C++" {
template <class QT>
static int lens_launch(void (*const *builds)(const QT), QT &Q, hrt_scene *s, const DLens &L, uint32_t w, uint32_t h, uint32_t first_sample,
                       uint32_t n_samples, uint64_t seed, uint32_t flags, float *d_frame, hipStream_t stream) {
    Q.w = w;
    Q.h = h;
    Q.lens = L;
    const int rc = radiance_launch(builds, Q, s, first_sample, n_samples, seed, flags & ~(uint32_t)HRT_FLAG_GAMMA, d_frame, w * h, stream);
    if (rc != HRT_OK || !(flags & HRT_FLAG_GAMMA)) return rc;
    return lens_gamma(d_frame, (uint64_t)Q.n * 3u, stream);
}

// Both forms of a lens frame, plain (NoRule) or lit (LitRule), checked in the header's order: lens_render_check's, the rule's,
// then the scene.  launch(L, d_frame, stream) is the fused launch; the blocking form runs it into a buffer of its own (BlockingCall).
template <class Rule, class Launch>
static int lens_frame_call(const std::string &who, bool dev, hrt_scene *s, const Rule &R, const hrt_lens *lens, uint32_t w, uint32_t h,
                           uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *out, void *stream, hrt_stats *stats, Launch launch) {
    DLens L;
    int rc = dev ? HRT_OK : blocking_accumulate_check(who, flags);
    if (rc == HRT_OK) rc = lens_render_check(who, lens, w, h, first_sample, n_samples, flags, out, dev ? "d_frame" : "out_rgb", L);
    if (rc == HRT_OK) rc = R.check(who);
    if (rc == HRT_OK) rc = R.enter(who, s);
    if (rc != HRT_OK) return rc;
    if (dev) return launch(L, out, (hipStream_t)stream);
    BlockingCall call;
    return call.run(s, (size_t)w * h * 3u * sizeof(float), out, (uint64_t)w * h * n_samples, stats,
                    [&](float *d_frame) { return launch(L, d_frame, nullptr); });
}
}  // extern "C++"

static int lens_frame_entry(const std::string &who, bool dev, hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample,
                            uint32_t n_samples, uint64_t seed, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return lens_frame_call(who, dev, s, NoRule{}, lens, w, h, first_sample, n_samples, flags, out, stream, stats,
                           [&](const DLens &L, float *d_frame, hipStream_t st) {
                               DLensRadiance Q;
                               return lens_launch(hrt_lens_kernel_builds, Q, s, L, w, h, first_sample, n_samples, seed, flags, d_frame, st);
                           });
}

int hrt_render_lens_device(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                           uint32_t flags, float *d_frame, void *stream) {
    return lens_frame_entry("hrt_render_lens_device", true, s, lens, w, h, first_sample, n_samples, seed, flags, d_frame, stream, nullptr);
}

// Blocking, into host memory.
int hrt_render_lens(hrt_scene *s, const hrt_lens *lens, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags, float *out_rgb,
                    hrt_stats *stats) {
    return lens_frame_entry("hrt_render_lens", false, s, lens, w, h, 0u, spp, seed, flags, out_rgb, nullptr, stats);
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

// ---- Batched lens views (include/hrt.h hrt_render_lens_views*)

// Checks 2..4 of the header's order: an empty batch is the caller's to return on, `views` is there, every lens passes lens_check
// (the message names the view).  Fills one block per view (all but err_abs, which needs the scene's extent).
static int lens_views_blocks(const std::string &who, const hrt_lens_view *views, uint32_t n_views, std::vector<DLensView> &blocks) {
    if (!views) return fail(HRT_ERR_INVALID, who + ": views is NULL");
    for (uint32_t v = 0; v < n_views; ++v) {
        const std::string where = who + ": views[" + std::to_string(v) + "].lens";
        DLensView B;
        const int lrc = lens_check(where, &views[v].lens, B.lens);
        if (lrc != HRT_OK) return g_error.compare(0, where.size(), where) == 0 ? lrc : fail(lrc, where + ": " + g_error);  // the camera's own message names neither
        B.seed_lo = (uint32_t)views[v].seed; B.seed_hi = (uint32_t)(views[v].seed >> 32);
        B.err_abs = 0.f; B.pad = 0u;
        blocks.push_back(B);
    }
    return HRT_OK;
}

// Check 9: the items of all views within what one frame may have.
static int lens_views_limit(const std::string &who, uint32_t n_views, uint32_t w, uint32_t h, uint64_t max_items) {
    const uint64_t items = (uint64_t)n_views * ((uint64_t)w * h);  // w * h <= max_items < 2^31: no overflow
    if (items > max_items)
        return fail(HRT_ERR_INVALID, who + ": n_views * w * h is " + std::to_string(items) + ", above the " + std::to_string(max_items) + " pixels one launch indexes");
    return HRT_OK;
}

// The checks hrt_render_lens_views_device and hrt_render_lens_views share, in the header's order (all before the scene).
static int lens_views_check(const std::string &who, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t first_sample,
                            uint32_t n_samples, uint32_t flags, const float *out, const char *out_name, std::vector<DLensView> &blocks) {
    { const int frc = lens_flags_check(who, flags); if (frc != HRT_OK) return frc; }
    if (n_views == 0u) return HRT_OK;
    { const int brc = lens_views_blocks(who, views, n_views, blocks); if (brc != HRT_OK) return brc; }
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    { const int src = samples_out_check(who, first_sample, n_samples, out, out_name); if (src != HRT_OK) return src; }
    return lens_views_limit(who, n_views, w, h, k_max_pixels);
}

// Puts the blocks into the scene's table on `stream` (the scene entered) and returns it (StagedTable::stage: the host waits for
// the table's last reader before a larger table replaces it, nothing else orders these launches); lens_views.staged() follows the
// launch that reads it.
static int lens_views_stage(hrt_scene *s, std::vector<DLensView> &blocks, hipStream_t stream, const DLensView **table) {
    for (DLensView &B : blocks) {  // fill_render's margin, per view
        const float *e = B.lens.eye;
        B.err_abs = margin_scale(s->bound, std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
    }
    return s->lens_views.stage(blocks, stream, table);
}

// The fused launch over all views into d_frames on `stream` (the scene entered), then the gamma over all frames.  Q and its
// builds: DLensViewsRadiance and hrt_lens_views_kernel_builds, or those of a lit batch (hrt_lit_frames.hip).
extern "C++" {
template <class QT>
static int lens_views_launch(void (*const *builds)(const QT), QT &Q, hrt_scene *s, std::vector<DLensView> &blocks, uint32_t w, uint32_t h,
                             uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *d_frames, hipStream_t stream) {
    { const int src = lens_views_stage(s, blocks, stream, &Q.views); if (src != HRT_OK) return src; }
    Q.w = w;
    Q.h = h;
    Q.npix = w * h;
    int rc = radiance_launch(builds, Q, s, first_sample, n_samples, 0u, flags & ~(uint32_t)HRT_FLAG_GAMMA, d_frames,
                             (uint32_t)blocks.size() * Q.npix, stream);  // no launch seed: every view has its own
    if (rc == HRT_OK) rc = s->lens_views.staged(stream);
    if (rc != HRT_OK || !(flags & HRT_FLAG_GAMMA)) return rc;
    return lens_gamma(d_frames, (uint64_t)Q.n * 3u, stream);
}

// Both forms of a batch of lens views, plain (NoRule) or lit (LitRule), checked in the header's order: lens_views_check's (an empty
// batch skips all but the flags), the rule's tail_after, (an empty batch returns,) the rule's volume, then the scene.
// launch(blocks, d_frames, stream) is the fused launch.
template <class Rule, class Launch>
static int lens_views_call(const std::string &who, bool dev, hrt_scene *s, const Rule &R, const hrt_lens_view *views, uint32_t n_views, uint32_t w,
                           uint32_t h, uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *out, void *stream, hrt_stats *stats,
                           Launch launch) {
    std::vector<DLensView> blocks;
    int rc = dev ? HRT_OK : blocking_accumulate_check(who, flags);
    if (rc == HRT_OK) rc = lens_views_check(who, views, n_views, w, h, first_sample, n_samples, flags, out, dev ? "d_frames" : "out_rgb", blocks);
    if (rc == HRT_OK) rc = R.check_tail(who);
    if (rc != HRT_OK) return rc;
    if (n_views == 0u) return empty_batch(stats);
    if ((rc = R.check_volume(who)) != HRT_OK) return rc;
    if ((rc = R.enter(who, s)) != HRT_OK) return rc;
    if (dev) return launch(blocks, out, (hipStream_t)stream);
    BlockingCall call;
    return call.run(s, (size_t)n_views * w * h * 3u * sizeof(float), out, (uint64_t)n_views * w * h * n_samples, stats,
                    [&](float *d_frames) { return launch(blocks, d_frames, nullptr); });
}
}  // extern "C++"

static int lens_views_entry(const std::string &who, bool dev, hrt_scene *s, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h,
                            uint32_t first_sample, uint32_t n_samples, uint32_t flags, float *out, void *stream, hrt_stats *stats) {
    return lens_views_call(who, dev, s, NoRule{}, views, n_views, w, h, first_sample, n_samples, flags, out, stream, stats,
                           [&](std::vector<DLensView> &blocks, float *d_frames, hipStream_t st) {
                               DLensViewsRadiance Q;
                               return lens_views_launch(hrt_lens_views_kernel_builds, Q, s, blocks, w, h, first_sample, n_samples, flags, d_frames, st);
                           });
}

int hrt_render_lens_views_device(hrt_scene *s, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t first_sample,
                                 uint32_t n_samples, uint32_t flags, float *d_frames, void *stream) {
    return lens_views_entry("hrt_render_lens_views_device", true, s, views, n_views, w, h, first_sample, n_samples, flags, d_frames, stream, nullptr);
}

// Blocking, into host memory.
int hrt_render_lens_views(hrt_scene *s, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t spp, uint32_t flags,
                          float *out_rgb, hrt_stats *stats) {
    return lens_views_entry("hrt_render_lens_views", false, s, views, n_views, w, h, 0u, spp, flags, out_rgb, nullptr, stats);
}

int hrt_render_lens_views_features(hrt_scene *s, const hrt_lens_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t first_sample,
                                   uint32_t n_samples, float *d_features, void *stream) {
    const std::string who = "hrt_render_lens_views_features";
    std::vector<DLensView> blocks;
    if (n_views == 0u) return HRT_OK;
    int rc = lens_views_blocks(who, views, n_views, blocks);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if ((uint64_t)first_sample + n_samples > 0xffffffffull) return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples overflows 32 bits");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if ((uintptr_t)d_features % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": d_features is not 4-byte aligned");
    if ((rc = lens_views_limit(who, n_views, w, h, k_max_records)) != HRT_OK) return rc;
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    DRender R;
    DCamera C;
    if ((rc = fill_render(s, &views[0].lens.cam, w, h, 1, 0, 0, 0, 1, R, C)) != HRT_OK) return rc;  // seed and margin are each view's own
    R.cam = nullptr;  // the lenses are in the table
    R.s0 = first_sample;
    const DLensView *table = nullptr;
    if ((rc = lens_views_stage(s, blocks, (hipStream_t)stream, &table)) != HRT_OK) return rc;
    const uint32_t n_items = n_views * w * h;
    hipLaunchKernelGGL(hrt_lens_views_features_kernel, dim3((n_items + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, R, table, s->bound, n_items,
                       n_samples, d_features);
    HIP_TRY(hipGetLastError());
    return s->lens_views.staged((hipStream_t)stream);
}
