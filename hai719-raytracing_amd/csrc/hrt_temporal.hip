// Temporal accumulation (include/hrt.h hrt_temporal_accumulate, hrt_history_*, hrt_render_temporal).
// Included by hrt_api.hip inside its extern "C" block, after hrt_denoise.hip, whose demodulation (dn_demodulate, dn_remodulate,
// dn_finite) and render scaffold (dn_render_pair, features_launch, dn_run) it shares.
//
// One kernel, one lane per pixel, workgroups of HRT_DN_TILE x HRT_DN_TILE pixels as the filter's passes: a wave covers 16 x 4
// pixels, so under a camera that moved a little its 4 x 64 taps fall in about five rows of the previous frame and neighbouring
// lanes share three of their four taps through the caches.  A lane reads its own records -- colour(s) 12 (24) bytes, features 48
// -- and up to four previous records of 64 (76) bytes, and writes 16 (28) bytes: about 0.4 KB a pixel, no reuse worth staging in
// LDS, bound by memory.  The records are read as the dwords they are (a feature record is 48 bytes from a base that is only known
// to be 4-byte aligned); the compiler merges them into dwordx3 / dwordx4 loads.
// The camera block of the current frame travels as a kernel argument, as in hrt_camera_rays_kernel; the previous camera as the
// twelve floats of its pose and the two projection constants.

struct DTemporal {
    DCamera cam;                                 // the current camera: camera_ray's constants
    float eye[3], right[3], up[3], forward[3];   // the previous camera as given
    float kx, ky;                                // (float)(cot / aspect), (float)cot of the previous camera
    uint32_t w, h;
    uint32_t has_prev, still;                    // a previous frame was given; its camera is the current one byte for byte
    float alpha_min, max_history, depth_tol, normal_tol, albedo_tol;
    const float *color, *half, *feat;
    const float *pcolor, *phalf, *pfeat, *phist;
    float *out, *out_half, *hist_out;
};

extern "C++" {
// |a - b|^2 of two 3-vectors in the filter's order
__device__ __forceinline__ float tp_dist2(const float *a, const float *b) {
    const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}
// a tolerance of +inf passes its test always
__device__ __forceinline__ bool tp_within(float v, float bound, float tol) { return tol == __builtin_inff() || v <= bound; }

// Step 1 of THE FILTER on one pixel: x (and xh) from colour c (and ch) with features f; false if the pixel is invalid.
template <bool HALF>
__device__ __forceinline__ bool tp_demodulate(const float *c, const float *ch, const float *f, float *x, float *xh) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const float e6 = f[6 + k] / 6.f;
        x[k] = dn_demodulate(c[k], e6, f[k]);
        ok = ok && dn_finite(x[k]);
        if (HALF) {
            xh[k] = dn_demodulate(ch[k], e6, f[k]);
            ok = ok && dn_finite(xh[k]);
        }
    }
    for (int k = 0; k < 10; ++k) ok = ok && dn_finite(f[k]);
    return ok;
}

template <bool HALF>
__device__ __forceinline__ void temporal_body(const DTemporal &T) {
    const uint32_t x = blockIdx.x * HRT_DN_TILE + (threadIdx.x % HRT_DN_TILE), y = blockIdx.y * HRT_DN_TILE + (threadIdx.x / HRT_DN_TILE);
    if (x >= T.w || y >= T.h) return;
    const size_t p = (size_t)y * T.w + x;
    float f[11], c[3], ch[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 11; ++k) f[k] = T.feat[p * HRT_FEATURE_FLOATS + k];
    for (int k = 0; k < 3; ++k) c[k] = T.color[p * 3u + k];
    if (HALF) for (int k = 0; k < 3; ++k) ch[k] = T.half[p * 3u + k];
    float r[3] = {c[0], c[1], c[2]}, rh[3] = {ch[0], ch[1], ch[2]}, n_out = 1.f;  // a restart pixel
    float xp[3], xhp[3];
    bool go = tp_demodulate<HALF>(c, ch, f, xp, xhp) && !(f[10] == 0.f) && T.has_prev != 0u;
    float px = (float)x, py = (float)y, zexp = 0.f;
    if (go) {
        const float zbar = f[9] / f[10];
        zexp = zbar;
        if (!T.still) {
            const hrtk::Ray ray = hrtk::camera_ray<false>(&T.cam, ((float)x + 0.5f) / (float)T.w, ((float)y + 0.5f) / (float)T.h, 0.f);
            const float s0 = (ray.o.x + zbar * ray.d.x) - T.eye[0], s1 = (ray.o.y + zbar * ray.d.y) - T.eye[1], s2 = (ray.o.z + zbar * ray.d.z) - T.eye[2];
            const float xc = (s0 * T.right[0] + s1 * T.right[1]) + s2 * T.right[2];
            const float yc = (s0 * T.up[0] + s1 * T.up[1]) + s2 * T.up[2];
            const float zc = (s0 * T.forward[0] + s1 * T.forward[1]) + s2 * T.forward[2];
            go = zc > 0.f;
            px = (((T.kx * xc) / zc + 1.f) * 0.5f) * (float)T.w - 0.5f;
            py = ((1.f - (T.ky * yc) / zc) * 0.5f) * (float)T.h - 0.5f;
            zexp = sqrtf((s0 * s0 + s1 * s1) + s2 * s2);
        }
    }
    if (go) {
        const float fix = floorf(px), fiy = floorf(py);
        const float fx = px - fix, fy = py - fiy;
        const float wt[4] = {(1.f - fx) * (1.f - fy), fx * (1.f - fy), (1.f - fx) * fy, fx * fy};
        const float zlim = T.depth_tol * fmaxf(zexp, 1e-3f);
        float sw = 0.f, sn = 0.f, sx[3] = {0.f, 0.f, 0.f}, sxh[3] = {0.f, 0.f, 0.f};
        for (int t = 0; t < 4; ++t) {
            // the tap's coordinates as floats first: px may be anything, NaN and +-inf included, and those are inside no image
            const float qxf = fix + (float)(t & 1), qyf = fiy + (float)(t >> 1);
            if (!(qxf >= 0.f && qxf < (float)T.w && qyf >= 0.f && qyf < (float)T.h)) continue;
            const size_t q = (size_t)(uint32_t)qyf * T.w + (uint32_t)qxf;
            const float hq = T.phist[q];
            if (!(hq >= 1.f)) continue;
            float g[11], cq[3], chq[3] = {0.f, 0.f, 0.f}, xq[3], xhq[3];
            for (int k = 0; k < 11; ++k) g[k] = T.pfeat[q * HRT_FEATURE_FLOATS + k];
            for (int k = 0; k < 3; ++k) cq[k] = T.pcolor[q * 3u + k];
            if (HALF) for (int k = 0; k < 3; ++k) chq[k] = T.phalf[q * 3u + k];
            if (!(tp_demodulate<HALF>(cq, chq, g, xq, xhq) && dn_finite(g[10]) && g[10] > 0.f)) continue;
            if (!tp_within(fabsf(zexp - g[9] / g[10]), zlim, T.depth_tol)) continue;
            if (!tp_within(tp_dist2(f + 3, g + 3), T.normal_tol, T.normal_tol)) continue;
            if (!tp_within(tp_dist2(f, g), T.albedo_tol, T.albedo_tol)) continue;
            const float wq = wt[t];
            sw = sw + wq;
            for (int k = 0; k < 3; ++k) sx[k] = sx[k] + wq * xq[k];
            if (HALF) for (int k = 0; k < 3; ++k) sxh[k] = sxh[k] + wq * xhq[k];
            sn = sn + wq * hq;
        }
        if (sw > 0.f) {
            const float n_new = fminf(sn / sw + 1.f, T.max_history);
            const float alpha = fmaxf(1.f / n_new, T.alpha_min);
            bool fin = true;
            float b[3], bh[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < 3; ++k) {
                const float xhist = sx[k] / sw;
                b[k] = dn_remodulate(xhist + alpha * (xp[k] - xhist), f[6 + k], f[k]);
                fin = fin && dn_finite(b[k]);
                if (HALF) {
                    const float xhhist = sxh[k] / sw;
                    bh[k] = dn_remodulate(xhhist + alpha * (xhp[k] - xhhist), f[6 + k], f[k]);
                    fin = fin && dn_finite(bh[k]);
                }
            }
            if (fin) {
                for (int k = 0; k < 3; ++k) { r[k] = b[k]; rh[k] = bh[k]; }
                n_out = n_new;
            }
        }
    }
    for (int k = 0; k < 3; ++k) T.out[p * 3u + k] = r[k];
    if (HALF) for (int k = 0; k < 3; ++k) T.out_half[p * 3u + k] = rh[k];
    T.hist_out[p] = n_out;
}
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_temporal_kernel(const DTemporal T) { temporal_body<false>(T); }
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_temporal_half_kernel(const DTemporal T) { temporal_body<true>(T); }

static int tp_check_params(const std::string &who, const hrt_temporal_params *p) {
    if (!p) return fail(HRT_ERR_INVALID, who + ": params is NULL");
    if (std::isnan(p->alpha_min) || !(p->alpha_min > 0.f) || p->alpha_min > 1.f) return fail(HRT_ERR_INVALID, who + ": alpha_min must be in (0, 1]");
    if (!std::isfinite(p->max_history) || p->max_history < 1.f) return fail(HRT_ERR_INVALID, who + ": max_history must be finite and >= 1");
    const float tol[3] = {p->depth_tol, p->normal_tol, p->albedo_tol};
    const char *names[3] = {"depth_tol", "normal_tol", "albedo_tol"};
    for (int k = 0; k < 3; ++k)
        if (std::isnan(tol[k]) || !(tol[k] > 0.f)) return fail(HRT_ERR_INVALID, who + ": " + names[k] + " must be > 0 (+inf switches the test off)");
    return HRT_OK;
}

// hrt_camera -> what the kernel reads of the PREVIOUS camera: its pose as given and the two constants of its projection, computed
// as make_camera computes them.  The camera must be one hrt_render accepts.
static int tp_camera(const std::string &who, const char *name, const hrt_camera *cam, DCamera &C) {
    if (make_camera(cam, C) != HRT_OK) return fail(HRT_ERR_INVALID, who + ": " + name + ": " + std::string(g_error));
    return HRT_OK;
}

int hrt_temporal_accumulate(const hrt_camera *cam, const hrt_camera *prev_cam, uint32_t w, uint32_t h, const float *d_color,
                            const float *d_color_half, const float *d_features, const float *d_prev_color, const float *d_prev_color_half,
                            const float *d_prev_features, const float *d_prev_history, const hrt_temporal_params *p, float *d_out,
                            float *d_out_half, float *d_history_out, void *stream) {
    const std::string who = "hrt_temporal_accumulate";
    int rc = tp_check_params(who, p);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if (!cam) return fail(HRT_ERR_INVALID, who + ": cam is NULL");
    if (!d_color) return fail(HRT_ERR_INVALID, who + ": d_color is NULL");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
    if ((d_out_half != nullptr) != (d_color_half != nullptr)) return fail(HRT_ERR_INVALID, who + ": d_out_half must be given exactly when d_color_half is");
    const bool prev = prev_cam || d_prev_color || d_prev_color_half || d_prev_features || d_prev_history;
    if (prev) {
        if (!prev_cam) return fail(HRT_ERR_INVALID, who + ": prev_cam is NULL but a d_prev_ pointer is given");
        if (!d_prev_color) return fail(HRT_ERR_INVALID, who + ": d_prev_color is NULL but prev_cam is given");
        if (!d_prev_features) return fail(HRT_ERR_INVALID, who + ": d_prev_features is NULL but prev_cam is given");
        if (!d_prev_history) return fail(HRT_ERR_INVALID, who + ": d_prev_history is NULL but prev_cam is given");
        if ((d_prev_color_half != nullptr) != (d_color_half != nullptr))
            return fail(HRT_ERR_INVALID, who + ": d_prev_color_half must be given exactly when d_color_half is");
    }
    const void *ins[] = {d_color, d_color_half, d_features, d_prev_color, d_prev_color_half, d_prev_features, d_prev_history};
    const void *outs[] = {d_out, d_out_half, d_history_out};
    for (const void *o : outs)
        for (const void *i : ins)
            if (o && o == i) return fail(HRT_ERR_INVALID, who + ": an output aliases an input");
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (outs[a] && outs[a] == outs[b]) return fail(HRT_ERR_INVALID, who + ": the outputs alias each other");
    DTemporal T;
    std::memset(&T, 0, sizeof(T));
    if ((rc = tp_camera(who, "cam", cam, T.cam)) != HRT_OK) return rc;
    if (prev) {
        DCamera unused;
        if ((rc = tp_camera(who, "prev_cam", prev_cam, unused)) != HRT_OK) return rc;
        const double rad = (double)prev_cam->fovy_deg / 2.0 * M_PI / 180.0;
        const double cot = std::cos(rad) / std::sin(rad);
        T.kx = (float)(cot / (double)prev_cam->aspect);
        T.ky = (float)cot;
        for (int k = 0; k < 3; ++k) {
            T.eye[k] = prev_cam->eye[k]; T.right[k] = prev_cam->right[k]; T.up[k] = prev_cam->up[k]; T.forward[k] = prev_cam->forward[k];
        }
        T.still = std::memcmp(cam, prev_cam, sizeof(hrt_camera)) == 0 ? 1u : 0u;
    }
    if (!d_history_out) return fail(HRT_ERR_INVALID, who + ": d_history_out is NULL");  // the last check: what gets here is valid but for this
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    T.w = w; T.h = h;
    T.has_prev = prev ? 1u : 0u;
    T.alpha_min = p->alpha_min; T.max_history = p->max_history;
    T.depth_tol = p->depth_tol; T.normal_tol = p->normal_tol; T.albedo_tol = p->albedo_tol;
    T.color = d_color; T.half = d_color_half; T.feat = d_features;
    T.pcolor = d_prev_color; T.phalf = d_prev_color_half; T.pfeat = d_prev_features; T.phist = d_prev_history;
    T.out = d_out; T.out_half = d_out_half; T.hist_out = d_history_out;
    const dim3 grid((w + HRT_DN_TILE - 1) / HRT_DN_TILE, (h + HRT_DN_TILE - 1) / HRT_DN_TILE), block(HRT_DN_TILE * HRT_DN_TILE);
    hipLaunchKernelGGL(d_color_half ? hrt_temporal_half_kernel : hrt_temporal_kernel, grid, block, 0, (hipStream_t)stream, T);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

// What one frame hands to the next.  Two sets of buffers: the frame reads set `cur` as the previous state and writes set 1 - cur.
struct hrt_history {
    hrt_scene *scene = nullptr;
    Scratch color[2], half[2], feat[2], len[2];
    int cur = 0;
    bool valid = false;   // set `cur` holds a frame
    uint32_t w = 0, h = 0;
    hrt_camera cam{};
};

int hrt_history_create(hrt_scene *scene, hrt_history **out) {
    const std::string who = "hrt_history_create";
    if (!out) return fail(HRT_ERR_INVALID, who + ": out is NULL");
    *out = nullptr;
    const int rc = enter_scene(who, scene, false);
    if (rc != HRT_OK) return rc;
    hrt_history *hist = new (std::nothrow) hrt_history;
    if (!hist) return fail(HRT_ERR_STATE, who + ": out of memory");
    hist->scene = scene;
    *out = hist;
    return HRT_OK;
}

void hrt_history_reset(hrt_history *hist) {
    if (hist) hist->valid = false;
}

// After hrt_shutdown the buffers are freed all the same, on whatever device is current, as hrt_scene_destroy frees a scene's (they
// used to be left behind).
void hrt_history_destroy(hrt_history *hist) {
    if (!hist) return;
    if (g_rt.ready && hist->scene) (void)use_device(hist->scene->device);
    delete hist;
}

int hrt_render_temporal(hrt_scene *s, hrt_history *hist, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp,
                        uint64_t seed, uint32_t flags, const hrt_temporal_params *tp, const hrt_denoise_var_params *dp, float *out_rgb,
                        float *out_history, hrt_stats *stats) {
    const std::string who = "hrt_render_temporal";
    DnFilter F{};
    int rc = tp_check_params(who, tp);
    if (rc == HRT_OK && dp) rc = dn_check_params(who, dp, F);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if (spp < 2u || (spp & 1u)) return fail(HRT_ERR_INVALID, who + ": spp must be even and at least 2 (got " + std::to_string(spp) + ")");
    if (feature_spp > spp) return fail(HRT_ERR_INVALID, who + ": feature_spp must be at most spp (got " + std::to_string(feature_spp) + " > " + std::to_string(spp) + ")");
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    if (!out_rgb) return fail(HRT_ERR_INVALID, who + ": out_rgb is NULL");
    if (!hist) return fail(HRT_ERR_INVALID, who + ": history is NULL");
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    if (hist->scene != s) return fail(HRT_ERR_INVALID, who + ": history belongs to another scene");
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t lin = flags & ~(uint32_t)HRT_FLAG_GAMMA;
    const size_t npix = (size_t)w * h, frame_bytes = npix * 3 * sizeof(float);
    if (hist->w != w || hist->h != h) hist->valid = false;  // another frame size: nothing to reproject
    const int prv = hist->cur, nxt = 1 - hist->cur;
    if ((rc = s->dn_frame.grow(frame_bytes)) != HRT_OK) return rc;
    if ((rc = s->dnv_frame_half.grow(frame_bytes)) != HRT_OK) return rc;
    if ((rc = s->dn_out.grow(frame_bytes)) != HRT_OK) return rc;
    if (dp && (rc = s->dn_scratch.grow(hrt_denoise_var_scratch_bytes(w, h))) != HRT_OK) return rc;
    if ((rc = hist->color[nxt].grow(frame_bytes)) != HRT_OK) return rc;
    if ((rc = hist->half[nxt].grow(frame_bytes)) != HRT_OK) return rc;
    if ((rc = hist->feat[nxt].grow(npix * HRT_FEATURE_FLOATS * sizeof(float))) != HRT_OK) return rc;
    if ((rc = hist->len[nxt].grow(npix * sizeof(float))) != HRT_OK) return rc;
    double ms_half = 0.0;
    float *const d_c = s->dn_frame.as<float>(), *const d_ch = s->dnv_frame_half.as<float>(), *const d_f = hist->feat[nxt].as<float>();
    float *const d_acc = hist->color[nxt].as<float>(), *const d_acch = hist->half[nxt].as<float>(), *const d_len = hist->len[nxt].as<float>();
    rc = dn_render_pair(s, cam, w, h, spp, seed, lin, d_c, d_ch, &ms_half);
    if (rc == HRT_OK) rc = features_launch(s, cam, w, h, 0, feature_spp, seed, d_f, nullptr);
    if (rc != HRT_OK) return rc;
    const bool prev = hist->valid;
    hist->valid = false;  // until this frame's state is complete
    rc = hrt_temporal_accumulate(cam, prev ? &hist->cam : nullptr, w, h, d_c, d_ch, d_f, prev ? hist->color[prv].as<float>() : nullptr,
                                 prev ? hist->half[prv].as<float>() : nullptr, prev ? hist->feat[prv].as<float>() : nullptr,
                                 prev ? hist->len[prv].as<float>() : nullptr, tp, d_acc, d_acch, d_len, nullptr);
    if (rc != HRT_OK) return rc;
    if (dp) {
        rc = dn_run(d_acc, d_acch, d_f, w, h, F, flags & HRT_FLAG_GAMMA, s->dn_scratch.p, s->dn_out.as<float>(), nullptr, nullptr);
        if (rc != HRT_OK) return rc;
    } else {  // the accumulated frame itself: hrt_finalize_tiles' arithmetic over the row-major frame, one sample
        const uint32_t n = (uint32_t)(npix * 3u);
        hipLaunchKernelGGL(hrt_finalize_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t) nullptr, (const float *)d_acc, s->dn_out.as<float>(), n,
                           1u, (flags & HRT_FLAG_GAMMA) ? 1u : 0u);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpy(out_rgb, s->dn_out.p, frame_bytes, hipMemcpyDeviceToHost));
    if (out_history) HIP_TRY(hipMemcpy(out_history, d_len, npix * sizeof(float), hipMemcpyDeviceToHost));
    hist->cur = nxt;
    hist->valid = true;
    hist->w = w; hist->h = h;
    hist->cam = *cam;
    if (stats) {
        double ms = 0.0;
        rc = hrt_last_kernel_ms(s, &ms);
        if (rc != HRT_OK) return rc;
        fill_stats(s, stats, t0, ms_half + ms, (uint64_t)w * h * spp);  // the trace launches' time
    }
    return HRT_OK;
}
