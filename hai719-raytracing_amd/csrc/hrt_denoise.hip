// Feature buffers and the edge-avoiding a-trous denoiser (include/hrt.h hrt_render_features, hrt_denoise, hrt_render_denoised).
// Included by hrt_api.hip inside its extern "C" block, after everything it builds on.
//
// Features: one lane per pixel.  Per sample it draws the camera ray exactly as the trace kernels do (rng.start, u, v, time,
// camera_ray), finds the first hit with closest_hit and shades it with shade() -- the device functions of hrt_aov_kernel -- and
// sums albedo, normal, emission, t and a hit count in sample order in fp32; the sums are divided by the count at the end.
//
// Denoiser (Dammertz et al., HPG 2010), all on the caller's stream:
//   hrt_dn_prep_kernel      demodulates the colour once (x = (c - e/6) / d) and packs each pixel's guides into two float4
//                           records {n.xyz, z} {a.rgb, 0}; a pixel whose x or guides are not finite gets x = NaN
//   hrt_dn_iter_kernel      one launch per iteration (step 2^i), 16x16-pixel workgroups, one lane per pixel: the 25 taps are read
//                           straight from global memory (colour record + two guide records, 48 bytes a tap) -- the guides of a
//                           1080p frame are 66 MB and stay in the Infinity Cache across iterations.  The last iteration
//                           remodulates (out = d*y + e/6) and applies the gamma.
// The colour ping-pongs between two float4 buffers of the scratch; see hrt_denoise_scratch_bytes.

#define HRT_DN_TILE 16u

// Sums of the first-hit features over samples [s0, s0 + n) of every pixel (n == 0: the pixel centre at time 0, hrt_aov_kernel's ray).
extern "C" __global__ void __launch_bounds__(256) hrt_features_kernel(const DRender R, uint32_t n, float *__restrict__ out) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R.w * R.h) return;
    const uint32_t x = idx % R.w, y = idx / R.w;
    Ctx cx;
    cx.S = (cscene)R.scene;
    cx.set_tables((gf4)cx.S->tabs, (gf1)c_u8_lut, cx.S);
    cx.lds = (lu4) nullptr;
    cx.lds_n = 0;  // every nodelet from global memory, as hrt_aov_kernel
    cx.err_abs = R.err_abs;
    cx.flags = R.flags;
    unsigned long long stamps_local[17] = {0};
    cx.st = stamps_local;
    const ccam cam = (ccam)R.cam;
    f3 alb = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f), emi = mk(0.f, 0.f, 0.f);
    float depth = 0.f, hits = 0.f;
    const uint32_t count = n ? n : 1u;
    for (uint32_t k = 0; k < count; ++k) {
        Ray ray;
        if (n == 0u) {
            ray = camera_ray(cam, ((float)x + 0.5f) / (float)R.w, ((float)y + 0.5f) / (float)R.h, 0.f);
        } else {  // the trace kernels' camera sample (main.cpp:188-192)
            Rng rng;
            rng.start(R.seed_lo, R.seed_hi, idx, R.s0 + k);
            const float u = ((float)x + rng.next()) / (float)R.w;
            const float v = ((float)y + rng.next()) / (float)R.h;
            const float tm = rng.next();
            ray = camera_ray(cam, u, v, tm);
        }
        const Hit h = closest_hit(cx, ray);
        if (h.kind) {
            const Surface sf = shade(cx, ray, h);
            alb = alb + sf.albedo;
            nrm = nrm + sf.n;
            emi = emi + sf.emission;
            depth = depth + h.t;
            hits = hits + 1.f;
        }
    }
    const float c = (float)count;
    float *o = out + (size_t)idx * HRT_FEATURE_FLOATS;
    o[0] = alb.x / c; o[1] = alb.y / c; o[2] = alb.z / c;
    o[3] = nrm.x / c; o[4] = nrm.y / c; o[5] = nrm.z / c;
    o[6] = emi.x / c; o[7] = emi.y / c; o[8] = emi.z / c;
    o[9] = depth / c; o[10] = hits / c; o[11] = 0.f;
}

__device__ __forceinline__ bool dn_finite(float v) { return __builtin_isfinite(v); }
__device__ __forceinline__ float dn_div(float a, float d) { return d > 0.f ? a / d : a; }  // demodulation divisor: albedo if > 0, else 1

// Demodulated colour (x.rgb, 0) and guides {n.xyz, z}, {a.rgb, 0} of every pixel.
extern "C" __global__ void __launch_bounds__(256) hrt_dn_prep_kernel(const float *__restrict__ color, const float *__restrict__ feat,
                                                                     uint32_t npix, float4 *__restrict__ xbuf, float4 *__restrict__ guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float *f = feat + (size_t)i * HRT_FEATURE_FLOATS;
    const float *c = color + (size_t)i * 3u;
    const float a0 = f[0], a1 = f[1], a2 = f[2];
    float x0 = dn_div(c[0] - f[6] / 6.f, a0), x1 = dn_div(c[1] - f[7] / 6.f, a1), x2 = dn_div(c[2] - f[8] / 6.f, a2);
    bool ok = dn_finite(x0) && dn_finite(x1) && dn_finite(x2);
    for (int k = 0; k < 10; ++k) ok = ok && dn_finite(f[k]);
    if (!ok) x0 = x1 = x2 = __builtin_nanf("");
    xbuf[i] = make_float4(x0, x1, x2, 0.f);
    guide[2 * (size_t)i] = make_float4(f[3], f[4], f[5], f[9]);
    guide[2 * (size_t)i + 1] = make_float4(a0, a1, a2, 0.f);
}

// One term of the exponent: 0 when the difference is 0 or the term is switched off (den = +inf), else num / den.
__device__ __forceinline__ float dn_term(float num, float den) { return (num == 0.f || den == __builtin_inff()) ? 0.f : num / den; }

// Iteration i of the filter (step s = 2^i) over x_in.  LAST: remodulate and write the rgb output (gamma with `gamma`).
extern "C++" {
template <bool LAST>
__device__ __forceinline__ void dn_iter(const float4 *__restrict__ xin, const float4 *__restrict__ guide, uint32_t w, uint32_t h,
                                        uint32_t step, float den_c, float den_n, float den_a, float sig_z, float4 *__restrict__ xout,
                                        const float *__restrict__ color, const float *__restrict__ feat, float *__restrict__ out, uint32_t gamma) {
    const uint32_t px = blockIdx.x * HRT_DN_TILE + (threadIdx.x % HRT_DN_TILE), py = blockIdx.y * HRT_DN_TILE + (threadIdx.x / HRT_DN_TILE);
    if (px >= w || py >= h) return;
    const size_t p = (size_t)py * w + px;
    const float4 xp = xin[p];
    float3 y = make_float3(xp.x, xp.y, xp.z);
    if (dn_finite(xp.x) && dn_finite(xp.y) && dn_finite(xp.z)) {
        const float4 gp0 = guide[2 * p], gp1 = guide[2 * p + 1];
        const float hw[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int k = -2; k <= 2; ++k) {
            const int qy = (int)py + k * (int)step;
            if (qy < 0 || qy >= (int)h) continue;
            for (int j = -2; j <= 2; ++j) {
                const int qx = (int)px + j * (int)step;
                if (qx < 0 || qx >= (int)w) continue;
                const float hh = hw[j + 2] * hw[k + 2];
                float wq;
                float4 xq;
                if (j == 0 && k == 0) {
                    xq = xp;
                    wq = hh;
                } else {
                    const size_t q = (size_t)qy * w + qx;
                    xq = xin[q];
                    if (!(dn_finite(xq.x) && dn_finite(xq.y) && dn_finite(xq.z))) continue;
                    const float4 gq0 = guide[2 * q], gq1 = guide[2 * q + 1];
                    const float dx0 = xp.x - xq.x, dx1 = xp.y - xq.y, dx2 = xp.z - xq.z;
                    const float dn0 = gp0.x - gq0.x, dn1 = gp0.y - gq0.y, dn2 = gp0.z - gq0.z;
                    const float da0 = gp1.x - gq1.x, da1 = gp1.y - gq1.y, da2 = gp1.z - gq1.z;
                    const float dz = gp0.w - gq0.w;
                    const float zs = sig_z * fmaxf(fmaxf(gp0.w, gq0.w), 1e-3f);
                    const float e = ((dn_term((dx0 * dx0 + dx1 * dx1) + dx2 * dx2, den_c) + dn_term((dn0 * dn0 + dn1 * dn1) + dn2 * dn2, den_n)) +
                                     dn_term((da0 * da0 + da1 * da1) + da2 * da2, den_a)) + dn_term(dz * dz, zs * zs);
                    wq = hh * expf(-e);
                }
                sw = sw + wq;
                s0 = s0 + wq * xq.x;
                s1 = s1 + wq * xq.y;
                s2 = s2 + wq * xq.z;
            }
        }
        y = make_float3(s0 / sw, s1 / sw, s2 / sw);
    }
    if (!LAST) {
        xout[p] = make_float4(y.x, y.y, y.z, 0.f);
        return;
    }
    const float *f = feat + p * HRT_FEATURE_FLOATS;
    const float *c = color + p * 3u;
    float r[3] = {y.x, y.y, y.z};
    bool fin = true;
    for (int k = 0; k < 3; ++k) {
        const float d = f[k] > 0.f ? f[k] : 1.f;
        r[k] = d * r[k] + f[6 + k] / 6.f;
        fin = fin && dn_finite(r[k]);
    }
    for (int k = 0; k < 3; ++k) {
        const float v = fin ? r[k] : c[k];  // a pixel whose result is not finite is written through as its input
        out[p * 3u + k] = gamma ? (float)pow((double)v, 1.0 / 2.2) : v;
    }
}
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dn_iter_kernel(const float4 *__restrict__ xin, const float4 *__restrict__ guide,
                                                                                          uint32_t w, uint32_t h, uint32_t step, float den_c, float den_n,
                                                                                          float den_a, float sig_z, float4 *__restrict__ xout) {
    dn_iter<false>(xin, guide, w, h, step, den_c, den_n, den_a, sig_z, xout, nullptr, nullptr, nullptr, 0u);
}
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dn_last_kernel(const float4 *__restrict__ xin, const float4 *__restrict__ guide,
                                                                                          uint32_t w, uint32_t h, uint32_t step, float den_c, float den_n,
                                                                                          float den_a, float sig_z, const float *__restrict__ color,
                                                                                          const float *__restrict__ feat, float *__restrict__ out, uint32_t gamma) {
    dn_iter<true>(xin, guide, w, h, step, den_c, den_n, den_a, sig_z, nullptr, color, feat, out, gamma);
}

// Checks shared by the entry points; `who` names the entry point in the message.
static int dn_check_params(const std::string &who, const hrt_denoise_params *p) {
    if (!p) return fail(HRT_ERR_INVALID, who + ": params is NULL");
    if (p->iterations < 1u || p->iterations > 8u)
        return fail(HRT_ERR_INVALID, who + ": iterations must be 1..8 (got " + std::to_string(p->iterations) + ")");
    const float sig[4] = {p->sigma_color, p->sigma_normal, p->sigma_albedo, p->sigma_depth};
    const char *names[4] = {"sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"};
    for (int k = 0; k < 4; ++k)
        if (std::isnan(sig[k]) || !(sig[k] > 0.f)) return fail(HRT_ERR_INVALID, who + ": " + names[k] + " must be > 0 (+inf switches the term off)");
    return HRT_OK;
}
static int dn_check_size(const std::string &who, uint32_t w, uint32_t h) {
    if (!w || !h) return fail(HRT_ERR_INVALID, who + ": w and h must be positive");
    if ((uint64_t)w * h > 0x7fffffffull / 16u) return fail(HRT_ERR_INVALID, who + ": image too large");
    return HRT_OK;
}

size_t hrt_denoise_scratch_bytes(uint32_t w, uint32_t h) { return (size_t)w * h * 4u * sizeof(float4); }

static int dn_run(const float *d_color, const float *d_feat, uint32_t w, uint32_t h, const hrt_denoise_params *p, uint32_t flags,
                  void *d_scratch, float *d_out, hipStream_t stream) {
    const size_t npix = (size_t)w * h;
    float4 *guide = (float4 *)d_scratch, *xa = guide + 2 * npix, *xb = xa + npix;
    hipLaunchKernelGGL(hrt_dn_prep_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, d_color, d_feat, (uint32_t)npix, xa, guide);
    HIP_TRY(hipGetLastError());
    const dim3 grid((w + HRT_DN_TILE - 1) / HRT_DN_TILE, (h + HRT_DN_TILE - 1) / HRT_DN_TILE), block(HRT_DN_TILE * HRT_DN_TILE);
    const float den_n = p->sigma_normal * p->sigma_normal, den_a = p->sigma_albedo * p->sigma_albedo;
    for (uint32_t i = 0; i < p->iterations; ++i) {
        const float sc = p->sigma_color * std::ldexp(1.f, -(int)i);  // sigma_c 2^-i: the colour term tightens every iteration
        const uint32_t step = 1u << i;
        if (i + 1 < p->iterations) {
            hipLaunchKernelGGL(hrt_dn_iter_kernel, grid, block, 0, stream, (const float4 *)xa, (const float4 *)guide, w, h, step, sc * sc,
                               den_n, den_a, p->sigma_depth, xb);
            std::swap(xa, xb);
        } else {
            hipLaunchKernelGGL(hrt_dn_last_kernel, grid, block, 0, stream, (const float4 *)xa, (const float4 *)guide, w, h, step, sc * sc,
                               den_n, den_a, p->sigma_depth, d_color, d_feat, d_out, (flags & HRT_FLAG_GAMMA) ? 1u : 0u);
        }
        HIP_TRY(hipGetLastError());
    }
    return HRT_OK;
}

int hrt_denoise(const float *d_color, const float *d_features, uint32_t w, uint32_t h, const hrt_denoise_params *p, uint32_t flags,
                void *d_scratch, float *d_out, void *stream) {
    const std::string who = "hrt_denoise";
    int rc = dn_check_params(who, p);
    if (rc == HRT_OK) rc = dn_check_size(who, w, h);
    if (rc != HRT_OK) return rc;
    if (flags & ~(uint32_t)HRT_FLAG_GAMMA) return fail(HRT_ERR_INVALID, who + ": flags may hold HRT_FLAG_GAMMA only");
    if (!d_color) return fail(HRT_ERR_INVALID, who + ": d_color is NULL");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if (!d_scratch) return fail(HRT_ERR_INVALID, who + ": d_scratch is NULL");
    if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    return dn_run(d_color, d_features, w, h, p, flags, d_scratch, d_out, (hipStream_t)stream);
}

// Feature launch on `stream`: the camera goes into the scene's feature block (its own: a trace launch on another stream may still
// read s->d_cam).  Feature launches of one scene are ordered: one on another stream first waits for the previous one.
static int features_launch(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                           uint64_t seed, float *d_features, hipStream_t stream) {
    DRender R;
    DCamera C;
    int rc = fill_render(s, cam, w, h, 1, seed, 0, 0, 1, R, C);
    if (rc != HRT_OK) return rc;
    if (!s->d_cam_feat) HIP_TRY(hipMalloc((void **)&s->d_cam_feat, sizeof(DCamera)));
    if (!s->ev_feat) HIP_TRY(hipEventCreateWithFlags(&s->ev_feat, hipEventDisableTiming));
    if (s->feat_used && s->feat_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, s->ev_feat, 0));
    s->h_cam_feat = C;
    HIP_TRY(hipMemcpyAsync(s->d_cam_feat, &s->h_cam_feat, sizeof(C), hipMemcpyHostToDevice, stream));
    R.cam = s->d_cam_feat;
    R.s0 = first_sample;
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_features_kernel, dim3((npix + 255) / 256), dim3(256), 0, stream, R, n_samples, d_features);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev_feat, stream));
    s->feat_used = true;
    s->feat_stream = stream;
    return HRT_OK;
}

int hrt_render_features(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                        uint64_t seed, float *d_features, void *stream) {
    const std::string who = "hrt_render_features";
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    int rc = dn_check_size(who, w, h);
    if (rc != HRT_OK) return rc;
    if ((uint64_t)first_sample + n_samples > 0xffffffffull) return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples overflows 32 bits");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    return features_launch(s, cam, w, h, first_sample, n_samples, seed, d_features, (hipStream_t)stream);
}

// Grows one scratch buffer of the scene to `bytes`.
static int dn_grow(void **ptr, size_t *cap, size_t bytes) {
    if (*cap >= bytes) return HRT_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr; *cap = 0;
    HIP_TRY(hipMalloc(ptr, bytes));
    *cap = bytes;
    return HRT_OK;
}

int hrt_render_denoised(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed,
                        uint32_t flags, const hrt_denoise_params *p, float *out_rgb, hrt_stats *stats) {
    const std::string who = "hrt_render_denoised";
    int rc = dn_check_params(who, p);
    if (rc == HRT_OK) rc = dn_check_size(who, w, h);
    if (rc != HRT_OK) return rc;
    if (!spp) return fail(HRT_ERR_INVALID, who + ": spp must be positive");
    if (feature_spp > spp) return fail(HRT_ERR_INVALID, who + ": feature_spp must be at most spp (got " + std::to_string(feature_spp) + " > " + std::to_string(spp) + ")");
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    if (!out_rgb) return fail(HRT_ERR_INVALID, who + ": out_rgb is NULL");
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "render: call hrt_init first");
    { const int drc = use_device(s->device); if (drc != HRT_OK) return drc; }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t tiles = hrt_tiles_total(w, h), npix = (size_t)w * h;
    if (s->tiles_cap < tiles * 64 * 3) {  // hrt_render's tile buffer (its capacity is counted in floats)
        if (s->d_tiles) (void)hipFree(s->d_tiles);
        s->d_tiles = nullptr; s->tiles_cap = 0;
        HIP_TRY(hipMalloc((void **)&s->d_tiles, tiles * 64 * 3 * sizeof(float)));
        s->tiles_cap = tiles * 64 * 3;
    }
    if ((rc = dn_grow((void **)&s->dn_frame, &s->dn_frame_cap, npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if ((rc = dn_grow((void **)&s->dn_feat, &s->dn_feat_cap, npix * HRT_FEATURE_FLOATS * sizeof(float))) != HRT_OK) return rc;
    if ((rc = dn_grow(&s->dn_scratch, &s->dn_scratch_cap, hrt_denoise_scratch_bytes(w, h))) != HRT_OK) return rc;
    if ((rc = dn_grow((void **)&s->dn_out, &s->dn_out_cap, npix * 3 * sizeof(float))) != HRT_OK) return rc;
    rc = hrt_render_tiles(s, cam, w, h, spp, seed, flags & ~(uint32_t)HRT_FLAG_GAMMA, 0, 1, s->d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_assemble_frame(s->d_tiles, (uint32_t)tiles, w, h, 1, s->dn_frame, nullptr);
    if (rc == HRT_OK) rc = hrt_check_last_launch(s);  // never denoise a frame the kernel did not finish
    if (rc == HRT_OK) rc = features_launch(s, cam, w, h, 0, feature_spp, seed, s->dn_feat, nullptr);
    if (rc == HRT_OK) rc = dn_run(s->dn_frame, s->dn_feat, w, h, p, flags & HRT_FLAG_GAMMA, s->dn_scratch, s->dn_out, nullptr);
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->dn_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        double ms = 0.0;
        rc = hrt_last_kernel_ms(s, &ms);
        if (rc != HRT_OK) return rc;
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->samples = (uint64_t)w * h * spp;
        stats->vgprs = (uint32_t)g_rt.attr.numRegs;
        stats->lds_bytes = s->last_lds;
        stats->waves_launched = s->last_waves;
    }
    return HRT_OK;
}
