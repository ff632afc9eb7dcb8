// The variance-guided a-trous denoiser (include/hrt.h hrt_denoise_var, hrt_render_denoised_var): the filter of hrt_denoise.hip with
// a colour width per pair of pixels, the sum of the estimated variances of the two pixels' own means (Schied et al., SVGF, HPG 2017,
// without its temporal half).  Included by hrt_api.hip after hrt_denoise.hip, whose helpers (dn_finite, dn_div, dn_term, the checks, dn_grow) it uses and
// whose kernels it leaves alone.
//
// All on the caller's stream, the launch shape of hrt_dn_iter_kernel (16x16-pixel workgroups, one lane per pixel, taps from global
// memory):
//   hrt_dnv_prep_kernel     demodulates both frames (all samples, first half) and writes {x.rgb, v}: the variance rides in the fourth
//                           float of the colour record the taps load anyway, so an iteration reads no more bytes per tap than
//                           hrt_dn_iter_kernel; the guide records are those of hrt_dn_prep_kernel
//   hrt_dnv_pre_kernel      one launch per prefilter pass: v smoothed with the guide weights, x copied
//   hrt_dnv_iter_kernel     one launch per iteration: x filtered with the colour width of each pair of pixels, v carried along
//   hrt_dnv_last_kernel     the last iteration: remodulates, applies the gamma, writes the variance map if one is wanted
// The {x, v} records ping-pong between the two float4 buffers of the scratch; see hrt_denoise_var_scratch_bytes.

// Demodulated colour and variance of the mean {x.rgb, v}, and the guides {n.xyz, z}, {a.rgb, 0} of every pixel.
extern "C" __global__ void __launch_bounds__(256) hrt_dnv_prep_kernel(const float *__restrict__ color, const float *__restrict__ half,
                                                                      const float *__restrict__ feat, uint32_t npix, float4 *__restrict__ xbuf,
                                                                      float4 *__restrict__ guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float *f = feat + (size_t)i * HRT_FEATURE_FLOATS;
    const float *c = color + (size_t)i * 3u;
    const float *ch = half + (size_t)i * 3u;
    const float a0 = f[0], a1 = f[1], a2 = f[2];
    const float e0 = f[6] / 6.f, e1 = f[7] / 6.f, e2 = f[8] / 6.f;
    float x0 = dn_div(c[0] - e0, a0), x1 = dn_div(c[1] - e1, a1), x2 = dn_div(c[2] - e2, a2);
    const float h0 = dn_div(ch[0] - e0, a0), h1 = dn_div(ch[1] - e1, a1), h2 = dn_div(ch[2] - e2, a2);
    bool ok = dn_finite(x0) && dn_finite(x1) && dn_finite(x2) && dn_finite(h0) && dn_finite(h1) && dn_finite(h2);
    for (int k = 0; k < 10; ++k) ok = ok && dn_finite(f[k]);
    const float d0 = x0 - h0, d1 = x1 - h1, d2 = x2 - h2;
    float v = (d0 * d0 + d1 * d1) + d2 * d2;
    if (!ok) x0 = x1 = x2 = __builtin_nanf("");
    if (!ok || !dn_finite(v)) v = 0.f;
    xbuf[i] = make_float4(x0, x1, x2, v);
    guide[2 * (size_t)i] = make_float4(f[3], f[4], f[5], f[9]);
    guide[2 * (size_t)i + 1] = make_float4(a0, a1, a2, 0.f);
}

// The guide terms of the exponent between p and q: (T(normal) + T(albedo)) + T(depth).
__device__ __forceinline__ float dnv_guides(const float4 gp0, const float4 gp1, const float4 gq0, const float4 gq1, float den_n, float den_a,
                                            float sig_z) {
    const float dn0 = gp0.x - gq0.x, dn1 = gp0.y - gq0.y, dn2 = gp0.z - gq0.z;
    const float da0 = gp1.x - gq1.x, da1 = gp1.y - gq1.y, da2 = gp1.z - gq1.z;
    const float dz = gp0.w - gq0.w;
    const float zs = sig_z * fmaxf(fmaxf(gp0.w, gq0.w), 1e-3f);
    return (dn_term((dn0 * dn0 + dn1 * dn1) + dn2 * dn2, den_n) + dn_term((da0 * da0 + da1 * da1) + da2 * da2, den_a)) + dn_term(dz * dz, zs * zs);
}

// MODE 0: a prefilter pass (v only, guide weights), 1: an iteration, 2: the last iteration (remodulate, gamma, variance map).
extern "C++" {
template <int MODE>
__device__ __forceinline__ void dnv_pass(const float4 *__restrict__ xin, const float4 *__restrict__ guide, uint32_t w, uint32_t h,
                                         uint32_t step, float sv2, float vfloor, float den_n, float den_a, float sig_z,
                                         float4 *__restrict__ xout, const float *__restrict__ color, const float *__restrict__ feat,
                                         float *__restrict__ out, float *__restrict__ var_out, uint32_t gamma) {
    const uint32_t px = blockIdx.x * HRT_DN_TILE + (threadIdx.x % HRT_DN_TILE), py = blockIdx.y * HRT_DN_TILE + (threadIdx.x / HRT_DN_TILE);
    if (px >= w || py >= h) return;
    const size_t p = (size_t)py * w + px;
    const float4 xp = xin[p];
    float3 y = make_float3(xp.x, xp.y, xp.z);
    float vy = xp.w;
    if (dn_finite(xp.x) && dn_finite(xp.y) && dn_finite(xp.z)) {
        const float4 gp0 = guide[2 * p], gp1 = guide[2 * p + 1];
        const float hw[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, sv = 0.f;
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
                    float e = dnv_guides(gp0, gp1, gq0, gq1, den_n, den_a, sig_z);
                    if (MODE != 0) {
                        const float dx0 = xp.x - xq.x, dx1 = xp.y - xq.y, dx2 = xp.z - xq.z;
                        const float den_c = sv2 == __builtin_inff() ? sv2 : sv2 * ((xp.w + xq.w) + vfloor);  // the width of this pair
                        e = dn_term((dx0 * dx0 + dx1 * dx1) + dx2 * dx2, den_c) + e;
                    }
                    wq = hh * expf(-e);
                }
                sw = sw + wq;
                if (MODE == 0) {
                    sv = sv + wq * xq.w;
                } else {
                    s0 = s0 + wq * xq.x;
                    s1 = s1 + wq * xq.y;
                    s2 = s2 + wq * xq.z;
                    sv = sv + (wq * wq) * xq.w;
                }
            }
        }
        if (MODE == 0) {
            vy = sv / sw;
        } else {
            y = make_float3(s0 / sw, s1 / sw, s2 / sw);
            vy = sv / (sw * sw);
        }
    }
    if (MODE != 2) {
        xout[p] = make_float4(y.x, y.y, y.z, vy);
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
    if (var_out) var_out[p] = vy;
}
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dnv_pre_kernel(const float4 *__restrict__ xin, const float4 *__restrict__ guide,
                                                                                          uint32_t w, uint32_t h, uint32_t step, float den_n, float den_a,
                                                                                          float sig_z, float4 *__restrict__ xout) {
    dnv_pass<0>(xin, guide, w, h, step, 0.f, 0.f, den_n, den_a, sig_z, xout, nullptr, nullptr, nullptr, nullptr, 0u);
}
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dnv_iter_kernel(const float4 *__restrict__ xin, const float4 *__restrict__ guide,
                                                                                           uint32_t w, uint32_t h, uint32_t step, float sv2, float vfloor,
                                                                                           float den_n, float den_a, float sig_z, float4 *__restrict__ xout) {
    dnv_pass<1>(xin, guide, w, h, step, sv2, vfloor, den_n, den_a, sig_z, xout, nullptr, nullptr, nullptr, nullptr, 0u);
}
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dnv_last_kernel(const float4 *__restrict__ xin, const float4 *__restrict__ guide,
                                                                                           uint32_t w, uint32_t h, uint32_t step, float sv2, float vfloor,
                                                                                           float den_n, float den_a, float sig_z, const float *__restrict__ color,
                                                                                           const float *__restrict__ feat, float *__restrict__ out,
                                                                                           float *__restrict__ var_out, uint32_t gamma) {
    dnv_pass<2>(xin, guide, w, h, step, sv2, vfloor, den_n, den_a, sig_z, nullptr, color, feat, out, var_out, gamma);
}

static int dnv_check_params(const std::string &who, const hrt_denoise_var_params *p) {
    if (!p) return fail(HRT_ERR_INVALID, who + ": params is NULL");
    if (p->iterations < 1u || p->iterations > 8u)
        return fail(HRT_ERR_INVALID, who + ": iterations must be 1..8 (got " + std::to_string(p->iterations) + ")");
    if (p->prefilter > 4u) return fail(HRT_ERR_INVALID, who + ": prefilter must be 0..4 (got " + std::to_string(p->prefilter) + ")");
    const float sig[4] = {p->sigma_variance, p->sigma_normal, p->sigma_albedo, p->sigma_depth};
    const char *names[4] = {"sigma_variance", "sigma_normal", "sigma_albedo", "sigma_depth"};
    for (int k = 0; k < 4; ++k)
        if (std::isnan(sig[k]) || !(sig[k] > 0.f)) return fail(HRT_ERR_INVALID, who + ": " + names[k] + " must be > 0 (+inf switches the term off)");
    if (!std::isfinite(p->variance_floor) || p->variance_floor < 0.f) return fail(HRT_ERR_INVALID, who + ": variance_floor must be finite and >= 0");
    return HRT_OK;
}

size_t hrt_denoise_var_scratch_bytes(uint32_t w, uint32_t h) { return (size_t)w * h * 4u * sizeof(float4); }

static int dnv_run(const float *d_color, const float *d_half, const float *d_feat, uint32_t w, uint32_t h, const hrt_denoise_var_params *p,
                   uint32_t flags, void *d_scratch, float *d_out, float *d_var_out, hipStream_t stream) {
    const size_t npix = (size_t)w * h;
    float4 *guide = (float4 *)d_scratch, *xa = guide + 2 * npix, *xb = xa + npix;
    hipLaunchKernelGGL(hrt_dnv_prep_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, d_color, d_half, d_feat, (uint32_t)npix, xa,
                       guide);
    HIP_TRY(hipGetLastError());
    const dim3 grid((w + HRT_DN_TILE - 1) / HRT_DN_TILE, (h + HRT_DN_TILE - 1) / HRT_DN_TILE), block(HRT_DN_TILE * HRT_DN_TILE);
    const float den_n = p->sigma_normal * p->sigma_normal, den_a = p->sigma_albedo * p->sigma_albedo;
    const float sv2 = p->sigma_variance * p->sigma_variance;
    for (uint32_t i = 0; i < p->prefilter; ++i) {
        hipLaunchKernelGGL(hrt_dnv_pre_kernel, grid, block, 0, stream, (const float4 *)xa, (const float4 *)guide, w, h, 1u << i, den_n, den_a,
                           p->sigma_depth, xb);
        HIP_TRY(hipGetLastError());
        std::swap(xa, xb);
    }
    for (uint32_t i = 0; i < p->iterations; ++i) {
        const uint32_t step = 1u << i;
        if (i + 1 < p->iterations) {
            hipLaunchKernelGGL(hrt_dnv_iter_kernel, grid, block, 0, stream, (const float4 *)xa, (const float4 *)guide, w, h, step, sv2,
                               p->variance_floor, den_n, den_a, p->sigma_depth, xb);
            std::swap(xa, xb);
        } else {
            hipLaunchKernelGGL(hrt_dnv_last_kernel, grid, block, 0, stream, (const float4 *)xa, (const float4 *)guide, w, h, step, sv2,
                               p->variance_floor, den_n, den_a, p->sigma_depth, d_color, d_feat, d_out, d_var_out,
                               (flags & HRT_FLAG_GAMMA) ? 1u : 0u);
        }
        HIP_TRY(hipGetLastError());
    }
    return HRT_OK;
}

int hrt_denoise_var(const float *d_color, const float *d_color_half, const float *d_features, uint32_t w, uint32_t h,
                    const hrt_denoise_var_params *p, uint32_t flags, void *d_scratch, float *d_out, float *d_variance_out, void *stream) {
    const std::string who = "hrt_denoise_var";
    int rc = dnv_check_params(who, p);
    if (rc == HRT_OK) rc = dn_check_size(who, w, h);
    if (rc != HRT_OK) return rc;
    if (flags & ~(uint32_t)HRT_FLAG_GAMMA) return fail(HRT_ERR_INVALID, who + ": flags may hold HRT_FLAG_GAMMA only");
    if (!d_color) return fail(HRT_ERR_INVALID, who + ": d_color is NULL");
    if (!d_color_half) return fail(HRT_ERR_INVALID, who + ": d_color_half is NULL");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if (!d_scratch) return fail(HRT_ERR_INVALID, who + ": d_scratch is NULL");
    if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    return dnv_run(d_color, d_color_half, d_features, w, h, p, flags, d_scratch, d_out, d_variance_out, (hipStream_t)stream);
}

int hrt_render_denoised_var(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed,
                            uint32_t flags, const hrt_denoise_var_params *p, float *out_rgb, float *out_variance, hrt_stats *stats) {
    const std::string who = "hrt_render_denoised_var";
    int rc = dnv_check_params(who, p);
    if (rc == HRT_OK) rc = dn_check_size(who, w, h);
    if (rc != HRT_OK) return rc;
    if (spp < 2u || (spp & 1u)) return fail(HRT_ERR_INVALID, who + ": spp must be even and at least 2 (got " + std::to_string(spp) + ")");
    if (feature_spp > spp) return fail(HRT_ERR_INVALID, who + ": feature_spp must be at most spp (got " + std::to_string(feature_spp) + " > " + std::to_string(spp) + ")");
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    if (!out_rgb) return fail(HRT_ERR_INVALID, who + ": out_rgb is NULL");
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "render: call hrt_init first");
    { const int drc = use_device(s->device); if (drc != HRT_OK) return drc; }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t tiles = hrt_tiles_total(w, h), npix = (size_t)w * h, tile_bytes = tiles * 64 * 3 * sizeof(float);
    if (s->tiles_cap < tiles * 64 * 3) {  // hrt_render's tile buffer (its capacity is counted in floats): the running sums
        if (s->d_tiles) (void)hipFree(s->d_tiles);
        s->d_tiles = nullptr; s->tiles_cap = 0;
        HIP_TRY(hipMalloc((void **)&s->d_tiles, tile_bytes));
        s->tiles_cap = tiles * 64 * 3;
    }
    if ((rc = dn_grow((void **)&s->dnv_half_tiles, &s->dnv_half_tiles_cap, tile_bytes)) != HRT_OK) return rc;
    if ((rc = dn_grow((void **)&s->dn_frame, &s->dn_frame_cap, npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if ((rc = dn_grow((void **)&s->dnv_frame_half, &s->dnv_frame_half_cap, npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if ((rc = dn_grow((void **)&s->dn_feat, &s->dn_feat_cap, npix * HRT_FEATURE_FLOATS * sizeof(float))) != HRT_OK) return rc;
    if ((rc = dn_grow(&s->dn_scratch, &s->dn_scratch_cap, hrt_denoise_var_scratch_bytes(w, h))) != HRT_OK) return rc;
    if ((rc = dn_grow((void **)&s->dn_out, &s->dn_out_cap, npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if (out_variance && (rc = dn_grow((void **)&s->dnv_var, &s->dnv_var_cap, npix * sizeof(float))) != HRT_OK) return rc;
    // Sums of samples [0, spp/2), a copy of them, then [spp/2, spp) on top: the full sums are hrt_render's, bit for bit.
    const uint32_t lin = flags & ~(uint32_t)HRT_FLAG_GAMMA, half = spp / 2u;
    double ms_half = 0.0;
    HIP_TRY(hipMemsetAsync(s->d_tiles, 0, tile_bytes, nullptr));
    rc = hrt_render_accumulate(s, cam, w, h, 0, half, seed, lin, 0, 1, s->d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_last_kernel_ms(s, &ms_half);  // waits for the launch and checks it (hrt_check_last_launch)
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s->dnv_half_tiles, s->d_tiles, tile_bytes, hipMemcpyDeviceToDevice, nullptr));
    rc = hrt_render_accumulate(s, cam, w, h, half, spp - half, seed, lin, 0, 1, s->d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_check_last_launch(s);  // never denoise a frame the kernel did not finish
    if (rc == HRT_OK) rc = hrt_finalize_tiles(s->dnv_half_tiles, (uint32_t)tiles, half, 0, s->dnv_half_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_finalize_tiles(s->d_tiles, (uint32_t)tiles, spp, 0, s->d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_assemble_frame(s->dnv_half_tiles, (uint32_t)tiles, w, h, 1, s->dnv_frame_half, nullptr);
    if (rc == HRT_OK) rc = hrt_assemble_frame(s->d_tiles, (uint32_t)tiles, w, h, 1, s->dn_frame, nullptr);
    if (rc == HRT_OK) rc = features_launch(s, cam, w, h, 0, feature_spp, seed, s->dn_feat, nullptr);
    if (rc == HRT_OK) rc = dnv_run(s->dn_frame, s->dnv_frame_half, s->dn_feat, w, h, p, flags & HRT_FLAG_GAMMA, s->dn_scratch, s->dn_out,
                                   out_variance ? s->dnv_var : nullptr, nullptr);
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->dn_out, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_variance) HIP_TRY(hipMemcpy(out_variance, s->dnv_var, npix * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        double ms = 0.0;
        rc = hrt_last_kernel_ms(s, &ms);
        if (rc != HRT_OK) return rc;
        stats->kernel_ms = ms_half + ms;  // the two trace launches
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->samples = (uint64_t)w * h * spp;
        stats->vgprs = (uint32_t)g_rt.attr.numRegs;
        stats->lds_bytes = s->last_lds;
        stats->waves_launched = s->last_waves;
    }
    return HRT_OK;
}
