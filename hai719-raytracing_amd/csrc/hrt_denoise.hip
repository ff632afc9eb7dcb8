// Feature buffers and the edge-avoiding a-trous denoiser (include/hrt.h hrt_render_features, hrt_denoise, hrt_render_denoised).
// Included by hrt_api.hip inside its extern "C" block, after everything it builds on.
//
// Features: one lane per pixel.  Per sample it draws the camera ray exactly as the trace kernels do (camera_sample), finds
// the first hit with closest_hit and shades it with shade() -- the device functions of hrt_aov_kernel -- and
// sums albedo, normal, emission, t and a hit count in sample order in fp32; the sums are divided by the count at the end.
//
// Denoisers, all on the caller's stream: the edge-avoiding a-trous filter (Dammertz et al., HPG 2010; hrt_denoise) and the same
// filter with a colour width per pair of pixels, the sum of the estimated variances of the two pixels' own means (Schied et al.,
// SVGF, HPG 2017, without its temporal half; hrt_denoise_var).  One prep template (dn_prep), one pass template (dn_pass), one
// ping-pong loop (dn_run) and one render scaffold (dn_render) serve both:
//   hrt_dn_prep_kernel      demodulates the colour once (x = (c - e/6) / d) and packs each pixel's guides into two float4
//   hrt_dnv_prep_kernel     records {n.xyz, z} {a.rgb, 0}; a pixel whose x or guides are not finite gets x = NaN.  The colour
//                           record is {x.rgb, v}: v = 0, or with the first half's frame the variance of the mean, which so rides
//                           in the float the taps load anyway
//   hrt_dnv_pre_kernel      one launch per prefilter pass: v smoothed with the guide weights, x copied
//   hrt_dn_iter_kernel      one launch per iteration (step 2^i), 16x16-pixel workgroups, one lane per pixel: the 25 taps are read
//   hrt_dnv_iter_kernel     straight from global memory (colour record + two guide records, 48 bytes a tap) -- the guides of a
//                           1080p frame are 66 MB and stay in the Infinity Cache across iterations; v is carried along
//   hrt_dn_last_kernel      the last iteration also remodulates (out = d*y + e/6), applies the gamma and, variance-guided, writes
//   hrt_dnv_last_kernel     the variance map if one is wanted
// The colour records ping-pong between two float4 buffers of the scratch; see hrt_denoise_scratch_bytes.

#define HRT_DN_TILE 16u

// Sample `sample` of pixel `pixel` of a w x h frame as the trace kernels draw it (main.cpp:188-192): draws 0..2 of the stream
// (seed, pixel, sample) are u, v and the time.  CP: where the camera block is read from (see camera_ray).
extern "C++" {
template <class CP>
__device__ __forceinline__ hrtk::Ray camera_sample(CP cam, uint32_t seed_lo, uint32_t seed_hi, uint32_t w, uint32_t h, uint32_t pixel, uint32_t sample) {
    const uint32_t x = pixel % w, y = pixel / w;
    hrtk::Rng rng;
    rng.start(seed_lo, seed_hi, pixel, sample);
    const float u = ((float)x + rng.next()) / (float)w;
    const float v = ((float)y + rng.next()) / (float)h;
    const float tm = rng.next();
    return hrtk::camera_ray<false>(cam, u, v, tm);
}
}  // extern "C++"

// Where features_body's rays come from: source(cx, R, n, idx, k, ray) makes the ray of pixel idx for the k-th sample of the launch
// (n == 0: the pixel centre at time 0) and returns false for a sample that is not traced, which counts as a miss; a source may set
// the context's margin for its ray.  FeatureCameraRays: the render's camera, the block R.cam points at.
extern "C++" {
struct FeatureCameraRays {
    __device__ __forceinline__ uint32_t items(const DRender &R) const { return R.w * R.h; }
    template <class CX>
    __device__ __forceinline__ bool operator()(CX &, const DRender &R, uint32_t n, uint32_t idx, uint32_t k, hrtk::Ray &ray) const {
        const ccam cam = (ccam)R.cam;
        if (n == 0u) {
            const uint32_t x = idx % R.w, y = idx / R.w;
            ray = hrtk::camera_ray(cam, ((float)x + 0.5f) / (float)R.w, ((float)y + 0.5f) / (float)R.h, 0.f);
        } else {
            ray = camera_sample(cam, R.seed_lo, R.seed_hi, R.w, R.h, idx, R.s0 + k);
        }
        return true;
    }
};

// Sums of the first-hit features over samples [s0, s0 + n) of every pixel (n == 0: the pixel centre at time 0, hrt_aov_kernel's ray).
// One lane per item, source.items(R) of them: the pixels of the frame, or for a source that maps an item to a pixel of one of
// several frames (LensViewFeatureRays, hrt_lens.hip) the pixels of all of them; record idx of `out` is item idx's.
template <class CX, class SRC>
__device__ __forceinline__ void features_body(const DRender &R, uint32_t n, float *__restrict__ out, const SRC &source) {
    using namespace hrtk;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= source.items(R)) return;
    CX cx;
    cx.S = (cscene)R.scene;
    cx.set_tables((gf4)cx.S->tabs, (gf1)c_u8_lut, cx.S);
    cx.lds = (lu4) nullptr;
    cx.lds_n = 0;  // every nodelet from global memory, as hrt_aov_kernel
    cx.err_abs = R.err_abs;
    cx.flags = R.flags;
    unsigned long long stamps_local[17] = {0};
    cx.st = stamps_local;
    f3 alb = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f), emi = mk(0.f, 0.f, 0.f);
    float depth = 0.f, hits = 0.f;
    const uint32_t count = n ? n : 1u;
    for (uint32_t k = 0; k < count; ++k) {
        Ray ray;
        Hit h;
        h.kind = 0u;
        if (source(cx, R, n, idx, k, ray)) h = closest_hit(cx, ray);
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
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(256) hrt_features_kernel(const DRender R, uint32_t n, float *__restrict__ out) {
    features_body<Ctx>(R, n, out, FeatureCameraRays{});
}

__device__ __forceinline__ bool dn_finite(float v) { return __builtin_isfinite(v); }
__device__ __forceinline__ float dn_div(float a, float d) { return d > 0.f ? a / d : a; }  // demodulation divisor: albedo if > 0, else 1
// One term of the exponent: 0 when the difference is 0 or the term is switched off (den = +inf), else num / den.
__device__ __forceinline__ float dn_term(float num, float den) { return (num == 0.f || den == __builtin_inff()) ? 0.f : num / den; }
// Steps 1 and 3 of THE FILTER for one channel (albedo a, e6 = emission / 6), shared with hrt_temporal.hip: x = (c - e/6) / d and back.
__device__ __forceinline__ float dn_demodulate(float c, float e6, float a) { return dn_div(c - e6, a); }
__device__ __forceinline__ float dn_remodulate(float y, float e, float a) {
    const float d = a > 0.f ? a : 1.f;
    return d * y + e / 6.f;
}

// The arguments of one pass of the filter over the colour records xin, the same list for every pass kernel.  cw: the colour term's
// denominator sigma_c^2, or variance-guided sigma_v^2, which the pair's variances and vfloor then scale.  A pass that is not the
// last writes xout; the last one reads color and feat again and writes out (and var_out, if it is wanted).
#define HRT_DN_PASS_PARAMS                                                                                                            \
    const float4 *__restrict__ xin, const float4 *__restrict__ guide, uint32_t w, uint32_t h, uint32_t step, float cw, float vfloor,   \
        float den_n, float den_a, float sig_z, float4 *__restrict__ xout, const float *__restrict__ color, const float *__restrict__ feat, \
        float *__restrict__ out, float *__restrict__ var_out, uint32_t gamma
#define HRT_DN_PASS_ARGS xin, guide, w, h, step, cw, vfloor, den_n, den_a, sig_z, xout, color, feat, out, var_out, gamma

extern "C++" {
// Demodulated colour {x.rgb, v} and guides {n.xyz, z}, {a.rgb, 0} of every pixel.  VAR: v is the variance of the mean, estimated
// from the frame of the first half of the samples; else 0.
template <bool VAR>
__device__ __forceinline__ void dn_prep(const float *__restrict__ color, const float *__restrict__ half, const float *__restrict__ feat,
                                        uint32_t npix, float4 *__restrict__ xbuf, float4 *__restrict__ guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float *f = feat + (size_t)i * HRT_FEATURE_FLOATS;
    const float *c = color + (size_t)i * 3u;
    const float a0 = f[0], a1 = f[1], a2 = f[2];
    const float e0 = f[6] / 6.f, e1 = f[7] / 6.f, e2 = f[8] / 6.f;
    float x0 = dn_demodulate(c[0], e0, a0), x1 = dn_demodulate(c[1], e1, a1), x2 = dn_demodulate(c[2], e2, a2);
    bool ok = dn_finite(x0) && dn_finite(x1) && dn_finite(x2);
    float v = 0.f;
    if (VAR) {
        const float *ch = half + (size_t)i * 3u;
        const float h0 = dn_demodulate(ch[0], e0, a0), h1 = dn_demodulate(ch[1], e1, a1), h2 = dn_demodulate(ch[2], e2, a2);
        ok = ok && dn_finite(h0) && dn_finite(h1) && dn_finite(h2);
        const float d0 = x0 - h0, d1 = x1 - h1, d2 = x2 - h2;
        v = (d0 * d0 + d1 * d1) + d2 * d2;
    }
    for (int k = 0; k < 10; ++k) ok = ok && dn_finite(f[k]);
    if (!ok) x0 = x1 = x2 = __builtin_nanf("");
    if (!ok || !dn_finite(v)) v = 0.f;
    xbuf[i] = make_float4(x0, x1, x2, v);
    guide[2 * (size_t)i] = make_float4(f[3], f[4], f[5], f[9]);
    guide[2 * (size_t)i + 1] = make_float4(a0, a1, a2, 0.f);
}

// MODE 0: a prefilter pass (VAR only: v smoothed with the guide weights, x copied), 1: an iteration, 2: the last iteration
// (remodulate, gamma, variance map).  The two filters associate the exponent differently -- fixed-width ((Tc + Tn) + Ta) + Tz,
// variance-guided Tc + ((Tn + Ta) + Tz) -- and both are pinned bit for bit: every expression below keeps its variant's order.
template <bool VAR, int MODE>
__device__ __forceinline__ void dn_pass(HRT_DN_PASS_PARAMS) {
    const uint32_t px = blockIdx.x * HRT_DN_TILE + (threadIdx.x % HRT_DN_TILE), py = blockIdx.y * HRT_DN_TILE + (threadIdx.x / HRT_DN_TILE);
    if (px >= w || py >= h) return;
    const size_t p = (size_t)py * w + px;
    const float4 xp = xin[p];
    float3 y = make_float3(xp.x, xp.y, xp.z);
    float vy = VAR ? xp.w : 0.f;
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
                    float tc = 0.f;
                    if (MODE != 0) {
                        const float dx0 = xp.x - xq.x, dx1 = xp.y - xq.y, dx2 = xp.z - xq.z;
                        const float den_c = (!VAR || cw == __builtin_inff()) ? cw : cw * ((xp.w + xq.w) + vfloor);  // the width of this pair
                        tc = dn_term((dx0 * dx0 + dx1 * dx1) + dx2 * dx2, den_c);
                    }
                    const float dn0 = gp0.x - gq0.x, dn1 = gp0.y - gq0.y, dn2 = gp0.z - gq0.z;
                    const float da0 = gp1.x - gq1.x, da1 = gp1.y - gq1.y, da2 = gp1.z - gq1.z;
                    const float dz = gp0.w - gq0.w;
                    const float zs = sig_z * fmaxf(fmaxf(gp0.w, gq0.w), 1e-3f);
                    const float tn = dn_term((dn0 * dn0 + dn1 * dn1) + dn2 * dn2, den_n), ta = dn_term((da0 * da0 + da1 * da1) + da2 * da2, den_a);
                    const float tz = dn_term(dz * dz, zs * zs);
                    float e;
                    if (MODE == 0) {
                        e = (tn + ta) + tz;
                    } else {
                        e = VAR ? tc + ((tn + ta) + tz) : ((tc + tn) + ta) + tz;
                    }
                    wq = hh * expf(-e);
                }
                sw = sw + wq;
                if (MODE != 0) {
                    s0 = s0 + wq * xq.x;
                    s1 = s1 + wq * xq.y;
                    s2 = s2 + wq * xq.z;
                }
                if (VAR) sv = sv + (MODE == 0 ? wq : wq * wq) * xq.w;
            }
        }
        if (MODE != 0) y = make_float3(s0 / sw, s1 / sw, s2 / sw);
        if (VAR) vy = sv / (MODE == 0 ? sw : sw * sw);
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
        r[k] = dn_remodulate(r[k], f[6 + k], f[k]);
        fin = fin && dn_finite(r[k]);
    }
    for (int k = 0; k < 3; ++k) {
        const float v = fin ? r[k] : c[k];  // a pixel whose result is not finite is written through as its input
        out[p * 3u + k] = gamma ? (float)pow((double)v, 1.0 / 2.2) : v;
    }
    if (VAR && var_out) var_out[p] = vy;
}
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(256) hrt_dn_prep_kernel(const float *__restrict__ color, const float *__restrict__ feat, uint32_t npix,
                                                                     float4 *__restrict__ xbuf, float4 *__restrict__ guide) {
    dn_prep<false>(color, nullptr, feat, npix, xbuf, guide);
}
extern "C" __global__ void __launch_bounds__(256) hrt_dnv_prep_kernel(const float *__restrict__ color, const float *__restrict__ half,
                                                                      const float *__restrict__ feat, uint32_t npix, float4 *__restrict__ xbuf,
                                                                      float4 *__restrict__ guide) {
    dn_prep<true>(color, half, feat, npix, xbuf, guide);
}
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dn_iter_kernel(HRT_DN_PASS_PARAMS) { dn_pass<false, 1>(HRT_DN_PASS_ARGS); }
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dn_last_kernel(HRT_DN_PASS_PARAMS) { dn_pass<false, 2>(HRT_DN_PASS_ARGS); }
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dnv_pre_kernel(HRT_DN_PASS_PARAMS) { dn_pass<true, 0>(HRT_DN_PASS_ARGS); }
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dnv_iter_kernel(HRT_DN_PASS_PARAMS) { dn_pass<true, 1>(HRT_DN_PASS_ARGS); }
extern "C" __global__ void __launch_bounds__(HRT_DN_TILE *HRT_DN_TILE) hrt_dnv_last_kernel(HRT_DN_PASS_PARAMS) { dn_pass<true, 2>(HRT_DN_PASS_ARGS); }

// The parameters of either filter (hrt_denoise_params, hrt_denoise_var_params).  sigma_c: sigma_color, or sigma_variance when var.
struct DnFilter {
    bool var;
    uint32_t iterations, prefilter;
    float sigma_c, sigma_n, sigma_a, sigma_z, vfloor;
};
// Checks shared by the entry points; `who` names the entry point in the message.
static int dn_check_filter(const std::string &who, const DnFilter &F) {
    if (F.iterations < 1u || F.iterations > 8u)
        return fail(HRT_ERR_INVALID, who + ": iterations must be 1..8 (got " + std::to_string(F.iterations) + ")");
    if (F.prefilter > 4u) return fail(HRT_ERR_INVALID, who + ": prefilter must be 0..4 (got " + std::to_string(F.prefilter) + ")");
    const float sig[4] = {F.sigma_c, F.sigma_n, F.sigma_a, F.sigma_z};
    const char *names[4] = {F.var ? "sigma_variance" : "sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"};
    for (int k = 0; k < 4; ++k)
        if (std::isnan(sig[k]) || !(sig[k] > 0.f)) return fail(HRT_ERR_INVALID, who + ": " + names[k] + " must be > 0 (+inf switches the term off)");
    if (!std::isfinite(F.vfloor) || F.vfloor < 0.f) return fail(HRT_ERR_INVALID, who + ": variance_floor must be finite and >= 0");
    return HRT_OK;
}
static int dn_check_params(const std::string &who, const hrt_denoise_params *p, DnFilter &F) {
    if (!p) return fail(HRT_ERR_INVALID, who + ": params is NULL");
    F = DnFilter{false, p->iterations, 0u, p->sigma_color, p->sigma_normal, p->sigma_albedo, p->sigma_depth, 0.f};
    return dn_check_filter(who, F);
}
static int dn_check_params(const std::string &who, const hrt_denoise_var_params *p, DnFilter &F) {
    if (!p) return fail(HRT_ERR_INVALID, who + ": params is NULL");
    F = DnFilter{true, p->iterations, p->prefilter, p->sigma_variance, p->sigma_normal, p->sigma_albedo, p->sigma_depth, p->variance_floor};
    return dn_check_filter(who, F);
}

size_t hrt_denoise_scratch_bytes(uint32_t w, uint32_t h) { return (size_t)w * h * 4u * sizeof(float4); }
size_t hrt_denoise_var_scratch_bytes(uint32_t w, uint32_t h) { return hrt_denoise_scratch_bytes(w, h); }

// Prep, then F.prefilter + F.iterations passes that ping-pong between the scratch's two colour buffers; the last one writes d_out.
static int dn_run(const float *d_color, const float *d_half, const float *d_feat, uint32_t w, uint32_t h, const DnFilter &F, uint32_t flags,
                  void *d_scratch, float *d_out, float *d_var_out, hipStream_t stream) {
    const size_t npix = (size_t)w * h;
    float4 *guide = (float4 *)d_scratch, *xa = guide + 2 * npix, *xb = xa + npix;
    const dim3 pgrid((unsigned)((npix + 255) / 256)), pblock(256);
    if (F.var) hipLaunchKernelGGL(hrt_dnv_prep_kernel, pgrid, pblock, 0, stream, d_color, d_half, d_feat, (uint32_t)npix, xa, guide);
    else hipLaunchKernelGGL(hrt_dn_prep_kernel, pgrid, pblock, 0, stream, d_color, d_feat, (uint32_t)npix, xa, guide);
    HIP_TRY(hipGetLastError());
    const dim3 grid((w + HRT_DN_TILE - 1) / HRT_DN_TILE, (h + HRT_DN_TILE - 1) / HRT_DN_TILE), block(HRT_DN_TILE * HRT_DN_TILE);
    const float den_n = F.sigma_n * F.sigma_n, den_a = F.sigma_a * F.sigma_a;
    for (uint32_t pass = 0; pass < F.prefilter + F.iterations; ++pass) {
        const bool pre = pass < F.prefilter, last = pass + 1 == F.prefilter + F.iterations;
        const uint32_t i = pre ? pass : pass - F.prefilter;
        const float sc = F.var ? F.sigma_c : F.sigma_c * std::ldexp(1.f, -(int)i);  // fixed width: sigma_c 2^-i, the colour term tightens every iteration
        void (*const k)(HRT_DN_PASS_PARAMS) = pre ? hrt_dnv_pre_kernel
                                            : (F.var ? (last ? hrt_dnv_last_kernel : hrt_dnv_iter_kernel) : (last ? hrt_dn_last_kernel : hrt_dn_iter_kernel));
        hipLaunchKernelGGL(k, grid, block, 0, stream, (const float4 *)xa, (const float4 *)guide, w, h, 1u << i, sc * sc, F.vfloor, den_n, den_a, F.sigma_z, xb,
                           d_color, d_feat, d_out, d_var_out, (flags & HRT_FLAG_GAMMA) ? 1u : 0u);
        HIP_TRY(hipGetLastError());
        std::swap(xa, xb);
    }
    return HRT_OK;
}

// hrt_denoise and hrt_denoise_var after their parameter check: d_half is wanted when F.var.
static int dn_denoise(const std::string &who, const float *d_color, const float *d_half, const float *d_features, uint32_t w, uint32_t h,
                      const DnFilter &F, uint32_t flags, void *d_scratch, float *d_out, float *d_var_out, void *stream) {
    const int rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if (flags & ~(uint32_t)HRT_FLAG_GAMMA) return fail(HRT_ERR_INVALID, who + ": flags may hold HRT_FLAG_GAMMA only");
    if (!d_color) return fail(HRT_ERR_INVALID, who + ": d_color is NULL");
    if (F.var && !d_half) return fail(HRT_ERR_INVALID, who + ": d_color_half is NULL");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if (!d_scratch) return fail(HRT_ERR_INVALID, who + ": d_scratch is NULL");
    if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    return dn_run(d_color, d_half, d_features, w, h, F, flags, d_scratch, d_out, d_var_out, (hipStream_t)stream);
}

int hrt_denoise(const float *d_color, const float *d_features, uint32_t w, uint32_t h, const hrt_denoise_params *p, uint32_t flags,
                void *d_scratch, float *d_out, void *stream) {
    DnFilter F;
    const int rc = dn_check_params("hrt_denoise", p, F);
    return rc != HRT_OK ? rc : dn_denoise("hrt_denoise", d_color, nullptr, d_features, w, h, F, flags, d_scratch, d_out, nullptr, stream);
}
int hrt_denoise_var(const float *d_color, const float *d_color_half, const float *d_features, uint32_t w, uint32_t h,
                    const hrt_denoise_var_params *p, uint32_t flags, void *d_scratch, float *d_out, float *d_variance_out, void *stream) {
    DnFilter F;
    const int rc = dn_check_params("hrt_denoise_var", p, F);
    return rc != HRT_OK ? rc : dn_denoise("hrt_denoise_var", d_color, d_color_half, d_features, w, h, F, flags, d_scratch, d_out, d_variance_out, stream);
}

// Feature launch on `stream`: the camera goes into the scene's feature block (its own: a trace launch on another stream may still
// read s->d_cam).  Feature launches of one scene are ordered: one on another stream first waits for the previous one.
static int features_launch(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                           uint64_t seed, float *d_features, hipStream_t stream) {
    DRender R;
    DCamera C;
    int rc = fill_render(s, cam, w, h, 1, seed, 0, 0, 1, R, C);
    if (rc != HRT_OK) return rc;
    if ((rc = s->d_cam_feat.grow(sizeof(DCamera))) != HRT_OK) return rc;
    if ((rc = s->feat_reader.wait_on(stream)) != HRT_OK) return rc;
    s->h_cam_feat = C;
    HIP_TRY(hipMemcpyAsync(s->d_cam_feat.p, &s->h_cam_feat, sizeof(C), hipMemcpyHostToDevice, stream));
    R.cam = s->d_cam_feat.as<DCamera>();
    R.s0 = first_sample;
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_features_kernel, dim3((npix + 255) / 256), dim3(256), 0, stream, R, n_samples, d_features);
    HIP_TRY(hipGetLastError());
    return s->feat_reader.mark(stream);
}

int hrt_render_features(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                        uint64_t seed, float *d_features, void *stream) {
    const std::string who = "hrt_render_features";
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    int rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if ((uint64_t)first_sample + n_samples > 0xffffffffull) return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples overflows 32 bits");
    if (!d_features) return fail(HRT_ERR_INVALID, who + ": d_features is NULL");
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    return features_launch(s, cam, w, h, first_sample, n_samples, seed, d_features, (hipStream_t)stream);
}

// The linear frame of hrt_render at spp samples (even) and the frame of its first half, row-major on the device: sums of samples
// [0, spp/2), a copy of them, then [spp/2, spp) on top -- the full sums are hrt_render's, bit for bit -- both finalised without
// gamma, every launch checked.  The scene's tile buffers are the scratch (grown here); ms_half: the first launch's kernel time.
static int dn_render_pair(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t lin,
                          float *d_frame, float *d_frame_half, double *ms_half) {
    const uint32_t tiles = hrt_tiles_total(w, h), half = spp / 2u;
    const size_t tile_bytes = (size_t)tiles * 64 * 3 * sizeof(float);
    int rc = s->tiles.grow(tile_bytes);
    if (rc == HRT_OK) rc = s->dnv_half_tiles.grow(tile_bytes);
    if (rc != HRT_OK) return rc;
    float *const d_tiles = s->tiles.as<float>(), *const d_half = s->dnv_half_tiles.as<float>();
    HIP_TRY(hipMemsetAsync(d_tiles, 0, tile_bytes, nullptr));
    rc = hrt_render_accumulate(s, cam, w, h, 0, half, seed, lin, 0, 1, d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_last_kernel_ms(s, ms_half);  // waits for the launch and checks it (hrt_check_last_launch)
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_half, d_tiles, tile_bytes, hipMemcpyDeviceToDevice, nullptr));
    rc = hrt_render_accumulate(s, cam, w, h, half, spp - half, seed, lin, 0, 1, d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_check_last_launch(s);  // never denoise a frame the kernel did not finish
    if (rc == HRT_OK) rc = hrt_finalize_tiles(d_half, tiles, half, 0, d_half, nullptr);
    if (rc == HRT_OK) rc = hrt_finalize_tiles(d_tiles, tiles, spp, 0, d_tiles, nullptr);
    if (rc == HRT_OK) rc = hrt_assemble_frame(d_half, tiles, w, h, 1, d_frame_half, nullptr);
    if (rc == HRT_OK) rc = hrt_assemble_frame(d_tiles, tiles, w, h, 1, d_frame, nullptr);
    return rc;
}

// The feature launch of HRT_GUIDES_FIRST_DIFFUSE (hrt_path_features.hip, which comes after the lens sources it is made of).
static int path_features_frame(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                               float *d_features, hipStream_t stream);

// hrt_render_denoised, hrt_render_denoised_var and their _guides forms after their checks of the parameters, the frame size and
// spp.  The frame is hrt_render's at spp samples, linear; F.var: with the first half's frame beside it (dn_render_pair).  guides:
// where the features come from, HRT_GUIDES_FIRST_HIT (the existing entry points) or HRT_GUIDES_FIRST_DIFFUSE.
static int dn_render(const std::string &who, hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp,
                     uint64_t seed, uint32_t flags, uint32_t guides, const DnFilter &F, float *out_rgb, float *out_variance, hrt_stats *stats) {
    if (guides > HRT_GUIDES_FIRST_DIFFUSE)
        return fail(HRT_ERR_INVALID, who + ": guides must be HRT_GUIDES_FIRST_HIT or HRT_GUIDES_FIRST_DIFFUSE (got " + std::to_string(guides) + ")");
    if (guides == HRT_GUIDES_FIRST_DIFFUSE && feature_spp == 0u)
        return fail(HRT_ERR_INVALID, who + ": feature_spp must be at least 1 with HRT_GUIDES_FIRST_DIFFUSE (a pixel-centre path has no stream)");
    if (feature_spp > spp) return fail(HRT_ERR_INVALID, who + ": feature_spp must be at most spp (got " + std::to_string(feature_spp) + " > " + std::to_string(spp) + ")");
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    if (!out_rgb) return fail(HRT_ERR_INVALID, who + ": out_rgb is NULL");
    int rc = enter_scene(who, s);
    if (rc != HRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t tiles = hrt_tiles_total(w, h), lin = flags & ~(uint32_t)HRT_FLAG_GAMMA;
    const size_t npix = (size_t)w * h, tile_bytes = (size_t)tiles * 64 * 3 * sizeof(float);
    if ((rc = s->tiles.grow(tile_bytes)) != HRT_OK) return rc;
    if ((rc = s->dn_frame.grow(npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if (F.var && (rc = s->dnv_frame_half.grow(npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if ((rc = s->dn_feat.grow(npix * HRT_FEATURE_FLOATS * sizeof(float))) != HRT_OK) return rc;
    if ((rc = s->dn_scratch.grow(hrt_denoise_scratch_bytes(w, h))) != HRT_OK) return rc;
    if ((rc = s->dn_out.grow(npix * 3 * sizeof(float))) != HRT_OK) return rc;
    if (out_variance && (rc = s->dnv_var.grow(npix * sizeof(float))) != HRT_OK) return rc;
    float *const d_tiles = s->tiles.as<float>();
    double ms_half = 0.0;
    if (F.var) {
        rc = dn_render_pair(s, cam, w, h, spp, seed, lin, s->dn_frame.as<float>(), s->dnv_frame_half.as<float>(), &ms_half);
    } else {
        rc = hrt_render_tiles(s, cam, w, h, spp, seed, lin, 0, 1, d_tiles, nullptr);
        if (rc == HRT_OK) rc = hrt_assemble_frame(d_tiles, tiles, w, h, 1, s->dn_frame.as<float>(), nullptr);
        if (rc == HRT_OK) rc = hrt_check_last_launch(s);  // never denoise a frame the kernel did not finish
    }
    if (rc == HRT_OK)
        rc = guides == HRT_GUIDES_FIRST_DIFFUSE ? path_features_frame(s, cam, w, h, 0, feature_spp, seed, s->dn_feat.as<float>(), nullptr)
                                                : features_launch(s, cam, w, h, 0, feature_spp, seed, s->dn_feat.as<float>(), nullptr);
    if (rc == HRT_OK) rc = dn_run(s->dn_frame.as<float>(), s->dnv_frame_half.as<float>(), s->dn_feat.as<float>(), w, h, F, flags & HRT_FLAG_GAMMA,
                                  s->dn_scratch.p, s->dn_out.as<float>(), out_variance ? s->dnv_var.as<float>() : nullptr, nullptr);
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->dn_out.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_variance) HIP_TRY(hipMemcpy(out_variance, s->dnv_var.p, npix * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) {
        double ms = 0.0;
        rc = hrt_last_kernel_ms(s, &ms);
        if (rc != HRT_OK) return rc;
        fill_stats(s, stats, t0, ms_half + ms, (uint64_t)w * h * spp);  // the trace launches' time
    }
    return HRT_OK;
}

static int dn_render_fixed(const std::string &who, hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp,
                           uint64_t seed, uint32_t flags, uint32_t guides, const hrt_denoise_params *p, float *out_rgb, hrt_stats *stats) {
    DnFilter F;
    int rc = dn_check_params(who, p, F);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if (!spp) return fail(HRT_ERR_INVALID, who + ": spp must be positive");
    return dn_render(who, s, cam, w, h, spp, feature_spp, seed, flags, guides, F, out_rgb, nullptr, stats);
}

int hrt_render_denoised(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed,
                        uint32_t flags, const hrt_denoise_params *p, float *out_rgb, hrt_stats *stats) {
    return dn_render_fixed("hrt_render_denoised", s, cam, w, h, spp, feature_spp, seed, flags, HRT_GUIDES_FIRST_HIT, p, out_rgb, stats);
}

int hrt_render_denoised_guides(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed,
                               uint32_t flags, uint32_t guides, const hrt_denoise_params *p, float *out_rgb, hrt_stats *stats) {
    return dn_render_fixed("hrt_render_denoised_guides", s, cam, w, h, spp, feature_spp, seed, flags, guides, p, out_rgb, stats);
}

static int dn_render_var(const std::string &who, hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp,
                         uint64_t seed, uint32_t flags, uint32_t guides, const hrt_denoise_var_params *p, float *out_rgb, float *out_variance,
                         hrt_stats *stats) {
    DnFilter F;
    int rc = dn_check_params(who, p, F);
    if (rc == HRT_OK) rc = check_frame(who, w, h, k_max_records);
    if (rc != HRT_OK) return rc;
    if (spp < 2u || (spp & 1u)) return fail(HRT_ERR_INVALID, who + ": spp must be even and at least 2 (got " + std::to_string(spp) + ")");
    return dn_render(who, s, cam, w, h, spp, feature_spp, seed, flags, guides, F, out_rgb, out_variance, stats);
}

int hrt_render_denoised_var(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed,
                            uint32_t flags, const hrt_denoise_var_params *p, float *out_rgb, float *out_variance, hrt_stats *stats) {
    return dn_render_var("hrt_render_denoised_var", s, cam, w, h, spp, feature_spp, seed, flags, HRT_GUIDES_FIRST_HIT, p, out_rgb, out_variance, stats);
}

int hrt_render_denoised_var_guides(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t feature_spp, uint64_t seed,
                                   uint32_t flags, uint32_t guides, const hrt_denoise_var_params *p, float *out_rgb, float *out_variance,
                                   hrt_stats *stats) {
    return dn_render_var("hrt_render_denoised_var_guides", s, cam, w, h, spp, feature_spp, seed, flags, guides, p, out_rgb, out_variance, stats);
}
