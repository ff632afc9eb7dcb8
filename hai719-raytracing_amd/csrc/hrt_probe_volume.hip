// Probe volumes (include/hrt.h "Probe volumes"): a regular grid of SH9 light probes that lives on the device, and one fused launch
// that evaluates it at caller-supplied surface points -- trilinear interpolation between the eight probes round a point, optionally
// weighted by how far each probe faces the surface, then the irradiance (or the radiance) in the direction of the normal.  Included
// by hrt_api.hip inside its extern "C" block, after hrt_probes.hip.
//
// Steps 1-3 of the rule (the cell and the weights) are hrt_probe_volume_cell.h, shared with the host; steps 4-6 are pv_fold_corner,
// pv_basis and pv_channel below, shared by the two mappings of the evaluation kernel:
//   eight lanes to a point (the default): the coefficients are repacked by hrt_probe_pack_kernel into records of
//     HRT_PROBE_RECORD_FLOATS floats, 128 bytes on a 128-byte boundary, and lane q of a group loads the 16-byte piece q of each
//     corner's record, so that a wave instruction reads eight whole 128-byte lines.  Lane q also works out corner q's probe and
//     weight for the group.  Each lane keeps the four a_j of its piece; the lanes 0..2 of the group then collect the nine
//     a_{3k+ch} of their channel with __shfl and store one float each;
//   a lane to a point (-DHRT_PROBE_EVAL_LANE_PER_POINT=1, the A/B build): one lane reads the eight records whole.
// Both evaluate the same expressions in the same order, so they give the same bits; which one ships is decided by measurement
// (DESIGN.md section 5 "Probe volumes", tools/probe_volume_bench.py).
//
// All of it is fp32 without fused multiply-add (the library is built with -ffp-contract=off), in the order the header writes.

#ifndef HRT_PROBE_EVAL_LANE_PER_POINT
#define HRT_PROBE_EVAL_LANE_PER_POINT 0
#endif
#define HRT_PV_WG 256u
#define HRT_PV_PIECES (HRT_PROBE_RECORD_FLOATS / 4u)  // float4 pieces per packed record, and lanes per point of the group mapping
static_assert(HRT_PROBE_RECORD_FLOATS == 32 && HRT_PV_PIECES == 8u, "a packed record is one 128-byte line of eight 16-byte pieces");
static_assert(3u * HRT_PROBE_COEFFS <= HRT_PROBE_RECORD_FLOATS, "the 27 coefficients fit a record");

struct hrt_probe_volume {
    probevol::Grid grid;
    uint32_t count = 0;   // nx * ny * nz
    int device = -1;      // the device that was current at hrt_probe_volume_create
    bool loaded = false;  // an update has been enqueued
    Scratch packed;       // count records of HRT_PROBE_RECORD_FLOATS floats
    bool has_depth = false;  // a depth update has been enqueued
    Scratch depth;        // count x HRT_PROBE_DEPTH_TEXELS moment pairs {m1, m2} ("Probe visibility"), allocated by the first depth update
};

extern "C++" {
namespace hrtk {

// Step 4 for one corner and one 16-byte piece of its record: a_j = a_j + w_m * p_m[j].
__device__ __forceinline__ void pv_fold_corner(float a[4], float w, const float4 &p) {
    a[0] = a[0] + w * p.x;
    a[1] = a[1] + w * p.y;
    a[2] = a[2] + w * p.z;
    a[3] = a[3] + w * p.w;
}

// Step 5: the basis of "Light probes" at (x, y, z), the expressions of ProbeRays::add.
__device__ __forceinline__ void pv_basis(float x, float y, float z, float Y[HRT_PROBE_COEFFS]) {
    Y[0] = 0.2820948f;
    Y[1] = 0.48860251f * y;
    Y[2] = 0.48860251f * z;
    Y[3] = 0.48860251f * x;
    Y[4] = 1.0925485f * (x * y);
    Y[5] = 1.0925485f * (y * z);
    Y[6] = 0.31539157f * (3.f * (z * z) - 1.f);
    Y[7] = 1.0925485f * (x * z);
    Y[8] = 0.54627422f * (x * x - y * y);
}

// Step 6 for one channel: a[k] = a_{3k+ch}.
__device__ __forceinline__ float pv_channel(const float a[HRT_PROBE_COEFFS], const float Y[HRT_PROBE_COEFFS], bool radiance) {
    const float F0 = 12.566371f, F1 = radiance ? 12.566371f : 8.3775804f, F2 = radiance ? 12.566371f : 3.1415927f;  // 4 pi, 8 pi / 3, pi
    float o = 0.f;
#pragma unroll
    for (uint32_t k = 0; k < HRT_PROBE_COEFFS; ++k) o = o + ((k == 0u ? F0 : k < 4u ? F1 : F2) * a[k]) * Y[k];
    return o;
}

}  // namespace hrtk
}  // extern "C++"

// One lane per 16-byte piece of a packed record: floats 4q .. 4q+3 of the probe's 27, zeros past them.
extern "C" __global__ void __launch_bounds__(HRT_PV_WG) hrt_probe_pack_kernel(const float *__restrict__ coeffs, uint32_t n_pieces,
                                                                               float4 *__restrict__ packed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // n_pieces <= 2^27
    if (i >= n_pieces) return;
    const uint32_t probe = i / HRT_PV_PIECES, q = i - probe * HRT_PV_PIECES;
    const float *src = coeffs + (size_t)probe * (3u * HRT_PROBE_COEFFS);
    float v[4];
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) v[c] = 4u * q + c < 3u * HRT_PROBE_COEFFS ? src[4u * q + c] : 0.f;
    packed[i] = make_float4(v[0], v[1], v[2], v[3]);
}

#if !HRT_PROBE_EVAL_LANE_PER_POINT
// Eight lanes to a point: 32 points per workgroup.  No lane leaves early (the shuffles want the whole group); a group past the
// end works on the last point and stores nothing.  A wave instruction serves eight points here, not 64, so whatever every lane of
// a group would repeat is shared out instead: lane q takes corner q of steps 2 and 3 (the facing term costs three divisions and
// two square roots a corner).
extern "C" __global__ void __launch_bounds__(HRT_PV_WG) hrt_probe_eval_kernel(const probevol::Grid g, const float4 *__restrict__ packed,
                                                                               const float4 *__restrict__ points, uint32_t n, uint32_t flags,
                                                                               float *__restrict__ out) {
    const uint32_t group = blockIdx.x * (HRT_PV_WG / HRT_PV_PIECES) + threadIdx.x / HRT_PV_PIECES, q = threadIdx.x % HRT_PV_PIECES;
    const uint32_t i = min(group, n - 1u);  // n >= 1
    const float4 r0 = points[2u * (size_t)i], r1 = points[2u * (size_t)i + 1u];
    const float P[3] = {r0.x, r0.y, r0.z}, N[3] = {r1.x, r1.y, r1.z};
    // steps 1-3, one corner to a lane: lane q of the group works out corner q and the group shares the results
    float Nn[3];
    const bool ok = probevol::normal(P, N, Nn);
    probevol::Axes ax;
    probevol::axes(g, P, ax);  // whatever P holds, every coordinate is inside the grid
    uint32_t my_index;
    float my_w = probevol::corner(g, ax, P, Nn, flags, q, my_index);
    if (flags & HRT_PROBE_EVAL_FACING) {
        float w[8];
#pragma unroll
        for (uint32_t m = 0; m < 8u; ++m) w[m] = __shfl(my_w, (int)m, (int)HRT_PV_PIECES);
        my_w = my_w / probevol::total(w);
    }
    if (!ok) my_w = 0.f;  // a degenerate point: its result is 0 below, whatever is loaded
    // step 4 for this lane's piece of the eight records
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    float4 p[8];
#pragma unroll
    for (uint32_t m = 0; m < 8u; ++m) p[m] = packed[(size_t)__shfl(my_index, (int)m, (int)HRT_PV_PIECES) * HRT_PV_PIECES + q];  // an index < nx * ny * nz
#pragma unroll
    for (uint32_t m = 0; m < 8u; ++m) pv_fold_corner(a, __shfl(my_w, (int)m, (int)HRT_PV_PIECES), p[m]);
    // lane ch < 3 of the group wants a_{3k+ch}: component (3k+ch) % 4 of lane (3k+ch) / 4.  Lanes 3..7 ask as lane 2 does.
    const uint32_t ch = min(q, 2u);
    float mine[HRT_PROBE_COEFFS];
#pragma unroll
    for (uint32_t k = 0; k < HRT_PROBE_COEFFS; ++k) {
        const uint32_t j = 3u * k + ch, from = j >> 2, c = j & 3u;
        const float t0 = __shfl(a[0], (int)from, (int)HRT_PV_PIECES), t1 = __shfl(a[1], (int)from, (int)HRT_PV_PIECES);
        const float t2 = __shfl(a[2], (int)from, (int)HRT_PV_PIECES), t3 = __shfl(a[3], (int)from, (int)HRT_PV_PIECES);
        mine[k] = c == 0u ? t0 : c == 1u ? t1 : c == 2u ? t2 : t3;
    }
    if (group >= n || q >= 3u) return;
    float Y[HRT_PROBE_COEFFS];
    pv_basis(Nn[0], Nn[1], Nn[2], Y);
    out[3u * (size_t)i + q] = ok ? pv_channel(mine, Y, (flags & HRT_PROBE_EVAL_RADIANCE) != 0u) : 0.f;
}
#define HRT_PV_POINTS_PER_WG (HRT_PV_WG / HRT_PV_PIECES)
#else
// A lane to a point: the eight records read whole by one lane.
extern "C" __global__ void __launch_bounds__(HRT_PV_WG) hrt_probe_eval_kernel(const probevol::Grid g, const float4 *__restrict__ packed,
                                                                               const float4 *__restrict__ points, uint32_t n, uint32_t flags,
                                                                               float *__restrict__ out) {
    const uint32_t i = blockIdx.x * HRT_PV_WG + threadIdx.x;  // n <= 2^31 - 1, rounded up to the workgroup: below 2^32
    if (i >= n) return;
    const float4 r0 = points[2u * (size_t)i], r1 = points[2u * (size_t)i + 1u];
    const float P[3] = {r0.x, r0.y, r0.z}, N[3] = {r1.x, r1.y, r1.z};
    uint32_t index[8];
    float weight[8], Nn[3];
    const bool ok = probevol::cell(g, P, N, flags, index, weight, Nn);
    float a[HRT_PV_PIECES][4];
#pragma unroll
    for (uint32_t q = 0; q < HRT_PV_PIECES; ++q) a[q][0] = a[q][1] = a[q][2] = a[q][3] = 0.f;
#pragma unroll
    for (uint32_t m = 0; m < 8u; ++m) {
        const float4 *rec = packed + (size_t)index[m] * HRT_PV_PIECES;
#pragma unroll
        for (uint32_t q = 0; q < HRT_PV_PIECES; ++q) pv_fold_corner(a[q], weight[m], rec[q]);
    }
    float Y[HRT_PROBE_COEFFS];
    pv_basis(Nn[0], Nn[1], Nn[2], Y);
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        float mine[HRT_PROBE_COEFFS];
#pragma unroll
        for (uint32_t k = 0; k < HRT_PROBE_COEFFS; ++k) mine[k] = a[(3u * k + ch) >> 2][(3u * k + ch) & 3u];
        out[3u * (size_t)i + ch] = ok ? pv_channel(mine, Y, (flags & HRT_PROBE_EVAL_RADIANCE) != 0u) : 0.f;
    }
}
#define HRT_PV_POINTS_PER_WG HRT_PV_WG
#endif

// ---- Probe visibility (include/hrt.h): the moments of a volume's depth maps and the look-up that weighs every corner by them.

// One lane per texel: the sums {W, A, B} to the moments {A / W, B / W}; a texel nobody looked through hides nothing.
extern "C" __global__ void __launch_bounds__(HRT_PV_WG) hrt_probe_depth_pack_kernel(const float *__restrict__ sums, uint32_t n_texels,
                                                                                     float2 *__restrict__ moments) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // n_texels <= 2^28
    if (i >= n_texels) return;
    const float W = sums[3u * (size_t)i], A = sums[3u * (size_t)i + 1u], B = sums[3u * (size_t)i + 2u];
    moments[i] = W > 0.f ? make_float2(A / W, B / W) : make_float2(__builtin_inff(), 0.f);
}

// hrt_probe_eval_kernel's eight lanes to a point, with step 3 of the visible look-up: lane q, which owns corner q of steps 2 and 3,
// additionally works out v, l and the texel of its corner, loads that texel's 8 bytes and scales its weight; the division by W
// is then unconditional.  The one mapping of this kernel: both builds of the library compile it.
#define HRT_PVV_POINTS_PER_WG (HRT_PV_WG / HRT_PV_PIECES)
extern "C" __global__ void __launch_bounds__(HRT_PV_WG) hrt_probe_eval_visible_kernel(const probevol::Grid g, const float4 *__restrict__ packed,
                                                                                       const float2 *__restrict__ moments,
                                                                                       const float4 *__restrict__ points, uint32_t n, uint32_t flags,
                                                                                       float *__restrict__ out) {
    const uint32_t group = blockIdx.x * HRT_PVV_POINTS_PER_WG + threadIdx.x / HRT_PV_PIECES, q = threadIdx.x % HRT_PV_PIECES;
    const uint32_t i = min(group, n - 1u);  // n >= 1
    const float4 r0 = points[2u * (size_t)i], r1 = points[2u * (size_t)i + 1u];
    const float P[3] = {r0.x, r0.y, r0.z}, N[3] = {r1.x, r1.y, r1.z};
    float Nn[3], Pb[3];
    bool ok = probevol::normal(P, N, Nn);
    ok = probevol::biased(P, Nn, r1.w, Pb) && ok;
    probevol::Axes ax;
    probevol::axes(g, P, ax);  // whatever P holds, every coordinate is inside the grid
    uint32_t my_index, my_texel;
    float my_w = probevol::corner(g, ax, P, Nn, flags, q, my_index);
    {
        const float l = probevol::toward(g, ax, Pb, q, my_texel);  // a texel below HRT_PROBE_DEPTH_TEXELS whatever Pb holds
        const float2 mm = moments[(size_t)my_index * HRT_PROBE_DEPTH_TEXELS + my_texel];
        my_w = my_w * probedepth::visibility(l, mm.x, mm.y);
        float w[8];
#pragma unroll
        for (uint32_t m = 0; m < 8u; ++m) w[m] = __shfl(my_w, (int)m, (int)HRT_PV_PIECES);
        my_w = my_w / probevol::total(w);
    }
    if (!ok) my_w = 0.f;  // a degenerate point: its result is 0 below, whatever is loaded
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    float4 p[8];
#pragma unroll
    for (uint32_t m = 0; m < 8u; ++m) p[m] = packed[(size_t)__shfl(my_index, (int)m, (int)HRT_PV_PIECES) * HRT_PV_PIECES + q];  // an index < nx * ny * nz
#pragma unroll
    for (uint32_t m = 0; m < 8u; ++m) pv_fold_corner(a, __shfl(my_w, (int)m, (int)HRT_PV_PIECES), p[m]);
    const uint32_t ch = min(q, 2u);
    float mine[HRT_PROBE_COEFFS];
#pragma unroll
    for (uint32_t k = 0; k < HRT_PROBE_COEFFS; ++k) {
        const uint32_t j = 3u * k + ch, from = j >> 2, c = j & 3u;
        const float t0 = __shfl(a[0], (int)from, (int)HRT_PV_PIECES), t1 = __shfl(a[1], (int)from, (int)HRT_PV_PIECES);
        const float t2 = __shfl(a[2], (int)from, (int)HRT_PV_PIECES), t3 = __shfl(a[3], (int)from, (int)HRT_PV_PIECES);
        mine[k] = c == 0u ? t0 : c == 1u ? t1 : c == 2u ? t2 : t3;
    }
    if (group >= n || q >= 3u) return;
    float Y[HRT_PROBE_COEFFS];
    pv_basis(Nn[0], Nn[1], Nn[2], Y);
    out[3u * (size_t)i + q] = ok ? pv_channel(mine, Y, (flags & HRT_PROBE_EVAL_RADIANCE) != 0u) : 0.f;
}

// The flags of an evaluation: the two of the header; every other bit is refused, by name where the library has one for it.
static int pv_flags_check(const std::string &who, uint32_t flags) {
    const struct { uint32_t bit; const char *name; } named[] = {
        {HRT_FLAG_WAVE_KERNEL, "HRT_FLAG_WAVE_KERNEL"}, {HRT_FLAG_STREAM_KERNEL, "HRT_FLAG_STREAM_KERNEL"},
        {HRT_FLAG_NO_SHADOW_CULL, "HRT_FLAG_NO_SHADOW_CULL"}, {HRT_FLAG_DUAL_KERNEL, "HRT_FLAG_DUAL_KERNEL"},
        {HRT_FLAG_EXACT_ONLY, "HRT_FLAG_EXACT_ONLY"}, {HRT_FLAG_MESH_BRUTE, "HRT_FLAG_MESH_BRUTE"},
        {HRT_RAYS_NORMALIZE, "HRT_RAYS_NORMALIZE"}, {HRT_RADIANCE_ACCUMULATE, "HRT_RADIANCE_ACCUMULATE"}};
    for (const auto &f : named)
        if (flags & f.bit)
            return fail(HRT_ERR_INVALID, who + ": flags: " + f.name + ": a probe look-up traces nothing; it takes HRT_PROBE_EVAL_RADIANCE and HRT_PROBE_EVAL_FACING");
    const uint32_t known = HRT_PROBE_EVAL_RADIANCE | HRT_PROBE_EVAL_FACING;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": flags: unknown bits " + std::to_string(flags & ~known));
    return HRT_OK;
}

// Checks 3..7 of the header's order.  `dev`: device pointers (d_ names, 16-byte records).
static int pv_eval_check(const std::string &who, const hrt_probe_volume *v, const float *points, uint32_t n, const float *out, bool dev,
                         bool needs_depth = false) {
    const std::string pn = dev ? "d_points" : "points", on = dev ? "d_out" : "out";
    const uintptr_t align = dev ? 16u : 4u;
    if (!v) return fail(HRT_ERR_INVALID, who + ": volume is NULL");
    if (!v->loaded) return fail(HRT_ERR_INVALID, who + ": the volume has no coefficients yet (hrt_probe_volume_update)");
    if (needs_depth && !v->has_depth) return fail(HRT_ERR_INVALID, who + ": the volume has no depth moments yet (hrt_probe_volume_update_depth)");
    if (!points) return fail(HRT_ERR_INVALID, who + ": " + pn + " is NULL");
    if ((uintptr_t)points % align) return fail(HRT_ERR_INVALID, who + ": " + pn + " is not " + std::to_string(align) + "-byte aligned");
    if (n > 0x7fffffffu) return fail(HRT_ERR_INVALID, who + ": n must be at most 2^31 - 1 (got " + std::to_string(n) + ")");
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + on + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + on + " is not 4-byte aligned");
    return HRT_OK;
}

// What a call on a volume does after its own checks: the library is initialised and the volume's device is current.
static int pv_enter(const std::string &who, const hrt_probe_volume *v) {
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    return use_device(v->device);
}

static int pv_launch(const hrt_probe_volume *v, const float *d_points, uint32_t n, uint32_t flags, float *d_out, hipStream_t stream) {
    const uint32_t grid = (uint32_t)(((uint64_t)n + HRT_PV_POINTS_PER_WG - 1u) / HRT_PV_POINTS_PER_WG);
    hipLaunchKernelGGL(hrt_probe_eval_kernel, dim3(grid), dim3(HRT_PV_WG), 0, stream, v->grid, v->packed.as<float4>(), (const float4 *)d_points, n, flags,
                       d_out);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

static int pv_pack(hrt_probe_volume *v, const float *d_coeffs, hipStream_t stream) {
    const uint32_t pieces = v->count * HRT_PV_PIECES;  // <= 2^27
    hipLaunchKernelGGL(hrt_probe_pack_kernel, dim3((pieces + HRT_PV_WG - 1u) / HRT_PV_WG), dim3(HRT_PV_WG), 0, stream, d_coeffs, pieces, v->packed.as<float4>());
    HIP_TRY(hipGetLastError());
    v->loaded = true;
    return HRT_OK;
}

int hrt_probe_volume_create(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, hrt_probe_volume **out) {
    const std::string who = "hrt_probe_volume_create";
    if (!out) return fail(HRT_ERR_INVALID, who + ": out is NULL");
    *out = nullptr;
    probevol::Grid g;
    std::string error;
    if (const int rc = probevol::make_grid(who, lo, hi, nx, ny, nz, g, error)) return fail(rc, error);
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    int device = -1;
    HIP_TRY(hipGetDevice(&device));
    if (const int rc = use_device(device)) return rc;  // a device hrt_init has prepared
    hrt_probe_volume *v = new (std::nothrow) hrt_probe_volume();
    if (!v) return fail(HRT_ERR_DEVICE, who + ": out of host memory");
    v->grid = g;
    v->count = nx * ny * nz;
    v->device = device;
    if (const int rc = v->packed.grow((size_t)v->count * HRT_PROBE_RECORD_FLOATS * sizeof(float))) {
        delete v;
        return rc;
    }
    *out = v;
    return HRT_OK;
}

void hrt_probe_volume_destroy(hrt_probe_volume *v) {
    if (!v) return;
    if (g_rt.ready) (void)use_device(v->device);
    delete v;  // hipFree waits for the launches that still read the buffer
}

static int pv_update_check(const std::string &who, const hrt_probe_volume *v, const float *coeffs, const char *name) {
    if (!v) return fail(HRT_ERR_INVALID, who + ": volume is NULL");
    if (!coeffs) return fail(HRT_ERR_INVALID, who + ": " + name + " is NULL");
    if ((uintptr_t)coeffs % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + name + " is not 4-byte aligned");
    return pv_enter(who, v);
}

int hrt_probe_volume_update_device(hrt_probe_volume *v, const float *d_coeffs, void *stream) {
    if (const int rc = pv_update_check("hrt_probe_volume_update_device", v, d_coeffs, "d_coeffs")) return rc;
    return pv_pack(v, d_coeffs, (hipStream_t)stream);
}

int hrt_probe_volume_update(hrt_probe_volume *v, const float *coeffs) {
    if (const int rc = pv_update_check("hrt_probe_volume_update", v, coeffs, "coeffs")) return rc;
    Scratch d_coeffs;
    if (const int rc = d_coeffs.from_host(coeffs, (size_t)v->count * 3u * HRT_PROBE_COEFFS * sizeof(float))) return rc;
    if (const int rc = pv_pack(v, d_coeffs.as<float>(), nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));  // before the staging copy goes
    return HRT_OK;
}

int hrt_probe_eval_device(const hrt_probe_volume *v, const float *d_points, uint32_t n, uint32_t flags, float *d_out, void *stream) {
    const std::string who = "hrt_probe_eval_device";
    int rc = pv_flags_check(who, flags);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = pv_eval_check(who, v, d_points, n, d_out, true)) != HRT_OK) return rc;
    if ((rc = pv_enter(who, v)) != HRT_OK) return rc;
    return pv_launch(v, d_points, n, flags, d_out, (hipStream_t)stream);
}

// Blocking, from and into host memory (BlockingCall; the points are a device buffer of the call's, too).
int hrt_probe_eval(const hrt_probe_volume *v, const float *points, uint32_t n, uint32_t flags, float *out, hrt_stats *stats) {
    const std::string who = "hrt_probe_eval";
    int rc = pv_flags_check(who, flags);
    if (rc != HRT_OK) return rc;
    if (n == 0u) return empty_batch(stats);
    if ((rc = pv_eval_check(who, v, points, n, out, false)) != HRT_OK) return rc;
    if ((rc = pv_enter(who, v)) != HRT_OK) return rc;
    BlockingCall call;
    Scratch d_points;
    if ((rc = d_points.from_host(points, (size_t)n * HRT_RAY_FLOATS * sizeof(float))) != HRT_OK) return rc;
    return call.run(nullptr, (size_t)n * 3u * sizeof(float), out, (uint64_t)n, stats,
                    [&](float *d_out) { return pv_launch(v, d_points.as<float>(), n, flags, d_out, nullptr); });
}

int hrt_probe_volume_weights(const float *lo, const float *hi, uint32_t nx, uint32_t ny, uint32_t nz, const float *point, uint32_t flags,
                             uint32_t index[8], float weight[8]) {
    const std::string who = "hrt_probe_volume_weights";
    if (const int rc = pv_flags_check(who, flags)) return rc;
    probevol::Grid g;
    std::string error;
    if (const int rc = probevol::make_grid(who, lo, hi, nx, ny, nz, g, error)) return fail(rc, error);
    if (!point) return fail(HRT_ERR_INVALID, who + ": point is NULL");
    if (!index) return fail(HRT_ERR_INVALID, who + ": index is NULL");
    if (!weight) return fail(HRT_ERR_INVALID, who + ": weight is NULL");
    float Nn[3];
    (void)probevol::cell(g, point, point + 4, flags, index, weight, Nn);  // a degenerate point: both zeroed
    return HRT_OK;
}

// ---- Probe visibility: the depth updates and the visible look-up.

static int pv_depth_check(const std::string &who, const hrt_probe_volume *v, const float *sums, const char *name) {
    if (!v) return fail(HRT_ERR_INVALID, who + ": volume is NULL");
    if (!sums) return fail(HRT_ERR_INVALID, who + ": " + name + " is NULL");
    if ((uintptr_t)sums % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + name + " is not 4-byte aligned");
    if (v->count > HRT_PROBE_DEPTH_VOLUME_MAX)
        return fail(HRT_ERR_INVALID, who + ": depth needs a volume of at most HRT_PROBE_DEPTH_VOLUME_MAX = " + std::to_string(HRT_PROBE_DEPTH_VOLUME_MAX) +
                                         " probes (this one has " + std::to_string(v->count) + ")");
    return pv_enter(who, v);
}

static int pv_depth_pack(hrt_probe_volume *v, const float *d_sums, hipStream_t stream) {
    const uint32_t texels = v->count * HRT_PROBE_DEPTH_TEXELS;  // <= 2^28
    if (const int rc = v->depth.grow((size_t)texels * sizeof(float2))) return rc;
    hipLaunchKernelGGL(hrt_probe_depth_pack_kernel, dim3((texels + HRT_PV_WG - 1u) / HRT_PV_WG), dim3(HRT_PV_WG), 0, stream, d_sums, texels, v->depth.as<float2>());
    HIP_TRY(hipGetLastError());
    v->has_depth = true;
    return HRT_OK;
}

int hrt_probe_volume_update_depth_device(hrt_probe_volume *v, const float *d_sums, void *stream) {
    if (const int rc = pv_depth_check("hrt_probe_volume_update_depth_device", v, d_sums, "d_sums")) return rc;
    return pv_depth_pack(v, d_sums, (hipStream_t)stream);
}

int hrt_probe_volume_update_depth(hrt_probe_volume *v, const float *sums) {
    if (const int rc = pv_depth_check("hrt_probe_volume_update_depth", v, sums, "sums")) return rc;
    Scratch d_sums;
    if (const int rc = d_sums.from_host(sums, (size_t)v->count * HRT_PROBE_DEPTH_FLOATS * sizeof(float))) return rc;
    if (const int rc = pv_depth_pack(v, d_sums.as<float>(), nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));  // before the staging copy goes
    return HRT_OK;
}

static int pv_launch_visible(const hrt_probe_volume *v, const float *d_points, uint32_t n, uint32_t flags, float *d_out, hipStream_t stream) {
    const uint32_t grid = (uint32_t)(((uint64_t)n + HRT_PVV_POINTS_PER_WG - 1u) / HRT_PVV_POINTS_PER_WG);
    hipLaunchKernelGGL(hrt_probe_eval_visible_kernel, dim3(grid), dim3(HRT_PV_WG), 0, stream, v->grid, v->packed.as<float4>(), v->depth.as<float2>(),
                       (const float4 *)d_points, n, flags, d_out);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

int hrt_probe_eval_visible_device(const hrt_probe_volume *v, const float *d_points, uint32_t n, uint32_t flags, float *d_out, void *stream) {
    const std::string who = "hrt_probe_eval_visible_device";
    int rc = pv_flags_check(who, flags);
    if (rc != HRT_OK || n == 0u) return rc;
    if ((rc = pv_eval_check(who, v, d_points, n, d_out, true, true)) != HRT_OK) return rc;
    if ((rc = pv_enter(who, v)) != HRT_OK) return rc;
    return pv_launch_visible(v, d_points, n, flags, d_out, (hipStream_t)stream);
}

// Blocking, from and into host memory, as hrt_probe_eval.
int hrt_probe_eval_visible(const hrt_probe_volume *v, const float *points, uint32_t n, uint32_t flags, float *out, hrt_stats *stats) {
    const std::string who = "hrt_probe_eval_visible";
    int rc = pv_flags_check(who, flags);
    if (rc != HRT_OK) return rc;
    if (n == 0u) return empty_batch(stats);
    if ((rc = pv_eval_check(who, v, points, n, out, false, true)) != HRT_OK) return rc;
    if ((rc = pv_enter(who, v)) != HRT_OK) return rc;
    BlockingCall call;
    Scratch d_points;
    if ((rc = d_points.from_host(points, (size_t)n * HRT_RAY_FLOATS * sizeof(float))) != HRT_OK) return rc;
    return call.run(nullptr, (size_t)n * 3u * sizeof(float), out, (uint64_t)n, stats,
                    [&](float *d_out) { return pv_launch_visible(v, d_points.as<float>(), n, flags, d_out, nullptr); });
}
