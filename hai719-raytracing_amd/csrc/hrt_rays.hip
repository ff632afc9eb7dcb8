// Ray queries on caller rays (include/hrt.h hrt_trace_rays): closest hit, closest hit + shading, occlusion.
// Included by hrt_api.hip inside its extern "C" block, after everything it builds on.  What a query on caller rays needs whatever
// it computes -- the ray record (query_ray), its margin and far-origin rule (query_margin), the context with the staged tree
// (query_context), and on the host the argument checks and the launch (query_check, query_launch) -- is here once, for this file
// and for the radiance queries of hrt_radiance.hip.
//
// One lane per ray, in a grid-stride loop over the batch: the grid is sized to the workgroups that can be resident at once, so a
// build with HRT_RAYS_STAGE_TREE can stage the top of the KD-trees (hrt_scene::lds_units nodelets, as trace_body does) into LDS
// once per workgroup and serve many rays from it; the default build reads every nodelet from global memory (measured faster).  A ray is two coalesced 16-byte loads; a record group is one 16-byte store.  The device functions are the
// trace path's own -- closest_hit() and shade() of hrt_aov_kernel / hrt_features_kernel, the primitives and mesh walks of
// shadow_blocked() -- so a query computes what a render would for the same ray.
//
// The filters' margin scale (CtxT::err_abs) is per ray here: 2e-6 (scene bound + |o| + 1) for a unit direction, +inf otherwise.
// A ray whose origin lies far outside the scene tests every triangle of a mesh whose box it enters instead of walking the tree: the
// walk locates cells at o + t d, and from 1e6 away that point is off the line by ulp(1e6) = 0.06, more than a cell.  DESIGN.md
// section 5 "Ray queries" has both derivations.

#define HRT_RAYS_WG 256u
#ifndef HRT_RAYS_FAR
#define HRT_RAYS_FAR 16.f  // an origin farther than this many (scene bound + 1) from the world origin counts as far (see query_margin)
#endif
#ifndef HRT_RAYS_STAGE_TREE
#define HRT_RAYS_STAGE_TREE 0  // -DHRT_RAYS_STAGE_TREE: the A/B build that stages the tree prefix (see hrt_trace_rays)
#endif

struct DRays {
    const DScene *scene;
    const float4 *rays;   // 2 float4 per ray: {o, time} {d, tmax}
    void *out;
    uint32_t n;
    uint32_t flags;
    uint32_t lds_units;   // leading kd units each workgroup stages into LDS (0: every nodelet from global memory)
    float bound;          // hrt_scene::bound: largest distance of any scene point from the origin
};

extern "C++" {
namespace hrtk {

__device__ __forceinline__ bool rays_finite(float v) { return __builtin_isfinite(v); }

// Record i, {o, time} {d, tmax}, of the batch of launch record Q (DRays or DRadiance: its rays and flags) as a Ray and its tmax;
// false if it is degenerate: a component that is not finite or a zero direction (include/hrt.h hrt_trace_rays).
// HRT_RAYS_NORMALIZE: the direction goes through the Ray constructor (Line.h:13-16), and a length that under- or overflows is
// degenerate too.  Q is taken whole, by reference, as the kernels' other helpers take it: handing its fields over by value cost
// hrt_radiance_kernel 20 more spilled VGPRs.
template <class QT>
__device__ __forceinline__ bool query_ray(const QT &Q, uint32_t i, Ray &ray, float &tmax) {
    const gf4 rays = (gf4)Q.rays;
    const float4 a = ld(rays, 2u * i), b = ld(rays, 2u * i + 1u);
    ray.o = mk(a.x, a.y, a.z);
    ray.time = a.w;
    ray.d = mk(b.x, b.y, b.z);
    tmax = b.w;
    bool ok = rays_finite(a.x) && rays_finite(a.y) && rays_finite(a.z) && rays_finite(a.w) && rays_finite(b.x) &&
              rays_finite(b.y) && rays_finite(b.z) && !(b.x == 0.f && b.y == 0.f && b.z == 0.f);
    if (ok && (Q.flags & HRT_RAYS_NORMALIZE)) {
        ray.d = normalize(ray.d);
        ok = rays_finite(ray.d.x) && rays_finite(ray.d.y) && rays_finite(ray.d.z) && !(ray.d.x == 0.f && ray.d.y == 0.f && ray.d.z == 0.f);
    }
    return ok;
}

// For a segment that starts at the caller's origin: the filters' margin scale (CtxT::err_abs), and the launch flags with
// HRT_FLAG_MESH_BRUTE added for an origin farther than `far` from the world origin (every triangle of a gated mesh is tested, no
// walk).  far = query_far(bound), which a kernel works out once.
__device__ __forceinline__ float query_far(float bound) { return HRT_RAYS_FAR * (bound + 1.f); }
__device__ __forceinline__ void query_margin(const Ray &ray, float bound, float far, uint32_t flags, float &err_abs, uint32_t &ray_flags) {
    const float olen = length(ray.o);
    err_abs = fabsf(dot(ray.d, ray.d) - 1.f) <= 1e-5f ? margin_scale(bound, olen) : __builtin_inff();
    ray_flags = olen > far ? (flags | HRT_FLAG_MESH_BRUTE | HRT_FLAG_FAR_ORIGIN) : flags;
}

// The context of a query kernel: tables from global memory, the leading lds_units nodelets staged into LDS by the whole workgroup
// (so every lane of it must call this), MESH_BRUTE honoured per ray.  `stamps`: 17 words of the caller's.
template <class CX>
__device__ __forceinline__ void query_context(CX &cx, const DScene *scene, uint32_t lds_units, uint32_t flags, unsigned long long *stamps) {
    extern __shared__ uint4 s_units[];
    cx.S = (cscene)scene;
    cx.set_tables((gf4)cx.S->tabs, (gf1)c_u8_lut, cx.S);
    cx.lds = (lu4)s_units;
    cx.lds_n = lds_units;
    cx.flags = flags;
    cx.err_abs = 0.f;
    cx.st = stamps;
    gu4 g_units = (gu4)cx.S->kd_units;
    for (uint32_t i = threadIdx.x; i < cx.lds_n; i += blockDim.x) s_units[i] = ld(g_units, i);
    __syncthreads();
}

// Scene::computeShadow (Scene.h:235-255) with every transparency 0: some object's own hit -- the value closest_hit compares for
// it -- lies in [EPSILON, tmax).  Objects in closest_hit's order, first one in range ends the query.  A mesh's own hit is its
// nearest triangle (the full walk, as closest_hit runs it), so a triangle in [0, EPSILON) still hides the farther ones.
template <class CX>
__device__ __forceinline__ bool rays_occluded(const CX &cx, const Ray &ray, float tmax) {
    cscene S = cx.S;
    cf4 sph = (cf4)S->spheres;
    const uint32_t ns = S->n_spheres;
    for (uint32_t i = 0; i < ns; ++i) {
        float t;
        if (sphere_t(ld(sph, 2 * i), ld(sph, 2 * i + 1), ray, t) && t < tmax && HRT_T_ACCEPT(t)) return true;
    }
    cf4 qd = (cf4)S->quads;
    const uint32_t nq = S->n_quads;
    if (!CX::exact && nq <= 64u) {  // prims_hit's filter with tmax as the bound: it keeps every square whose exact t can be < tmax
        uint64_t cand = nq <= 32u ? (uint64_t)quad_filter<uint32_t>(cx, ray, tmax) : quad_filter<uint64_t>(cx, ray, tmax);
        while (cand) {
            const uint32_t i = (uint32_t)__builtin_ctzll(cand);
            cand &= cand - 1ull;
            float t, u, v;
            if (quad_t(cx.tq + HRT_QUAD_ROWS * i, ray, tmax, t, u, v)) return true;
        }
    } else {
        for (uint32_t i = 0; i < nq; ++i) {
            float t, u, v;
            if (quad_t(qd + HRT_QUAD_ROWS * i, ray, tmax, t, u, v)) return true;
        }
    }
    const uint32_t m = S->n_meshes ? mesh_gates(cx, ray) : 0u;
    if (m) {
        const f3 inv = ray_inv<CX::exact>(ray);
        const uint32_t nm = min(S->n_meshes, 32u);
        for (uint32_t i = 0; i < nm; ++i) {  // wave-uniform loop; a lane that found its answer sits the rest out
            if (!(m & (1u << i))) continue;
            float t, u, v;
            uint32_t tri;
            if (mesh_traverse(cx, (cmesh)S->meshes + i, ray, inv, t, tri, u, v) && t < tmax && HRT_T_ACCEPT(t)) return true;
        }
    }
    return false;
}

// MODE: HRT_QUERY_CLOSEST, HRT_QUERY_SHADE or HRT_QUERY_OCCLUDED.  EXACT: the proof build (HRT_FLAG_EXACT_ONLY).
template <uint32_t MODE, bool EXACT>
__device__ __forceinline__ void rays_body(const DRays &Q) {
    CtxT<EXACT, false, false, true> cx;
    unsigned long long stamps_local[17] = {0};
    query_context(cx, Q.scene, Q.lds_units, Q.flags, stamps_local);
    const uint32_t stride = gridDim.x * blockDim.x;
    const float far = query_far(Q.bound);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < Q.n; i += stride) {
        Ray ray;
        float tmax;
        const bool ok = query_ray(Q, i, ray, tmax) && tmax > 0.f;  // a tmax that is NaN or <= 0 is degenerate here
        query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, cx.flags);
        if (MODE == HRT_QUERY_OCCLUDED) {
            const bool occ = ok && rays_occluded(cx, ray, fminf(tmax, HRT_FLT_MAX));
            ((uint32_t *)Q.out)[i] = occ ? 1u : 0u;
            continue;
        }
        Hit h;
        h.kind = 0u;
        if (ok) {
            h = closest_hit(cx, ray);
            if (!(h.t < tmax)) h.kind = 0u;
        }
        uint4 r0 = make_uint4(0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu);
        if (h.kind) {
            const uint32_t prim = h.kind == 3u ? __float_as_uint(ld((gf4)cx.S->tris, HRT_TRI_ROWS * h.tri + 3u).x) : 0xFFFFFFFFu;
            r0 = make_uint4(__float_as_uint(h.t), h.kind, h.index, prim);
        }
        uint4 *o = (uint4 *)Q.out + (size_t)i * (MODE == HRT_QUERY_SHADE ? 4u : 1u);
        o[0] = r0;
        if (MODE == HRT_QUERY_SHADE) {
            uint4 r1 = make_uint4(0u, 0u, 0u, 0u), r2 = r1, r3 = r1;
            if (h.kind) {
                const Surface sf = shade(cx, ray, h);
                r1 = make_uint4(__float_as_uint(sf.n.x), __float_as_uint(sf.n.y), __float_as_uint(sf.n.z), __float_as_uint(sf.transparency));
                r2 = make_uint4(__float_as_uint(sf.albedo.x), __float_as_uint(sf.albedo.y), __float_as_uint(sf.albedo.z), __float_as_uint(sf.index_medium));
                r3 = make_uint4(__float_as_uint(sf.emission.x), __float_as_uint(sf.emission.y), __float_as_uint(sf.emission.z), sf.type);
            }
            o[1] = r1; o[2] = r2; o[3] = r3;
        }
    }
}

}  // namespace hrtk
}  // extern "C++"

extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_rays_closest_kernel(const DRays Q) { rays_body<HRT_QUERY_CLOSEST, false>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_rays_shade_kernel(const DRays Q) { rays_body<HRT_QUERY_SHADE, false>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_rays_occluded_kernel(const DRays Q) { rays_body<HRT_QUERY_OCCLUDED, false>(Q); }
// HRT_FLAG_EXACT_ONLY: the proof builds (no filters, no v_rcp_f32; see CtxT)
extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_rays_closest_exact_kernel(const DRays Q) { rays_body<HRT_QUERY_CLOSEST, true>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_rays_shade_exact_kernel(const DRays Q) { rays_body<HRT_QUERY_SHADE, true>(Q); }
extern "C" __global__ void __launch_bounds__(HRT_RAYS_WG) hrt_rays_occluded_exact_kernel(const DRays Q) { rays_body<HRT_QUERY_OCCLUDED, true>(Q); }

// The checks hrt_trace_rays and hrt_trace_radiance share, in their order: the flags (the common ones and the entry point's
// `extra` bits), the pointers when there is a ray to read (d_keys may be NULL; d_out aligned to out_align bytes), the batch size.
static int query_check(const std::string &who, uint32_t flags, uint32_t extra, const void *d_rays, const void *d_keys, const void *d_out,
                       uintptr_t out_align, uint32_t n) {
    const uint32_t known = HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE | HRT_RAYS_NORMALIZE | extra;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": unknown flags bits " + std::to_string(flags & ~known));
    { const int brc = check_mesh_brute(who, flags); if (brc != HRT_OK) return brc; }
    if (n > 0u) {
        if (!d_rays) return fail(HRT_ERR_INVALID, who + ": d_rays is NULL");
        if ((uintptr_t)d_rays % 16u) return fail(HRT_ERR_INVALID, who + ": d_rays is not 16-byte aligned");
        if ((uintptr_t)d_keys % 4u) return fail(HRT_ERR_INVALID, who + ": d_keys is not 4-byte aligned");
        if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
        if ((uintptr_t)d_out % out_align) return fail(HRT_ERR_INVALID, who + ": d_out is not " + std::to_string(out_align) + "-byte aligned");
    }
    if (n > 0x7fffffffu) return fail(HRT_ERR_INVALID, who + ": n must be at most 2^31 - 1 (got " + std::to_string(n) + ")");
    return HRT_OK;
}

// Launches query kernel k over the Q.n rays of Q (DRays or DRadiance; the scene entered), one lane per ray in a grid-stride loop.
// stage_tree: the workgroups stage the top of the KD-trees into LDS (unless HRT_FLAG_NO_LDS_TREE) -- at most 64 KiB, so there is
// no attribute to raise.  The grid is the workgroups that can be resident at once, or as many as the batch fills.
extern "C++" {
template <class QT>
static int query_launch(void (*k)(const QT), QT &Q, const hrt_scene *s, bool stage_tree, uint32_t wg, void *stream) {
    Q.scene = s->d_scene.as<DScene>();
    Q.bound = s->bound;
    Q.lds_units = (stage_tree && !(Q.flags & HRT_FLAG_NO_LDS_TREE)) ? std::min<uint32_t>(s->lds_units, 4096u) : 0u;
    const size_t lds_bytes = (size_t)Q.lds_units * 16u;
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k, (int)wg, lds_bytes));
    const uint64_t resident = (uint64_t)std::max(per_cu, 1) * (uint64_t)std::max(g_rt.cus, 1);
    const uint64_t needed = ((uint64_t)Q.n + wg - 1u) / wg;
    hipLaunchKernelGGL(k, dim3((uint32_t)std::min(resident, needed)), dim3(wg), lds_bytes, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}
}  // extern "C++"

int hrt_trace_rays(hrt_scene *s, const float *d_rays, uint32_t n, uint32_t mode, uint32_t flags, void *d_out, void *stream) {
    const std::string who = "hrt_trace_rays";
    if (mode > HRT_QUERY_OCCLUDED) return fail(HRT_ERR_INVALID, who + ": mode must be HRT_QUERY_CLOSEST, _SHADE or _OCCLUDED (got " + std::to_string(mode) + ")");
    int rc = query_check(who, flags, 0u, d_rays, nullptr, d_out, mode == HRT_QUERY_OCCLUDED ? 4u : 16u, n);
    if (rc == HRT_OK) rc = enter_scene(who, s, n != 0u);  // also checked for an empty batch, which leaves the current device alone
    if (rc != HRT_OK || n == 0u) return rc;
    DRays Q;
    Q.rays = (const float4 *)d_rays;
    Q.out = d_out;
    Q.n = n;
    Q.flags = flags;
    void (*const kernels[2][3])(const DRays) = {
        {hrt_rays_closest_kernel, hrt_rays_shade_kernel, hrt_rays_occluded_kernel},
        {hrt_rays_closest_exact_kernel, hrt_rays_shade_exact_kernel, hrt_rays_occluded_exact_kernel}};
    // The tree prefix is NOT staged by default: measured on MI355X (DESIGN.md section 5 "Ray queries"), staging it costs more than it
    // saves for CLOSEST and OCCLUDED (-10..-15 %) and is even for SHADE.  HRT_RAYS_STAGE_TREE builds keep the staged form for A/B runs.
    return query_launch(kernels[(flags & HRT_FLAG_EXACT_ONLY) ? 1 : 0][mode], Q, s, HRT_RAYS_STAGE_TREE, HRT_RAYS_WG, stream);
}
