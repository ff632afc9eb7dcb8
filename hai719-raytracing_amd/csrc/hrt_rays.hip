// Ray queries on caller rays (include/hrt.h hrt_trace_rays): closest hit, closest hit + shading, occlusion.
// Included by hrt_api.hip inside its extern "C" block, after everything it builds on.
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
#define HRT_RAYS_FAR 16.f  // an origin farther than this many (scene bound + 1) from the world origin counts as far (see rays_body)
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
    extern __shared__ uint4 s_units[];
    CtxT<EXACT, false, false, true> cx;
    cx.S = (cscene)Q.scene;
    cx.set_tables((gf4)cx.S->tabs, (gf1)c_u8_lut, cx.S);
    cx.lds = (lu4)s_units;
    cx.lds_n = Q.lds_units;
    cx.flags = Q.flags;
    unsigned long long stamps_local[17] = {0};
    cx.st = stamps_local;
    {
        gu4 g_units = (gu4)cx.S->kd_units;
        for (uint32_t i = threadIdx.x; i < cx.lds_n; i += blockDim.x) s_units[i] = ld(g_units, i);
    }
    __syncthreads();
    const gf4 rays = (gf4)Q.rays;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < Q.n; i += stride) {
        const float4 a = ld(rays, 2u * i), b = ld(rays, 2u * i + 1u);
        Ray ray;
        ray.o = mk(a.x, a.y, a.z);
        ray.time = a.w;
        ray.d = mk(b.x, b.y, b.z);
        const float tmax = b.w;
        bool ok = rays_finite(a.x) && rays_finite(a.y) && rays_finite(a.z) && rays_finite(a.w) && rays_finite(b.x) &&
                  rays_finite(b.y) && rays_finite(b.z) && !(b.x == 0.f && b.y == 0.f && b.z == 0.f) && tmax > 0.f;
        if (ok && (Q.flags & HRT_RAYS_NORMALIZE)) {  // the Ray constructor (Line.h:13-16); a length that under- or overflows is degenerate
            ray.d = normalize(ray.d);
            ok = rays_finite(ray.d.x) && rays_finite(ray.d.y) && rays_finite(ray.d.z) && !(ray.d.x == 0.f && ray.d.y == 0.f && ray.d.z == 0.f);
        }
        const float a2 = dot(ray.d, ray.d);
        const float olen = length(ray.o);
        cx.err_abs = fabsf(a2 - 1.f) <= 1e-5f ? 2e-6f * (Q.bound + olen + 1.f) : __builtin_inff();
        // an origin far outside the scene: every triangle of a gated mesh is tested (mesh_brute), no walk
        cx.flags = (olen > HRT_RAYS_FAR * (Q.bound + 1.f)) ? (Q.flags | HRT_FLAG_MESH_BRUTE) : Q.flags;
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

int hrt_trace_rays(hrt_scene *s, const float *d_rays, uint32_t n, uint32_t mode, uint32_t flags, void *d_out, void *stream) {
    const std::string who = "hrt_trace_rays";
    if (mode > HRT_QUERY_OCCLUDED) return fail(HRT_ERR_INVALID, who + ": mode must be HRT_QUERY_CLOSEST, _SHADE or _OCCLUDED (got " + std::to_string(mode) + ")");
    const uint32_t known = HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE | HRT_RAYS_NORMALIZE;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": unknown flags bits " + std::to_string(flags & ~known));
    if ((flags & HRT_FLAG_MESH_BRUTE) && !(flags & HRT_FLAG_EXACT_ONLY)) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY");
    if (n > 0u) {
        if (!d_rays) return fail(HRT_ERR_INVALID, who + ": d_rays is NULL");
        if ((uintptr_t)d_rays % 16u) return fail(HRT_ERR_INVALID, who + ": d_rays is not 16-byte aligned");
        if (!d_out) return fail(HRT_ERR_INVALID, who + ": d_out is NULL");
        const uintptr_t align = mode == HRT_QUERY_OCCLUDED ? 4u : 16u;
        if ((uintptr_t)d_out % align) return fail(HRT_ERR_INVALID, who + ": d_out is not " + std::to_string(align) + "-byte aligned");
    }
    if (n > 0x7fffffffu) return fail(HRT_ERR_INVALID, who + ": n must be at most 2^31 - 1 (got " + std::to_string(n) + ")");
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    if (n == 0u) return HRT_OK;
    { const int drc = use_device(s->device); if (drc != HRT_OK) return drc; }
    DRays Q;
    Q.scene = s->d_scene;
    Q.rays = (const float4 *)d_rays;
    Q.out = d_out;
    Q.n = n;
    Q.flags = flags;
    // The tree prefix is NOT staged by default: measured on MI355X (DESIGN.md section 5 "Ray queries"), staging it costs more than it
    // saves for CLOSEST and OCCLUDED (-10..-15 %) and is even for SHADE.  HRT_RAYS_STAGE_TREE builds keep the staged form for A/B runs.
#ifdef HRT_RAYS_STAGE_TREE
    Q.lds_units = (flags & HRT_FLAG_NO_LDS_TREE) ? 0u : std::min<uint32_t>(s->lds_units, 4096u);  // <= 64 KiB: no attribute to raise
#else
    Q.lds_units = 0u;
#endif
    Q.bound = s->bound;
    const bool exact = (flags & HRT_FLAG_EXACT_ONLY) != 0u;
    void (*const kernels[2][3])(const DRays) = {
        {hrt_rays_closest_kernel, hrt_rays_shade_kernel, hrt_rays_occluded_kernel},
        {hrt_rays_closest_exact_kernel, hrt_rays_shade_exact_kernel, hrt_rays_occluded_exact_kernel}};
    void (*const k)(const DRays) = kernels[exact ? 1 : 0][mode];
    const size_t lds_bytes = (size_t)Q.lds_units * 16u;
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k, (int)HRT_RAYS_WG, lds_bytes));
    const uint64_t resident = (uint64_t)std::max(per_cu, 1) * (uint64_t)std::max(g_rt.cus, 1);
    const uint64_t needed = ((uint64_t)n + HRT_RAYS_WG - 1u) / HRT_RAYS_WG;
    const uint32_t grid = (uint32_t)std::min(resident, needed);
    hipLaunchKernelGGL(k, dim3(grid), dim3(HRT_RAYS_WG), lds_bytes, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}
