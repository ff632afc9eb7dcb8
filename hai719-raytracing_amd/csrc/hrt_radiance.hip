// Radiance queries on caller rays (include/hrt.h hrt_trace_radiance) and the camera rays of a frame (hrt_camera_rays).
// Included by hrt_api.hip inside its extern "C" block, after hrt_rays.hip (the query helpers) and hrt_denoise.hip (camera_sample).
//
// hrt_radiance_kernel is trace_body (hrt_kernels.hip) with the camera taken out: one lane per ray, and per sample one path whose
// first segment is the caller's ray, then the same stages -- A (spheres, squares, mesh gates), B (mesh walks, deferred until
// HRT_MESH_BATCH lanes of the wave are parked or nobody else can move), C (shade, direct light, scatter, sky) -- with the same
// pruning and the same sum.  A lane that finishes the last sample of its ray stores it and takes its next ray by a grid stride
// at once, without waiting for the rest of the wave; work is assigned by lane index alone, so no scene state is touched (the
// call may overlap a render of the same scene).  The ray record is read again at the start of every sample (two 16-byte loads)
// instead of being kept in registers across the path.
//
// Filter margin and far origins are query_margin's (hrt_rays.hip, DESIGN.md section 5 "Ray queries"): the margin holds for the
// whole path (bounce origins lie within `bound`); the far-origin flag for its first segment only, bounce segments are walked.

#define HRT_RADIANCE_WG 256u
#ifndef HRT_RADIANCE_MIN_WAVES
#define HRT_RADIANCE_MIN_WAVES 5  // waves per SIMD the register allocator leaves room for; A/B on MI355X, 1080p x 16 samples, tree from
                                  // global memory: 4 -> 5 is +20 % on Cornell+mesh, +14 % on the pool, +15 % on random_spheres (DESIGN.md
                                  // section 5 "Radiance queries")
#endif
#ifndef HRT_RADIANCE_STAGE_TREE
#define HRT_RADIANCE_STAGE_TREE 0  // -DHRT_RADIANCE_STAGE_TREE: the A/B build that stages the tree prefix (see hrt_trace_radiance)
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

// Where a lane's first segments come from (radiance_body's SRC).  RecordRays: record i of the caller's batch, one ray for all its
// samples, keyed by Q.keys.  A source with per_sample (LensRays, LensViewRays, LensTileRays, hrt_lens.hip) makes the ray of every sample itself
// -- SRC::sample(Q, i, sample, ray), false for a sample that is not traced -- and says how item i's samples are keyed: SRC::key(Q, i)
// and SRC::seed(Q, i, lo, hi).  LensRays: lane i is pixel i with key i and the launch's seed.  LensTileRays: item i is a lane of
// a listed 8 x 8 tile, keyed by that lane's pixel.
struct RecordRays {
    static constexpr bool per_sample = false;
};

// A per-sample source with wave_items (ProbeRays, hrt_probes.hip) spreads the samples of one item over the 64 lanes of a WAVE and
// keeps what a finished sample is added to itself.  Q.n then counts lanes (64 per item), lane i works for item i / 64, and the
// source says which samples are the lane's -- s = SRC::first(Q, i), then every 64th below SRC::end(Q, i), counted from first_sample
// --, takes every finished sample (SRC::add) and, once no lane of the wave has a sample left, closes the item (SRC::finish, in
// which all 64 lanes take part) before the wave takes its next one (SRC::begin).  Every other source is untouched by this: all of
// it is behind `if constexpr`.
template <class SRC, class = void>
struct src_wave_items { static constexpr bool value = false; };
template <class SRC>
struct src_wave_items<SRC, std::enable_if_t<SRC::wave_items>> { static constexpr bool value = true; };

// Where a path ends before its bounces run out (radiance_body's TAIL).  NoTail: nowhere -- every family but those of
// hrt_lit_paths.hip, whose policies end a path at its Q.tail_after-th diffuse hit WITHOUT scattering there: kind 1 gathers there
// (TAIL::gather: the look-up of a probe volume), kind 2 writes the path's end out instead of its colour (TAIL::reached /
// ::unreached / ::degenerate: 16 floats per ray where the others store 3).  Kind 3 (hrt_path_features.hip) is kind 2 with K = 1 and a
// feature record for a tail record: it keeps the emission seen on the way in `rad` (no direct light, no sky) and the summed hit
// distances in `depth`, and where the source makes the ray of every sample it folds the records of an item's samples in the item's
// output (TAIL::begin / ::finish).  A path with a tail is not pruned.  Every other family is untouched by this: all of it is behind
// `if constexpr`.
struct NoTail {
    static constexpr int kind = 0;
};

template <bool LIGHTS, bool EXACT, class SRC = RecordRays, class QT = DRadiance, class TAIL = NoTail>
__device__ __forceinline__ void radiance_body(const QT &Q) {
    constexpr bool WAVE = src_wave_items<SRC>::value;
    CtxT<EXACT, false, false, true> cx;
    unsigned long long stamps_local[17] = {0};
    query_context(cx, Q.scene, Q.lds_units, Q.flags, stamps_local);
    const bool has_mesh = cx.S->n_meshes != 0u;
    const bool prune = TAIL::kind == 0 && !EXACT && cx.S->prune_ok != 0u;  // as trace_body
    const bool sky_is_zero = cx.S->skybox_image < 0 && cx.S->dark_sky != 0;
    const bool accumulate = (Q.flags & HRT_RADIANCE_ACCUMULATE) != 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    const float far = query_far(Q.bound);

    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // this lane's ray
    uint32_t key = 0;        // its RNG key
    uint32_t first_flags = Q.flags;  // cx.flags of its first segments (+ MESH_BRUTE for a far origin)
    f3 sum = mk(0.f, 0.f, 0.f);
    uint32_t s = 0;          // next sample of this lane's ray
    [[maybe_unused]] uint32_t count = 0;  // a wave_items source: where the samples of the wave's item end (s runs in steps of 64)
    int remaining = 0;       // bounces left on the current path; 0 = needs a new path
    [[maybe_unused]] uint32_t diffuse = 0;  // a TAIL: the diffuse hits of the current path so far
    [[maybe_unused]] float depth = 0.f;     // TAIL kind 3: the hit distances of the current path so far
    Ray ray;
    ray.o = mk(0.f, 0.f, 0.f); ray.d = mk(0.f, 0.f, 1.f); ray.time = 0.f;
    f3 thr = mk(1.f, 1.f, 1.f), rad = mk(0.f, 0.f, 0.f);
    Rng rng;
    rng.k0 = rng.k1 = rng.i = 0;
    float tmax;              // of the record: a path's first segment has no far end
    Hit h;
    h.kind = 0; h.index = 0; h.t = HRT_FLT_MAX; h.tri = 0; h.a0 = 0.f; h.a1 = 0.f;
    uint32_t parked = 0;     // meshes whose box this lane's ray enters and that are still to be walked
    uint32_t stage = 0;      // 0: needs stage A   1: parked for stage B   2: ready for stage C   3: pruned   4: a sample that is not traced
    bool live = false;

    // The lane's next ray from i on that is not degenerate: its key, margin, flags and starting sum.  A degenerate ray adds
    // nothing: 0 in mean mode, its sums left as they are under HRT_RADIANCE_ACCUMULATE.
    // A per-sample source has no ray yet: every pixel is live, and a sample that is not traced is skipped where it is made.
    auto next_ray = [&]() {
        live = false;
        if constexpr (WAVE) {  // the wave's next item: this lane's share of its samples, nothing of `sum` or Q.out
            if (i < Q.n) {
                SRC::begin(Q, i);
                key = SRC::key(Q, i);
                s = SRC::first(Q, i);
                count = SRC::end(Q, i);
                live = s < count;
            }
            return;
        }
        if constexpr (SRC::per_sample) {
            live = i < Q.n;
        } else {
            for (; i < Q.n; i += stride) {
                if (query_ray(Q, i, ray, tmax)) {
                    live = true;
                    break;
                }
                if constexpr (TAIL::kind >= 2) {
                    TAIL::degenerate(Q, i);
                } else if (!accumulate) { float *o_ = Q.out + (size_t)i * 3u; o_[0] = 0.f; o_[1] = 0.f; o_[2] = 0.f; }
            }
        }
        if (live) {
            if constexpr (SRC::per_sample) {
                key = SRC::key(Q, i);
            } else {
                key = Q.keys ? Q.keys[i] : i;
                query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, first_flags);
            }
            sum = mk(0.f, 0.f, 0.f);
            if constexpr (TAIL::kind == 3) {
                if constexpr (SRC::per_sample) TAIL::begin(Q, i);  // the item's sums, from +0
            } else {
                if (accumulate) { const float *a_ = Q.out + (size_t)i * 3u; sum = mk(a_[0], a_[1], a_[2]); }
            }
            s = 0;
        }
    };

    // Whether the wave has work.  A wave_items source: the item boundary -- the wave meets here once none of its lanes has a
    // sample left, closes the item with all 64 lanes and takes the next one by a wave-granular grid stride (Q.n and the stride are
    // multiples of 64, so i < Q.n holds for a whole wave or for none of it).
    auto more = [&]() -> bool {
        if constexpr (WAVE) {
            while (__ballot(live) == 0ull && __ballot(i < Q.n) != 0ull) {
                SRC::finish(Q, i);
                i += stride;
                next_ray();
            }
        }
        return __ballot(live) != 0ull;
    };

    next_ray();
    while (more()) {
        // ---- stage A: (re)start a path, spheres + squares, mesh gates
        if (live && stage == 0u) {
            bool traced = true;    // a per-sample source may make a sample that is not traced: it ends at once, nothing is added
            if (remaining == 0) {  // sample first_sample + s of ray i: the caller's ray, RNG stream (seed, key, sample) from draw 3
                if constexpr (SRC::per_sample) {  // this sample's own ray, and the margin and far-origin flag of that ray
                    traced = SRC::sample(Q, i, Q.first_sample + s, ray);
                    if (traced) query_margin(ray, Q.bound, far, Q.flags, cx.err_abs, first_flags);
                } else {
                    (void)query_ray(Q, i, ray, tmax);
                }
                if constexpr (SRC::per_sample) {
                    uint32_t seed_lo, seed_hi;
                    SRC::seed(Q, i, seed_lo, seed_hi);
                    rng.start(seed_lo, seed_hi, key, Q.first_sample + s);
                } else {
                    rng.start(Q.seed_lo, Q.seed_hi, key, Q.first_sample + s);
                }
                rng.i = 3u;  // draws 0..2 are the camera's u, v, time
                cx.flags = first_flags;
                thr = mk(1.f, 1.f, 1.f);
                rad = mk(0.f, 0.f, 0.f);
                remaining = 6;  // MAXBOUNCES
                if constexpr (TAIL::kind != 0) diffuse = 0u;
                if constexpr (TAIL::kind == 3) depth = 0.f;
            }
            if (SRC::per_sample && !traced) {
                h.kind = 0u; parked = 0u; stage = 4u;  // ends below
            } else {
                h = prims_hit(cx, ray);
                parked = has_mesh ? mesh_gates(cx, ray) : 0u;
                stage = parked ? 1u : 2u;
            }
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
            [[maybe_unused]] bool fired = false;            // a TAIL: this hit is the path's tail
            [[maybe_unused]] f3 G = mk(0.f, 0.f, 0.f);      // TAIL kind 1: what it gathers there
            [[maybe_unused]] const uint32_t segment = 7u - (uint32_t)remaining;  // TAIL kind 2: the segments traced so far, this one included
            if (stage == 3u || (SRC::per_sample && stage == 4u)) {
                ended = true;  // pruned on its last segment (stage A), or not traced: nothing is added
            } else if (h.kind == 0u) {
                if constexpr (TAIL::kind != 3) rad = rad + thr * sky(cx, ray.d, remaining);
                ended = true;
            } else {
                const Surface sf = shade(cx, ray, h);
                f3 direct = mk(0.f, 0.f, 0.f);
                if (LIGHTS) direct = direct_light(cx, sf, ray, rng);
                if constexpr (TAIL::kind == 3) {  // the draws of `direct` move the stream; its value is not a feature
                    rad = rad + thr * sf.emission;
                    depth = depth + h.t;
                } else {
                    rad = rad + thr * (direct + sf.emission);
                }
                thr = thr * sf.albedo;
                if constexpr (TAIL::kind == 3) fired = sf.type == 0u;
                else if constexpr (TAIL::kind != 0) fired = sf.type == 0u && ++diffuse == Q.tail_after;
                if constexpr (TAIL::kind == 1) { if (fired) G = TAIL::gather(Q, sf.p, sf.n); }
                if constexpr (TAIL::kind == 2) { if (fired) TAIL::reached(Q, i, sf.p, ray.time, sf.n, thr, segment, rad); }
                if constexpr (TAIL::kind == 3) { if (fired) TAIL::template reached<SRC::per_sample>(Q, i, thr, sf.n, rad, depth); }
                if (fired) {
                    ended = true;  // without scattering
                } else {
                    scatter(sf, ray, rng);
                    cx.flags = Q.flags;  // bounce segments are walked
                    --remaining;
                    ended = (remaining == 0) || (prune && thr.x == 0.f && thr.y == 0.f && thr.z == 0.f);
                }
            }
            if (ended) {
                if constexpr (TAIL::kind == 2) { if (!fired) TAIL::unreached(Q, i, segment, rad); }
                if constexpr (TAIL::kind == 3) { if (!fired && !(SRC::per_sample && stage == 4u)) TAIL::template unreached<SRC::per_sample>(Q, i, rad); }
                if constexpr (WAVE) {  // the sink is the source's: it gets what a one-sample query stores, 0 + rad / 6
                    if constexpr (TAIL::kind == 1) {  // (rad / 6) + thr * G where the tail was reached
                        if (stage != 4u)
                            SRC::add(Q, i, Q.first_sample + s,
                                     mk(0.f, 0.f, 0.f) + (fired ? mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f) + thr * G : mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f)));
                    } else {
                        if (stage != 4u) SRC::add(Q, i, Q.first_sample + s, mk(0.f, 0.f, 0.f) + mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f));
                    }
                } else if (!(SRC::per_sample && stage == 4u)) {
                    if constexpr (TAIL::kind == 3) {
                        // the record is in the output
                    } else if constexpr (TAIL::kind == 1) {
                        sum = sum + (fired ? mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f) + thr * G : mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f));
                    } else {
                        sum = sum + mk(rad.x / 6.f, rad.y / 6.f, rad.z / 6.f);  // Scene.h:348
                    }
                }
                remaining = 0;
                if constexpr (WAVE) {
                    if (count - s <= 64u) live = false;  // out of samples: idle until the wave meets in more()
                    else s += 64u;
                } else if (++s == Q.n_samples) {  // the ray is done: its mean (or running sum), then the lane's next ray
                    if constexpr (TAIL::kind == 3) {  // kind 3 has written its record, or holds the item's sums there
                        if constexpr (SRC::per_sample) TAIL::finish(Q, i);
                    } else if constexpr (TAIL::kind != 2) {  // kind 2 has written its record
                        const float ns = accumulate ? 1.f : (float)Q.n_samples;  // x / 1.f is exact
                        float *o = Q.out + (size_t)i * 3u;
                        o[0] = sum.x / ns; o[1] = sum.y / ns; o[2] = sum.z / ns;
                    }
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
    const Ray r = camera_sample(&C, seed_lo, seed_hi, w, h, pixel, sample);
    out[2u * pixel] = make_float4(r.o.x, r.o.y, r.o.z, r.time);
    out[2u * pixel + 1u] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_inff());
}

// A family of kernels: the four builds of one body over launch record QT -- plain, lights, and the two proof builds of
// HRT_FLAG_EXACT_ONLY (no filters, no v_rcp_f32; see CtxT) -- and their table, indexed lights | exact << 1 (radiance_launch).
// BOUNDS and PROOF_BOUNDS are the parenthesised __launch_bounds__ of the first and the last two; BODY<lights, exact, ...>(Q) is the
// body, the variadic arguments its template arguments after the two flags.
#define HRT_KERNEL_FAMILY(base, QT, BOUNDS, PROOF_BOUNDS, BODY, ...)                                                                    \
    extern "C" __global__ void __launch_bounds__ BOUNDS base(const QT Q) { BODY<false, false, __VA_ARGS__>(Q); }                       \
    extern "C" __global__ void __launch_bounds__ BOUNDS base##_lights(const QT Q) { BODY<true, false, __VA_ARGS__>(Q); }               \
    extern "C" __global__ void __launch_bounds__ PROOF_BOUNDS base##_exact(const QT Q) { BODY<false, true, __VA_ARGS__>(Q); }          \
    extern "C" __global__ void __launch_bounds__ PROOF_BOUNDS base##_lights_exact(const QT Q) { BODY<true, true, __VA_ARGS__>(Q); }    \
    static void (*const base##_builds[4])(const QT) = {base, base##_lights, base##_exact, base##_lights_exact};

// A family of radiance_body kernels over source SRC (the proof builds are not tuned: 2 waves per SIMD, as trace_body's).
#define HRT_RADIANCE_FAMILY(base, SRC, QT) \
    HRT_KERNEL_FAMILY(base, QT, (HRT_RADIANCE_WG, HRT_RADIANCE_MIN_WAVES), (HRT_RADIANCE_WG, 2), radiance_body, SRC)

HRT_RADIANCE_FAMILY(hrt_radiance_kernel, RecordRays, DRadiance)

struct DLensViewsRadiance;  // hrt_lens.hip: the one record without a launch seed (every view has its own), and what derives from it

extern "C++" {
template <class QT>
static void radiance_seed(QT &Q, uint64_t seed) {
    if constexpr (!std::is_base_of_v<DLensViewsRadiance, QT>) {
        Q.seed_lo = (uint32_t)seed;
        Q.seed_hi = (uint32_t)(seed >> 32);
    }
}

// THE launch of a radiance_body family (the scene entered): fills what every record has -- the caller has set its family's own
// fields -- picks the build and launches it over n items into `out` on `stream`.
// The tree prefix is NOT staged by default: measured on MI355X (DESIGN.md section 5 "Radiance queries"), its 36 KiB per workgroup
// cost a fifth of the resident waves at 5 waves per SIMD and -12..-16 % on the mesh scenes.  HRT_RADIANCE_STAGE_TREE builds keep
// the staged form for A/B runs (HRT_FLAG_NO_LDS_TREE turns it off there).
template <class QT>
static int radiance_launch(void (*const *builds)(const QT), QT &Q, const hrt_scene *s, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                           uint32_t flags, float *out, uint32_t n, void *stream) {
    Q.out = out;
    Q.n = n;
    Q.flags = flags;
    Q.first_sample = first_sample;
    Q.n_samples = n_samples;
    radiance_seed(Q, seed);
    const uint32_t build = (s->d.n_lights != 0u ? 1u : 0u) | ((flags & HRT_FLAG_EXACT_ONLY) ? 2u : 0u);
    return query_launch(builds[build], Q, s, HRT_RADIANCE_STAGE_TREE, HRT_RADIANCE_WG, stream);
}

// THE blocking host form of a family (hrt_render_lens, hrt_render_lens_views, hrt_bake): a result buffer and two timing events of
// the call's own (owners: gone on every way out), so that this form, too, leaves the scene's state alone.
struct BlockingCall {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    // launch(d_out) on the null stream between the events, its `bytes` of result into `out`, and the stats of `samples` samples.
    template <class F>
    int run(const hrt_scene *s, size_t bytes, float *out, uint64_t samples, hrt_stats *stats, F launch) {
        Scratch d_out;
        Event ev0, ev1;
        float ms = 0.f;
        if (const int rc = d_out.grow(bytes)) return rc;
        if (const int rc = ev0.ready()) return rc;
        if (const int rc = ev1.ready()) return rc;
        HIP_TRY(hipEventRecord(ev0, nullptr));
        if (const int rc = launch(d_out.as<float>())) return rc;
        HIP_TRY(hipEventRecord(ev1, nullptr));
        HIP_TRY(hipMemcpy(out, d_out.p, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        if (stats) {
            fill_stats(s, stats, t0, (double)ms, samples);
            stats->lds_bytes = 0u;  // the tree is read from global memory
            stats->waves_launched = 0u;
        }
        return HRT_OK;
    }
    // The same for a batch in host memory: its n records of `record_bytes` and its keys (NULL: none) are device buffers of the
    // call's, too -- launch(d_records, d_keys, d_out, the null stream).
    template <class F>
    int run_batch(const hrt_scene *s, const float *records, size_t record_bytes, const uint32_t *keys, uint32_t n, size_t bytes, float *out,
                  uint64_t samples, hrt_stats *stats, F launch) {
        Scratch d_records, d_keys;
        if (const int rc = d_records.from_host(records, (size_t)n * record_bytes)) return rc;
        if (keys)
            if (const int rc = d_keys.from_host(keys, (size_t)n * sizeof(uint32_t))) return rc;
        return run(s, bytes, out, samples, stats,
                   [&](float *d_out) { return launch(d_records.as<float>(), d_keys.as<uint32_t>(), d_out, nullptr); });
    }
};
}  // extern "C++"

// The two forms of an entry point share one body with the form as a parameter (`dev`: the device form -- d_ names, a stream, no
// stats).  What only the blocking form has, first of all its checks: running sums would have to be on the device.
static int blocking_accumulate_check(const std::string &who, uint32_t flags) {
    if (flags & HRT_RADIANCE_ACCUMULATE)
        return fail(HRT_ERR_INVALID, who + ": flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (" + who + "_device)");
    return HRT_OK;
}

// An empty batch, of either form (the device form has no stats): nothing is launched, the stats are zeroed.
static int empty_batch(hrt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return HRT_OK;
}

// What a plain entry point has where its lit sibling has a LitRule (hrt_probe_lit.hip): nothing to check, and the scene to enter.
struct NoRule {
    int check_tail(const std::string &) const { return HRT_OK; }
    int check_volume(const std::string &) const { return HRT_OK; }
    int check(const std::string &) const { return HRT_OK; }
    int enter(const std::string &who, hrt_scene *s) const { return enter_scene(who, s); }
};

// The flags of a fused launch (lens frames, bakes).  one_form: why the kernel-form flags are refused; no_normalize: why
// HRT_RAYS_NORMALIZE is; no_gamma: why HRT_FLAG_GAMMA is, NULL where it is accepted.
static int fused_flags_check(const std::string &who, uint32_t flags, const char *one_form, const char *no_normalize, const char *no_gamma) {
    const struct { uint32_t bit; const char *name; const char *why; } refused[] = {
        {HRT_FLAG_WAVE_KERNEL, "HRT_FLAG_WAVE_KERNEL", one_form},
        {HRT_FLAG_STREAM_KERNEL, "HRT_FLAG_STREAM_KERNEL", one_form},
        {HRT_FLAG_DUAL_KERNEL, "HRT_FLAG_DUAL_KERNEL", one_form},
        {HRT_FLAG_NO_SHADOW_CULL, "HRT_FLAG_NO_SHADOW_CULL", "the query kernels have no such build"},
        {HRT_RAYS_NORMALIZE, "HRT_RAYS_NORMALIZE", no_normalize},
        {no_gamma ? HRT_FLAG_GAMMA : 0u, "HRT_FLAG_GAMMA", no_gamma}};
    for (const auto &f : refused)
        if (flags & f.bit) return fail(HRT_ERR_INVALID, who + ": flags: " + f.name + ": " + f.why);
    const uint32_t known = HRT_FLAG_EXACT_ONLY | HRT_FLAG_MESH_BRUTE | HRT_FLAG_NO_LDS_TREE | HRT_RADIANCE_ACCUMULATE | HRT_FLAG_GAMMA;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": flags: unknown bits " + std::to_string(flags & ~known));
    { const int brc = check_mesh_brute(who, flags); if (brc != HRT_OK) return brc; }
    if ((flags & HRT_FLAG_GAMMA) && (flags & HRT_RADIANCE_ACCUMULATE))
        return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_GAMMA cannot be combined with HRT_RADIANCE_ACCUMULATE (running sums are linear)");
    return HRT_OK;
}

// The samples and the output of a fused launch.
static int samples_out_check(const std::string &who, uint32_t first_sample, uint32_t n_samples, const float *out, const char *out_name) {
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is not 4-byte aligned");
    return HRT_OK;
}

// The last checks of an entry point that writes rays as records (hrt_camera_rays, hrt_lens_rays, hrt_bake_rays).
static int rays_out_check(const std::string &who, const float *d_rays) {
    if (!d_rays) return fail(HRT_ERR_INVALID, who + ": d_rays is NULL");
    if ((uintptr_t)d_rays % 16u) return fail(HRT_ERR_INVALID, who + ": d_rays is not 16-byte aligned");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    return HRT_OK;
}

// The pointers come before n_samples here (include/hrt.h), and d_out may be NULL for an empty batch: not samples_out_check's order.
int hrt_trace_radiance(hrt_scene *s, const float *d_rays, const uint32_t *d_keys, uint32_t n, uint32_t first_sample, uint32_t n_samples,
                       uint64_t seed, uint32_t flags, float *d_out, void *stream) {
    const std::string who = "hrt_trace_radiance";
    int rc = query_check(who, flags, HRT_RADIANCE_ACCUMULATE, d_rays, d_keys, d_out, 4u, n);
    if (rc != HRT_OK) return rc;
    if (n_samples == 0u) return fail(HRT_ERR_INVALID, who + ": n_samples must be positive");
    if ((uint64_t)first_sample + n_samples > 0x100000000ull)
        return fail(HRT_ERR_INVALID, who + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)");
    rc = enter_scene(who, s, n != 0u);  // also checked for an empty batch, which leaves the current device alone
    if (rc != HRT_OK || n == 0u) return rc;
    DRadiance Q;
    Q.rays = (const float4 *)d_rays;
    Q.keys = d_keys;
    return radiance_launch(hrt_radiance_kernel_builds, Q, s, first_sample, n_samples, seed, flags, d_out, n, stream);
}

int hrt_camera_rays(const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t sample, uint64_t seed, float *d_rays, void *stream) {
    const std::string who = "hrt_camera_rays";
    if (!cam) return fail(HRT_ERR_INVALID, who + ": cam is NULL");
    DCamera C;
    { const int crc = make_camera(cam, C); if (crc != HRT_OK) return crc; }  // refused as hrt_render refuses it
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    { const int rrc = rays_out_check(who, d_rays); if (rrc != HRT_OK) return rrc; }
    const uint32_t npix = w * h;
    hipLaunchKernelGGL(hrt_camera_rays_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, C, w, h, sample,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (float4 *)d_rays);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}
