// Adaptive sampling (include/hrt.h hrt_render_adaptive*): per-tile sample counts set by a noise estimate.  Included by hrt_api.hip
// inside its extern "C" block, after everything it builds on.
//
// The scheme, per 8x8 tile of the rank:
//   round 0   samples [0, min/2) of every tile                                     (trace kernel, accumulating into the sums)
//   round 1   samples [min/2, min) of every tile, then every tile is JUDGED
//   round k   the tiles still active get min(n, max - n) more (the count doubles, clipped at max), then are judged again
// Judging a tile compares its sums before the round (S_old, n_old samples) with those after it (S_new, n_new), per in-image pixel
// in fp32:  A = S_old / n_old,  B = S_new / n_new,  e = (|B.r - A.r| + |B.g - A.g| + |B.b - A.b|) / sqrtf(1e-4 + |B.r| + |B.g| + |B.b|)
// (the two-buffer estimate: the old sums are the first half of the new ones); a pixel whose e is NaN counts as 0.  The tile stays
// active while max e >= threshold and n_new < max.  Active tiles all share one count (they have been active in every round), so a round is one launch of samples
// [n_old, n_new) over the list of active tiles.  A tile's decision reads only its own pixels, and a sample's random numbers depend
// only on (seed, pixel, sample): every tile ends with the bits of a plain render at its count, whatever the rank partition.
//
// Per round, all on the caller's stream:  gather (active tiles' sums -> compact buffer)  ->  trace kernel over the list, samples
// [n_old, n_new) added in sample order  ->  hrt_check_last_launch  ->  judge (one wave per tile)  ->  compact (next list, ascending)
// -> read back the 4-byte length of the next list, which sizes the next launch and ends the loop at 0.  Then the sums become means
// by each tile's own count (and gamma).

#define HRT_AD_WG 256u  // gather / judge / finalize: 4 waves, one tile each

// Active tile k (rank slot list[k], or k itself when list is NULL: every tile) -> slot k of the compact buffer.
extern "C" __global__ void __launch_bounds__(HRT_AD_WG) hrt_ad_gather_kernel(const float *__restrict__ full, const uint32_t *__restrict__ list,
                                                                              uint32_t n, float *__restrict__ compact) {
    const uint32_t k = blockIdx.x * (HRT_AD_WG / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= n) return;
    const uint32_t slot = list ? list[k] : k;
    const float *src = full + ((size_t)slot * 64u + lane) * 3u;
    float *dst = compact + ((size_t)k * 64u + lane) * 3u;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

// One wave per active tile, one lane per pixel: the tile's error (wave max of e over its in-image pixels), S_new back into the
// full buffer, the tile's count, and keep[k] = whether it takes part in the next round.
extern "C" __global__ void __launch_bounds__(HRT_AD_WG) hrt_ad_judge_kernel(const float *__restrict__ compact, float *__restrict__ full,
                                                                             const uint32_t *__restrict__ list, uint32_t n, uint32_t n_old,
                                                                             uint32_t n_new, float threshold, uint32_t max_spp, uint32_t w,
                                                                             uint32_t h, uint32_t rank, uint32_t world, uint32_t tiles_x,
                                                                             uint32_t *__restrict__ counts, uint32_t *__restrict__ keep) {
    const uint32_t k = blockIdx.x * (HRT_AD_WG / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= n) return;  // wave-uniform
    const uint32_t slot = list ? list[k] : k;
    const uint32_t tile = rank + slot * world;
    const uint32_t px = (tile % tiles_x) * 8u + (lane & 7u), py = (tile / tiles_x) * 8u + (lane >> 3);
    const float *b = compact + ((size_t)k * 64u + lane) * 3u;
    float *a = full + ((size_t)slot * 64u + lane) * 3u;
    const float b0 = b[0], b1 = b[1], b2 = b[2];
    float e = 0.f;  // every e is >= 0: lanes outside the image leave the max alone
    if (px < w && py < h) {
#pragma clang fp contract(off)
        const float fo = (float)n_old, fn = (float)n_new;
        const float A0 = a[0] / fo, A1 = a[1] / fo, A2 = a[2] / fo;
        const float B0 = b0 / fn, B1 = b1 / fn, B2 = b2 / fn;
        e = (fabsf(B0 - A0) + fabsf(B1 - A1) + fabsf(B2 - A2)) / sqrtf(1e-4f + fabsf(B0) + fabsf(B1) + fabsf(B2));
        e = e >= 0.f ? e : 0.f;  // a mean that is inf or NaN gives e = NaN: such a pixel counts as 0 (include/hrt.h)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e = fmaxf(e, __shfl_xor(e, off));
    a[0] = b0; a[1] = b1; a[2] = b2;
    if (lane == 0) {
        counts[slot] = n_new;
        keep[k] = (e >= threshold && n_new < max_spp) ? 1u : 0u;
    }
}

// The next list: the rank slots of the kept tiles in ASCENDING order (neighbouring tiles stay together in a streaming-kernel unit;
// the order changes no pixel).  ONE workgroup walks the flags 1024 at a time: ballot + popcount give each kept tile its place
// within its wave, a scan of the 16 wave totals places the waves, and the running base carries over to the next 1024.  *count
// receives the list's length.  (One flag per active tile -- 32 400 at 1080p, 32 passes -- against a trace launch of milliseconds.)
extern "C" __global__ void __launch_bounds__(1024) hrt_ad_compact_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ list,
                                                                          uint32_t n, uint32_t *__restrict__ next, uint32_t *__restrict__ count) {
    __shared__ uint32_t wave_total[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 1024u) {
        const uint32_t k = b0 + tid;
        const bool on = k < n && keep[k] != 0u;
        const uint64_t m = __ballot(on);
        if (lane == 0) wave_total[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = base, total = 0;
        for (uint32_t v = 0; v < 16u; ++v) {
            const uint32_t t = wave_total[v];
            if (v < wave) off += t;
            total += t;
        }
        if (on) next[off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = list ? list[k] : k;
        base += total;
        __syncthreads();  // wave_total is rewritten by the next 1024
    }
    if (tid == 0) *count = base;
}

// sums -> means by each tile's own count, then gamma: the arithmetic of hrt_finalize_kernel (bit-identical when all counts are equal).
// In place (out may alias sums).
extern "C" __global__ void __launch_bounds__(HRT_AD_WG) hrt_ad_finalize_kernel(const float *sums, float *out, uint32_t n_tiles,
                                                                                const uint32_t *__restrict__ counts, uint32_t gamma) {
    const uint32_t k = blockIdx.x * (HRT_AD_WG / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= n_tiles) return;
    const float nspp = (float)counts[k];
    const size_t i = ((size_t)k * 64u + lane) * 3u;
    for (uint32_t c = 0; c < 3u; ++c) {
        float v = sums[i + c] / nspp;
        if (gamma) v = (float)pow((double)v, 1.0 / 2.2);
        out[i + c] = v;
    }
}

// Checked BEFORE the scene and the library state, so that a machine without a GPU can test it.  The parameters alone (also
// hrt_render_lens_adaptive*'s, hrt_lens_adaptive.hip), then with the camera.
static int adaptive_params_check(const std::string &w, const hrt_adaptive *p) {
    if (!p) return fail(HRT_ERR_INVALID, w + ": params is NULL");
    if (p->min_spp < 2u || (p->min_spp & 1u)) return fail(HRT_ERR_INVALID, w + ": min_spp must be even and at least 2 (got " + std::to_string(p->min_spp) + ")");
    if (p->max_spp < p->min_spp) return fail(HRT_ERR_INVALID, w + ": max_spp must be at least min_spp (got " + std::to_string(p->max_spp) + " < " + std::to_string(p->min_spp) + ")");
    if (std::isnan(p->threshold) || p->threshold < 0.f) return fail(HRT_ERR_INVALID, w + ": threshold must be a non-negative number (+inf allowed)");
    return HRT_OK;
}
static int adaptive_check(const char *who, const hrt_adaptive *p, const hrt_camera *cam) {
    const int rc = adaptive_params_check(who, p);
    if (rc != HRT_OK) return rc;
    if (!cam) return fail(HRT_ERR_INVALID, std::string(who) + ": camera is NULL");
    return HRT_OK;
}

// Waits for the trace launch just made, refuses it if the kernel gave up, and adds its event time.
static int adaptive_trace_done(hrt_scene *s, double *kernel_ms) {
    const int rc = hrt_check_last_launch(s);
    if (rc != HRT_OK) return rc;
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, s->ev0, s->ev1));
    *kernel_ms += (double)f;
    return HRT_OK;
}

// The scene's ad_words as a call over n tiles carves it: two tile lists, the judge's keep flags and the count map (n words each),
// then the length of the next list.
struct AdWords {
    uint32_t *lists[2], *keep, *counts, *counter;
    AdWords(hrt_scene *s, size_t n) {
        lists[0] = s->ad_words.as<uint32_t>(); lists[1] = lists[0] + n; keep = lists[1] + n; counts = keep + n; counter = counts + n;
    }
    static size_t bytes(size_t n) { return (4u * n + 1u) * sizeof(uint32_t); }
};

// What the rounds run over: the frame, and the n_tiles tiles that rank of world owns (the lens path: every tile, 0 of 1).
struct AdFrame { uint32_t w, h, tiles_x, n_tiles, rank, world; };

// The rounds, for the camera path (adaptive_run) and the lens path (lens_adaptive_run, hrt_lens_adaptive.hip) alike: d_sums
// (n_tiles tiles, tile-major) ends with the means, d_counts with each tile's count (NULL: the scene's own count map).
//   trace(list, n, first, add, sums, round)   adds samples [first, first + add) of the n tiles of list (NULL: all) onto sums
//   synced(round)                             the round's synchronise has happened
// The HIP calls, in order, all on `stream`: ad_compact and ad_words grown; the sums zeroed; trace of round 0, [0, min/2) onto
// d_sums.  Then per round from 1, while the list is not empty: gather -> trace onto the compact buffer -> judge -> compact -> the
// 4-byte length of the next list copied back -> hipStreamSynchronize -> synced -> done += add, the lists swap.  At length 0 the
// finalize kernel.  Whatever else a path does per round (the camera path waits for its trace launch and reads its time, so a
// kernel that gave up ends the call before the judge; the lens path records events) it does inside its two callables.
extern "C++" {
template <class Trace, class Synced>
static int adaptive_rounds(hrt_scene *s, const AdFrame &F, const hrt_adaptive *p, bool gamma, float *d_sums, uint32_t *d_counts,
                           hipStream_t stream, Trace trace, Synced synced) {
    const uint32_t n_tiles = F.n_tiles;
    const size_t sum_bytes = (size_t)n_tiles * 192u * sizeof(float);
    int rc;
    if ((rc = s->ad_compact.grow(sum_bytes)) != HRT_OK || (rc = s->ad_words.grow(AdWords::bytes(n_tiles))) != HRT_OK) return rc;
    float *const compact = s->ad_compact.as<float>();
    const AdWords A(s, n_tiles);
    if (!d_counts) d_counts = A.counts;
    const uint32_t half = p->min_spp / 2u;

    HIP_TRY(hipMemsetAsync(d_sums, 0, sum_bytes, stream));
    if ((rc = trace(nullptr, n_tiles, 0u, half, d_sums, 0u)) != HRT_OK) return rc;  // round 0
    uint32_t done = half, n = n_tiles, next = 0;
    const uint32_t *active = nullptr;  // round 1: every tile
    for (uint32_t round = 1; n != 0u; ++round) {
        const uint32_t add = round == 1u ? half : std::min(done, p->max_spp - done);
        const dim3 grid((n + HRT_AD_WG / 64u - 1u) / (HRT_AD_WG / 64u));
        hipLaunchKernelGGL(hrt_ad_gather_kernel, grid, dim3(HRT_AD_WG), 0, stream, d_sums, active, n, compact);
        HIP_TRY(hipGetLastError());
        if ((rc = trace(active, n, done, add, compact, round)) != HRT_OK) return rc;
        hipLaunchKernelGGL(hrt_ad_judge_kernel, grid, dim3(HRT_AD_WG), 0, stream, compact, d_sums, active, n, done, done + add,
                           p->threshold, p->max_spp, F.w, F.h, F.rank, F.world, F.tiles_x, d_counts, A.keep);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hrt_ad_compact_kernel, dim3(1), dim3(1024), 0, stream, A.keep, active, n, A.lists[round & 1u], A.counter);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&next, A.counter, sizeof(next), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if ((rc = synced(round)) != HRT_OK) return rc;
        done += add;
        active = A.lists[round & 1u];
        n = next;
    }
    hipLaunchKernelGGL(hrt_ad_finalize_kernel, dim3((n_tiles + HRT_AD_WG / 64u - 1u) / (HRT_AD_WG / 64u)), dim3(HRT_AD_WG), 0, stream, d_sums, d_sums,
                       n_tiles, d_counts, gamma ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}
}  // extern "C++"

// The tail of the two blocking forms: the scene's count map of a whole w x h frame to the host and, if wanted, on to
// out_tile_spp; *samples (if wanted): the in-image samples, every in-image pixel having its tile's count.
static int adaptive_counts_to_host(hrt_scene *s, uint32_t w, uint32_t h, uint32_t *out_tile_spp, uint64_t *samples) {
    const uint32_t tiles = hrt_tiles_total(w, h), tx = (w + HRT_TILE - 1) / HRT_TILE;
    std::vector<uint32_t> counts(tiles);
    HIP_TRY(hipMemcpy(counts.data(), AdWords(s, tiles).counts, (size_t)tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_tile_spp) std::memcpy(out_tile_spp, counts.data(), (size_t)tiles * sizeof(uint32_t));
    if (!samples) return HRT_OK;
    *samples = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t x0 = (t % tx) * HRT_TILE, y0 = (t / tx) * HRT_TILE;
        *samples += (uint64_t)std::min<uint32_t>(HRT_TILE, w - x0) * std::min<uint32_t>(HRT_TILE, h - y0) * counts[t];
    }
    return HRT_OK;
}

// The rounds over this rank's tiles with the trace kernels.  fill_render comes first (the frame, the partition; the scene's
// device), and a rank without tiles is done before anything is grown or touched.  Every trace launch is waited for at once.
static int adaptive_run(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, const hrt_adaptive *p, uint64_t seed, uint32_t flags,
                        uint32_t rank, uint32_t world, float *d_sums, uint32_t *d_counts, hipStream_t stream, double *kernel_ms) {
    *kernel_ms = 0.0;
    DRender R;
    DCamera C;
    const int rc = fill_render(s, cam, w, h, p->min_spp, seed, flags, rank, world, R, C);
    if (rc != HRT_OK) return rc;
    if (R.tiles_owned == 0u) return HRT_OK;
    TraceJob job{w, h, 0u, 0u, seed, flags, d_sums, stream};
    job.rank = rank; job.world = world; job.accumulate = true;
    return adaptive_rounds(
        s, AdFrame{w, h, R.tiles_x, R.tiles_owned, rank, world}, p, (flags & HRT_FLAG_GAMMA) != 0u, d_sums, d_counts, stream,
        [&](const uint32_t *list, uint32_t n, uint32_t first, uint32_t add, float *sums, uint32_t) -> int {
            job.s0 = first; job.spp = add; job.d_tiles = sums; job.list = list; job.list_n = n;  // list_n counts only with a list
            const int trc = launch_trace(s, cam, job);
            return trc != HRT_OK ? trc : adaptive_trace_done(s, kernel_ms);
        },
        [](uint32_t) -> int { return HRT_OK; });
}

int hrt_render_adaptive_tiles(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, const hrt_adaptive *params, uint64_t seed,
                              uint32_t flags, uint32_t rank, uint32_t world, float *d_tiles, uint32_t *d_tile_spp, void *stream) {
    int rc = adaptive_check("hrt_render_adaptive_tiles", params, cam);
    if (rc != HRT_OK) return rc;
    if (!d_tiles) return fail(HRT_ERR_INVALID, "hrt_render_adaptive_tiles: d_tiles is NULL");
    if (!d_tile_spp) return fail(HRT_ERR_INVALID, "hrt_render_adaptive_tiles: d_tile_spp is NULL");
    if ((rc = enter_scene("hrt_render_adaptive_tiles", s)) != HRT_OK) return rc;
    double ms = 0.0;
    return adaptive_run(s, cam, w, h, params, seed, flags, rank, world, d_tiles, d_tile_spp, (hipStream_t)stream, &ms);
}

int hrt_render_adaptive(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, const hrt_adaptive *params, uint64_t seed,
                        uint32_t flags, float *out_rgb, uint32_t *out_tile_spp, hrt_stats *stats) {
    int rc = adaptive_check("hrt_render_adaptive", params, cam);
    if (rc != HRT_OK) return rc;
    if (!out_rgb) return fail(HRT_ERR_INVALID, "hrt_render_adaptive: out_rgb is NULL");
    if ((rc = enter_scene("hrt_render_adaptive", s)) != HRT_OK) return rc;
    if ((rc = check_frame("hrt_render_adaptive", w, h, k_max_pixels)) != HRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t tiles = hrt_tiles_total(w, h);
    const size_t frame_bytes = (size_t)w * h * 3 * sizeof(float);
    if ((rc = s->tiles.grow((size_t)tiles * 64 * 3 * sizeof(float))) != HRT_OK || (rc = s->frame.grow(frame_bytes)) != HRT_OK) return rc;
    double ms = 0.0;
    rc = adaptive_run(s, cam, w, h, params, seed, flags, 0, 1, s->tiles.as<float>(), nullptr, nullptr, &ms);  // the count map: the scene's
    if (rc == HRT_OK) rc = hrt_assemble_frame(s->tiles.as<float>(), tiles, w, h, 1, s->frame.as<float>(), nullptr);
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->frame.p, frame_bytes, hipMemcpyDeviceToHost));
    uint64_t samples = 0;
    if ((rc = adaptive_counts_to_host(s, w, h, out_tile_spp, stats ? &samples : nullptr)) != HRT_OK) return rc;
    if (stats) fill_stats(s, stats, t0, ms, samples);
    return HRT_OK;
}
