// Batched views (include/hrt.h hrt_render_views*): many cameras of one scene in ONE trace launch.  Included by hrt_api.hip inside
// its extern "C" block, after everything it builds on.
//
// N views of w x h become one work queue of N x tiles items: item j is tile j % tiles of view j / tiles (rank 0 of world 1).  The
// *_views builds of the trace kernels (hrt_kernels.hip trace_body, hrt_stream.hip stream_body; template axis VIEWS) take the camera,
// the seed and the filters' margin of an item from its view's block (hrt_device.h DView) instead of the launch's argument block,
// and write item-major tile sums; one assemble launch then writes every view's row-major frame.  A sample is keyed (seed of its
// view, pixel inside its view, sample) and folded in sample order as ever, so frame v has the bits of hrt_render of view v.

// Item-major tile sums of all views -> view-major, row-major frames.
extern "C" __global__ void __launch_bounds__(256) hrt_assemble_views_kernel(const float *__restrict__ tiles, uint32_t tiles_per_view, uint32_t w,
                                                                            uint32_t h, uint32_t n_pixels, float *__restrict__ frames) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;  // pixel of all views: n_pixels = views * w * h <= 2^30 (HRT_VIEWS_MAX_TILES)
    if (idx >= n_pixels) return;
    const uint32_t view = idx / (w * h), p = idx % (w * h), x = p % w, y = p / w;
    const uint32_t tile = (y / 8u) * ((w + 7u) / 8u) + (x / 8u), lane = (y & 7u) * 8u + (x & 7u);
    const float *src = tiles + (((size_t)view * tiles_per_view + tile) * 64u + lane) * 3u;
    float *dst = frames + (size_t)idx * 3u;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

// Checked BEFORE the scene and the library state, so that a machine without a GPU can test it.  Fills one block per view (all but
// err_abs, which needs the scene's extent).
static int views_check(const std::string &who, const hrt_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t spp, uint32_t flags,
                       const float *out, const char *out_name, std::vector<DView> &blocks) {
    if (flags & HRT_FLAG_DUAL_KERNEL) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_DUAL_KERNEL: there is no batched build of the two-stream kernel");
    if (flags & HRT_FLAG_EXACT_ONLY) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_EXACT_ONLY: there are no batched proof builds");
    if (flags & HRT_FLAG_MESH_BRUTE) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_MESH_BRUTE: there are no batched proof builds");
    const uint32_t known = HRT_FLAG_GAMMA | HRT_FLAG_NO_LDS_TREE | HRT_FLAG_WAVE_KERNEL | HRT_FLAG_STREAM_KERNEL | HRT_FLAG_NO_SHADOW_CULL;
    if (flags & ~known) return fail(HRT_ERR_INVALID, who + ": flags: unknown bits " + std::to_string(flags & ~known));
    if (n_views == 0u) return HRT_OK;
    if (!views) return fail(HRT_ERR_INVALID, who + ": views is NULL");
    { const int frc = check_frame(who, w, h, k_max_pixels); if (frc != HRT_OK) return frc; }
    if (!spp) return fail(HRT_ERR_INVALID, who + ": spp must be positive");
    if (w > 65535u || h > 65535u) return fail(HRT_ERR_INVALID, who + ": w and h must be below 65536 (tile origins are packed in 16 + 16 bits)");
    blocks.resize(n_views);
    for (uint32_t v = 0; v < n_views; ++v) {
        if (make_camera(&views[v].cam, blocks[v].cam) != HRT_OK) return fail(HRT_ERR_INVALID, who + ": views[" + std::to_string(v) + "].cam: " + g_error);
        blocks[v].seed_lo = (uint32_t)views[v].seed; blocks[v].seed_hi = (uint32_t)(views[v].seed >> 32);
        blocks[v].err_abs = 0.f; blocks[v].pad = 0u;
    }
    if (!out) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is NULL");
    if ((uintptr_t)out % sizeof(float)) return fail(HRT_ERR_INVALID, who + ": " + out_name + " is not 4-byte aligned");
    if ((uint64_t)n_views * hrt_tiles_total(w, h) > HRT_VIEWS_MAX_TILES)
        return fail(HRT_ERR_INVALID, who + ": n_views x tiles per view is " + std::to_string((uint64_t)n_views * hrt_tiles_total(w, h)) +
                                     ", above HRT_VIEWS_MAX_TILES = " + std::to_string(HRT_VIEWS_MAX_TILES));
    return HRT_OK;
}

// Stages the blocks, launches the trace kernel over all views' tiles and assembles the frames into d_frames, all on `stream`.
static int views_launch(hrt_scene *s, const hrt_view *views, std::vector<DView> &blocks, uint32_t w, uint32_t h, uint32_t spp, uint32_t flags,
                        float *d_frames, hipStream_t stream) {
    const uint32_t n_views = (uint32_t)blocks.size(), tiles = hrt_tiles_total(w, h);
    for (uint32_t v = 0; v < n_views; ++v) {  // fill_render's margin, per view
        const float *e = views[v].cam.eye;
        blocks[v].err_abs = margin_scale(s->bound, std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
    }
    // No host wait before a larger table replaces the old one (nor before larger tile sums do): launch_trace orders the launches of
    // one scene behind its own event, and the upload is its to enqueue, behind that wait (StagedTable::upload).
    int rc = s->views.fill(blocks, false);
    if (rc == HRT_OK) rc = s->vw_tiles.grow((size_t)n_views * tiles * 64u * 3u * sizeof(float));
    // The tile sums are read by the assemble launch, behind the event launch_trace orders launches by: a batched launch on another
    // stream waits for the previous one's frames as well.
    if (rc == HRT_OK) rc = s->views.reader.wait_on(stream);
    if (rc != HRT_OK) return rc;
    TraceJob job{w, h, 0u, spp, 0u, flags, s->vw_tiles.as<float>(), stream};
    job.n_views = n_views;
    rc = launch_trace(s, &views[0].cam, job);
    if (rc != HRT_OK) return rc;
    const uint32_t n_pixels = n_views * w * h;
    hipLaunchKernelGGL(hrt_assemble_views_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, s->vw_tiles.as<float>(), tiles, w, h,
                       n_pixels, d_frames);
    HIP_TRY(hipGetLastError());
    return s->views.staged(stream);
}

int hrt_render_views_device(hrt_scene *s, const hrt_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t spp, uint32_t flags,
                            float *d_frames, void *stream) {
    const std::string who = "hrt_render_views_device";
    std::vector<DView> blocks;
    int rc = views_check(who, views, n_views, w, h, spp, flags, d_frames, "d_frames", blocks);
    if (rc != HRT_OK || n_views == 0u) return rc;
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    return views_launch(s, views, blocks, w, h, spp, flags, d_frames, (hipStream_t)stream);
}

int hrt_render_views(hrt_scene *s, const hrt_view *views, uint32_t n_views, uint32_t w, uint32_t h, uint32_t spp, uint32_t flags,
                     float *out_rgb, hrt_stats *stats) {
    const std::string who = "hrt_render_views";
    std::vector<DView> blocks;
    int rc = views_check(who, views, n_views, w, h, spp, flags, out_rgb, "out_rgb", blocks);
    if (rc != HRT_OK) return rc;
    if (n_views == 0u) return empty_batch(stats);
    if ((rc = enter_scene(who, s)) != HRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t bytes = (size_t)n_views * w * h * 3u * sizeof(float);
    if ((rc = s->vw_frames.grow(bytes)) != HRT_OK) return rc;
    if ((rc = views_launch(s, views, blocks, w, h, spp, flags, s->vw_frames.as<float>(), nullptr)) != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->vw_frames.p, bytes, hipMemcpyDeviceToHost));
    if ((rc = hrt_check_last_launch(s)) != HRT_OK) return rc;  // never hand back frames the kernel did not finish
    if (stats) {
        double ms = 0.0;
        if ((rc = hrt_last_kernel_ms(s, &ms)) != HRT_OK) return rc;
        fill_stats(s, stats, t0, ms, (uint64_t)n_views * w * h * spp);
    }
    return HRT_OK;
}
