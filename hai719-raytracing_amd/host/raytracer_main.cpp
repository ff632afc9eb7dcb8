// Headless driver: what the reference does on key 'r' (main.cpp:321-325 ->
// ray_trace_from_camera(), main.cpp:200-263), with the GLUT window replaced by
// command-line arguments.  Scene set-up stays in host C++; the per-pixel x
// per-sample loop runs on the GPU behind hrt_render().
//
//   raytracer [--scene cornell_box|cornell_mesh|random_spheres|mesh_in_box|backrooms_pool]
//             [--w 850] [--h 480] [--spp 20] [--seed 1] [--out ./rendu.ppm] [--assets DIR] [--gpu 0]
//             [--kd gpu]                         build the KD-trees' split search on the GPU (hrt_kd_build_gpu; the same trees)
//             [--gpus N | --devices 0,1,2,...]   image tiles across several GPUs of this node (hrt_multi_*; an ordinal may repeat)
//             [--adaptive THRESHOLD [--spp-min 8]] adaptive sampling (hrt_render_adaptive): per 8x8 tile from --spp-min up to --spp
//                                                  samples per pixel, until the tile's noise estimate is below THRESHOLD (one GPU)
//             [--denoise FEATURE_SPP [--denoise-iters N]] denoised frame (hrt_render_denoised): --spp samples, first-hit features of the
//                                                  first FEATURE_SPP of them (0 = pixel centres), the a-trous filter with its default
//                                                  parameters and N iterations (one GPU)
//             [--denoise-var FEATURE_SPP [--denoise-iters N]] variance-guided denoised frame (hrt_render_denoised_var): --spp samples
//                                                  (even), the colour width of every pair of pixels set by the noise of their own means (one GPU)
//             [--denoise-guides first|diffuse]   with --denoise or --denoise-var: where the filter's features are taken -- at the first
//                                                  hit (the default; the same bytes as without the option) or at the first DIFFUSE
//                                                  hit of every sample's path, mirror and glass followed (hrt_render_denoised_guides,
//                                                  hrt_render_denoised_var_guides; FEATURE_SPP >= 1).  With --lens the frame, the
//                                                  features and the filter of that lens (hrt_render_lens_device,
//                                                  hrt_render_lens_features or hrt_render_lens_path_features, hrt_denoise*); not
//                                                  with --temporal
//             [--temporal FRAMES [--orbit DEGREES] [--denoise-var FEATURE_SPP]] FRAMES frames of --spp samples (even) with seeds seed,
//                                                  seed + 1, ..., each accumulated onto the reprojected last one (hrt_render_temporal); the
//                                                  camera turns about the scene's up axis by DEGREES / FRAMES per frame; with --denoise-var
//                                                  every frame's accumulated pair goes through the variance-guided filter; the last
//                                                  frame is written (one GPU)
//             [--views N [--orbit DEGREES]]        N cameras, each turned DEGREES further about the scene's up axis than the one before,
//                                                  rendered in ONE launch (hrt_render_views) with seeds seed, seed + 1, ...; written as
//                                                  NAME_000.ppm, NAME_001.ppm, ... for --out NAME.ppm (one GPU)
//             [--lens perspective|ortho|equirect|fisheye [--aperture R --focus D] [--lens-extent X]] a lens camera (hrt_render_lens): the
//                                                  thin lens of radius R focused at depth D (perspective), the view volume's height X
//                                                  (ortho), a 360 x 180 degree panorama (equirect), X degrees of equidistant fisheye
//                                                  (one GPU; no --temporal, --gpus; --denoise and --denoise-var only with
//                                                  --denoise-guides).  With --adaptive
//                                                  THRESHOLD [--spp-min N]: per-tile counts under the lens (hrt_render_lens_adaptive).
//                                                  With --views N [--orbit DEGREES]: N lens frames in ONE launch
//                                                  (hrt_render_lens_views), cameras and seeds and files as --views has them
//             [--bake-quad INDEX [--bake-side 1|-1] [--bake-bias B]] a lightmap (hrt_bake): --w x --h texels over quad INDEX of the
//                                                  flattened scene (hrt_bake_quad_points: texel centres, the quad's normal times
//                                                  the side, +1 the lit one), --spp cosine-weighted samples per texel; written
//                                                  row-major in the frame's linear units, radiance / 6, without gamma (one GPU,
//                                                  no other mode)
//             [--probe-grid NX,NY,NZ --probe-box x0,y0,z0,x1,y1,z1] light probes (hrt_probes): an NX x NY x NZ grid of probes at the
//                                                  cell centres of the box (hrt_probe_grid_points), --spp uniform directions per
//                                                  probe; --out is TEXT, one line per probe: its position, then the 27 means
//                                                  (9 SH coefficients x rgb, radiance / 6, no factor), %.9g (one GPU, not with
//                                                  --lens, --bake-quad, --views or --adaptive)
//             [--probe-quad INDEX [--probe-side 1|-1] [--probe-facing]] with --probe-grid and --probe-box: a lightmap from the
//                                                  probes (hrt_probe_eval) instead of the text: the grid is traced as above,
//                                                  loaded into a probe volume and evaluated at the --w x --h texel centres of
//                                                  quad INDEX (hrt_bake_quad_points, bias 0; --probe-facing weights the probes
//                                                  by how far they face the surface); written as --bake-quad writes its own
//             [--probe-visible [--probe-rmax R]]   with --probe-quad: the depth of the same grid is traced too (hrt_probe_depth,
//                                                  the same seed and samples, depths cut at R; default 1.5 x the diagonal of a
//                                                  grid cell) and the lightmap is that of the look-up with visibility
//                                                  (hrt_probe_eval_visible): probes behind a wall are weighted out
//             [--probe-bounces K [--probe-keep H]] with --probe-quad or --probe-lit: the grid is not path-traced but RELIT: from zero
//                                                  coefficients, K rounds of hrt_probes_lit_device against the volume as it stands
//                                                  (round r takes samples [r x spp, (r + 1) x spp); --probe-facing and
//                                                  --probe-visible apply to the rounds' look-ups too, the depth being traced before
//                                                  round 0), each written back with hrt_probe_volume_update_device, or with
//                                                  --probe-keep H in [0, 1) blended in (hrt_probe_volume_blend_device)
//             [--probe-lit]                        with --probe-grid and --probe-box, instead of --probe-quad: a --w x --h camera
//                                                  frame lit by the volume: all samples in ONE fused launch into running sums
//                                                  (hrt_render_lit_device); means and gamma by hrt_finalize_tiles, written as a
//                                                  render is.  With --lens ... the frame of that lens (a pinhole without); with
//                                                  --views N [--orbit DEGREES] N lit frames in one launch
//                                                  (hrt_render_lit_views_device), cameras, seeds and files as --views has them
//             [--probe-tail K]                     with --probe-lit or --probe-bounces, K in 1 .. 6: their paths follow mirror and glass
//                                                  and end in the volume at their K-th diffuse hit (hrt_trace_lit_paths,
//                                                  hrt_probes_lit_paths_device) instead of at their first hit of any kind
//             [--bake-lit]                         with --bake-quad INDEX, --probe-grid and --probe-box: the FINAL GATHER -- the grid
//                                                  is path-traced (or relit with --probe-bounces K [--probe-keep H]) and the
//                                                  lightmap of quad INDEX is written by ONE hrt_bake_lit_device call instead of
//                                                  hrt_bake: every sample's path ends in the volume at its first hit, or with
//                                                  --probe-tail K at its K-th diffuse hit; --probe-facing and --probe-visible
//                                                  describe the look-up there; --bake-side and --bake-bias the points, as ever
//             --probe-lit --adaptive THRESHOLD [--spp-min N]  the lit frame with per-tile counts (hrt_render_lit_adaptive), --lens
//                                                  honoured; prints the mean spp, as --lens --adaptive does (not with --views)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>  // --probe-bounces and --probe-lit drive the device forms: buffers of this program's own

#include "../../include/hrt.h"
#include "scene.h"

using namespace hrt_host;

static unsigned int SCREENWIDTH = 850, SCREENHEIGHT = 480;  // main.cpp:52-53
static unsigned int nsamples = 20;                          // DEFAULT_NSAMPLES, Constants.h:10
static Scene scene;
static hrt_scene *device_scene = nullptr;
static uint64_t seed = 1;
static std::string out_path = "./rendu.ppm";
static bool adaptive = false;  // --adaptive: hrt_render_adaptive from min_spp up to nsamples
static hrt_adaptive adaptive_params = {8u, 0u, 0.f};
static bool denoise = false;  // --denoise: hrt_render_denoised with the default parameters (the same as the Python DenoiseParams())
static uint32_t feature_spp = 0;
static hrt_denoise_params denoise_params = {4u, 8.0f, 0.05f, 0.4f, 0.05f};
static bool denoise_var = false;  // --denoise-var: hrt_render_denoised_var with the default parameters (the Python DenoiseVarParams())
static hrt_denoise_var_params denoise_var_params = {4u, 2u, 8.0f, 0.05f, 0.4f, 0.05f, 1e-8f};
static int denoise_guides = -1;  // --denoise-guides: HRT_GUIDES_FIRST_HIT or HRT_GUIDES_FIRST_DIFFUSE; -1: not given (first-hit guides)
static uint32_t temporal_frames = 0;  // --temporal: hrt_render_temporal over that many frames, the default hrt_temporal_params
static double orbit_degrees = 0.0;    // --orbit: the camera's turn about the up axis over the whole run
static uint32_t n_views = 0;          // --views: hrt_render_views over that many cameras, --orbit degrees apart
static bool use_lens = false;          // --lens: hrt_render_lens with the default camera behind the projection
static hrt_lens lens_params = {{}, HRT_LENS_PERSPECTIVE, 0.f, 1.f, 0.f};
static long bake_quad = -1;             // --bake-quad: hrt_bake over the texels of that quad of the flattened scene
static int32_t bake_side = 1;
static float bake_bias = 1e-4f;
static bool probe_grid_given = false, probe_box_given = false;  // --probe-grid with --probe-box: hrt_probes over a grid of probes
static uint32_t probe_n[3] = {0u, 0u, 0u};
static float probe_box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
static bool probe_quad_given = false, probe_side_given = false, probe_facing = false;  // --probe-quad: hrt_probe_eval over the texels of that quad
static bool probe_visible = false, probe_rmax_given = false;  // --probe-visible: hrt_probe_depth + hrt_probe_eval_visible
static float probe_rmax = 0.f;
static long probe_quad = -1;
static int32_t probe_side = 1;
static bool probe_bounces_given = false, probe_keep_given = false, probe_lit = false;  // --probe-bounces: hrt_probes_lit_device rounds; --probe-lit: hrt_trace_lit
static long probe_bounces = 0;
static bool bake_lit = false;  // --bake-lit: the lightmap of --bake-quad by hrt_bake_lit_device against the grid's volume
static long probe_tail = 0;  // --probe-tail K: the lit launches are "Lit paths" with tail_after = K; 0: not given, one segment
static float probe_keep = 0.f;
static hrt_temporal_params temporal_params = {0.02f, 64.f, 0.05f, 0.1f, 0.05f};  // the Python TemporalParams()

// Drop-in for ray_trace_from_camera(): same inputs (current scene, nsamples, window size, camera),
// same output file and quantisation; returns non-zero instead of printing-and-returning on failure.
static hrt_multi *multi = nullptr;  // --gpus / --devices: the same frame, tiles across several GPUs

// cam turned by `degrees` about the world's up axis (y) through the origin
static hrt_camera orbited(const hrt_camera &cam, double degrees) {
    const double a = degrees * M_PI / 180.0, c = std::cos(a), s = std::sin(a);
    hrt_camera out = cam;
    const float *from[4] = {cam.eye, cam.right, cam.up, cam.forward};
    float *to[4] = {out.eye, out.right, out.up, out.forward};
    for (int k = 0; k < 4; ++k) {
        to[k][0] = (float)(c * from[k][0] + s * from[k][2]);
        to[k][2] = (float)(-s * from[k][0] + c * from[k][2]);
    }
    return out;
}

// --temporal: the frame loop.  Frame k has seed + k and the camera turned by k * orbit / frames; the last frame is written.
static int ray_trace_frames() {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    std::vector<float> image((size_t)w * h * 3, 0.f), lengths((size_t)w * h, 0.f);
    const hrt_camera cam0 = default_camera((float)w / (float)h);
    std::cout << "Ray tracing " << temporal_frames << " frames of a " << w << " x " << h << " image on the GPU using " << nsamples
              << " samples per pixel each, accumulated over time (orbit " << orbit_degrees << " degrees)"
              << (denoise_var ? ", denoised by variance (features of " + std::to_string(feature_spp) + " samples, " + std::to_string(denoise_var_params.iterations) + " iterations)" : std::string())
              << std::endl;
    hrt_history *history = nullptr;
    int rc = hrt_history_create(device_scene, &history);
    double kernel_ms = 0.0, total_ms = 0.0;
    for (uint32_t k = 0; rc == HRT_OK && k < temporal_frames; ++k) {
        const hrt_camera cam = orbited(cam0, orbit_degrees * (double)k / (double)temporal_frames);
        hrt_stats st;
        rc = hrt_render_temporal(device_scene, history, &cam, w, h, nsamples, denoise_var ? feature_spp : 0u, seed + k, HRT_FLAG_GAMMA, &temporal_params,
                                 denoise_var ? &denoise_var_params : nullptr, image.data(), lengths.data(), &st);
        if (rc == HRT_OK) { kernel_ms += st.kernel_ms; total_ms += st.total_ms; }
    }
    hrt_history_destroy(history);
    if (rc != HRT_OK) {
        std::cout << "hrt_render_temporal failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    double mean = 0.0;
    for (float v : lengths) mean += v;
    std::cout << "  Done in " << total_ms / 1000.0 << " seconds (kernels " << kernel_ms << " ms, mean history of the last frame "
              << mean / (double)lengths.size() << " frames)" << std::endl;
    rc = hrt_write_ppm(out_path.c_str(), image.data(), w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// The file of view k of --views: NAME_kkk.ppm for --out NAME.ppm.
static std::string view_path(uint32_t k) {
    const size_t dot = out_path.rfind('.'), slash = out_path.rfind('/');
    const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
    const std::string stem = has_ext ? out_path.substr(0, dot) : out_path, ext = has_ext ? out_path.substr(dot) : std::string(".ppm");
    char num[16];
    std::snprintf(num, sizeof(num), "_%03u", k);
    return stem + num + ext;
}

// --views: N cameras in one launch.  View k has seed + k and the camera turned by k * orbit; frame k goes to NAME_kkk.ppm.
// With --lens every view is that lens behind its camera (hrt_render_lens_views).
static int ray_trace_views() {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    const size_t frame = (size_t)w * h * 3;
    std::vector<float> images(frame * n_views, 0.f);
    const hrt_camera cam0 = default_camera((float)w / (float)h);
    std::vector<hrt_view> views(use_lens ? 0u : n_views);
    std::vector<hrt_lens_view> lens_views(use_lens ? n_views : 0u);
    for (uint32_t k = 0; k < n_views; ++k) {
        const hrt_camera cam = orbited(cam0, orbit_degrees * (double)k);
        if (use_lens) { lens_views[k].lens = lens_params; lens_views[k].lens.cam = cam; lens_views[k].seed = seed + k; }
        else { views[k].cam = cam; views[k].seed = seed + k; }
    }
    static const char *const names[] = {"perspective", "orthographic", "equirectangular", "fisheye"};
    std::cout << "Ray tracing " << n_views << " views of " << w << " x " << h << " pixels, " << orbit_degrees << " degrees apart, on the GPU in one launch using "
              << nsamples << " samples per pixel";
    if (use_lens)
        std::cout << " through a " << names[lens_params.projection] << " lens (aperture " << lens_params.aperture_radius << ", focus "
                  << lens_params.focus_distance << ", extent " << lens_params.extent << ")";
    std::cout << std::endl;
    hrt_stats st;
    int rc = use_lens ? hrt_render_lens_views(device_scene, lens_views.data(), n_views, w, h, nsamples, HRT_FLAG_GAMMA, images.data(), &st)
                      : hrt_render_views(device_scene, views.data(), n_views, w, h, nsamples, HRT_FLAG_GAMMA, images.data(), &st);
    if (rc != HRT_OK) {
        std::cout << (use_lens ? "hrt_render_lens_views" : "hrt_render_views") << " failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::cout << "  Done in " << st.total_ms / 1000.0 << " seconds (kernel " << st.kernel_ms << " ms, " << (double)st.samples / st.kernel_ms / 1e3
              << " Msamples/s)" << std::endl;
    for (uint32_t k = 0; rc == HRT_OK && k < n_views; ++k) rc = hrt_write_ppm(view_path(k).c_str(), images.data() + frame * k, w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// --lens: one frame through a lens camera; with --adaptive, per-tile sample counts from --spp-min up to --spp
static int ray_trace_lens() {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    std::vector<float> image((size_t)w * h * 3, 0.f);
    lens_params.cam = default_camera((float)w / (float)h);
    static const char *const names[] = {"perspective", "orthographic", "equirectangular", "fisheye"};
    std::cout << "Ray tracing a " << w << " x " << h << " image on the GPU using " << nsamples << " samples per pixel through a "
              << names[lens_params.projection] << " lens (aperture " << lens_params.aperture_radius << ", focus " << lens_params.focus_distance
              << ", extent " << lens_params.extent << ")";
    if (adaptive) std::cout << " (adaptive from " << adaptive_params.min_spp << " samples per pixel, threshold " << adaptive_params.threshold << ")";
    std::cout << std::endl;
    hrt_stats st;
    adaptive_params.max_spp = nsamples;
    int rc = adaptive ? hrt_render_lens_adaptive(device_scene, &lens_params, w, h, &adaptive_params, seed, HRT_FLAG_GAMMA, image.data(), nullptr, &st)
                      : hrt_render_lens(device_scene, &lens_params, w, h, nsamples, seed, HRT_FLAG_GAMMA, image.data(), &st);
    if (rc != HRT_OK) {
        std::cout << (adaptive ? "hrt_render_lens_adaptive" : "hrt_render_lens") << " failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::cout << "  Done in " << st.total_ms / 1000.0 << " seconds (kernel " << st.kernel_ms << " ms, " << (double)st.samples / st.kernel_ms / 1e3
              << " Msamples/s";
    if (adaptive) std::cout << ", mean " << (double)st.samples / ((double)w * h) << " spp";
    std::cout << ")" << std::endl;
    rc = hrt_write_ppm(out_path.c_str(), image.data(), w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// --bake-quad: a --w x --h lightmap of one quad of the flattened scene
static int bake_lightmap(const hrt_scene_desc &desc) {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    std::vector<float> points((size_t)w * h * HRT_RAY_FLOATS), map((size_t)w * h * 3, 0.f);
    int rc = hrt_bake_quad_points(&desc.quads[bake_quad], w, h, bake_side, 0.f, bake_bias, points.data());
    if (rc != HRT_OK) {
        std::cout << "hrt_bake_quad_points failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::cout << "Baking a " << w << " x " << h << " lightmap of quad " << bake_quad << " (side " << bake_side << ", bias " << bake_bias
              << ") on the GPU using " << nsamples << " samples per texel" << std::endl;
    hrt_stats st;
    rc = hrt_bake(device_scene, points.data(), nullptr, w * h, nsamples, seed, 0u, map.data(), &st);
    if (rc != HRT_OK) {
        std::cout << "hrt_bake failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::cout << "  Done in " << st.total_ms / 1000.0 << " seconds (kernel " << st.kernel_ms << " ms, " << (double)st.samples / st.kernel_ms / 1e3
              << " Msamples/s)" << std::endl;
    rc = hrt_write_ppm(out_path.c_str(), map.data(), w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// A device buffer of this program's own, freed on every way out.
struct DeviceBuffer {
    void *p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    template <class T> T *as() const { return (T *)p; }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes) == hipSuccess; }
};

static int device_failed(const char *what) {
    std::cout << what << " failed: " << hipGetErrorString(hipGetLastError()) << std::endl;
    return HRT_ERR_DEVICE;
}

// --lens with --denoise or --denoise-var and --denoise-guides: the lens frame (and, variance-guided, the frame of the first half of
// its samples), the features the lens saw -- first-hit or first-diffuse -- and the filter, all on the null stream; the guided renders
// of a pinhole camera do the same inside the library.
static int ray_trace_lens_denoised() {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    const size_t npix = (size_t)w * h;
    lens_params.cam = default_camera((float)w / (float)h);
    std::cout << "Ray tracing a " << w << " x " << h << " image on the GPU using " << nsamples << " samples per pixel through a lens, denoised"
              << (denoise_var ? " by variance" : "") << " (" << (denoise_guides == (int)HRT_GUIDES_FIRST_DIFFUSE ? "first-diffuse" : "first-hit")
              << " features of " << feature_spp << " samples)" << std::endl;
    DeviceBuffer d_frame, d_half, d_feat, d_scratch, d_out;
    if (!d_frame.alloc(npix * 3 * sizeof(float)) || !d_half.alloc(npix * 3 * sizeof(float)) || !d_feat.alloc(npix * HRT_FEATURE_FLOATS * sizeof(float)) ||
        !d_scratch.alloc(hrt_denoise_scratch_bytes(w, h)) || !d_out.alloc(npix * 3 * sizeof(float)))
        return device_failed("hipMalloc");
    int rc = hrt_render_lens_device(device_scene, &lens_params, w, h, 0u, nsamples, seed, 0u, d_frame.as<float>(), nullptr);
    if (rc == HRT_OK && denoise_var) rc = hrt_render_lens_device(device_scene, &lens_params, w, h, 0u, nsamples / 2u, seed, 0u, d_half.as<float>(), nullptr);
    if (rc == HRT_OK)
        rc = denoise_guides == (int)HRT_GUIDES_FIRST_DIFFUSE
                 ? hrt_render_lens_path_features(device_scene, &lens_params, w, h, 0u, feature_spp, seed, d_feat.as<float>(), nullptr)
                 : hrt_render_lens_features(device_scene, &lens_params, w, h, 0u, feature_spp, seed, d_feat.as<float>(), nullptr);
    if (rc == HRT_OK)
        rc = denoise_var ? hrt_denoise_var(d_frame.as<float>(), d_half.as<float>(), d_feat.as<float>(), w, h, &denoise_var_params, HRT_FLAG_GAMMA, d_scratch.p,
                                           d_out.as<float>(), nullptr, nullptr)
                         : hrt_denoise(d_frame.as<float>(), d_feat.as<float>(), w, h, &denoise_params, HRT_FLAG_GAMMA, d_scratch.p, d_out.as<float>(), nullptr);
    if (rc != HRT_OK) {
        std::cout << "the denoised lens frame failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::vector<float> image(npix * 3, 0.f);
    if (hipMemcpy(image.data(), d_out.p, image.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return device_failed("hipMemcpy");
    rc = hrt_write_ppm(out_path.c_str(), image.data(), w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// The eval_flags of the lit launches: what --probe-facing and --probe-visible say of the look-up.
static uint32_t lit_eval_flags() { return (probe_facing ? HRT_PROBE_EVAL_FACING : 0u) | (probe_visible ? HRT_LIT_VISIBLE : 0u); }

// --probe-bounces: from zero coefficients, K rounds of gather-and-write-back on the null stream; `sh` receives the last round's
// coefficients.
static int relight_probes(hrt_probe_volume *volume, const std::vector<float> &probes, size_t n, std::vector<float> &sh) {
    std::cout << "Relighting the probes over " << probe_bounces << " rounds of " << nsamples << " samples per probe (keep " << probe_keep << ")" << std::endl;
    int rc = hrt_probe_volume_update(volume, sh.data());  // zeros
    if (rc != HRT_OK) return rc;
    DeviceBuffer d_probes, d_sh;
    if (!d_probes.alloc(probes.size() * sizeof(float)) || !d_sh.alloc(sh.size() * sizeof(float))) return device_failed("hipMalloc");
    if (hipMemcpy(d_probes.p, probes.data(), probes.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return device_failed("hipMemcpy");
    for (long r = 0; rc == HRT_OK && r < probe_bounces; ++r) {
        const uint32_t first = (uint32_t)((uint64_t)r * nsamples);
        rc = probe_tail ? hrt_probes_lit_paths_device(device_scene, volume, d_probes.as<float>(), nullptr, (uint32_t)n, first, nsamples, seed, 0u,
                                                      lit_eval_flags(), 0.f, (uint32_t)probe_tail, d_sh.as<float>(), nullptr)
                        : hrt_probes_lit_device(device_scene, volume, d_probes.as<float>(), nullptr, (uint32_t)n, first, nsamples, seed, 0u,
                                                lit_eval_flags(), 0.f, d_sh.as<float>(), nullptr);
        if (rc == HRT_OK)
            rc = probe_keep > 0.f ? hrt_probe_volume_blend_device(volume, d_sh.as<float>(), probe_keep, nullptr)
                                  : hrt_probe_volume_update_device(volume, d_sh.as<float>(), nullptr);
    }
    if (rc != HRT_OK) return rc;
    if (hipMemcpy(sh.data(), d_sh.p, sh.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return device_failed("hipMemcpy");
    return HRT_OK;
}

// --probe-lit: the frame whose paths end in the volume -- ONE fused launch of all samples into running sums (hrt_render_lit_device;
// with --views the batch, hrt_render_lit_views_device, cameras, seeds and files as --views has them), then the render's output stage.
static int probe_lit_frame(hrt_probe_volume *volume) {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    if (adaptive) {  // per-tile counts from --spp-min up to --spp (hrt_render_lit_adaptive; never with --views)
        hrt_lens lens = lens_params;  // without --lens the pinhole
        lens.cam = default_camera((float)w / (float)h);
        std::vector<float> image((size_t)w * h * 3, 0.f);
        std::cout << "Ray tracing a " << w << " x " << h << " image lit by the probes on the GPU using " << adaptive_params.min_spp << " to " << nsamples
                  << " samples per pixel (adaptive, threshold " << adaptive_params.threshold << ")" << std::endl;
        hrt_stats st;
        adaptive_params.max_spp = nsamples;
        int arc = hrt_render_lit_adaptive(device_scene, volume, &lens, w, h, &adaptive_params, seed, HRT_FLAG_GAMMA, lit_eval_flags(), 0.f,
                                          (uint32_t)probe_tail, image.data(), nullptr, &st);
        if (arc != HRT_OK) {
            std::cout << "hrt_render_lit_adaptive failed: " << hrt_last_error() << std::endl;
            return arc;
        }
        std::cout << "  Done in " << st.total_ms / 1000.0 << " seconds (kernel " << st.kernel_ms << " ms, " << (double)st.samples / st.kernel_ms / 1e3
                  << " Msamples/s, mean " << (double)st.samples / ((double)w * h) << " spp)" << std::endl;
        arc = hrt_write_ppm(out_path.c_str(), image.data(), w, h);
        if (arc != HRT_OK) std::cout << hrt_last_error() << std::endl;
        return arc;
    }
    const uint32_t frames = n_views ? n_views : 1u;
    const uint32_t npix = w * h, n_tiles = (uint32_t)(((uint64_t)frames * npix + 63u) / 64u);  // the sums padded to whole tiles of 64 pixels for hrt_finalize_tiles
    const hrt_camera cam0 = default_camera((float)w / (float)h);
    std::vector<hrt_lens_view> views(frames);
    for (uint32_t k = 0; k < frames; ++k) {
        views[k].lens = lens_params;  // without --lens the pinhole
        views[k].lens.cam = n_views ? orbited(cam0, orbit_degrees * (double)k) : cam0;
        views[k].seed = seed + k;
    }
    if (n_views) std::cout << "Ray tracing " << n_views << " views of " << w << " x " << h << " pixels, " << orbit_degrees << " degrees apart,";
    else std::cout << "Ray tracing a " << w << " x " << h << " image";
    std::cout << " lit by the probes on the GPU using " << nsamples << " samples per pixel" << std::endl;
    DeviceBuffer d_sum;
    const size_t sum_bytes = (size_t)n_tiles * 64u * 3u * sizeof(float);
    if (!d_sum.alloc(sum_bytes)) return device_failed("hipMalloc");
    if (hipMemset(d_sum.p, 0, sum_bytes) != hipSuccess) return device_failed("hipMemset");
    int rc = n_views ? hrt_render_lit_views_device(device_scene, volume, views.data(), n_views, w, h, 0u, nsamples, HRT_RADIANCE_ACCUMULATE, lit_eval_flags(),
                                                   0.f, (uint32_t)probe_tail, d_sum.as<float>(), nullptr)
                     : hrt_render_lit_device(device_scene, volume, &views[0].lens, w, h, 0u, nsamples, seed, HRT_RADIANCE_ACCUMULATE, lit_eval_flags(), 0.f,
                                             (uint32_t)probe_tail, d_sum.as<float>(), nullptr);
    if (rc == HRT_OK) rc = hrt_finalize_tiles(d_sum.as<float>(), n_tiles, nsamples, HRT_FLAG_GAMMA, d_sum.as<float>(), nullptr);
    if (rc != HRT_OK) {
        std::cout << "the probe-lit frame failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::vector<float> images((size_t)frames * npix * 3u, 0.f);
    if (hipMemcpy(images.data(), d_sum.p, images.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return device_failed("hipMemcpy");
    if (!n_views) {
        rc = hrt_write_ppm(out_path.c_str(), images.data(), w, h);
    } else {
        for (uint32_t k = 0; rc == HRT_OK && k < n_views; ++k) rc = hrt_write_ppm(view_path(k).c_str(), images.data() + (size_t)npix * 3u * k, w, h);
    }
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// --bake-lit: the lightmap of --bake-quad whose paths end in the volume -- ONE fused launch of all samples (hrt_bake_lit_device),
// written as --bake-quad writes its own.
static int bake_lit_lightmap(const hrt_scene_desc &desc, hrt_probe_volume *volume) {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    std::vector<float> points((size_t)w * h * HRT_RAY_FLOATS), map((size_t)w * h * 3, 0.f);
    int rc = hrt_bake_quad_points(&desc.quads[bake_quad], w, h, bake_side, 0.f, bake_bias, points.data());
    if (rc != HRT_OK) {
        std::cout << "hrt_bake_quad_points failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::cout << "Baking a " << w << " x " << h << " lightmap of quad " << bake_quad << " (side " << bake_side << ", bias " << bake_bias
              << ") lit by the probes on the GPU using " << nsamples << " samples per texel" << std::endl;
    DeviceBuffer d_points, d_map;
    if (!d_points.alloc(points.size() * sizeof(float)) || !d_map.alloc(map.size() * sizeof(float))) return device_failed("hipMalloc");
    if (hipMemcpy(d_points.p, points.data(), points.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return device_failed("hipMemcpy");
    rc = hrt_bake_lit_device(device_scene, volume, d_points.as<float>(), nullptr, w * h, 0u, nsamples, seed, 0u, lit_eval_flags(), 0.f,
                             (uint32_t)probe_tail, d_map.as<float>(), nullptr);
    if (rc != HRT_OK) {
        std::cout << "hrt_bake_lit_device failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    if (hipMemcpy(map.data(), d_map.p, map.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return device_failed("hipMemcpy");
    rc = hrt_write_ppm(out_path.c_str(), map.data(), w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

// The r_max of --probe-visible: --probe-rmax, or 1.5 x the diagonal of a grid cell, in fp32.
static float probe_depth_rmax() {
    if (probe_rmax_given) return probe_rmax;
    float e[3];
    for (int a = 0; a < 3; ++a) e[a] = (probe_box[3 + a] - probe_box[a]) / (float)probe_n[a];
    return 1.5f * std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

// --probe-grid: the SH coefficients of a grid of light probes, as text -- or with --probe-quad the lightmap they give on a quad, or
// with --probe-lit the camera frame they light; with --probe-bounces the coefficients are relit instead of path-traced
static int light_probes(const hrt_scene_desc &desc) {
    const size_t n = (size_t)probe_n[0] * probe_n[1] * probe_n[2];
    std::vector<float> probes(n * HRT_PROBE_FLOATS), sh(n * 3u * HRT_PROBE_COEFFS, 0.f);
    int rc = hrt_probe_grid_points(probe_box, probe_box + 3, probe_n[0], probe_n[1], probe_n[2], 0.f, probes.data());
    if (rc != HRT_OK) {
        std::cout << "hrt_probe_grid_points failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    hrt_stats st;
    hrt_probe_volume *volume = nullptr;
    const bool needs_volume = probe_quad_given || probe_lit || probe_bounces_given || bake_lit;
    auto leave = [&](int code, const char *what) {
        if (code != HRT_OK && what) std::cout << what << " failed: " << hrt_last_error() << std::endl;
        hrt_probe_volume_destroy(volume);
        return code;
    };
    auto trace_depth = [&]() {  // the depth of the grid, the same seed and samples, into the volume
        const float r_max = probe_depth_rmax();
        std::cout << "Tracing the depth of the probes (r_max " << r_max << ")" << std::endl;
        std::vector<float> sums(n * HRT_PROBE_DEPTH_FLOATS, 0.f);
        int drc = hrt_probe_depth(device_scene, probes.data(), nullptr, (uint32_t)n, nsamples, seed, r_max, 0u, sums.data(), &st);
        if (drc == HRT_OK) drc = hrt_probe_volume_update_depth(volume, sums.data());
        return drc;
    };
    if (probe_bounces_given) {
        rc = hrt_probe_volume_create(probe_box, probe_box + 3, probe_n[0], probe_n[1], probe_n[2], &volume);
        if (rc == HRT_OK && probe_visible) rc = trace_depth();
        if (rc == HRT_OK) rc = relight_probes(volume, probes, n, sh);
        if (rc != HRT_OK) return leave(rc, "relighting the probe volume");
    } else {
        std::cout << "Tracing " << probe_n[0] << " x " << probe_n[1] << " x " << probe_n[2] << " light probes on the GPU using " << nsamples
                  << " samples per probe" << std::endl;
        rc = hrt_probes(device_scene, probes.data(), nullptr, (uint32_t)n, nsamples, seed, 0u, sh.data(), &st);
        if (rc != HRT_OK) {
            std::cout << "hrt_probes failed: " << hrt_last_error() << std::endl;
            return rc;
        }
        std::cout << "  Done in " << st.total_ms / 1000.0 << " seconds (kernel " << st.kernel_ms << " ms, " << (double)st.samples / st.kernel_ms / 1e3
                  << " Msamples/s)" << std::endl;
        if (needs_volume) {
            rc = hrt_probe_volume_create(probe_box, probe_box + 3, probe_n[0], probe_n[1], probe_n[2], &volume);
            if (rc == HRT_OK) rc = hrt_probe_volume_update(volume, sh.data());
            if (rc == HRT_OK && probe_visible) rc = trace_depth();
            if (rc != HRT_OK) return leave(rc, "the probe volume");
        }
    }
    if (probe_lit) return leave(probe_lit_frame(volume), nullptr);
    if (bake_lit) return leave(bake_lit_lightmap(desc, volume), nullptr);
    if (probe_quad_given) {
        const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
        std::vector<float> points((size_t)w * h * HRT_RAY_FLOATS), map((size_t)w * h * 3, 0.f);
        rc = hrt_bake_quad_points(&desc.quads[probe_quad], w, h, probe_side, 0.f, 0.f, points.data());
        if (rc != HRT_OK) return leave(rc, "hrt_bake_quad_points");
        std::cout << "Evaluating the probes over a " << w << " x " << h << " lightmap of quad " << probe_quad << " (side " << probe_side
                  << (probe_facing ? ", facing weights" : "") << ")" << std::endl;
        rc = probe_visible ? hrt_probe_eval_visible(volume, points.data(), w * h, probe_facing ? HRT_PROBE_EVAL_FACING : 0u, map.data(), &st)
                           : hrt_probe_eval(volume, points.data(), w * h, probe_facing ? HRT_PROBE_EVAL_FACING : 0u, map.data(), &st);
        if (rc != HRT_OK) return leave(rc, "the probe volume");
        std::cout << "  Done (kernel " << st.kernel_ms << " ms)" << std::endl;
        rc = hrt_write_ppm(out_path.c_str(), map.data(), w, h);
        if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
        return leave(rc, nullptr);
    }
    hrt_probe_volume_destroy(volume);
    FILE *f = std::fopen(out_path.c_str(), "w");
    if (!f) {
        std::cout << "cannot write " << out_path << std::endl;
        return HRT_ERR_INVALID;
    }
    for (size_t i = 0; i < n; ++i) {
        std::fprintf(f, "%.9g %.9g %.9g", probes[i * HRT_PROBE_FLOATS], probes[i * HRT_PROBE_FLOATS + 1], probes[i * HRT_PROBE_FLOATS + 2]);
        for (unsigned k = 0; k < 3u * HRT_PROBE_COEFFS; ++k) std::fprintf(f, " %.9g", sh[i * 3u * HRT_PROBE_COEFFS + k]);
        std::fprintf(f, "\n");
    }
    return std::fclose(f) == 0 ? HRT_OK : HRT_ERR_INVALID;
}

// "a,b,c" as exactly `count` numbers; false otherwise
static bool parse_list(const std::string &v, int count, double *out) {
    const char *p = v.c_str();
    for (int i = 0; i < count; ++i) {
        char *end = nullptr;
        out[i] = std::strtod(p, &end);
        if (end == p || *end != (i + 1 < count ? ',' : '\0')) return false;
        p = end + 1;
    }
    return true;
}

static int ray_trace_from_camera() {
    const unsigned w = SCREENWIDTH, h = SCREENHEIGHT;
    std::vector<float> image((size_t)w * h * 3, 0.f);
    const hrt_camera cam = default_camera((float)w / (float)h);
    if (adaptive)
        std::cout << "Ray tracing a " << w << " x " << h << " image on the GPU using " << adaptive_params.min_spp << " to " << nsamples
                  << " samples per pixel (adaptive, threshold " << adaptive_params.threshold << ")" << std::endl;
    else
        std::cout << "Ray tracing a " << w << " x " << h << " image on the GPU using " << nsamples << " samples per pixel"
                  << (denoise ? ", denoised (features of " + std::to_string(feature_spp) + " samples, " + std::to_string(denoise_params.iterations) + " iterations)" : std::string())
                  << (denoise_var ? ", denoised by variance (features of " + std::to_string(feature_spp) + " samples, " + std::to_string(denoise_var_params.iterations) + " iterations)" : std::string())
                  << std::endl;
    hrt_stats st;
    adaptive_params.max_spp = nsamples;
    int rc = multi ? hrt_multi_render(multi, &cam, w, h, nsamples, seed, HRT_FLAG_GAMMA, image.data(), &st)
             : adaptive ? hrt_render_adaptive(device_scene, &cam, w, h, &adaptive_params, seed, HRT_FLAG_GAMMA, image.data(), nullptr, &st)
             : denoise_var && denoise_guides == (int)HRT_GUIDES_FIRST_DIFFUSE
                 ? hrt_render_denoised_var_guides(device_scene, &cam, w, h, nsamples, feature_spp, seed, HRT_FLAG_GAMMA, HRT_GUIDES_FIRST_DIFFUSE, &denoise_var_params, image.data(), nullptr, &st)
             : denoise && denoise_guides == (int)HRT_GUIDES_FIRST_DIFFUSE
                 ? hrt_render_denoised_guides(device_scene, &cam, w, h, nsamples, feature_spp, seed, HRT_FLAG_GAMMA, HRT_GUIDES_FIRST_DIFFUSE, &denoise_params, image.data(), &st)
             : denoise_var ? hrt_render_denoised_var(device_scene, &cam, w, h, nsamples, feature_spp, seed, HRT_FLAG_GAMMA, &denoise_var_params, image.data(), nullptr, &st)
             : denoise  ? hrt_render_denoised(device_scene, &cam, w, h, nsamples, feature_spp, seed, HRT_FLAG_GAMMA, &denoise_params, image.data(), &st)
                        : hrt_render(device_scene, &cam, w, h, nsamples, seed, HRT_FLAG_GAMMA, image.data(), &st);
    if (rc != HRT_OK) {
        std::cout << (adaptive ? "hrt_render_adaptive" : denoise_var ? "hrt_render_denoised_var" : denoise ? "hrt_render_denoised" : "hrt_render") << " failed: " << hrt_last_error() << std::endl;
        return rc;
    }
    std::cout << "  Done in " << st.total_ms / 1000.0 << " seconds (kernel " << st.kernel_ms << " ms, "
              << (double)st.samples / st.kernel_ms / 1e3 << " Msamples/s";
    if (adaptive) std::cout << ", mean " << (double)st.samples / ((double)w * h) << " spp";
    std::cout << ")" << std::endl;
    rc = hrt_write_ppm(out_path.c_str(), image.data(), w, h);
    if (rc != HRT_OK) std::cout << hrt_last_error() << std::endl;
    return rc;
}

int main(int argc, char **argv) {
    std::string name = "cornell_box", assets = "assets";
    int gpu = 0;
    bool kd_on_gpu = false;
    std::vector<int> devices;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--probe-facing" || k == "--probe-visible" || k == "--probe-lit" || k == "--bake-lit") {  // the options without a value
            (k == "--probe-facing" ? probe_facing : k == "--probe-visible" ? probe_visible : k == "--probe-lit" ? probe_lit : bake_lit) = true;
            --i;
            continue;
        }
        if (i + 1 >= argc) break;
        const std::string v = argv[i + 1];
        if (k == "--scene") name = v;
        else if (k == "--w") SCREENWIDTH = (unsigned)atoi(v.c_str());
        else if (k == "--h") SCREENHEIGHT = (unsigned)atoi(v.c_str());
        else if (k == "--spp") nsamples = (unsigned)atoi(v.c_str());
        else if (k == "--seed") seed = strtoull(v.c_str(), nullptr, 10);
        else if (k == "--out") out_path = v;
        else if (k == "--assets") assets = v;
        else if (k == "--gpu") gpu = atoi(v.c_str());
        else if (k == "--kd") kd_on_gpu = v == "gpu";
        else if (k == "--adaptive") { adaptive = true; adaptive_params.threshold = strtof(v.c_str(), nullptr); }
        else if (k == "--spp-min") adaptive_params.min_spp = (unsigned)atoi(v.c_str());
        else if (k == "--denoise") { denoise = true; feature_spp = (uint32_t)strtoul(v.c_str(), nullptr, 10); }
        else if (k == "--denoise-var") { denoise_var = true; feature_spp = (uint32_t)strtoul(v.c_str(), nullptr, 10); }
        else if (k == "--denoise-guides") {
            if (v == "first") denoise_guides = (int)HRT_GUIDES_FIRST_HIT;
            else if (v == "diffuse") denoise_guides = (int)HRT_GUIDES_FIRST_DIFFUSE;
            else { std::cerr << "--denoise-guides takes first or diffuse (got " << v << ")" << std::endl; return 2; }
        }
        else if (k == "--denoise-iters") denoise_params.iterations = denoise_var_params.iterations = (uint32_t)strtoul(v.c_str(), nullptr, 10);
        else if (k == "--temporal") temporal_frames = (uint32_t)strtoul(v.c_str(), nullptr, 10);
        else if (k == "--views") n_views = (uint32_t)strtoul(v.c_str(), nullptr, 10);
        else if (k == "--orbit") orbit_degrees = strtod(v.c_str(), nullptr);
        else if (k == "--lens") {
            use_lens = true;
            if (v == "perspective") lens_params.projection = HRT_LENS_PERSPECTIVE;
            else if (v == "ortho") lens_params.projection = HRT_LENS_ORTHOGRAPHIC;
            else if (v == "equirect") lens_params.projection = HRT_LENS_EQUIRECT;
            else if (v == "fisheye") lens_params.projection = HRT_LENS_FISHEYE;
            else { std::cerr << "--lens takes perspective, ortho, equirect or fisheye (got " << v << ")" << std::endl; return 2; }
        }
        else if (k == "--aperture") lens_params.aperture_radius = strtof(v.c_str(), nullptr);
        else if (k == "--focus") lens_params.focus_distance = strtof(v.c_str(), nullptr);
        else if (k == "--lens-extent") lens_params.extent = strtof(v.c_str(), nullptr);
        else if (k == "--bake-quad") bake_quad = strtol(v.c_str(), nullptr, 10);
        else if (k == "--bake-side") bake_side = (int32_t)strtol(v.c_str(), nullptr, 10);
        else if (k == "--bake-bias") bake_bias = strtof(v.c_str(), nullptr);
        else if (k == "--probe-grid") {
            double g[3];
            if (!parse_list(v, 3, g) || !(g[0] >= 1 && g[1] >= 1 && g[2] >= 1) || g[0] > 4294967295. || g[1] > 4294967295. || g[2] > 4294967295.) {
                std::cerr << "--probe-grid takes NX,NY,NZ, three positive counts (got " << v << ")" << std::endl;
                return 2;
            }
            if (g[0] * g[1] * g[2] > 2147483647.) {  // exact in double wherever it is near the bound; refused before anything is sized by it
                std::cerr << "--probe-grid " << v << ": NX * NY * NZ must be at most 2^31 - 1" << std::endl;
                return 2;
            }
            for (int a = 0; a < 3; ++a) probe_n[a] = (uint32_t)g[a];
            probe_grid_given = true;
        }
        else if (k == "--probe-box") {
            double b[6];
            if (!parse_list(v, 6, b)) {
                std::cerr << "--probe-box takes x0,y0,z0,x1,y1,z1, the two corners of the box (got " << v << ")" << std::endl;
                return 2;
            }
            for (int a = 0; a < 6; ++a) probe_box[a] = (float)b[a];
            probe_box_given = true;
        }
        else if (k == "--probe-quad") { probe_quad = strtol(v.c_str(), nullptr, 10); probe_quad_given = true; }
        else if (k == "--probe-bounces") {
            char *end = nullptr;
            probe_bounces = strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end != '\0' || probe_bounces <= 0 || probe_bounces > 1000000) {
                std::cerr << "--probe-bounces takes a positive number of rounds (got " << v << ")" << std::endl;
                return 2;
            }
            probe_bounces_given = true;
        }
        else if (k == "--probe-tail") {
            char *end = nullptr;
            probe_tail = strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end != '\0' || probe_tail < 1 || probe_tail > (long)HRT_MAXBOUNCES) {
                std::cerr << "--probe-tail takes a number of diffuse hits in 1 .. " << HRT_MAXBOUNCES << " (got " << v << ")" << std::endl;
                return 2;
            }
        }
        else if (k == "--probe-keep") {
            char *end = nullptr;
            probe_keep = std::strtof(v.c_str(), &end);
            if (end == v.c_str() || *end != '\0' || !(probe_keep >= 0.f && probe_keep < 1.f)) {
                std::cerr << "--probe-keep takes a fraction in [0, 1) (got " << v << ")" << std::endl;
                return 2;
            }
            probe_keep_given = true;
        }
        else if (k == "--probe-rmax") { probe_rmax = (float)atof(v.c_str()); probe_rmax_given = true; }
        else if (k == "--probe-side") { probe_side = (int32_t)strtol(v.c_str(), nullptr, 10); probe_side_given = true; }
        else if (k == "--gpus") { devices.clear(); for (int d = 0; d < atoi(v.c_str()); ++d) devices.push_back(d); }
        else if (k == "--devices") {
            devices.clear();
            for (size_t a = 0; a < v.size();) { size_t b = v.find(',', a); if (b == std::string::npos) b = v.size(); devices.push_back(atoi(v.substr(a, b - a).c_str())); a = b + 1; }
        }
        else { std::cerr << "unknown option " << k << std::endl; return 2; }
    }
    if (adaptive && !devices.empty()) {
        std::cerr << "--adaptive renders on one GPU: it cannot be combined with --gpus / --devices" << std::endl;
        return 2;
    }
    if (denoise && adaptive) {
        std::cerr << "--denoise filters a uniform render: it cannot be combined with --adaptive" << std::endl;
        return 2;
    }
    if (denoise && !devices.empty()) {
        std::cerr << "--denoise renders on one GPU: it cannot be combined with --gpus / --devices" << std::endl;
        return 2;
    }
    if (denoise_var && adaptive) {
        std::cerr << "--denoise-var filters a uniform render: it cannot be combined with --adaptive" << std::endl;
        return 2;
    }
    if (denoise_var && !devices.empty()) {
        std::cerr << "--denoise-var renders on one GPU: it cannot be combined with --gpus / --devices" << std::endl;
        return 2;
    }
    if (denoise_var && denoise) {
        std::cerr << "--denoise-var and --denoise are two filters: give one of them" << std::endl;
        return 2;
    }
    if (denoise_var && (nsamples < 2u || (nsamples & 1u))) {
        std::cerr << "--denoise-var compares the two halves of the samples: --spp must be even and at least 2" << std::endl;
        return 2;
    }
    const bool temporal = temporal_frames != 0u;
    if (temporal && (adaptive || denoise || !devices.empty())) {
        std::cerr << "--temporal accumulates uniform renders on one GPU: it cannot be combined with --adaptive, --denoise or --gpus / --devices (--denoise-var is its filter)" << std::endl;
        return 2;
    }
    if (temporal && (nsamples < 2u || (nsamples & 1u))) {
        std::cerr << "--temporal keeps the two halves of every frame's samples: --spp must be even and at least 2" << std::endl;
        return 2;
    }
    if (n_views != 0u && (adaptive || denoise || denoise_var || temporal || !devices.empty())) {
        std::cerr << "--views renders plain frames on one GPU: it cannot be combined with --adaptive, --denoise, --denoise-var, --temporal or --gpus / --devices" << std::endl;
        return 2;
    }
    if (denoise_guides != -1 && !denoise && !denoise_var) {
        std::cerr << "--denoise-guides says where a filter's features come from: give --denoise or --denoise-var" << std::endl;
        return 2;
    }
    if (denoise_guides != -1 && temporal) {
        std::cerr << "--denoise-guides cannot be combined with --temporal: the reprojection reads the first-hit depth, which a path depth is not" << std::endl;
        return 2;
    }
    if (denoise_guides == (int)HRT_GUIDES_FIRST_DIFFUSE && feature_spp == 0u) {
        std::cerr << "--denoise-guides diffuse follows the paths of the samples: FEATURE_SPP must be at least 1 (a pixel-centre path has no stream)" << std::endl;
        return 2;
    }
    if (use_lens && (((denoise || denoise_var) && denoise_guides == -1) || temporal || !devices.empty())) {
        std::cerr << "--lens renders plain or adaptive frames on one GPU: it cannot be combined with --denoise or --denoise-var (unless --denoise-guides is given), --temporal or --gpus / --devices" << std::endl;
        return 2;
    }
    if (!use_lens && (lens_params.aperture_radius != 0.f || lens_params.focus_distance != 1.f || lens_params.extent != 0.f)) {
        std::cerr << "--aperture, --focus and --lens-extent describe a lens: give --lens perspective|ortho|equirect|fisheye" << std::endl;
        return 2;
    }
    if (!temporal && n_views == 0u && orbit_degrees != 0.0) {
        std::cerr << "--orbit turns the camera over the frames of --temporal or the cameras of --views: give --temporal FRAMES or --views N" << std::endl;
        return 2;
    }
    if (probe_grid_given != probe_box_given) {
        std::cerr << (probe_grid_given ? "--probe-grid NX,NY,NZ needs the box of the grid: give --probe-box x0,y0,z0,x1,y1,z1"
                                       : "--probe-box x0,y0,z0,x1,y1,z1 needs the counts of the grid: give --probe-grid NX,NY,NZ") << std::endl;
        return 2;
    }
    if (probe_quad_given && !probe_grid_given) {
        std::cerr << "--probe-quad looks a probe grid up over a quad: give --probe-grid NX,NY,NZ and --probe-box x0,y0,z0,x1,y1,z1" << std::endl;
        return 2;
    }
    if (probe_lit && !probe_grid_given) {
        std::cerr << "--probe-lit lights a camera frame from a probe grid: give --probe-grid NX,NY,NZ and --probe-box x0,y0,z0,x1,y1,z1" << std::endl;
        return 2;
    }
    if (probe_lit && probe_quad_given) {
        std::cerr << "--probe-lit writes a camera frame, --probe-quad a lightmap: give one of them" << std::endl;
        return 2;
    }
    if (bake_lit && (bake_quad == -1 || !probe_grid_given)) {
        std::cerr << "--bake-lit bakes a lightmap whose paths end in a probe grid: give --bake-quad INDEX, --probe-grid NX,NY,NZ and --probe-box x0,y0,z0,x1,y1,z1" << std::endl;
        return 2;
    }
    if (bake_lit && (probe_lit || probe_quad_given)) {
        std::cerr << "--bake-lit writes a gathered lightmap, --probe-lit a camera frame, --probe-quad a looked-up lightmap: give one of them" << std::endl;
        return 2;
    }
    if (probe_tail && !probe_bounces_given && !probe_lit && !bake_lit) {
        std::cerr << "--probe-tail says where the paths of --probe-lit and --probe-bounces end: give one of them" << std::endl;
        return 2;
    }
    if (probe_keep_given && !probe_bounces_given) {
        std::cerr << "--probe-keep blends the rounds of --probe-bounces: give --probe-bounces K" << std::endl;
        return 2;
    }
    if (probe_bounces_given && !probe_quad_given && !probe_lit && !bake_lit) {
        std::cerr << "--probe-bounces relights the probe grid of a lightmap or a frame: give --probe-quad INDEX or --probe-lit" << std::endl;
        return 2;
    }
    if (probe_bounces_given && (uint64_t)probe_bounces * nsamples > 0x100000000ull) {
        std::cerr << "--probe-bounces x --spp must be at most 2^32 (sample indices do not wrap)" << std::endl;
        return 2;
    }
    if (!probe_quad_given && (probe_side_given || (probe_facing && !probe_lit && !bake_lit))) {
        std::cerr << (probe_side_given ? "--probe-side" : "--probe-facing") << " describes the look-up of a probe grid over a quad: give --probe-quad INDEX" << std::endl;
        return 2;
    }
    if (!probe_quad_given && !probe_lit && !bake_lit && (probe_visible || probe_rmax_given)) {
        std::cerr << (probe_visible ? "--probe-visible" : "--probe-rmax") << " describes the look-up of a probe grid over a quad: give --probe-quad INDEX" << std::endl;
        return 2;
    }
    if (probe_rmax_given && !probe_visible) {
        std::cerr << "--probe-rmax cuts the depths of --probe-visible: give --probe-visible" << std::endl;
        return 2;
    }
    if (probe_rmax_given && !(std::isfinite(probe_rmax) && probe_rmax > 0.f)) {
        std::cerr << "--probe-rmax takes a finite positive distance (got " << probe_rmax << ")" << std::endl;
        return 2;
    }
    if (probe_side != 1 && probe_side != -1) {
        std::cerr << "--probe-side takes 1 or -1 (got " << probe_side << ")" << std::endl;
        return 2;
    }
    const bool probes = probe_grid_given;
    if (probes) {
        const char *other = use_lens && !probe_lit ? "--lens" : bake_quad != -1 && !bake_lit ? "--bake-quad" : n_views != 0u && !probe_lit ? "--views" : adaptive && !probe_lit ? "--adaptive" : denoise ? "--denoise"
                            : denoise_var ? "--denoise-var" : temporal ? "--temporal" : !devices.empty() ? "--gpus / --devices" : nullptr;
        if (other) {
            std::cerr << "--probe-grid traces light probes on one GPU: it cannot be combined with " << other << std::endl;
            return 2;
        }
    }
    const bool bake = bake_quad != -1;
    if (bake && (adaptive || denoise || denoise_var || temporal || n_views != 0u || use_lens || !devices.empty())) {
        std::cerr << "--bake-quad bakes a lightmap on one GPU: it cannot be combined with a render mode or --gpus / --devices" << std::endl;
        return 2;
    }
    if (!bake && (bake_side != 1 || bake_bias != 1e-4f)) {
        std::cerr << "--bake-side and --bake-bias describe a lightmap: give --bake-quad INDEX" << std::endl;
        return 2;
    }
    scene.asset_root = assets;
    if (!scene.setup_by_name(name, (float)SCREENWIDTH / (float)SCREENHEIGHT, seed)) {
        std::cerr << scene.error << std::endl;
        return EXIT_FAILURE;  // the reference exit()s on a missing mesh (Mesh.cpp:12-13)
    }
    if (kd_on_gpu) {  // the trees' split search on the device (hrt_kd_build_gpu): the same trees, built before the scene is uploaded
        if (hrt_init(devices.empty() ? gpu : devices[0]) != HRT_OK) { std::cerr << hrt_last_error() << std::endl; return EXIT_FAILURE; }
        scene.kd_params.builder = hrt_kd_build_gpu;
    }
    std::unique_ptr<FlatScene> flat = scene.flatten();
    if (bake && (bake_quad < 0 || (unsigned long)bake_quad >= flat->desc.n_quads)) {  // before any device is touched
        std::cerr << "--bake-quad " << bake_quad << ": the scene has " << flat->desc.n_quads << " quads" << std::endl;
        return 2;
    }
    if (probe_quad_given && (probe_quad < 0 || (unsigned long)probe_quad >= flat->desc.n_quads)) {  // before any device is touched
        std::cerr << "--probe-quad " << probe_quad << ": the scene has " << flat->desc.n_quads << " quads" << std::endl;
        return 2;
    }
    const int up = devices.empty() ? (hrt_init(gpu) != HRT_OK ? HRT_ERR_DEVICE : hrt_scene_create(&flat->desc, &device_scene))
                                   : hrt_multi_create(&flat->desc, (uint32_t)devices.size(), devices.data(), &multi);
    if (up != HRT_OK) {
        std::cerr << hrt_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    if (multi) {  // which gather the tiles take to slot 0, and anything creation fell back from
        const std::string note = hrt_last_error();
        std::cout << "Image tiles across " << devices.size() << " GPU slot(s), gather: " << hrt_multi_gather(multi)
                  << (note.empty() ? "" : " (" + note + ")") << std::endl;
    }
    int rc = probes ? light_probes(flat->desc) : bake ? bake_lightmap(flat->desc) : n_views ? ray_trace_views() : use_lens ? (denoise || denoise_var ? ray_trace_lens_denoised() : ray_trace_lens()) : temporal ? ray_trace_frames() : ray_trace_from_camera();  // the 'r' key, once or frame after frame
    hrt_scene_destroy(device_scene);
    hrt_multi_destroy(multi);
    hrt_shutdown();
    return rc == HRT_OK ? 0 : EXIT_FAILURE;
}
