"""The variance-guided denoiser on the GPU (include/hrt.h hrt_denoise_var, hrt_render_denoised_var) against the numpy statement
(tests/denoise_var_ref.py): bit for bit in the exact regime, within the fixed-width filter's tolerance where the weights go through
expf, the whole-frame call against its parts, non-finite frames, scratch reuse, the CLI, and the quality against converged renders."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dv
from scene_util import overflow_scene, same_nonfinite
from test_gpu_denoise import assert_close, aov, build, rmse
from test_gpu_denoise_edges import device_coord_frame, diff_text, same

pytestmark = pytest.mark.gpu

F32 = np.float32
EXACT = dict(sigma_variance=np.inf, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=1e-30)  # denoise_ref.EXACT for this rule


def dev_denoise_var(gpu, c, half, f, flags=0, variance=True, **params):
    """hrt_denoise_var on numpy arrays or torch tensors -> (frame, variance map) as numpy arrays (the map None if not asked for)."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, F32)).cuda() if isinstance(a, np.ndarray) else a
    c, half, f = up(c), up(half), up(f)
    h, w = c.shape[0], c.shape[1]
    scratch = torch.empty(gpu.denoise_var_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    var = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda") if variance else None
    s = torch.cuda.current_stream()
    gpu.denoise_var(c.data_ptr(), half.data_ptr(), f.data_ptr(), w, h, gpu.DenoiseVarParams(**params), flags, scratch.data_ptr(),
                    out.data_ptr(), var.data_ptr() if variance else 0, s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy(), (var.cpu().numpy() if variance else None)


def params_dict(p):
    return {k: getattr(p, k) for k, _ in p._fields_}


# 1. the exact regime: every weight is h_j h_k or 0, so frame and variance map equal the statement bit for bit
@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (41, 67), (256, 256)])
def test_exact_regime_bit_for_bit_for_every_iteration_and_prefilter_count(gpu, h, w):
    c, f = dr.hard_edge_frame(h, w, seed=h * 1000 + w, block=(3, 4))
    half, _ = dr.hard_edge_frame(h, w, seed=h * 1000 + w + 77, block=(3, 4))  # an independent hash frame
    for it in range(1, 9):
        for pre in range(0, 5):
            ref, vref = dv.denoise_var(c, half, f, iterations=it, prefilter=pre, **EXACT)
            got, vgot = dev_denoise_var(gpu, c, half, f, iterations=it, prefilter=pre, **EXACT)
            assert same(got, ref), f"{h}x{w} iterations {it} prefilter {pre}: {diff_text(got, ref)}"
            assert np.array_equal(vgot.view(np.uint32), vref.view(np.uint32)), \
                f"{h}x{w} iterations {it} prefilter {pre}: variance differs on {int((vgot != vref).sum())} pixels"
    assert (vref > 0).any() or h * w == 1


def test_exact_regime_without_a_variance_map_and_with_a_floor(gpu):
    h, w = 41, 67
    c, f = dr.hard_edge_frame(h, w, seed=4)
    half, _ = dr.hard_edge_frame(h, w, seed=5)
    ref, _ = dv.denoise_var(c, half, f, iterations=3, prefilter=1, **EXACT)
    got, none = dev_denoise_var(gpu, c, half, f, variance=False, iterations=3, prefilter=1, **EXACT)
    assert none is None and same(got, ref)
    got, _ = dev_denoise_var(gpu, c, half, f, iterations=3, prefilter=1, variance_floor=0.25, **EXACT)  # +inf width: the floor is idle
    assert same(got, ref)


@pytest.mark.parametrize("iterations,prefilter,k", [(4, 2, 64), (8, 4, 24)])
def test_exact_regime_1080p_on_windows(gpu, iterations, prefilter, k):
    import torch
    h, w, seed = 1080, 1920, 21
    c, f = device_coord_frame(h, w, seed)
    half, _ = device_coord_frame(h, w, seed + 50)
    scratch = torch.empty(gpu.denoise_var_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    var = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    p = gpu.DenoiseVarParams(iterations=iterations, prefilter=prefilter, **EXACT)
    gpu.denoise_var(c.data_ptr(), half.data_ptr(), f.data_ptr(), w, h, p, 0, scratch.data_ptr(), out.data_ptr(), var.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del c, f, half

    def get(a, b, pp, q):  # the crop reaches dv.reach(iterations, prefilter) beyond the window
        cc, ff = dr.coord_window(a, b, pp, q, seed)
        hh, _ = dr.coord_window(a, b, pp, q, seed + 50)
        return cc, hh, ff

    windows = [(0, k, 0, k), (h - k, h, w - k, w)] if iterations == 8 else \
        [(0, k, 0, k), (h - k, h, w - k, w), (0, k, w - k, w), (h // 2, h // 2 + k, w // 2, w // 2 + k), (h - k, h, 900, 900 + k)]
    for y0, y1, x0, x1 in windows:
        ref, vref = dv.denoise_var_window(get, h, w, y0, y1, x0, x1, iterations, prefilter, **EXACT)
        got, vgot = out[y0:y1, x0:x1].cpu().numpy(), var[y0:y1, x0:x1].cpu().numpy()
        assert same(got, ref), f"window rows {y0}:{y1} cols {x0}:{x1}: {diff_text(got, ref)}"
        assert np.array_equal(vgot.view(np.uint32), vref.view(np.uint32)), f"window rows {y0}:{y1} cols {x0}:{x1}: variance differs"


# 2. finite sigmas: the weights go through expf; the tolerance of the fixed-width filter's test (assert_close: 1e-5 relative, floor 1e-3)
# The FRAME is compared over the whole chain of passes.  The VARIANCE MAP is compared pass by pass (test_every_pass_... below): the
# map of one iteration sets the widths, hence the exponents, of the next and enters the sums with squared weights, so over a chain the
# two sides' expf roundings feed back and the map drifts (measured over whole chains at 256x256: 0.07, 0.2, 0.5, 1.2, 1.5, 1.9, 3.0, 2.2
# times the tolerance after 1 .. 8 iterations, on at most 86 of 65 536 pixels; below it at every other size; the frame at most 0.18).
# Fed with the device's own previous {x, v}, one pass has no feedback and the tolerance applies to it as it stands.
def assert_close_var(got, ref, what):
    """assert_close for the one-channel variance map."""
    assert_close(got[..., None], ref[..., None], what)


def colour_space_frame(h, w, seed):
    """synthetic_features with every albedo negated and no emitter, and a colour frame with its half: d = 1 and e = 0 everywhere, so
    x = c and the filter's output IS its last {x}, while normal, albedo and depth still differ across the guide edges."""
    f = dr.synthetic_features(h, w, seed=seed)
    f[..., 0:3] = -f[..., 0:3]
    f[..., 6:9] = 0
    rng = np.random.default_rng(300 + seed)
    c = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    half = (c + rng.normal(0, 0.1, (h, w, 3))).astype(F32)
    return c, half, f


@pytest.mark.parametrize("h,w", [(256, 256), (41, 67)])
@pytest.mark.parametrize("prefilter", [0, 2])
def test_every_pass_of_the_device_follows_the_statement_from_the_devices_own_state(gpu, h, w, prefilter):
    c, half, f = colour_space_frame(h, w, seed=prefilter)
    kw = dict(prefilter=prefilter, sigma_variance=3.0, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1, variance_floor=1e-6)
    x, v = dev_denoise_var(gpu, c, half, f, iterations=1, **kw)   # the prefilter passes and iteration 0: nothing feeds back yet
    ref, vref = dv.denoise_var(c, half, f, iterations=1, **kw)
    assert_close(x, ref, f"{h}x{w} pre {prefilter} iteration 0")
    assert_close_var(v, vref, f"{h}x{w} pre {prefilter} iteration 0 variance")
    for i in range(1, 8):  # iteration i alone: the statement's pass on the device's {x, v} after iterations 0 .. i-1
        assert np.isfinite(x).all() and np.isfinite(v).all()
        xn, vn = dev_denoise_var(gpu, c, half, f, iterations=i + 1, **kw)
        xr, vr = dv.pass_(x, v, f, i, kw["sigma_variance"], kw["variance_floor"], kw["sigma_normal"], kw["sigma_albedo"], kw["sigma_depth"],
                          prefilter=False)
        assert_close(xn, xr, f"{h}x{w} pre {prefilter} iteration {i}")
        assert_close_var(vn, vr, f"{h}x{w} pre {prefilter} iteration {i} variance")
        x, v = xn, vn


@pytest.mark.parametrize("h,w", [(256, 256), (41, 67), (300, 1), (1, 300)])
@pytest.mark.parametrize("iterations,prefilter", [(1, 0), (2, 1), (3, 4), (4, 2), (5, 2), (6, 3), (7, 0), (8, 1)])
def test_device_filter_matches_the_numpy_statement(gpu, h, w, iterations, prefilter):
    f = dr.synthetic_features(h, w, seed=iterations)
    rng = np.random.default_rng(100 + iterations)
    c = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    c[f[..., 6] > 0] = F32(5.0 / 6.0)
    half = (c + rng.normal(0, 0.1, (h, w, 3))).astype(F32)
    kw = dict(iterations=iterations, prefilter=prefilter, sigma_variance=3.0, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1, variance_floor=1e-6)
    got, vgot = dev_denoise_var(gpu, c, half, f, **kw)
    ref, vref = dv.denoise_var(c, half, f, **kw)
    assert_close(got, ref, f"{h}x{w} it {iterations} pre {prefilter}")
    if iterations == 1:  # one iteration has no feedback: the map too
        assert_close_var(vgot, vref, f"{h}x{w} it {iterations} pre {prefilter} variance")
    if iterations in (1, 5):  # gamma, and the default parameters
        p = params_dict(gpu.DenoiseVarParams(iterations=iterations))
        g, _ = dev_denoise_var(gpu, c, half, f, gpu.FLAG_GAMMA, **p)
        assert_close(g, dv.denoise_var(c, half, f, gamma=True, **p)[0], "gamma")


def test_device_filter_matches_the_numpy_statement_on_a_rendered_frame(gpu):
    w, h = 160, 90
    _, _, dev, cam = build(gpu, "cornell_mesh", w, h)
    img, _ = dev.render(cam, w, h, 8, 1)
    half, _ = dev.render(cam, w, h, 4, 1)
    for n in (0, 4):
        f = dev.render_features(cam, w, h, 0, n, 1)
        p = params_dict(gpu.DenoiseVarParams())
        got, vgot = dev_denoise_var(gpu, img, half, f, **p)
        ref, vref = dv.denoise_var(img, half, f, **p)
        assert_close(got, ref, f"cornell_mesh features n={n}")
        assert_close_var(vgot, vref, f"cornell_mesh features n={n} variance")


# 3. the whole-frame call equals its parts, for every kernel form, and filters hrt_render(spp)
def test_render_denoised_var_equals_its_parts_and_every_kernel_form(gpu):
    w, h, spp, fspp, seed = 120, 68, 8, 4, 5
    _, _, dev, cam = build(gpu, "cornell_mesh", w, h)
    p = gpu.DenoiseVarParams()
    for flags in (0, gpu.FLAG_GAMMA):
        whole, vwhole = dev.render_denoised_var(cam, w, h, spp, fspp, seed, flags, p, variance=True)
        img, _ = dev.render(cam, w, h, spp, seed)
        half, _ = dev.render(cam, w, h, spp // 2, seed)
        f = dev.render_features(cam, w, h, 0, fspp, seed)
        parts, vparts = dev_denoise_var(gpu, img, half, f, flags, **params_dict(p))
        assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
        assert np.array_equal(vwhole.view(np.uint32), vparts.view(np.uint32))
        assert np.array_equal(dev.render_denoised_var(cam, w, h, spp, fspp, seed, flags, p).view(np.uint32), whole.view(np.uint32))
        for form in (gpu.FLAG_WAVE_KERNEL, gpu.FLAG_DUAL_KERNEL, gpu.FLAG_STREAM_KERNEL):
            other, vother = dev.render_denoised_var(cam, w, h, spp, fspp, seed, flags | form, p, variance=True)
            assert np.array_equal(other.view(np.uint32), whole.view(np.uint32)), f"kernel form {form}"
            assert np.array_equal(vother.view(np.uint32), vwhole.view(np.uint32)), f"kernel form {form}: variance"
    st = gpu.Stats()
    dev.render_denoised_var(cam, w, h, spp, 0, seed, 0, p, st)
    assert st.kernel_ms > 0 and st.samples == w * h * spp


def test_render_denoised_var_filters_the_frame_of_render(gpu):
    # one iteration whose every off-centre weight is 0 (guide widths 1e-30 on per-sample features, which differ between neighbours
    # wherever a surface is hit; colour width +inf) is the identity up to d * ((h0 h0 x) / (h0 h0)) + e/6: compare with that of render's frame
    w, h, spp, seed = 96, 54, 6, 3
    _, _, dev, cam = build(gpu, "random_spheres", w, h)
    img, _ = dev.render(cam, w, h, spp, seed)
    half, _ = dev.render(cam, w, h, spp // 2, seed)
    f = dev.render_features(cam, w, h, 0, spp, seed)
    p = gpu.DenoiseVarParams(iterations=1, prefilter=0, **EXACT)
    whole, v = dev.render_denoised_var(cam, w, h, spp, spp, seed, 0, p, variance=True)
    ref, vref = dv.denoise_var(img, half, f, **params_dict(p))
    assert same(whole, ref) and np.array_equal(v.view(np.uint32), vref.view(np.uint32))
    x, v0, _ = dv.prepare(img, half, f)
    assert (v0 > 0).mean() > 0.5, "the two halves should differ on most pixels"
    with pytest.raises(gpu.HrtError, match="spp must be even"):
        dev.render_denoised_var(cam, w, h, 7, 1, seed)


# 4. non-finite frames
def test_non_finite_pixels_pass_through_and_finite_ones_stay_finite(gpu):
    w, h, spp = 64, 48, 8
    host = overflow_scene(gpu, "emission", False)
    desc = host.flatten()
    dev = gpu.DeviceScene(desc)
    cam = gpu.default_camera(w / h)
    img, _ = dev.render(cam, w, h, spp, 1)
    den, var = dev.render_denoised_var(cam, w, h, spp, 2, 1, variance=True)
    nf = ~np.isfinite(img)
    assert nf.any(), "the scene should overflow"
    assert same_nonfinite(den[nf], img[nf]).all()
    fin = np.isfinite(img).all(axis=-1)
    assert np.isfinite(den[fin]).all()
    assert np.isfinite(var).all() and (var[~fin] == 0).all()


# 5. scratch reuse across sizes, and beside the fixed-width filter
def test_scratch_is_reused_across_sizes_and_filters(gpu):
    _, _, dev, cam_s = build(gpu, "cornell_mesh", 96, 54)
    cam_l = gpu.default_camera(1920 / 1080)
    a = dev.render_denoised_var(cam_s, 96, 54, 4, 2, 7)
    old = dev.render_denoised(cam_s, 96, 54, 4, 2, 7)
    b, vb = dev.render_denoised_var(cam_l, 1920, 1080, 2, 1, 7, variance=True)
    c = dev.render_denoised_var(cam_s, 96, 54, 4, 2, 7)
    _, _, fresh_s, _ = build(gpu, "cornell_mesh", 96, 54)
    _, _, fresh_l, _ = build(gpu, "cornell_mesh", 1920, 1080)
    ref_s = fresh_s.render_denoised_var(cam_s, 96, 54, 4, 2, 7)
    assert np.array_equal(a.view(np.uint32), ref_s.view(np.uint32)) and np.array_equal(c.view(np.uint32), ref_s.view(np.uint32))
    rb, rvb = fresh_l.render_denoised_var(cam_l, 1920, 1080, 2, 1, 7, variance=True)
    assert np.array_equal(b.view(np.uint32), rb.view(np.uint32)) and np.array_equal(vb.view(np.uint32), rvb.view(np.uint32))
    assert np.array_equal(old.view(np.uint32), fresh_s.render_denoised(cam_s, 96, 54, 4, 2, 7).view(np.uint32))
    assert np.array_equal(dev.render(cam_s, 96, 54, 4, 7)[0], fresh_s.render(cam_s, 96, 54, 4, 7)[0])  # the sums buffer is hrt_render's


# 6. the CLI
def cli(args, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "hai719-raytracing_amd", "raytracer")
    out = tmp_path / "d.ppm"
    r = subprocess.run([exe, "--scene", "cornell_mesh", "--w", "192", "--h", "108", "--out", str(out), "--assets", os.path.join(root, "assets")] + args,
                       capture_output=True, text=True, timeout=300)
    return r, out


def test_cli_writes_a_frame_and_refuses_what_it_cannot_combine(gpu, tmp_path):
    r, out = cli(["--spp", "8", "--denoise-var", "2", "--denoise-iters", "3"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes().startswith(b"P3\n192 108\n255\n")
    assert "denoised by variance" in r.stdout and "3 iterations" in r.stdout
    for extra, word in ((["--adaptive", "0.05"], "--adaptive"), (["--gpus", "1"], "--gpus"), (["--denoise", "2"], "--denoise"),
                        (["--spp", "7"], "even")):
        r, _ = cli(["--spp", "8", "--denoise-var", "2"] + extra, tmp_path)
        assert r.returncode == 2 and word in r.stderr and "--denoise-var" in r.stderr, (extra, r.stderr)


# 7. quality against a 4096-spp render: the set-up of test_denoised_frames_are_closer_to_the_converged_render
# RMSE ratios denoised / noisy at 480x270 (profiles/denoise_var_report.json, DESIGN.md section 5 "Variance-guided denoising"),
# fixed-width -> variance-guided at seeds 1, 2, 3, 4:
#   cornell_mesh   4 spp  0.6771 0.6735 0.6667 0.6797 -> 0.6364 0.6345 0.6279 0.6420   excess -0.0407 -0.0390 -0.0388 -0.0377
#   cornell_mesh  16 spp  0.6383 0.6586 0.6434 0.6535 -> 0.6359 0.6582 0.6406 0.6561   excess -0.0024 -0.0004 -0.0028 +0.0026
#   cornell_mesh  64 spp  0.6695 0.6711 0.6676 0.6698 -> 0.6658 0.6684 0.6672 0.6678   excess -0.0037 -0.0027 -0.0004 -0.0020
# CORNELL_MARGIN: how far the variance-guided ratio may exceed the fixed-width filter's ratio of the same run on cornell_mesh: the
# excess measured at seed 1 plus the spread (max - min) of the excess over seeds 1..4: 0.0030, 0.0054, 0.0033.
CORNELL_MARGIN = {4: -0.0407 + 0.0030, 16: -0.0024 + 0.0054, 64: -0.0037 + 0.0033}


@pytest.mark.parametrize("spp", [4, 16, 64])
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
def test_variance_guided_frames_are_closer_to_the_converged_render(gpu, name, spp):
    w, h, seed = 480, 270, 1
    _, _, dev, cam = build(gpu, name, w, h)
    ref, _ = dev.render(cam, w, h, 4096, seed)
    noisy, _ = dev.render(cam, w, h, spp, seed)
    old = dev.render_denoised(cam, w, h, spp, spp, seed)       # the fixed-width filter, its defaults: the yardstick
    new = dev.render_denoised_var(cam, w, h, spp, spp, seed)
    rn = rmse(noisy, ref)
    r_old, r_new = rmse(old, ref) / rn, rmse(new, ref) / rn
    print(f"QUALITY {name} spp {spp}: noisy {rn:.5f} fixed-width ratio {r_old:.4f} variance-guided ratio {r_new:.4f}")
    assert r_new < 1.0, f"{name} @ {spp}: the variance-guided frame is worse than the noisy one ({r_new:.4f})"
    if name == "random_spheres" and spp in (16, 64):
        assert r_new < r_old, f"{name} @ {spp}: variance-guided {r_new:.4f} is not below fixed-width {r_old:.4f}"
    if name == "cornell_mesh":
        assert r_new <= r_old + CORNELL_MARGIN[spp], f"{name} @ {spp}: variance-guided {r_new:.4f} vs fixed-width {r_old:.4f}"
    if name == "cornell_mesh" and spp == 16:
        assert abs(new.mean() / ref.mean() - 1.0) <= 0.01
        hit = aov(gpu, dev, cam, w, h, 0)
        key = hit[..., 1] * 1e6 + hit[..., 2]
        sil = np.zeros((h, w), bool)
        sil[:, 1:] |= key[:, 1:] != key[:, :-1]
        sil[:, :-1] |= key[:, :-1] != key[:, 1:]
        sil[1:] |= key[1:] != key[:-1]
        sil[:-1] |= key[:-1] != key[1:]
        assert sil.sum() > 100
        assert rmse(new[sil], ref[sil]) <= rmse(noisy[sil], ref[sil]), "silhouettes got worse"
