"""The NumPy statement of the variance-guided denoiser (tests/denoise_var_ref.py) against cases that can be worked out by hand."""
import numpy as np

import denoise_ref as dr
import denoise_var_ref as dv

F32 = np.float32
OFF = dict(sigma_normal=np.inf, sigma_albedo=np.inf, sigma_depth=np.inf)


def flat_features(h, w, albedo=1.0):
    f = np.zeros((h, w, 12), F32)
    f[..., 0:3] = albedo
    f[..., 4] = 1
    f[..., 9] = 2
    f[..., 10] = 1
    return f


def test_a_constant_frame_comes_back_unchanged_with_zero_variance():
    # every weight is a dyadic h_j h_k and every x is 0.5: all sums are exact, at the borders too
    h, w = 23, 31
    f = flat_features(h, w, albedo=0.5)
    c = np.full((h, w, 3), 0.25, F32)
    for pre in (0, 2):
        for sv in (8.0, np.inf):
            for floor in (0.0, 1e-8):
                out, v = dv.denoise_var(c, c, f, iterations=4, prefilter=pre, sigma_variance=sv, variance_floor=floor)
                assert np.array_equal(out, c) and (v == 0).all()


def test_with_the_colour_term_off_and_no_prefilter_the_frame_is_the_fixed_width_filters():
    h, w = 41, 67
    f = dr.synthetic_features(h, w, seed=3)
    rng = np.random.default_rng(5)
    c = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    half = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    for it in (1, 3, 5):
        for g in (dict(sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1), dict(sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=1e-30)):
            out, _ = dv.denoise_var(c, half, f, iterations=it, prefilter=0, sigma_variance=np.inf, **g)
            ref = dr.denoise(c, f, iterations=it, sigma_color=np.inf, **g)
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    out, _ = dv.denoise_var(c, half, f, iterations=2, prefilter=0, sigma_variance=np.inf, gamma=True)
    assert np.array_equal(out, dr.denoise(c, f, iterations=2, sigma_color=np.inf, gamma=True))


def test_the_variance_is_the_squared_distance_to_the_half_frame_in_demodulated_units():
    f = flat_features(4, 5, albedo=0.5)
    f[0, 0, 6:9] = 3.0  # an emitter: e/6 = 0.5 leaves both frames before the division
    c = np.full((4, 5, 3), 1.0, F32)
    half = c.copy()
    half[..., 0] = 0.75
    half[..., 2] = 1.5
    x, v, d = dv.prepare(c, half, f)
    assert (d == 0.5).all() and (x[1:] == 2.0).all() and (x[0, 0] == 1.0).all()
    assert (v == F32(0.5 ** 2 + 1.0 ** 2)).all()  # the albedo doubles both differences; the emission cancels


def test_the_carried_variance_of_a_constant_map_shrinks_by_the_kernels_sum_of_squares():
    # all weights h_j h_k: v <- v sum (h_j h_k)^2 / (sum h_j h_k)^2 = v (70/256)^2 per iteration, away from the borders
    h, w = 80, 90
    f = flat_features(h, w)
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    v = np.ones((h, w), F32)
    shrink = (70.0 / 256.0) ** 2
    want = 1.0
    for i in range(4):
        x, v = dv.pass_(x, v, f, i, np.inf, 0.0, np.inf, np.inf, np.inf, prefilter=False)
        want *= shrink
        r = dr.radius(i + 1)
        inner = v[r:h - r, r:w - r]
        if i < 2:
            assert (inner == F32(want)).all(), i             # 4900^2 / 2^32 still fits fp32: exact
        else:
            assert np.allclose(inner, want, rtol=1e-6, atol=0), i
        assert (v >= F32(want * (1 - 1e-6))).all()           # fewer taps near a border average less
    # a prefilter pass leaves a constant map alone, everywhere
    _, vp = dv.pass_(x, np.full((h, w), 3.0, F32), f, 1, np.inf, 0.0, np.inf, np.inf, np.inf, prefilter=True)
    assert (vp == 3.0).all()


def test_a_converged_pixel_keeps_its_value_and_a_noisy_one_is_averaged():
    # left half: the two frames agree (v = 0 on both pixels of a pair, floor 0): only equal neighbours are accepted, the checkerboard survives exactly;
    # right half: the half frame is far away (wide colour term): the checkerboard is smoothed
    h, w = 32, 64
    f = flat_features(h, w)
    ys, xs = np.mgrid[0:h, 0:w]
    c = np.repeat((((ys + xs) % 2) * 0.5 + 0.25).astype(F32)[..., None], 3, -1)
    half = c.copy()
    half[:, w // 2:] += F32(1.0)
    out, v = dv.denoise_var(c, half, f, iterations=3, prefilter=0, sigma_variance=4.0, variance_floor=0.0, **OFF)
    assert np.array_equal(out[:, :w // 2 - 14], c[:, :w // 2 - 14])  # 14: the reach of three iterations
    right = out[4:-4, w // 2 + 8:-4]
    assert np.abs(right - 0.5).max() < 0.02
    assert (v[:, :w // 2 - 14] == 0).all() and (v[:, w // 2:] > 0).all() and (v[:, w // 2:] < 3.0).all()


def test_pixels_invalid_in_either_frame_pass_through_and_are_skipped_as_taps():
    h, w = 20, 24
    f = dr.synthetic_features(h, w, seed=1)
    rng = np.random.default_rng(2)
    c = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    half = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    c[3, 4, 1] = np.inf
    half[10, 11, 0] = np.nan
    f[15, 5, 9] = np.inf
    out, v = dv.denoise_var(c, half, f, iterations=3, prefilter=2, sigma_variance=2.0)
    for (y, x) in ((3, 4), (10, 11), (15, 5)):
        assert np.array_equal(out[y, x].view(np.uint32), c[y, x].view(np.uint32)) and v[y, x] == 0
    ok = np.isfinite(c).all(-1)
    assert np.isfinite(out[ok]).all() and np.isfinite(v).all()
    # a frame without those pixels' neighbours' help differs only within the rule's reach
    c2, h2, f2 = c.copy(), half.copy(), f.copy()
    c2[3, 4, 1], h2[10, 11, 0], f2[15, 5, 9] = 0.5, 0.5, 2.0
    out2, _ = dv.denoise_var(c2, h2, f2, iterations=1, prefilter=0, sigma_variance=2.0)
    out1, _ = dv.denoise_var(c, half, f, iterations=1, prefilter=0, sigma_variance=2.0)
    far = np.ones((h, w), bool)
    for (y, x) in ((3, 4), (10, 11), (15, 5)):
        far[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = False
    assert np.array_equal(out1[far], out2[far])


def test_an_overflowing_variance_counts_as_zero():
    f = flat_features(3, 3)
    c = np.full((3, 3, 3), 1e30, F32)
    half = np.full((3, 3, 3), -1e30, F32)
    _, v, _ = dv.prepare(c, half, f)
    assert (v == 0).all()
    out, v = dv.denoise_var(c, half, f, iterations=2, prefilter=1)
    assert np.isfinite(out).all() and (v == 0).all()


def test_a_window_of_the_frame_equals_the_whole_frame_there():
    h, w = 70, 90
    c, f = dr.hard_edge_frame(h, w, seed=2)
    half, _ = dr.hard_edge_frame(h, w, seed=12)
    exact = dict(sigma_variance=np.inf, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=1e-30)
    full, vfull = dv.denoise_var(c, half, f, iterations=2, prefilter=2, **exact)
    get = lambda y0, y1, x0, x1: (c[y0:y1, x0:x1], half[y0:y1, x0:x1], f[y0:y1, x0:x1])
    for (y0, y1, x0, x1) in ((0, 10, 0, 10), (30, 45, 40, 60), (60, 70, 80, 90)):
        win, vwin = dv.denoise_var_window(get, h, w, y0, y1, x0, x1, 2, 2, **exact)
        assert np.array_equal(win.view(np.uint32), full[y0:y1, x0:x1].view(np.uint32))
        assert np.array_equal(vwin.view(np.uint32), vfull[y0:y1, x0:x1].view(np.uint32))
    assert dv.reach(2, 2) == 12 and dv.reach(8, 0) == dr.radius(8) and dv.reach(1, 4) == 2 + 30


def test_the_prefilter_smooths_the_variance_inside_a_guide_region_only():
    h, w = 30, 40
    f = flat_features(h, w)
    f[:, 20:, 3:6] = (1, 0, 0)  # another normal on the right
    c = np.full((h, w, 3), 0.5, F32)
    half = c.copy()
    half[10, 10] += F32(0.5)   # one noisy pixel on the left
    x, v, _ = dv.prepare(c, half, f)
    assert v[10, 10] == F32(0.75) and v.sum() == F32(0.75)
    _, v1 = dv.pass_(x, v, f, 0, 8.0, 0.0, 1e-30, 1e-30, 1e-30, prefilter=True)
    assert v1[10, 10] == F32(0.75 * 36 / 256) and v1[10, 12] == F32(0.75 * 6 / 256) and v1[8, 8] == F32(0.75 / 256)
    _, v2 = dv.pass_(x, v1, f, 1, 8.0, 0.0, 1e-30, 1e-30, 1e-30, prefilter=True)
    assert (v2[:, 20:] == 0).all() and (v2[5:16, 5:16] > 0).all()
