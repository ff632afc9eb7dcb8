"""Properties of the numpy statement of the denoiser (tests/denoise_ref.py, include/hrt.h hrt_denoise).  No GPU."""
import math

import numpy as np
import pytest

import denoise_ref as dr

F32 = np.float32
INF = math.inf


def noisy(h, w, seed, base=0.5, spread=0.3):
    return (base + np.random.default_rng(seed).uniform(-spread, spread, (h, w, 3))).astype(F32)


def scalar_denoise(c, f, iterations, sc, sn, sa, sz):
    """The header's rule once more, one pixel and one tap at a time in Python floats rounded to fp32 after every operation."""
    h, w, _ = c.shape
    r = lambda v: float(F32(v))
    d = [[[r(f[y, x, k]) if f[y, x, k] > 0 else 1.0 for k in range(3)] for x in range(w)] for y in range(h)]
    X = [[[r(r(c[y, x, k] - r(f[y, x, 6 + k] / 6.0)) / d[y][x][k]) for k in range(3)] for x in range(w)] for y in range(h)]
    hw = [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16]
    sq = lambda a, b: r(r(r(a[0] * a[0]) + r(a[1] * a[1])) + r(a[2] * a[2])) if b is None else None
    T = lambda num, den: 0.0 if (num == 0 or den == INF) else (INF if den == 0 else r(num / den))
    for i in range(iterations):
        s = 1 << i
        sci = r(r(sc) * 2.0 ** -i)
        Y = [[None] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                xp = X[y][x]
                sw, sx = 0.0, [0.0, 0.0, 0.0]
                for k in range(-2, 3):
                    for j in range(-2, 3):
                        qy, qx = y + k * s, x + j * s
                        if not (0 <= qy < h and 0 <= qx < w):
                            continue
                        hh = r(hw[j + 2] * hw[k + 2])
                        if j == 0 and k == 0:
                            wq, xq = hh, xp
                        else:
                            xq = X[qy][qx]
                            dx = [r(xp[m] - xq[m]) for m in range(3)]
                            dn = [r(f[y, x, 3 + m] - f[qy, qx, 3 + m]) for m in range(3)]
                            da = [r(f[y, x, m] - f[qy, qx, m]) for m in range(3)]
                            dz = r(f[y, x, 9] - f[qy, qx, 9])
                            zs = r(r(sz) * max(f[y, x, 9], f[qy, qx, 9], 1e-3))
                            e = r(r(r(T(sq(dx, None), r(sci * sci)) + T(sq(dn, None), r(r(sn) * r(sn)))) + T(sq(da, None), r(r(sa) * r(sa))))
                                  + T(r(dz * dz), r(zs * zs)))
                            wq = r(hh * math.exp(-e))
                        sw = r(sw + wq)
                        sx = [r(sx[m] + r(wq * xq[m])) for m in range(3)]
                Y[y][x] = [r(sx[m] / sw) for m in range(3)]
        X = Y
    return np.array([[[r(r(d[y][x][k] * X[y][x][k]) + r(f[y, x, 6 + k] / 6.0)) for k in range(3)] for x in range(w)] for y in range(h)], F32)


def test_vectorised_statement_matches_the_scalar_one():
    f = dr.synthetic_features(9, 11, seed=3)
    c = noisy(9, 11, 4)
    c[f[..., 6] > 0] = 5.0 / 6.0
    got = dr.denoise(c, f, iterations=3, sigma_color=0.4, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1)
    ref = scalar_denoise(c, f, 3, 0.4, 0.3, 0.2, 0.1)
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("iterations", [1, 3, 8])
def test_constant_colour_over_constant_features_is_a_fixed_point(iterations):
    h, w = 20, 23
    f = np.zeros((h, w, 12), F32)
    f[..., 0:3] = (0.5, 0.25, 0.8)
    f[..., 3:6] = (0, 1, 0)
    f[..., 9] = 4.0
    c = np.broadcast_to(np.array([0.3, 0.1, 0.7], F32), (h, w, 3)).copy()
    out = dr.denoise(c, f, iterations=iterations)
    np.testing.assert_allclose(out, c, rtol=1e-6)


def test_a_vanishing_colour_sigma_returns_the_input():
    """sigma_color = 1e-30: (sigma 2^-i)^2 underflows to 0, every off-centre tap with another colour gets weight exactly 0."""
    f = dr.synthetic_features(17, 19, seed=1)
    c = noisy(17, 19, 2)
    out = dr.denoise(c, f, iterations=4, sigma_color=1e-30)
    np.testing.assert_allclose(out, c, rtol=2e-7, atol=1e-7)


@pytest.mark.parametrize("guide", ["normal", "albedo", "depth"])
def test_a_step_in_a_guide_is_not_crossed(guide):
    """Left and right halves differ in one guide only (colour term off): each side's output stays within its own side's values
    and keeps its own side's mean."""
    h, w = 24, 32
    f = np.zeros((h, w, 12), F32)
    f[..., 0:3] = 0.5
    f[..., 3:6] = (0, 0, 1)
    f[..., 9] = 3.0
    left = np.zeros((h, w), bool)
    left[:, : w // 2] = True
    params = dict(iterations=5, sigma_color=INF, sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)
    if guide == "normal":
        f[~left, 3:6] = (1, 0, 0)
        params["sigma_normal"] = 0.1
    elif guide == "albedo":
        f[~left, 0:3] = 0.9
        params["sigma_albedo"] = 0.05
    else:
        f[~left, 9] = 9.0
        params["sigma_depth"] = 0.05
    c = noisy(h, w, 5, base=0.4, spread=0.2)
    c[~left] += F32(1.0)
    out = dr.denoise(c, f, **params)
    for side in (left, ~left):
        lo, hi = c[side].min(axis=0), c[side].max(axis=0)
        assert (out[side] >= lo - 1e-6).all() and (out[side] <= hi + 1e-6).all()
        np.testing.assert_allclose(out[side].mean(axis=0), c[side].mean(axis=0), rtol=0.02)
    # and the filter does smooth within a side
    assert out[left].std() < 0.5 * c[left].std()


def test_a_non_finite_pixel_passes_through_and_its_neighbours_ignore_it():
    f = dr.synthetic_features(16, 18, seed=2)
    c = noisy(16, 18, 3)
    bad = c.copy()
    bad[5, 7] = (np.nan, 0.5, 0.5)
    bad[10, 3] = (np.inf, np.inf, np.inf)
    out = dr.denoise(bad, f, iterations=3)
    assert np.isnan(out[5, 7, 0]) and (out[5, 7, 1:] == 0.5).all()
    assert np.isinf(out[10, 3]).all()
    # a neighbour gives a pixel of colour 1e30 weight exactly 0 (the squared difference overflows): same neighbours' result
    huge = c.copy()
    huge[5, 7] = 1e30
    huge[10, 3] = 1e30
    ref = dr.denoise(huge, f, iterations=3)
    keep = np.ones((16, 18), bool)
    keep[5, 7] = keep[10, 3] = False
    assert np.isfinite(out[keep]).all()
    np.testing.assert_array_equal(out[keep], ref[keep])
    # a pixel with a non-finite guide passes through too
    f2 = f.copy()
    f2[2, 2, 3] = np.nan
    out2 = dr.denoise(c, f2, iterations=2)
    np.testing.assert_array_equal(out2[2, 2], c[2, 2])


@pytest.mark.parametrize("axis", [0, 1])
def test_the_result_is_symmetric_under_flipping_the_image(axis):
    f = dr.synthetic_features(21, 26, seed=4)
    c = noisy(21, 26, 6)
    out = dr.denoise(c, f, iterations=4, sigma_color=0.5)
    flipped = dr.denoise(np.flip(c, axis), np.flip(f, axis), iterations=4, sigma_color=0.5)
    np.testing.assert_allclose(np.flip(flipped, axis), out, rtol=2e-6, atol=1e-7)


def test_gamma_is_applied_after_remodulation():
    f = dr.synthetic_features(8, 9, seed=5)
    c = noisy(8, 9, 7)
    lin = dr.denoise(c, f, iterations=2)
    g = dr.denoise(c, f, iterations=2, gamma=True)
    np.testing.assert_array_equal(g, np.power(lin.astype(np.float64), 1 / 2.2).astype(F32))


def test_finite_input_gives_finite_output_at_extremes():
    f = dr.synthetic_features(12, 12, seed=6)
    c = noisy(12, 12, 8)
    c[::3, ::2] = F32(3e38)
    c[1::4, 1::3] = F32(-3e38)
    out = dr.denoise(c, f, iterations=3, sigma_color=INF)
    assert np.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------- exact regime
def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


@pytest.mark.parametrize("h,w,iterations", [(13, 15, 3), (1, 9, 2), (9, 1, 2), (6, 6, 1), (11, 8, 4), (5, 17, 3)])
def test_the_exact_regime_equals_the_scalar_statement_bit_for_bit(h, w, iterations):
    c, f = dr.hard_edge_frame(h, w, seed=h + w, block=(3, 4))
    got = dr.denoise(c, f, iterations=iterations, **dr.EXACT)
    ref = scalar_denoise(c, f, iterations, INF, dr.EXACT["sigma_normal"], dr.EXACT["sigma_albedo"], dr.EXACT["sigma_depth"])
    assert same_bits(got, ref)


def test_the_exact_regime_has_only_spline_weights_or_zero():
    """Every weight is h_j h_k or 0 and at least one off-centre tap is kept and one is dropped: the frame exercises both."""
    c, f = dr.hard_edge_frame(20, 24, seed=2, block=(3, 4))
    x, _ = dr.demodulate(c, f)
    seen = set()
    real_exp = np.exp

    def spy(v):
        seen.update(np.unique(v).tolist())
        return real_exp(v)
    dr.iterate(x, f, 0, **dr.EXACT, exp=spy)
    assert seen == {0.0, -INF}


def test_coordinate_patterns_are_the_same_bits_in_torch_and_numpy():
    torch = pytest.importorskip("torch")
    ys, xs = np.mgrid[0:37, 0:53].astype(np.int64)
    ys[0, :3], xs[0, :3] = (134217726, 0, 7), (0, 134217726, 99999)
    for seed in (0, 5):
        c, f = dr.coord_frame(ys, xs, seed)
        tc, tf = dr.coord_frame(torch.from_numpy(ys), torch.from_numpy(xs), seed)
        assert same_bits(c, tc.numpy()) and same_bits(f, tf.numpy())
    assert len(np.unique(f[..., 9])) > 4 and (c >= 0).all() and np.isfinite(c).all()


# ---------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("params", [dict(dr.EXACT), dict(sigma_color=0.6, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1),
                                    dict(sigma_color=INF, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1)],
                         ids=["exact", "colour-on", "colour-off"])
def test_the_statement_on_a_window_with_its_margin_equals_the_full_frame(params):
    h, w, iterations = 40, 300, 4
    c, f = dr.hard_edge_frame(h, w, seed=7)
    c = (c + noisy(h, w, 3, base=0.0, spread=0.2)).astype(F32)
    full = dr.denoise(c, f, iterations=iterations, **params)
    get = lambda y0, y1, x0, x1: (c[y0:y1, x0:x1], f[y0:y1, x0:x1])
    for y0, y1, x0, x1 in ((0, 5, 0, 7), (35, 40, 293, 300), (10, 30, 100, 160), (0, 40, 140, 141), (17, 18, 0, 300), (0, 40, 0, 300)):
        win = dr.denoise_window(get, h, w, y0, y1, x0, x1, iterations, **params)
        assert same_bits(win, full[y0:y1, x0:x1]), (y0, y1, x0, x1)


def test_a_window_of_a_coordinate_frame_equals_the_whole_frame():
    h, w, iterations = 70, 33, 5
    c, f = dr.hard_edge_frame(h, w, seed=3)
    full = dr.denoise(c, f, iterations=iterations, **dr.EXACT)
    win = dr.denoise_window(lambda y0, y1, x0, x1: dr.coord_window(y0, y1, x0, x1, 3), h, w, 30, 40, 0, 33, iterations, **dr.EXACT)
    assert same_bits(win, full[30:40])


# ---------------------------------------------------------------------------------------------------------------- expf bound
def perturbed_exp(ulps, seed):
    """exp with each value moved by up to `ulps` fp32 ulp (rounding included) in a random direction."""
    rng = np.random.default_rng(seed)

    def f(v):
        e = np.exp(v.astype(np.float64))
        step = np.spacing(e.astype(F32)).astype(np.float64)
        moved = e + rng.uniform(-1, 1, e.shape) * (ulps - 0.5) * step
        return moved.astype(F32)
    return f


def bound_case(h, w, seed):
    f = dr.synthetic_features(h, w, seed=seed)
    f[..., 3:6] += np.random.default_rng(seed).normal(0, 0.05, (h, w, 3)).astype(F32)  # guides that give every E a value
    c = noisy(h, w, seed + 1, base=0.5, spread=0.5)
    return c, f


@pytest.mark.parametrize("iterations,sc", [(1, 0.6), (1, 0.05), (1, INF), (3, INF), (8, INF)])
def test_the_expf_bound_holds_for_exponentials_within_its_ulps(iterations, sc):
    h, w = 24, 37
    c, f = bound_case(h, w, iterations)
    params = dict(sigma_color=sc, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1)
    ref = dr.denoise(c, f, iterations=iterations, **params)
    bound = dr.expf_bound(c, f, iterations, **params)
    assert np.isfinite(bound).all()
    worst = 0.0
    for seed in range(3):
        got = dr.denoise(c, f, iterations=iterations, exp=perturbed_exp(dr.EXP_ULP, seed), **params)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), f"{int((err > bound).sum())} values beyond the bound"
        worst = max(worst, float((err / bound).max()))
    if sc != 0.05:  # (at 0.05 the colour term leaves only weights of 0 and the centre)
        assert worst > 0.002, "the perturbation should use a visible part of the bound"
    # a worst-case bound, but not a vacuous one
    assert bound.max() <= 1e-4 * iterations * np.abs(ref).max()


def test_the_expf_bound_is_exceeded_by_an_exponential_off_by_a_thousandth():
    h, w = 24, 37
    c, f = bound_case(h, w, 9)
    params = dict(sigma_color=INF, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1)
    ref = dr.denoise(c, f, iterations=2, **params)
    bound = dr.expf_bound(c, f, 2, **params)
    got = dr.denoise(c, f, iterations=2, exp=lambda v: (np.exp(v.astype(np.float64)) * (1 + 2.0 ** -10)).astype(F32), **params)
    assert (np.abs(got.astype(np.float64) - ref) > bound).any()


def test_the_expf_bound_refuses_the_colour_term_over_several_iterations():
    c, f = bound_case(8, 8, 1)
    with pytest.raises(ValueError):
        dr.expf_bound(c, f, 2, 0.5, 0.3, 0.2, 0.1)


# ---------------------------------------------------------------------------------------------------------------- oracle features
@pytest.mark.parametrize("name,w,h", [("cornell_mesh", 24, 14), ("backrooms_pool", 17, 11), ("random_spheres", 20, 12)])
def test_oracle_features_follow_the_aov_and_the_paths(hrt, oracle, name, w, h):
    host = hrt.HostScene().setup(name, w / h, 1)
    desc = host.flatten()
    cam = hrt.default_camera(w / h)
    o = oracle.OracleScene(desc)
    f = o.features(cam, w, h, 0, 0, 1)
    aov = {k: (np.zeros_like(v) + v).astype(F32) for k, v in o.aov(cam, w, h).items()}  # sums start from +0: -0 becomes +0
    assert same_bits(f[..., 0:3], aov["albedo"]) and same_bits(f[..., 3:6], aov["normal"]) and same_bits(f[..., 6:9], aov["emission"])
    assert same_bits(f[..., 9], aov["hit"][..., 0]) and same_bits(f[..., 10], (aov["hit"][..., 1] != 0).astype(F32))
    assert (f[..., 11] == 0).all()
    seed, first = (7 << 32) | 5, 11
    one = o.features(cam, w, h, first, 1, seed)
    for y in range(h):
        for x in range(w):
            row = oracle.trace_path(o, cam, w, h, x, y, first, seed, cap=1)[0]
            assert one[y, x, 9] == row[9] and one[y, x, 10] == float(row[7] != 0), (x, y)
    # n samples: the ordered fp32 sum of the one-sample features divided by n; a pixel list gives the same rows
    acc = np.zeros((h, w, 12), F32)
    for s in range(3):
        acc = (acc + o.features(cam, w, h, first + s, 1, seed)).astype(F32)
    three = o.features(cam, w, h, first, 3, seed)
    assert same_bits(three, (acc / F32(3)).astype(F32))
    pick = np.array([w * h - 1, 0, 5, w * h // 2], np.uint32)
    assert same_bits(o.features(cam, w, h, first, 3, seed, pick), three.reshape(-1, 12)[pick])
