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
