"""The NumPy rule of lit rays (tests/probe_lit_ref.py, include/hrt.h "Lit rays") on hand-made cases: no GPU, no library."""
import numpy as np
import pytest

import probe_lit_ref as pl
import probe_volume_ref as pv

F32, U32 = np.float32, np.uint32
BOX, COUNTS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (2, 2, 2)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def constant_volume(L):
    """Coefficients of a constant environment of value L per channel: a probe stores the means of Y_k x value, so band 0 alone,
    c00 = Y0 * L."""
    c = np.zeros((8, 9, 3), F32)
    c[:, 0, :] = F32(0.2820948) * np.asarray(L, F32)
    return c


def test_a_constant_volume_gives_albedo_times_its_value_on_top_of_the_head():
    """A constant environment of value L evaluates to L (the header's UNITS), whatever the point and the normal; the value of a
    diffuse hit is then head + albedo * L."""
    L = np.array([0.5, 0.25, 2.0], F32)
    o = np.array([[0, 0, 0], [0.3, -0.2, 0.9], [5, 5, 5]], F32)
    d = np.array([[0, 0, 1], [1, 0, 0], [0, -1, 0]], F32)
    t = np.array([0.5, 0.25, 3.0], F32)
    n = np.array([[0, 0, -1], [-1, 0, 0], [0, 1, 0]], F32)
    pts = pl.point_records(o, d, t, n, 0.0, 1e-3)
    assert np.array_equal(pts[:, 0:3], np.array([[0, 0, 0.5], [0.55, -0.2, 0.9], [5, 2, 5]], F32)) and (pts[:, 7] == F32(1e-3)).all()
    for flags in (0, pl.FACING):
        G = pl.gather(*BOX, COUNTS, constant_volume(L), None, pts, flags)
        assert np.allclose(G, L[None, :], rtol=2e-6), flags
        head, albedo = np.array([[1, 2, 3]] * 3, F32), np.array([[0.5, 0.5, 0.5], [1, 0, 0.25], [0, 0, 0]], F32)
        v = pl.sample_value(head, albedo, [True, True, True], G)
        assert np.array_equal(bits(v), bits(head + albedo * G))
        assert np.array_equal(v[2], head[2]), "a black surface takes nothing from the volume"


def test_mirror_glass_and_misses_get_no_tail_and_a_degenerate_record_gathers_zero():
    head, albedo = np.array([[1, 2, 3]] * 4, F32), np.full((4, 3), 0.75, F32)
    G = np.full((4, 3), 9.0, F32)
    v = pl.sample_value(head, albedo, [True, False, False, True], G)
    assert np.array_equal(v[1], head[1]) and np.array_equal(v[2], head[2]) and np.array_equal(v[0], head[0] + F32(0.75) * F32(9))
    pts = pl.point_records(np.zeros((3, 3), F32), np.array([[0, 0, 1]] * 3, F32), np.array([1, np.inf, 1], F32),
                           np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0]], F32), 0.0, 0.0)
    G = pl.gather(*BOX, COUNTS, constant_volume([1, 1, 1]), None, pts, 0)
    assert G[0].all() and not G[1].any() and not G[2].any()


def test_the_gather_refuses_what_the_header_refuses():
    pts = pl.point_records(np.zeros((1, 3)), np.array([[0, 0, 1]]), np.array([1.0]), np.array([[0, 0, 1]]), 0.0, 0.0)
    for flags in (pl.RADIANCE, 8, pl.RADIANCE | pl.FACING):
        with pytest.raises(AssertionError):
            pl.gather(*BOX, COUNTS, constant_volume([1, 1, 1]), None, pts, flags)


def test_samples_add_in_ascending_order_and_divide_once():
    v = np.array([[[1e8, 1, 0]], [[1, 1, 0]], [[-1e8, 1, 3]]], F32)
    mean = pl.ray_output(v)
    assert np.array_equal(mean, (((F32(0) + v[0]) + v[1]) + v[2]) / F32(3)) and mean[0, 0] == 0, "1e8 + 1 rounds to 1e8 first"
    base = np.array([[1, 2, 3]], F32)
    assert np.array_equal(pl.ray_output(v, base=base), ((base + v[0]) + v[1]) + v[2])
    assert np.array_equal(bits(pl.ray_output(v[:1])), bits(v[0])), "one sample: 0 + value, / 1"


def test_blend_is_the_hysteresis_expression_and_keep_zero_is_the_update():
    rng = np.random.default_rng(1)
    p, c = rng.standard_normal((8, 9, 3)).astype(F32), rng.standard_normal((8, 9, 3)).astype(F32)
    k = F32(0.7)
    assert np.array_equal(bits(pl.blend(p, c, 0.7)), bits((k * p) + ((F32(1) - k) * c)))
    assert np.array_equal(bits(pl.blend(p, c, 0.0)), bits(c))
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(AssertionError):
            pl.blend(p, c, bad)


def test_the_furnace_series():
    assert pl.furnace(6.0, 0.5, 1) == 1.0 and pl.furnace(6.0, 0.5, 2) == 1.5
    assert abs(pl.furnace(6.0, 0.5, 8) - 2 * (1 - 0.5 ** 8)) < 1e-12 and pl.furnace(6.0, 0.5, 8) > 1.9
    # relighting a constant room by the rule itself: coefficients c00 = Y0 * value, value_{r+1} = e / 6 + rho * G(value_r)
    value = F32(0)
    pts = pl.point_records(np.zeros((1, 3), F32), np.array([[0, 0, 1]], F32), np.array([1.0], F32), np.array([[0, 0, -1]], F32), 0.0, 0.0)
    for r in range(1, 9):
        G = pl.gather(*BOX, COUNTS, constant_volume([value] * 3), None, pts, 0)
        value = pl.sample_value(np.full((1, 3), 1.0, F32), np.full((1, 3), 0.5, F32), [True], G)[0, 0]
        assert abs(float(value) - pl.furnace(6.0, 0.5, r)) < 1e-5 * r, r
