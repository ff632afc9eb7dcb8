"""The NumPy statement of the baking rule (tests/bake_ref.py) on its own, without a GPU: every direction is a unit vector in the
hemisphere of its normal for the normals the frame has to get right, the directions follow the cosine law, the degenerate cases are
the header's -- and BAKE_TOL, the tolerance of tests/test_gpu_bake.py, is what its derivation says."""
import numpy as np
import pytest

import bake_ref

F32 = np.float32


def test_directions_are_unit_vectors_in_the_hemisphere_of_the_normal():
    pts = bake_ref.rule_points()
    for sample, seed in bake_ref.DRAWS + ((17, 7),):
        for keys in (None, bake_ref.keys_for(len(pts))):
            r, deg = bake_ref.rays(pts, sample, seed, keys)
            # (1e-20, 0, 0): its squared length, 1e-40, is a DENORMAL of fp32, not 0, so by the rule as the header states it the
            # normal normalises (to 1 within the denormal's 1e-5) and the point is traced; (1e-23, 0, 0) is the normal whose squared
            # length underflows to 0, and that point is degenerate
            assert F32(1e-20) * F32(1e-20) != 0 and F32(1e-23) * F32(1e-23) == 0
            assert deg.tolist() == [False] * 6 + [True] + [False] * (len(pts) - 7)
            d = r[~deg, 4:7].astype(np.float64)
            N = pts[~deg, 4:7].astype(np.float64)
            Nn = N / np.linalg.norm(N, axis=1)[:, None]
            assert np.abs((d * d).sum(1) - 1).max() <= 1e-5  # the bound query_margin needs
            assert ((d * Nn).sum(1) >= -bake_ref.BAKE_TOL).all()
            # the origin is the point pushed along the normal by the bias; time and tmax are carried
            O = pts[~deg, 0:3].astype(np.float64) + bake_ref.BIAS * Nn
            assert np.abs(r[~deg, 0:3] - O).max() <= 1e-6
            assert np.array_equal(r[:, 3], pts[:, 3]) and (r[:, 7] == np.inf).all()
    # the five named normals: +z gives the local sample itself up to the frame's signs, a non-unit normal is normalised first
    r, _ = bake_ref.rays(pts[:5], 0, 1)
    assert r[0, 6] > 0 and r[1, 6] < 0 and r[2, 4] > 0 and r[3, 5] > 0
    scaled = pts[4:5].copy()
    scaled[:, 4:7] = (0, 0.6, 0.8)
    assert np.abs(bake_ref.rays(scaled, 0, 1, np.array([4], np.uint32))[0][:, 4:7] - r[4:5, 4:7]).max() <= 1e-6


@pytest.mark.parametrize("seed,key,want", [(7, 0, 0.33), (2 ** 63 + 5, 12345, 1.34)])
def test_the_cosine_law(seed, key, want):
    """With the density cos(theta) / pi the mean of cos(theta) = d . Nn is 2/3 and its variance 1/2 - 4/9 = 1/18: over 4096 samples
    the standard error is sqrt(1/18) / 64."""
    n = 4096
    pt = bake_ref.records([[0.5, -1, 2]], [[1, 2, -2]])
    Nn = np.array([1, 2, -2], np.float64) / 3
    cos = np.array([bake_ref.rays(pt, s, seed, np.array([key], np.uint32))[0][0, 4:7].astype(np.float64) @ Nn for s in range(n)])
    se = np.sqrt(1 / 18) / 64
    off = abs(cos.mean() - 2 / 3) / se
    print(f"(seed, key) = ({seed}, {key}): mean cos {cos.mean():.6f}, {off:.2f} standard errors from 2/3")
    assert off <= 5
    assert abs(off - want) < 0.01  # the figure the issue records for the rule


def test_degenerate_points_and_records():
    pts = bake_ref.degenerate_records()
    assert bake_ref.point_degenerate(pts).tolist() == [True, True, False, True]  # N = (1e-20, 0, 0) normalises: see above
    more = bake_ref.edge_records()
    assert bake_ref.point_degenerate(more).tolist() == [True] * 6 + [False, False]
    allp = np.concatenate([pts, more])
    r, deg = bake_ref.rays(allp, 3, 9)
    assert deg.tolist() == [True, True, False, True] + [True] * 6 + [False, True]
    assert np.array_equal(r[deg, 0:4].view(np.uint32), allp[deg, 0:4].view(np.uint32))  # {P, time} bit for bit, NaNs included
    assert (r[deg, 4:7].view(np.uint32) == 0).all() and (r[:, 7] == np.inf).all()


def test_the_generators_state_the_headers_expressions():
    q = bake_ref.quad_points((-2, -2, 2), (2, -2, 2), (-2, -2, -2), 4, 2)
    assert q.shape == (8, 8) and np.array_equal(q[:, 4:7], np.tile(np.array([0, 1, 0], F32), (8, 1)))  # cross(+x, -z) = +y
    assert np.array_equal(q[:, 0], np.tile(np.array([-1.5, -0.5, 0.5, 1.5], F32), 2)) and (q[:, 1] == -2).all()
    assert np.array_equal(q[:, 2], np.repeat(np.array([1, -1], F32), 4))
    assert np.array_equal(bake_ref.quad_points((-2, -2, 2), (2, -2, 2), (-2, -2, -2), 4, 2, side=-1)[:, 4:7], -q[:, 4:7])
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9]], F32)
    m = bake_ref.mesh_points(pos, [[0, 1, 2], [0, 2, 3]], time=0.5)
    assert np.array_equal(m[:, 4:7], np.array([[1, 0, 1], [0, 0, 1], [1, 0, 1], [1, 0, 0], [0, 0, 0]], F32))
    assert np.array_equal(m[:, 0:3], pos) and (m[:, 3] == 0.5).all()
    assert bake_ref.point_degenerate(m).tolist() == [False, False, False, False, True]  # the unused vertex


def test_bake_tol_is_four_times_the_fp32_to_fp64_gap_of_the_gpu_tests_inputs(hrt, oracle):
    gap = 0.0
    for name in bake_ref.CONTRACT_SCENES:
        pts = bake_ref.contract_points(hrt, name)
        assert pts.shape == (bake_ref.W * bake_ref.H + 4, 8)
        assert (~bake_ref.point_degenerate(pts)).sum() >= 100, name  # the frame sees the scene
        g = bake_ref.fp_gap(pts, bake_ref.DRAWS, (None, bake_ref.keys_for(len(pts))))
        print(f"{name}: largest |fp32 - fp64| component difference {g:.6e}")
        gap = max(gap, g)
    print(f"largest gap {gap:.6e}; BAKE_GAP {bake_ref.BAKE_GAP:.6e}; BAKE_TOL {bake_ref.BAKE_TOL:.3e}")
    assert 0 < gap < 1e-4
    assert abs(bake_ref.BAKE_GAP / gap - 1) < 0.01 and bake_ref.BAKE_TOL == 4 * bake_ref.BAKE_GAP, (gap, bake_ref.BAKE_GAP)
