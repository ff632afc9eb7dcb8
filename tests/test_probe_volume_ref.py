"""The rule of probe volumes (tests/probe_volume_ref.py, the NumPy statement of include/hrt.h "Probe volumes") against closed
forms worked out in fp64: units, the band factors, trilinear reproduction of linear fields, clamping, the facing weights, and the
literals the header and the kernel write.  No GPU and no library: what is held here is the rule itself; tests/test_probe_volume_abi.py
and tests/test_gpu_probe_volume.py hold the code to the rule bit for bit.

Tolerances.  EPS = 2^-24 is the unit roundoff of fp32.  An output is a sum of nine terms (F_k a_k) Y_k; a_k is a sum of eight
products w_m p_m, the weights are products of three factors (seven more operations each with `facing`).  A first-order bound on the
rounding of one output is therefore (8 + 8 + 3 + 10 + 4 + 9) EPS = 42 EPS times the sum of the magnitudes of the terms; the tests
below use 64 EPS times that sum (`bound`), which also covers the five basis literals and three factors being rounded to fp32
(half an ulp each).  Where the issue states a bound -- 2 ulp for a constant environment, 4 ulp for the weight sum -- that bound is
used as stated."""
import os
import re

import numpy as np
import pytest

import probe_ref
import probe_volume_ref as pv

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
Y0 = np.sqrt(1 / (4 * np.pi))
C1 = np.sqrt(3 / (4 * np.pi))
BOX = ((-1.7, 0.3, 2.1), (2.9, 1.1, 7.6))
COUNTS = (3, 2, 4)
N_PROBES = 24


def records(P, N):
    P, N = np.atleast_2d(np.asarray(P, F32)), np.atleast_2d(np.asarray(N, F32))
    pts = np.zeros((len(P), 8), F32)
    pts[:, 0:3], pts[:, 4:7] = P, N
    return pts


def hull(box, counts):
    lo, hi, n = np.asarray(box[0], F64), np.asarray(box[1], F64), np.asarray(counts, F64)
    return lo + (0.5 / n) * (hi - lo), hi - (0.5 / n) * (hi - lo)


def inside(rng, k, box=BOX, counts=COUNTS):
    a, b = hull(box, counts)
    return (a + rng.random((k, 3)) * (b - a)).astype(F32)


def unit(rng, k):
    v = rng.standard_normal((k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ulps(got, want):
    want = np.asarray(want, F32)
    return np.abs(np.asarray(got, F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)


# ------------------------------------------------------------------------------------------------------------------- literals
def test_the_band_factors_are_the_closed_forms_rounded_to_fp32():
    want = (F32(4 * np.pi), F32(8 * np.pi / 3), F32(np.pi))
    assert pv.header_band_literals() == want and (pv.F_BAND0, pv.F_BAND1, pv.F_BAND2) == want
    assert "12.566371f for every k" in pv.header_text()
    with open(os.path.join(os.path.dirname(pv._HEADER), "..", "hai719-raytracing_amd", "csrc", "hrt_probe_volume.hip")) as f:
        src = f.read()
    m = re.search(r"const float F0 = ([0-9.]+)f, F1 = radiance \? ([0-9.]+)f : ([0-9.]+)f, F2 = radiance \? ([0-9.]+)f : ([0-9.]+)f;", src)
    assert tuple(F32(x) for x in m.groups()) == (want[0], want[0], want[1], want[0], want[2])
    assert pv.F_BAND0 == F32(4) * pv.F_BAND2  # so a band-2 environment is scaled by exactly 1/4


def test_the_basis_constants_are_the_closed_forms_rounded_to_fp32():
    closed = {"Y0": np.sqrt(1 / (4 * np.pi)), "Y1": np.sqrt(3 / (4 * np.pi)), "Y4": np.sqrt(15 / (4 * np.pi)), "Y6": np.sqrt(5 / (16 * np.pi)),
              "Y8": np.sqrt(15 / (16 * np.pi))}
    text = pv.header_text()
    for name, ref_const in (("Y0", probe_ref.C0), ("Y1", probe_ref.C1), ("Y4", probe_ref.C2), ("Y6", probe_ref.C3), ("Y8", probe_ref.C4)):
        lit = re.search(r"\b" + name + r" = ([0-9.]+)f", text).group(1)
        assert F32(lit) == F32(closed[name]) == ref_const, (name, lit)
    with open(os.path.join(os.path.dirname(pv._HEADER), "..", "hai719-raytracing_amd", "csrc", "hrt_probe_volume.hip")) as f:
        body = re.search(r"void pv_basis\(.*?\n}", f.read(), re.S).group(0)
    assert sorted({F32(x) for x in re.findall(r"([0-9]\.[0-9]{5,})f", body)}) == sorted(F32(v) for v in closed.values())


# ---------------------------------------------------------------------------------------------------------------------- units
@pytest.mark.parametrize("radiance", [False, True])
@pytest.mark.parametrize("facing", [False, True])
def test_a_constant_environment_gives_its_value(radiance, facing):
    """c_0 = Y0 L and nothing else: L within 2 ulp.  The weights must be exact for that bound -- a single probe, probe centres of a
    grid whose arithmetic is exact, and cell midpoints -- and at arbitrary points the (rounded) weights add what `bound` allows."""
    rng = np.random.default_rng(1)
    L = np.array([0.7, 1.0, 123.456], F32)
    one = np.zeros((1, 9, 3), F32)
    one[0, 0] = F32(Y0) * L
    pts = records(rng.standard_normal((50, 3)) * 5, unit(rng, 50))
    got = pv.evaluate(*BOX, (1, 1, 1), one, pts, radiance, facing)
    u = ulps(got, np.broadcast_to(L, got.shape))
    print(f"1 x 1 x 1, radiance {radiance}, facing {facing}: {u.max():.2f} ulp")
    assert u.max() <= 2
    many = np.zeros((N_PROBES, 9, 3), F32)
    many[:, 0] = F32(Y0) * L
    box = ((0, 0, 0), (3, 2, 4))  # centres at halves, cells of size 1: every weight below is a dyadic fraction
    P = np.array([[0.5, 0.5, 0.5], [2.5, 1.5, 3.5], [1.0, 1.0, 2.0], [1.25, 0.75, 3.0], [-4, 9, 2.5]], F32)
    if not facing:
        got = pv.evaluate(*box, COUNTS, many, records(P, unit(rng, len(P))), radiance, facing)
        u = ulps(got, np.broadcast_to(L, got.shape))
        print(f"3 x 2 x 4 at dyadic points, radiance {radiance}: {u.max():.2f} ulp")
        assert u.max() <= 2
    pts = records(inside(rng, 200), unit(rng, 200))
    got = pv.evaluate(*BOX, COUNTS, many, pts, radiance, facing).astype(F64)
    assert (np.abs(got - L.astype(F64)) <= 64 * EPS * L.astype(F64)).all()


@pytest.mark.parametrize("facing", [False, True])
def test_a_linear_environment(facing):
    """L(w) = 1 + a . w has c_0 = Y0 and band 1 = C1 (a_y, a_z, a_x) / 3: irradiance / pi = 1 + (2/3) a . N, radiance 1 + a . N."""
    rng = np.random.default_rng(2)
    a = np.array([0.3, -0.5, 0.2])
    c = np.zeros((N_PROBES, 9, 3), F32)
    c[:, 0, :] = Y0
    c[:, 1, :], c[:, 2, :], c[:, 3, :] = C1 * a[1] / 3, C1 * a[2] / 3, C1 * a[0] / 3
    N = unit(rng, 300)
    pts = records(inside(rng, 300), N * rng.uniform(0.01, 50, (300, 1)))  # the length of the normal does not matter
    Nn = pts[:, 4:7].astype(F64) / np.linalg.norm(pts[:, 4:7].astype(F64), axis=1, keepdims=True)
    bound = 64 * EPS * (1 + np.abs(a).sum())
    for radiance, scale in ((False, 2 / 3), (True, 1.0)):
        got = pv.evaluate(*BOX, COUNTS, c, pts, radiance, facing).astype(F64)
        want = 1 + scale * (Nn @ a)
        err = np.abs(got - want[:, None]).max()
        print(f"linear environment, radiance {radiance}, facing {facing}: max error {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def test_band_two_is_scaled_by_a_quarter():
    """L = Y6: c_6 = 1 / 4 pi.  Radiance mode gives Y6(N); the clamped-cosine convolution scales band 2 by (pi / 4) / pi."""
    rng = np.random.default_rng(3)
    c = np.zeros((N_PROBES, 9, 3), F32)
    c[:, 6, :] = 1 / (4 * np.pi)
    pts = records(inside(rng, 100), unit(rng, 100))
    rad = pv.evaluate(*BOX, COUNTS, c, pts, radiance=True)
    irr = pv.evaluate(*BOX, COUNTS, c, pts, radiance=False)
    assert np.array_equal(irr, rad * F32(0.25)) and rad.any()  # 4 pi and pi differ by a power of two: exact
    z = pts[:, 6].astype(F64) / np.linalg.norm(pts[:, 4:7].astype(F64), axis=1)
    want = np.sqrt(5 / (16 * np.pi)) * (3 * z * z - 1)
    assert np.abs(rad.astype(F64) - want[:, None]).max() <= 64 * EPS * np.sqrt(5 / (16 * np.pi)) * 4


# ------------------------------------------------------------------------------------------------------------- interpolation
def test_a_field_linear_in_space_is_reproduced_inside_the_hull_and_clamped_outside():
    rng = np.random.default_rng(4)
    for box, counts in ((BOX, COUNTS), (((-1.0, 2.0, 0.0), (1.0, -0.5, 3.0)), (2, 2, 2)), (BOX, (4, 1, 1))):
        n = int(np.prod(counts))
        ijk = np.stack(np.meshgrid(*[np.arange(k) for k in counts], indexing="ij"), -1).reshape(-1, 3)
        index = (ijk[:, 2] * counts[1] + ijk[:, 1]) * counts[0] + ijk[:, 0]
        centre = pv.centres(*box, counts, ijk).astype(F64)
        A, b = rng.standard_normal((3, 3)), rng.standard_normal(3)  # channel ch holds A[ch] . P + b[ch]
        for a in range(3):
            if counts[a] == 1:
                A[:, a] = 0  # one probe on an axis: the field cannot vary along it
        c = np.zeros((n, 9, 3), F32)
        c[index, 0, :] = (centre @ A.T + b) * Y0  # radiance mode then gives the field itself: 4 pi Y0 Y0 = 1
        P = inside(rng, 200, box, counts)
        got = pv.evaluate(*box, counts, c, records(P, unit(rng, 200)), radiance=True).astype(F64)
        want = P.astype(F64) @ A.T + b
        size = (np.abs(centre) @ np.abs(A.T)).max() + np.abs(b).max()
        # the position enters through g = (P - lo) s - .5, whose rounding moves the point by a few EPS of the box: 64 EPS of the field's size covers both
        assert np.abs(got - want).max() <= 64 * EPS * size, (counts, np.abs(got - want).max())
        # outside: the value at the point clamped to the hull of the centres
        lo_h, hi_h = hull(box, counts)
        lo_h, hi_h = np.minimum(lo_h, hi_h), np.maximum(lo_h, hi_h)
        Q = (P.astype(F64) + rng.choice([-1, 0, 1], (200, 3)) * 10 * np.abs(np.asarray(box[1], F64) - np.asarray(box[0], F64))).astype(F32)
        N = unit(rng, 200)
        out = pv.evaluate(*box, counts, c, records(Q, N), radiance=True).astype(F64)
        clamped = np.clip(Q.astype(F64), lo_h, hi_h)
        assert np.abs(out - (clamped @ A.T + b)).max() <= 64 * EPS * size
        same = pv.evaluate(*box, counts, c, records(clamped.astype(F32), N), radiance=True).astype(F64)
        assert np.abs(out - same).max() <= 64 * EPS * size


# -------------------------------------------------------------------------------------------------------------------- facing
def test_facing_weights_sum_to_one_and_prefer_the_probes_in_front():
    rng = np.random.default_rng(5)
    pts = records(np.concatenate([inside(rng, 300), inside(rng, 100) * 3]), unit(rng, 400))
    _, w, _, deg = pv.weights(*BOX, COUNTS, pts, facing=True)
    assert not deg.any() and (w >= 0).all()
    total = w.astype(F64).sum(axis=1)
    print(f"facing weights: |sum - 1| <= {np.abs(total - 1).max() / 2.0 ** -23:.2f} ulp")
    assert np.abs(total - 1).max() <= 4 * 2.0 ** -23
    # two probes at x = .5 and 1.5, the point half way, the normal towards the second: (c + 1) / 2 is 0 behind and 1 in front
    index, w, _, _ = pv.weights((0, 0, 0), (2, 1, 1), (2, 1, 1), records([1.0, 0.5, 0.5], [1, 0, 0]), facing=True)
    assert index[0, :2].tolist() == [0, 1] and not w[0, 2:].any()
    assert abs(w[0, 0] / w[0, 1] - 0.2 / 1.2) <= 4 * EPS and abs(float(w[0, 0]) + float(w[0, 1]) - 1) <= 2 * EPS
    plain = pv.weights((0, 0, 0), (2, 1, 1), (2, 1, 1), records([1.0, 0.5, 0.5], [1, 0, 0]), facing=False)[1]
    assert plain[0, :2].tolist() == [0.5, 0.5]
    # a point exactly at a probe: l == 0 there, c = 0, and that probe keeps all the weight
    _, w, _, _ = pv.weights((0, 0, 0), (2, 1, 1), (2, 1, 1), records([0.5, 0.5, 0.5], [0, 1, 0]), facing=True)
    assert w[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_degenerate_points_give_zeros():
    c = np.ones((N_PROBES, 9, 3), F32)
    pts = records([[0, 0.5, 3]] * 5, [[0, 0, 1]] * 5)
    pts[0, 1] = np.nan
    pts[1, 4:7] = 0
    pts[2, 5] = np.inf
    pts[3, 4:7] = (1e-30, 0, 0)
    for radiance in (False, True):
        for facing in (False, True):
            got = pv.evaluate(*BOX, COUNTS, c, pts, radiance, facing)
            assert not got[:4].any() and got[4].all() and np.isfinite(got).all()
