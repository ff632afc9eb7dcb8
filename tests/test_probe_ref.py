"""The NumPy statement of the light-probe rule (tests/probe_ref.py) without a GPU: the nine constants are the closed forms, the
directions are unit vectors and uniform on the sphere, the sum has the header's order, and PROBE_TOL is the measured rounding
allowance of the direction rule."""
import math

import numpy as np
import pytest

import bake_ref
import probe_ref

F32, U32 = np.float32, np.uint32
BLOCK = probe_ref.BLOCK


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def test_the_nine_constants_are_the_closed_forms_rounded_to_fp32():
    pi = math.pi
    assert probe_ref.C0 == F32(math.sqrt(1 / (4 * pi)))
    assert probe_ref.C1 == F32(math.sqrt(3 / (4 * pi)))
    assert probe_ref.C2 == F32(math.sqrt(15 / (4 * pi)))
    assert probe_ref.C3 == F32(math.sqrt(5 / (16 * pi)))
    assert probe_ref.C4 == F32(math.sqrt(15 / (16 * pi)))
    Y = probe_ref.basis(np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], F32))
    assert Y[0].tolist() == [probe_ref.C0, 0, probe_ref.C1, 0, 0, 0, probe_ref.C3 * F32(2), 0, 0]
    assert Y[1].tolist() == [probe_ref.C0, 0, 0, probe_ref.C1, 0, 0, -probe_ref.C3, 0, probe_ref.C4]
    assert Y[2].tolist() == [probe_ref.C0, probe_ref.C1, 0, 0, 0, 0, -probe_ref.C3, 0, -probe_ref.C4]


def test_the_block_is_the_headers_and_the_bindings(hrt):
    assert BLOCK == hrt.PROBE_BLOCK and BLOCK % 64 == 0
    assert (hrt.PROBE_FLOATS, hrt.PROBE_COEFFS) == (4, probe_ref.COEFFS)


def test_rays_are_unit_directions_and_keep_the_record():
    for name in probe_ref.CONTRACT_SCENES:
        p = probe_ref.contract_probes(name)
        assert probe_ref.probe_degenerate(p).tolist() == [False] * (len(p) - 2) + [True, True]
        for sample, seed in probe_ref.DRAWS:
            for keys in (None, bake_ref.keys_for(len(p))):
                r, deg = probe_ref.rays(p, sample, seed, keys)
                assert np.array_equal(deg, probe_ref.probe_degenerate(p))
                assert np.array_equal(bits(r[:, 0:4]), bits(p)) and np.isinf(r[:, 7]).all()
                d = r[~deg, 4:7].astype(np.float64)
                assert (np.abs((d * d).sum(axis=1) - 1) <= 1e-5).all()  # the project's bound for a unit direction
                assert (r[deg, 4:7] == 0).all()


@pytest.mark.parametrize("seed,key,numpy_off", [(7, 0, 1.18), (2 ** 63 + 5, 12345, 1.37)])
def test_the_directions_are_uniform_on_the_sphere(seed, key, numpy_off):
    """Over n = 4096 samples of one (seed, key) the means of x, y, z and of Y4..Y8 are within 5 standard errors of 0.  For a
    direction uniform on the sphere E[x] = E[y] = E[z] = 0 and E[x^2] = E[y^2] = E[z^2] = 1/3 (they are equal and sum to 1), so
    the standard error of a mean component is sqrt(1 / (3 n)) = 0.00902.  Y1..Y8 are orthonormal on the sphere: the integral of
    Y_k over it is 0 and that of Y_k^2 is 1, so under the uniform density 1 / (4 pi) E[Y_k] = 0 and E[Y_k^2] = 1 / (4 pi), and the
    standard error of a mean Y_k is sqrt(1 / (4 pi n)) = 0.00441 (for Y4 = c xy: E[x^2 y^2] = 1/15 and c^2 = 15 / (4 pi))."""
    n = 4096
    d = np.concatenate([probe_ref.directions(seed, np.array([key]), s) for s in range(n)])
    Y = probe_ref.basis(d).astype(np.float64)
    se_d, se_y = math.sqrt(1 / (3 * n)), math.sqrt(1 / (4 * math.pi * n))
    off = np.concatenate([np.abs(d.astype(np.float64).mean(axis=0)) / se_d, np.abs(Y[:, 4:9].mean(axis=0)) / se_y])
    print(f"(seed, key) = ({seed}, {key}): offsets of x, y, z, Y4..Y8 in standard errors {np.round(off, 3).tolist()}")
    assert (off <= 5).all() and abs(off.max() - numpy_off) < 0.01
    # and the band-1 values are the components: Y2 = c1 z has the mean c1 * mean(z)
    assert abs(Y[:, 2].mean() - float(probe_ref.C1) * d[:, 2].astype(np.float64).mean()) < 1e-6


def scalar_fold(y, v, block):
    """The header's sum for one (coefficient, channel) in plain Python on fp32 scalars."""
    t = F32(0)
    for b in range(0, len(v), block):
        lanes = [F32(0)] * 64
        for j in range(b, min(len(v), b + block)):
            lanes[j % 64] = F32(lanes[j % 64] + F32(y[j] * v[j]))
        m = 32
        while m:
            for l in range(m):
                lanes[l] = F32(lanes[l] + lanes[l + m])
            m //= 2
        t = F32(t + lanes[0])
    return t


@pytest.mark.parametrize("S", sorted({1, 63, 64, 65, BLOCK, BLOCK + 1, 2 * BLOCK + 1}))
def test_fold_has_the_headers_order(S):
    rng = np.random.default_rng(S)
    Y = (rng.normal(size=(S, 2, 9)) * np.exp(rng.uniform(-8, 8, size=(S, 2, 9)))).astype(F32)
    v = (rng.normal(size=(S, 2, 3)) * np.exp(rng.uniform(-8, 8, size=(S, 2, 3)))).astype(F32)
    deg = np.zeros((S, 2), bool)
    deg[:, 1] = rng.random(S) < 0.25  # the second item skips a quarter of its samples
    got = probe_ref.fold(Y, v, deg)
    assert got.shape == (2, 9, 3) and got.dtype == F32
    for k, c in ((0, 0), (4, 1), (8, 2)):
        assert bits(got[0, k, c]) == bits(scalar_fold(Y[:, 0, k], v[:, 0, c], BLOCK))
        keep = ~deg[:, 1]
        skipped = scalar_fold(np.where(keep, Y[:, 1, k], F32(0)), np.where(keep, v[:, 1, c], F32(0)), BLOCK)  # + 0.f changes nothing
        assert got[1, k, c] == skipped
    # integers add exactly in any order
    ones = probe_ref.fold(np.ones((S, 1, 9), F32), np.ones((S, 1, 3), F32), np.zeros((S, 1), bool))
    assert (ones == S).all()


def test_fold_by_hand_where_the_order_shows():
    """65 samples: 1e8 at j = 0 and -1e8 at j = 64 share lane 0 and cancel there; the 1 at j = 1 is lane 1's and survives the
    halving.  Added in sample order the 1 would be lost in 1e8 + 1."""
    v = np.zeros((65, 1, 3), F32)
    v[0], v[1], v[64] = 1e8, 1.0, -1e8
    Y = np.ones((65, 1, 9), F32)
    assert (probe_ref.fold(Y, v, np.zeros((65, 1), bool), block=256) == 1).all()
    assert F32(F32(F32(1e8) + F32(1)) + F32(-1e8)) == 0
    # a block boundary at 64 puts j = 64 into block 1: block 0 holds 1e8 + 1 = 1e8, the total is 0
    assert (probe_ref.fold(Y, v, np.zeros((65, 1), bool), block=64) == 0).all()
    # a lane with no samples holds 0, a lone sample comes through untouched, a degenerate one adds nothing
    one = probe_ref.fold(np.full((1, 1, 9), 0.5, F32), np.full((1, 1, 3), 3.0, F32), np.zeros((1, 1), bool))
    assert (one == 1.5).all()
    assert (bits(probe_ref.fold(np.ones((3, 1, 9), F32), np.ones((3, 1, 3), F32), np.ones((3, 1), bool))) == 0).all()


def test_probe_tol_is_four_times_the_measured_gap():
    gap = 0.0
    for name in probe_ref.CONTRACT_SCENES:
        p = probe_ref.contract_probes(name)
        g = probe_ref.fp_gap(p, keys=(None, bake_ref.keys_for(len(p))))
        print(f"{name}: largest fp32 - fp64 difference of a direction component {g:.6e}")
        gap = max(gap, g)
    assert abs(gap - probe_ref.PROBE_GAP) <= 1e-12 and probe_ref.PROBE_TOL == 4 * probe_ref.PROBE_GAP
    assert probe_ref.PROBE_TOL < 1e-5  # tighter than the project's own bound for a unit direction


def test_the_pools_interior_probe_is_inside_its_flamingo_by_the_oracles_hit_parity(hrt):
    """The contract probe of backrooms_pool that is to start inside a closed mesh does: in each of 256 directions the flamingo's
    front faces are crossed exactly once more going out than going in (the walk culls back faces, so the crossings going out are
    counted on the ray that comes back).  The same count is 0 for the grid probes, which are outside it, and 1 for points a little
    way from the probe in every direction, so the probe is not at a seam."""
    desc = hrt.HostScene().setup("backrooms_pool", 19 / 11, 1).flatten()
    rng = np.random.default_rng(2)
    dirs = rng.normal(size=(256, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    probes = probe_ref.contract_probes("backrooms_pool")
    inside = probes[probe_ref.INSIDE, 0:3].astype(np.float64)
    assert inside.tolist() == [float(F32(x)) for x in probe_ref.BOXES["backrooms_pool"][2]]
    w = probe_ref.mesh_winding(desc, probe_ref.POOL_MESH, inside, dirs)
    assert (w == 1).all(), np.unique(w, return_counts=True)
    for k in range(6):
        near = inside + 0.05 * dirs[k]
        assert (probe_ref.mesh_winding(desc, probe_ref.POOL_MESH, near, dirs[:64]) == 1).all(), k
    for k in (0, 5, 11):
        assert (probe_ref.mesh_winding(desc, probe_ref.POOL_MESH, probes[k, 0:3].astype(np.float64), dirs[:64]) == 0).all(), k


def test_the_grid_is_the_cell_centres():
    g = probe_ref.grid((0, 0, 0), (4, 2, 2), 4, 2, 1, time=0.25)
    assert g.shape == (8, 4) and g[:, 3].tolist() == [0.25] * 8
    assert g[:, 0].tolist() == [0.5, 1.5, 2.5, 3.5] * 2 and g[:, 1].tolist() == [0.5] * 4 + [1.5] * 4 and g[:, 2].tolist() == [1.0] * 8
    assert probe_ref.grid((1, 2, 3), (3, 2, -1), 1, 1, 1)[0].tolist() == [2.0, 2.0, 1.0, 0.0]
