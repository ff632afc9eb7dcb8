"""The octahedral depth map without a GPU (include/hrt.h "Probe visibility"): hrt_probe_depth_direction and hrt_probe_depth_texel --
the shared header csrc/hrt_probe_depth_oct.h, as the kernels run it -- equal tests/probe_depth_ref.py bit for bit: on the 64 centres,
on texel edges and diagonals, on the six axes, on z = +-0 and on a few thousand random vectors of wildly different lengths; every
centre maps back to its own texel; and the NumPy statement itself holds the properties the rule promises."""
import numpy as np
import pytest

import probe_depth_ref as pd

F32, U32 = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def edge_vectors():
    """Vectors on texel edges and corners of the octahedral square, on both hemispheres, of several lengths."""
    g = (np.arange(9, dtype=F32) * F32(.25) - F32(1))
    px, py = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    z = (F32(1) - np.abs(px)) - np.abs(py)
    keep = z >= 0
    up = np.stack([px, py, z], axis=1)[keep]
    down = up * np.array([1, 1, -1], F32)
    return np.concatenate([up, down, up * F32(1e-20), down * F32(3e12), up * F32(7.3)]).astype(F32)


def special_vectors():
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    diagonals = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    planar = [(a, b, z) for a in (1, -1, .5, -.25) for b in (1, -1, .25, -.5) for z in (0.0, -0.0)]
    face = [(a, 0, b) for a in (1, -1) for b in (1, -1)] + [(0, a, b) for a in (1, -1) for b in (1, -1)]
    tiny = [(1e-42, 0, 0), (-1e-30, 1e-30, -0.0), (3e38, 3e38, 3e38), (1e-45, -1e-45, 1e-45)]
    return np.array(axes + diagonals + planar + face + tiny, F32)


def random_vectors(n=4000, seed=17):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-30, 31, (n, 1))).astype(F32)


def test_directions_equal_the_numpy_rule_bit_for_bit_and_map_back(hrt):
    want = pd.direction(np.arange(pd.TEXELS))
    assert np.allclose(np.linalg.norm(want.astype(np.float64), axis=1), 1, atol=2e-7)
    assert len({tuple(r) for r in bits(want).tolist()}) == 64, "64 different directions"
    for e in range(pd.TEXELS):
        d = hrt.probe_depth_direction(e)
        assert d.dtype == F32 and np.array_equal(bits(d), bits(want[e])), (e, d.tolist(), want[e].tolist())
        assert hrt.probe_depth_texel(d) == e == int(pd.texel(want[e])), e
        assert hrt.probe_depth_texel(d * F32(1e-12)) == e and hrt.probe_depth_texel(d * F32(5e20)) == e, "a vector need not be unit"
    # the diamond |px| + |py| = 1 passes through texel centres: 16 centres lie on the equator, 24 on either side
    assert ((want[:, 2] > 0).sum(), (want[:, 2] < 0).sum(), (want[:, 2] == 0).sum()) == (24, 24, 16)


@pytest.mark.parametrize("which", ["edges", "special", "random"])
def test_texels_equal_the_numpy_rule_bit_for_bit(hrt, which):
    v = {"edges": edge_vectors, "special": special_vectors, "random": random_vectors}[which]()
    want = pd.texel(v)
    assert want.dtype == U32 and (want < pd.TEXELS).all()
    got = np.array([hrt.probe_depth_texel(x) for x in v], U32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (which, bad[:5].tolist(), v[bad[:3]].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())
    if which == "random":
        assert len(set(want.tolist())) == 64, "every texel is reached"
        # a texel's vectors lie round its centre: within the 8 x 8 map's widest texel, whose half-diagonal is below 30 degrees
        c = pd.direction(want).astype(np.float64)
        u = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1)[:, None]
        assert ((c * u).sum(axis=1) > np.cos(np.radians(30))).all()


def test_the_fold_and_the_moments_of_the_numpy_rule():
    rng = np.random.default_rng(2)
    d = rng.standard_normal((130, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)
    r = rng.uniform(0.5, 4, 130).astype(F32)
    live = np.ones(130, bool)
    live[[3, 64, 129]] = False
    t = pd.fold(d, r, live)
    t64 = pd.fold(d, r, live, dtype=np.float64)
    assert t.dtype == F32 and t.shape == (64, 3) and np.allclose(t, t64, rtol=1e-5, atol=0)
    # blocks of 64: the total is the sum of the block values, each folded from 0
    parts = [pd.fold(d[a:b], r[a:b], live[a:b]) for a, b in ((0, 64), (64, 128), (128, 130))]
    assert np.array_equal(bits(t), bits((parts[0] + parts[1]) + parts[2]))
    assert not pd.fold(d, r, np.zeros(130, bool)).any(), "degenerate samples add nothing"
    m = pd.moments(t[None])[0]
    assert (m[:, 0] >= r.min() * (1 - 1e-6)).all() and (m[:, 0] <= r.max() * (1 + 1e-6)).all(), "a weighted mean of the depths"
    assert (m[:, 1] >= m[:, 0] * m[:, 0] * (1 - 1e-5)).all()
    empty = pd.moments(np.zeros((1, 64, 3), F32))[0]
    assert np.isposinf(empty[:, 0]).all() and not empty[:, 1].any()


def test_the_visibility_factor_of_the_numpy_rule():
    one, floor = F32(1), F32(.001)
    v = pd.visibility
    assert v(0.0, 0.5, 0.3) == one and v(2.0, np.inf, 0.0) == one and v(1.5, 1.5, 9.0) == one and v(0.2, 1.0, 1.0) == one
    assert v(2.0, 1.0, 1.0) == floor, "no variance: hidden"
    assert v(2.0, 1.0, 0.5) == floor, "m2 < m1^2: the variance is clamped to 0"
    c = F32(.5) / (F32(.5) + F32(1))  # var .5, q 1
    assert v(2.0, 1.0, 1.5) == (c * c) * c
    assert floor < v(1.1, 1.0, 1.5) < one
