"""The division by a known divisor ON THE DEVICE (csrc/hrt_div.h as the shipped streaming builds compile it), through three
hrt_debug_kat kinds: div_known, normalize_shared and the reciprocal form of quad_t, each with its IEEE 1.f / c taken on the
device, as stream_body's staging takes it.  References: numpy's float32 division (IEEE) and the existing device kinds
(KAT_NORMALIZE, KAT_QUAD), which tests/test_gpu_kat.py pins to the reference's own vectors.  Every comparison is on the bits.

The guard edges here are also the ONLY place where the fallback branch of div_known runs on the device: no ray of a frame has a
component outside [2^-60, 2^61), so the frame tests (tests/test_gpu_div_forms.py, tests/test_gpu_exact.py) never reach it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 1 << 20
EDGE = np.array([0.0, 1e-45, 1.1754942e-38, 2.0 ** -126, 2.0 ** -61, np.nextafter(F32(2.0 ** -60), F32(0)), 2.0 ** -60, 1.0, 3.0, 2.0 ** 60,
                 np.nextafter(F32(2.0 ** 61), F32(0)), 2.0 ** 61, 3.4028235e38, np.inf, np.nan], F32)
EDGE = np.concatenate([EDGE, -EDGE])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def in_window(rng, n):
    """Floats of either sign with a uniformly drawn exponent inside the window and a random significand."""
    bits = (rng.integers(67, 188, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))
    return bits.view(F32)


def test_div_known_on_the_device_is_the_division(gpu):
    rng = np.random.default_rng(11)
    a, c = in_window(rng, N), in_window(rng, N)
    ea, ec = np.meshgrid(EDGE, EDGE, indexing="ij")               # every pair of edge values, then edges against ordinary values
    k = ea.size
    a[:k], c[:k] = ea.ravel(), ec.ravel()
    a[k:k + EDGE.size], c[2 * k:2 * k + EDGE.size] = EDGE, EDGE
    a[3 * k:3 * k + 4096] = rng.integers(0, 1 << 32, 4096, dtype=np.uint32).view(F32)   # arbitrary bit patterns
    c[4 * k:4 * k + 4096] = rng.integers(0, 1 << 32, 4096, dtype=np.uint32).view(F32)
    c[5 * k:5 * k + 64] = np.ldexp(F32(np.uint32(0x3FFFFFFF).view(F32)), rng.integers(-59, 60, 64)).astype(F32)  # all-ones significands
    got = gpu.debug_kat(gpu.KAT_DIV_KNOWN, np.stack([a, c], -1))[:, 0]
    with np.errstate(all="ignore"):
        want = a / c
    ok = same_bits(got, want)
    assert ok.all(), f"{(~ok).sum()} of {N} quotients differ, first (a, c, got, want): {[(a[i], c[i], got[i], want[i]) for i in np.flatnonzero(~ok)[:5]]}"
    fast = (np.abs(c) >= 2.0 ** -60) & (np.abs(c) < 2.0 ** 61) & (((np.abs(a) >= 2.0 ** -60) & (np.abs(a) < 2.0 ** 61)) | (a == 0))
    assert fast.sum() > N // 2 and (~fast).sum() > 2000           # both sides of the guard


def test_normalize_shared_on_the_device_is_the_three_divisions(gpu):
    rng = np.random.default_rng(12)
    q = N // 4
    cube = (-1 + 2 * (rng.integers(0, 1 << 24, (q, 3)).astype(F32) * F32(2.0 ** -24))).astype(F32)   # Rng::unit_vector's components
    unit = gpu.debug_kat(gpu.KAT_NORMALIZE, cube)
    zero = cube.copy()
    zero[np.arange(q), rng.integers(0, 3, q)] = np.where(rng.integers(0, 2, q) == 0, F32(0.0), F32(-0.0))
    wild = rng.integers(0, 1 << 32, (q, 3), dtype=np.uint32).view(F32).copy()
    wild[:EDGE.size, 0] = EDGE
    wild[EDGE.size:2 * EDGE.size] = np.stack([EDGE, np.ones_like(EDGE), np.zeros_like(EDGE)], -1)
    v = np.concatenate([cube, unit, zero, wild])
    got = gpu.debug_kat(gpu.KAT_NORMALIZE_SHARED, v)
    plain = gpu.debug_kat(gpu.KAT_NORMALIZE, v)                    # Vec3.h:46 with three IEEE divisions, pinned by tests/test_gpu_kat.py
    ok = same_bits(got, plain).all(axis=1)
    assert ok.all(), f"{(~ok).sum()} of {len(v)} vectors differ from the three divisions, first {v[np.flatnonzero(~ok)[:5]].tolist()}"
    with np.errstate(all="ignore"):                                # and against numpy float32, one rounding per operation in Vec3.h's order
        L = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        want = v / L[:, None]
    ok = same_bits(got, want).all(axis=1)
    assert ok.all(), f"{(~ok).sum()} of {len(v)} vectors differ from numpy"


SIDE_ONES = float(np.nextafter(F32(2), F32(0)))                    # a side length whose significand is all ones
QUADS = {  # v0, v1, v3, motion, glass
    "all_ones_sides": ((0, 0, 0), (SIDE_ONES, 0, 0), (0, SIDE_ONES, 0), (0, 0, 0), 0),
    "sides_1e-3": ((0, 0, 0), (1e-3, 0, 0), (0, 1e-3, 0), (0, 0, 0), 0),
    "sides_1e3": ((-500, -500, 0), (500, -500, 0), (-500, 500, 0), (0, 0, 0), 0),
    "moving_tilted": ((-1, -0.5, 0.2), (0.7, -0.2, 0.9), (-1.3, 1.1, 0.4), (0.0, 0.3, 0.1), 0),
    "glass_tilted": ((-1, -0.5, 0.2), (0.7, -0.2, 0.9), (-1.3, 1.1, 0.4), (0, 0, 0), 1),
}


@pytest.mark.parametrize("name", list(QUADS))
def test_quad_t_with_reciprocals_is_quad_t(gpu, name):
    v0, v1, v3, motion, glass = QUADS[name]
    v0, v1, v3 = (np.array(x, np.float64) for x in (v0, v1, v3))
    if name == "all_ones_sides":
        r = F32(v1[0]) - F32(v0[0])
        assert np.sqrt(r * r) == F32(SIDE_ONES) and (F32(SIDE_ONES).view(np.uint32) & np.uint32(0x7FFFFF)) == 0x7FFFFF
    prim = np.array([*v0, *v1, *v3, *motion, glass], F32)
    rng = np.random.default_rng(13)
    size = max(np.linalg.norm(v1 - v0), np.linalg.norm(v3 - v0))
    uv = rng.uniform(-0.25, 1.25, (N, 2))                          # aimed at the square's plane: most inside, some on and past the edges
    uv[:4096] = rng.integers(0, 2, (4096, 2))                      # ... the corners and edges themselves
    uv[4096:8192, 0] = rng.integers(0, 2, 4096)
    target = v0 + uv[:, :1] * (v1 - v0) + uv[:, 1:] * (v3 - v0)
    origin = target + rng.normal(size=(N, 3)) * size * 3.0
    rays = np.concatenate([origin, target - origin, rng.uniform(0, 1, (N, 1))], axis=1).astype(F32)
    rays[8192:8192 + 1024, 3:6] = rng.normal(size=(1024, 3)).astype(F32)   # arbitrary directions: misses
    got = gpu.debug_kat(gpu.KAT_QUAD_RCP, rays, prim=prim)
    want = gpu.debug_kat(gpu.KAT_QUAD, rays, prim=prim)
    assert 0.2 * N < want[:, 0].sum() < N                           # hits and misses both
    ok = same_bits(got, want).all(axis=1)
    assert ok.all(), f"{name}: {(~ok).sum()} of {N} rays differ, first {np.flatnonzero(~ok)[:5].tolist()}"
