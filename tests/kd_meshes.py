"""Seeded synthetic meshes for the KD build tests (tests/test_kd_ref.py, tests/test_gpu_kdbuild_edges.py): each family aims at a
place where a level-by-level device build can part from the host's recursion.  Every function returns (positions (nv, 3) fp32,
indices (nt, 3) uint32); the host layer scales positions by HRT_TRIANGLE_SCALING before building."""
import numpy as np

f32 = np.float32


def _tris(centers, size, rng):
    """One small random triangle around each center."""
    c = np.asarray(centers, f32)
    off = rng.uniform(-1, 1, size=(len(c), 3, 3)).astype(f32) * f32(size)
    p = (c[:, None, :] + off).reshape(-1, 3).astype(f32)
    return p, np.arange(len(p), dtype=np.uint32).reshape(-1, 3)


def soup(n, seed, size=0.05, scale=1.0, offset=0.0):
    """n small triangles uniformly in [-1, 1]^3 (times scale, plus offset)."""
    rng = np.random.default_rng(seed)
    p, i = _tris(rng.uniform(-1, 1, size=(n, 3)), size, rng)
    return (p * f32(scale) + f32(offset)).astype(f32), i


def clustered(n, seed):
    """n triangles in a few clusters of different sizes (the random soups of the fuzz tool)."""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(1, 6))
    centers = rng.uniform(-1, 1, size=(k, 3))
    spread = rng.uniform(0.02, 0.6, size=k)
    which = rng.integers(0, k, size=n)
    c = centers[which] + rng.normal(size=(n, 3)) * spread[which, None]
    p, i = _tris(c, float(rng.uniform(0.005, 0.05)), rng)
    return p, i


def lattice(nx, ny, nz, size=0.25):
    """Identical triangles on an integer lattice (centered on the origin): equal-cost planes in many places."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(f32)
    g -= f32([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2])
    t = np.array([[0, 0, 0], [size, 0, 0], [0, size, size]], f32)
    p = (g[:, None, :] + t[None]).reshape(-1, 3).astype(f32)
    return p, np.arange(len(p), dtype=np.uint32).reshape(-1, 3)


def cube_symmetric(n, seed):
    """n random triangles, each with its 6 coordinate permutations and their mirror images: x, y and z price the same."""
    rng = np.random.default_rng(seed)
    c = np.round(rng.uniform(-3.5, 3.5, size=(n, 1, 3)) * 8) / 8
    base = c + np.round(rng.uniform(-0.5, 0.5, size=(n, 3, 3)) * 8) / 8  # dyadic: exact sums
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    tris = [base[:, :, list(q)] * s for q in perms for s in (1, -1)]
    p = np.concatenate(tris).reshape(-1, 3).astype(f32)
    return p, np.arange(len(p), dtype=np.uint32).reshape(-1, 3)


def shared_planes(k, seed):
    """Slabs of triangles whose upper bounds are the next slab's lower bounds, mirrored about x = 0: a low candidate and a high
    one of equal cost at different positions."""
    rng = np.random.default_rng(seed)
    tris = []
    for s in range(-k, k):
        for _ in range(3):
            y, z = rng.uniform(-1, 1, 2)
            tris.append([[s, y, z], [s + 1, y + 0.1, z], [s + 0.5, y, z + 0.1]])
    t = np.array(tris, f32)
    t = np.concatenate([t, t * f32([-1, 1, 1])])
    p = t.reshape(-1, 3).astype(f32)
    return p, np.arange(len(p), dtype=np.uint32).reshape(-1, 3)


def signed_zero(n, seed, negative_first):
    """Triangles on both sides of the planes x = 0, y = 0 and z = 0 with vertices ON them written as -0.0 and +0.0, in an order
    that puts one sign first."""
    rng = np.random.default_rng(seed)
    tris = []
    for k in range(n):
        a = k % 3
        side = 1 if k % 2 else -1
        t = rng.uniform(0.05, 1.0, size=(3, 3)) * side
        t[:, (a + 1) % 3] *= rng.choice([-1, 1])
        t[0, a] = 0.0
        t[1, a] = 0.0
        zero_sign = (k // 2) % 2 == 0
        if negative_first:
            zero_sign = not zero_sign
        t[0, a] = -0.0 if zero_sign else 0.0
        t[1, a] = 0.0 if zero_sign else -0.0
        tris.append(t)
    p = np.array(tris, f32).reshape(-1, 3)
    return p, np.arange(len(p), dtype=np.uint32).reshape(-1, 3)


def planar(n, seed):
    """n triangles in the plane z = 0: one axis without extent."""
    p, i = soup(n, seed, size=0.1)
    p[:, 2] = 0.0
    return p, i


def long_thin(n_small, n_long, seed):
    """Small triangles plus long thin ones across the whole mesh on every axis: straddling references make a level's reference
    count grow before it shrinks."""
    rng = np.random.default_rng(seed)
    p, i = soup(n_small, seed, size=0.03)
    longs = []
    for k in range(n_long):
        a = k % 3
        c = rng.uniform(-1, 1, 3)
        t = np.array([c, c, c], f32)
        t[0, a], t[1, a], t[2, a] = -1.0, 1.0, 0.0
        t[2, (a + 1) % 3] += 0.01
        longs.append(t)
    q = np.concatenate([p, np.array(longs, f32).reshape(-1, 3)])
    return q.astype(f32), np.arange(len(q), dtype=np.uint32).reshape(-1, 3)


def random_case(seed):
    """One of the fuzz tool's random soups with random build limits and cost constants: (positions, indices, leaf_max, max_depth,
    {env var: value})."""
    rng = np.random.default_rng(seed + 777)
    n = int(rng.choice([3, 17, 64, 255, 300, 513, 700]))
    p, i = clustered(n, seed) if rng.random() < 0.6 else soup(n, seed, size=float(rng.uniform(0.01, 0.1)))
    leaf_max = int(rng.choice([1, 2, 4, 9, 64]))
    max_depth = int(rng.choice([0, 0, 1, 3, 12, 40]))
    env = {}
    if rng.random() < 0.5:
        env["HRT_KD_CT"] = str(rng.choice([0.0, 0.5, 1.0, 2.0]))
    if rng.random() < 0.5:
        env["HRT_KD_CI"] = str(rng.choice([0.5, 1.5, 3.0, 0.01]))
    if rng.random() < 0.5:
        env["HRT_KD_EB"] = str(rng.choice([0.0, 0.3, 0.8, 1.0]))
    return p, i, leaf_max, max_depth, env
