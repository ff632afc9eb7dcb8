"""THE RULE of baking (include/hrt.h "Baking") in NumPy, and the two host point generators.

`rays(points, sample, seed, keys)` gives the records hrt_bake_rays writes and the mask of degenerate samples, in fp32 in the order
the header writes (NumPy neither fuses nor reassociates); `dtype=np.float64` evaluates the same expressions, from the same fp32
draws, constants and point records, in double -- the yardstick BAKE_TOL below comes from.  The RNG stream is lens_ref.draws.
`quad_points` and `mesh_points` restate hrt_bake_quad_points and hrt_bake_mesh_points, fp32 in the order written."""
import numpy as np

import lens_ref
import oracle_lib

F32 = np.float32
U32 = np.uint32
TWO_PI = F32(6.2831855)

# Tolerance per ray component between the device's rays and rays() for the points and draws of tests/test_gpu_bake.py (the records
# of contract_points() for CONTRACT_SCENES x DRAWS below, without keys and with keys_for()): 4 x the largest difference, over every
# component of every non-degenerate ray of those inputs, between the rule evaluated in fp32 and in fp64 from the same draws
# (fp_gap(): 1.802769e-06, reached on an origin among the farthest hit points of random_spheres, 47 units from the world origin,
# where half an ulp of the coordinate is 1.9e-06; 1.05e-06 on cornell_mesh and backrooms_pool).  That gap is the rounding the
# rule itself allows an fp32 evaluation; the factor leaves room for what NumPy and the device do not share -- sinf and cosf, each
# within a few ulp of the true value on either side -- while sqrtf, copysignf and the divisions are exact or correctly rounded on
# both.  A CPU-side measurement: nothing of the code under test enters it.  tests/test_bake_ref.py holds the constant to the
# measurement.
BAKE_GAP = 1.802769e-06
BAKE_TOL = 4 * BAKE_GAP

CONTRACT_SCENES = ["cornell_mesh", "random_spheres", "backrooms_pool"]
W, H = 19, 11  # the frame whose pixel-centre rays give the contract points
BIAS = 1e-4
DRAWS = ((0, 1), (5, 2 ** 63 + 12345))  # (sample, seed)


def keys_for(n):
    """The key array of the tests: distinct, out of order, beyond 2^31."""
    return ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % (2 ** 32)).astype(U32)


# ----------------------------------------------------------------------------------------------------------------------- rule
def _normalize(a):
    L = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a / L[:, None]


def _finite(a):
    return np.isfinite(a).all(axis=1)


def _zero(a):
    return (a == 0).all(axis=1)


def point_degenerate(points, dtype=F32):
    """The mask of degenerate POINTS: a float that is not finite, bias < 0, N == 0, or a normalised N that is not finite or is 0."""
    p = np.asarray(points, F32)
    with np.errstate(all="ignore"):
        Nn = _normalize(p[:, 4:7].astype(dtype))
        return ~_finite(p) | (p[:, 7] < 0) | _zero(p[:, 4:7]) | ~_finite(Nn) | _zero(Nn)


def rays(points, sample, seed, keys=None, dtype=F32):
    """The records of hrt_bake_rays(points, keys, sample, seed) -- (n, 8) in `dtype` -- and the mask of degenerate samples."""
    T = dtype
    p = np.asarray(points, F32)
    n = len(p)
    k = np.arange(n) if keys is None else np.asarray(keys)
    b0 = lens_ref.draws(seed, k, sample, 0).astype(T)
    b1 = lens_ref.draws(seed, k, sample, 1).astype(T)
    P, N, bias = p[:, 0:3].astype(T), p[:, 4:7].astype(T), p[:, 7].astype(T)
    one = T(1)
    with np.errstate(all="ignore"):
        deg = point_degenerate(p, T)
        Nn = _normalize(N)
        r = np.sqrt(b0)
        phi = T(TWO_PI) * b1
        x, y, z = r * np.cos(phi), r * np.sin(phi), np.sqrt(one - b0)
        sg = np.copysign(one, Nn[:, 2])
        a = -one / (sg + Nn[:, 2])
        b = (Nn[:, 0] * Nn[:, 1]) * a
        Tv = np.stack([one + (sg * (Nn[:, 0] * Nn[:, 0])) * a, sg * b, (-sg) * Nn[:, 0]], axis=1)
        Bv = np.stack([b, sg + (Nn[:, 1] * Nn[:, 1]) * a, -Nn[:, 1]], axis=1)
        d = _normalize((x[:, None] * Tv + y[:, None] * Bv) + z[:, None] * Nn)
        O = P + bias[:, None] * Nn
        deg = deg | ~_finite(O) | ~_finite(d) | _zero(d)
    out = np.empty((n, 8), T)
    out[:, 0:3] = O
    out[:, 4:7] = d
    out[deg, 4:7] = 0
    out[:, 3], out[:, 7] = p[:, 3], np.inf
    if T is F32:  # the degenerate record keeps the bits of P and time, NaN payloads included
        out.view(U32)[deg, 0:4] = p.view(U32)[deg, 0:4]
    else:
        out[deg, 0:3] = P[deg]
    return out, deg


def fp_gap(points, draws=DRAWS, keys=(None,)):
    """Largest |fp32 - fp64| over every component of every non-degenerate ray of `points` x `draws` x `keys`."""
    gap = 0.0
    cols = [0, 1, 2, 4, 5, 6]
    for sample, seed in draws:
        for k in keys:
            r32, d32 = rays(points, sample, seed, k)
            r64, d64 = rays(points, sample, seed, k, np.float64)
            ok = ~(d32 | d64)
            gap = max(gap, float(np.abs(r32[ok][:, cols].astype(np.float64) - r64[ok][:, cols]).max()))
    return gap


# --------------------------------------------------------------------------------------------------------------------- points
def records(P, N, time=0.0, bias=BIAS):
    P, N = np.asarray(P, F32).reshape(-1, 3), np.asarray(N, F32).reshape(-1, 3)
    r = np.empty((len(P), 8), F32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = P, time, N, bias
    return r


def hit_points(ray_records, shade_records, bias=BIAS):
    """Bake points at the hits of SHADE records (hrt_trace_rays, mode SHADE) of `ray_records`: P = o + t * d in fp32, N the SHADE
    normal, time the ray's.  A miss has t = 0 and N = 0: the point is the ray's origin, and degenerate."""
    rr, sr = np.asarray(ray_records, F32), np.asarray(shade_records, F32)
    P = rr[:, 0:3] + sr[:, 0:1] * rr[:, 4:7]
    return records(P, sr[:, 4:7], rr[:, 3], bias)


def degenerate_records():
    """The four hand-made degenerate records every point set of the GPU tests ends with."""
    r = records([[np.nan, 1, 2], [0.5, 0.25, -1], [1, 2, 3], [0, 1, 0]], [[0, 1, 0], [0, 0, 0], [1e-20, 0, 0], [0, 0, 1]])
    r[3, 7] = -1.0
    return r


def edge_records():
    """Records at the edges of the degenerate rule, for the tests of the rule: a NaN time, an infinite normal, a normal whose
    squared length underflows to 0 (two ways), a zero normal spelt -0, one whose length overflows, a bias of -0 (NOT degenerate),
    and a bias that overflows the origin (the point is not degenerate, its samples are)."""
    r = records([[1, 2, 3]] * 7 + [[3e38, 0, 0]],
                [[0, 0, 1], [np.inf, 0, 0], [0, 1e-30, 1e-30], [1e-23, 0, 0], [0, 0, -0.0], [3e38, 3e38, 3e38], [0, 1, 0], [1, 0, 0]])
    r[0, 3] = np.nan
    r[6, 7] = -0.0
    r[7, 7] = 3e38
    return r


_contract = {}


def contract_points(hrt, name):
    """The 19 x 11 SHADE hit points of the default camera's pixel-centre rays on scene `name` -- P = o + t * d in fp32, N the hit's
    shading normal, bias 1e-4, time 0; a miss is the ray's origin with N = 0, a degenerate point -- plus degenerate_records().  The
    hits are the CPU oracle's (t and normal of its first-hit AOVs, which tests/test_gpu_rays.py holds hrt_trace_rays' SHADE records
    to), so the points exist without a GPU; tests/test_gpu_bake.py checks them against the device's own SHADE records."""
    if name not in _contract:
        host = hrt.HostScene().setup(name, W / H, 1)
        _contract[name] = frame_points(host.flatten(), hrt.default_camera(W / H))
    return _contract[name].copy()


def frame_points(desc, cam):
    """contract_points' construction for any flattened description and the camera of its W x H frame."""
    y, x = np.mgrid[0:H, 0:W]
    uv = np.stack([(x.ravel().astype(F32) + F32(0.5)) / F32(W), (y.ravel().astype(F32) + F32(0.5)) / F32(H)], axis=1)
    cr = oracle_lib.camera_rays(cam, uv)
    aov = oracle_lib.OracleScene(desc).aov(cam, W, H)
    shade = np.zeros((W * H, 16), F32)
    shade[:, 0] = aov["hit"].reshape(-1, 3)[:, 0]
    shade[:, 4:7] = aov["normal"].reshape(-1, 3)
    rays = np.empty((W * H, 8), F32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = cr[:, 0:3], 0.0, cr[:, 3:6], np.inf
    return np.concatenate([hit_points(rays, shade), degenerate_records()])


def rule_points():
    """The points of the CPU tests of the rule: the normals the frame has to get right, and a few hundred random ones."""
    rng = np.random.default_rng(11)
    N = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, -0.0), (0, 3, 4), (1e-20, 0, 0), (1e-23, 0, 0)]
    v = rng.normal(size=(300, 3)) * np.exp(rng.uniform(-3, 3, size=(300, 1)))
    N = np.concatenate([np.array(N, F32), v.astype(F32)])
    P = rng.uniform(-4, 4, size=(len(N), 3)).astype(F32)
    return records(P, N)


# ------------------------------------------------------------------------------------------------------------------ generators
def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)


def quad_points(v0, v1, v3, tw, th, side=1, time=0.0, bias=BIAS):
    """hrt_bake_quad_points: texel (i, j) at index j * tw + i."""
    v0, v1, v3 = (np.asarray(v, F32) for v in (v0, v1, v3))
    with np.errstate(all="ignore"):
        R, U = v1 - v0, v3 - v0
        c = _cross(R, U)
        n = c / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        N = F32(side) * n
        j, i = np.divmod(np.arange(tw * th), tw)
        fu = (i.astype(F32) + F32(0.5)) / F32(tw)
        fv = (j.astype(F32) + F32(0.5)) / F32(th)
        P = (v0[None] + fu[:, None] * R[None]) + fv[:, None] * U[None]
    return records(P, np.tile(N, (tw * th, 1)), time, bias)


def mesh_points(positions, indices, time=0.0, bias=BIAS):
    """hrt_bake_mesh_points: per vertex the sum of its triangles' cross products, in ascending triangle order."""
    p = np.asarray(positions, F32).reshape(-1, 3)
    N = np.zeros_like(p)
    with np.errstate(all="ignore"):
        for tri in np.asarray(indices, np.int64).reshape(-1, 3):
            c = _cross(p[tri[1]] - p[tri[0]], p[tri[2]] - p[tri[0]])
            for v in dict.fromkeys(int(t) for t in tri):  # once per triangle, whatever it names twice
                N[v] = N[v] + c
    return records(p, N, time, bias)
