"""THE RULE of light probes (include/hrt.h "Light probes") in NumPy: the direction of a sample, the nine basis values, the
fixed-order sum, and the host grid generator.

`rays(probes, sample, seed, keys)` gives the records hrt_probe_rays writes and the mask of degenerate samples, in fp32 in the order
the header writes (NumPy neither fuses nor reassociates); `dtype=np.float64` evaluates the same expressions, from the same fp32
draws and constants, in double -- the yardstick PROBE_TOL below comes from.  `basis(d)` is Y0..Y8 of unit directions, `fold` the
sum over per-sample values in the header's order: lanes, halving, blocks.  The RNG stream is lens_ref.draws.  BLOCK is read from
the header."""
import os
import re

import numpy as np

import bake_ref
import lens_ref

F32 = np.float32
U32 = np.uint32
TWO_PI = F32(6.2831855)
COEFFS = 9

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hrt.h")
with open(_HEADER) as _f:
    BLOCK = int(re.search(r"#define HRT_PROBE_BLOCK (\d+)u", _f.read()).group(1))

# The nine constants of the basis, as the header writes them.
C0, C1, C2, C3, C4 = F32(0.2820948), F32(0.48860251), F32(1.0925485), F32(0.31539157), F32(0.54627422)

# Tolerance per direction component between the device's rays and rays() for the probes and draws of tests/test_gpu_probes.py
# (contract_probes() of CONTRACT_SCENES x DRAWS below, without keys and with bake_ref.keys_for()): 4 x the largest difference, over
# every component of every non-degenerate direction of those inputs, between the rule evaluated in fp32 and in fp64 from the same
# draws (fp_gap(): 2.444524e-07, the same on every scene -- the rule has no origin arithmetic, so unlike BAKE_GAP the
# size of the scene does not enter).  That gap is the rounding the rule itself allows an fp32 evaluation; the factor leaves room
# for what NumPy and the device do not share -- sinf and cosf, each within a few ulp of the true value on either side -- while
# sqrtf, fmaxf and the divisions are exact or correctly rounded on both.  A CPU-side measurement: nothing of the code under test
# enters it.  tests/test_probe_ref.py holds the constant to the measurement.
PROBE_GAP = 2.444524e-07
PROBE_TOL = 4 * PROBE_GAP

CONTRACT_SCENES = bake_ref.CONTRACT_SCENES
DRAWS = bake_ref.DRAWS  # (sample, seed)
# Per scene: the box of its 3 x 2 x 2 grid, and a point inside a closed object of the scene: the centre of the Cornell box's glass
# sphere and of random_spheres' fixed one, and for backrooms_pool a point inside the body of its flamingo mesh (mesh POOL_MESH of
# the flattened scene, in its upper part, 0.13 from the nearest vertex, where about one direction in seven sees light).  The mesh walk culls back faces, so from inside nothing of the mesh is seen;
# tests/test_probe_ref.py shows on the CPU that the point is inside all the same, by the oracle's hit parity: along every
# direction the mesh's front faces are crossed once more going out (seen from far away, looking back) than going in.
POOL_MESH = 0
BOXES = {"cornell_mesh": ((-1.6, -0.4, -1.2), (1.6, 1.6, 1.6), (1.0, -1.25, 0.5)),
         "random_spheres": ((-6.0, -3.0, -14.0), (6.0, 3.0, -4.0), (-1.0, -2.5, -8.0)),
         "backrooms_pool": ((-2.0, -1.0, -4.0), (2.0, 1.0, 0.0), (0.129, -1.327, -3.944))}


# ----------------------------------------------------------------------------------------------------------------------- rule
def directions(seed, keys, sample, dtype=F32):
    """d of sample `sample` for every key (samples broadcast against keys): (n, 3) in `dtype`."""
    T = dtype
    b0 = lens_ref.draws(seed, keys, sample, 0).astype(T)
    b1 = lens_ref.draws(seed, keys, sample, 1).astype(T)
    one, two = T(1), T(2)
    z = one - two * b0
    r = np.sqrt(np.maximum(T(0), one - z * z))
    phi = T(TWO_PI) * b1
    v = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    L = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v / L[:, None]


def probe_degenerate(probes):
    return ~np.isfinite(np.asarray(probes, F32)).all(axis=1)


def rays(probes, sample, seed, keys=None, dtype=F32):
    """The records of hrt_probe_rays(probes, keys, sample, seed) -- (n, 8) in `dtype` -- and the mask of degenerate samples."""
    p = np.asarray(probes, F32)
    n = len(p)
    k = np.arange(n) if keys is None else np.asarray(keys)
    with np.errstate(all="ignore"):
        d = directions(seed, k, sample, dtype)
        deg = probe_degenerate(p) | ~np.isfinite(d).all(axis=1) | (d == 0).all(axis=1)
    out = np.empty((n, 8), dtype)
    out[:, 0:4] = p
    out[:, 4:7] = d
    out[deg, 4:7] = 0
    out[:, 7] = np.inf
    if dtype is F32:  # the record keeps the bits of P and time, NaN payloads included
        out.view(U32)[:, 0:4] = p.view(U32)
    return out, deg


def basis(d):
    """Y0..Y8 of directions d (n, 3), fp32 in the header's order: (n, 9)."""
    d = np.asarray(d, F32)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full(len(d), C0, F32), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * (F32(3) * (z * z) - F32(1)),
                     C2 * (x * z), C4 * (x * x - y * y)], axis=1).astype(F32)


def fold(Y, v, deg, block=None):
    """The total t of the header's sum: Y (S, n, 9) basis values, v (S, n, 3) per-sample values, deg (S, n) degenerate samples, for
    local sample indices j = 0..S-1 -> (n, 9, 3) fp32.  Lane partials in ascending j, halving over 64 lanes, blocks ascending."""
    block = BLOCK if block is None else block
    Y, v, deg = np.asarray(Y, F32), np.asarray(v, F32), np.asarray(deg, bool)
    S, n = v.shape[0], v.shape[1]
    t = np.zeros((n, COEFFS, 3), F32)
    for b in range(0, S, block):
        a = np.zeros((64, n, COEFFS, 3), F32)
        for j in range(b, min(S, b + block)):
            lane = j % 64
            term = Y[j][:, :, None] * v[j][:, None, :]
            a[lane] = np.where(deg[j][:, None, None], a[lane], a[lane] + term)
        m = 32
        while m:
            a[:m] = a[:m] + a[m:2 * m]
            m //= 2
        t = t + a[0]
    return t


def fp_gap(probes, draws=DRAWS, keys=(None,)):
    """Largest |fp32 - fp64| over every direction component of every non-degenerate ray of `probes` x `draws` x `keys`."""
    gap = 0.0
    for sample, seed in draws:
        for k in keys:
            r32, d32 = rays(probes, sample, seed, k)
            r64, d64 = rays(probes, sample, seed, k, np.float64)
            ok = ~(d32 | d64)
            gap = max(gap, float(np.abs(r32[ok][:, 4:7].astype(np.float64) - r64[ok][:, 4:7]).max()))
    return gap


# --------------------------------------------------------------------------------------------------------------------- probes
def grid(lo, hi, nx, ny, nz, time=0.0):
    """hrt_probe_grid_points: probe (i, j, k) at index (k * ny + j) * nx + i."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    idx = np.arange(nx * ny * nz)
    cell = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1).astype(F32)
    count = np.array([nx, ny, nz], F32)
    out = np.empty((len(idx), 4), F32)
    with np.errstate(all="ignore"):
        out[:, 0:3] = lo[None] + ((cell + F32(0.5)) / count[None]) * (hi - lo)[None]
    out[:, 3] = time
    return out


def degenerate_records():
    """The two hand-made degenerate records every contract probe set ends with: a NaN position and an infinite time."""
    r = np.array([[np.nan, 1, 2, 0], [0.5, 0.25, -1, np.inf]], F32)
    return r


def contract_probes(name):
    """The 3 x 2 x 2 grid inside scene `name`, the probe inside its glass sphere or closed mesh (index INSIDE), and
    degenerate_records()."""
    lo, hi, inside = BOXES[name]
    return np.concatenate([grid(lo, hi, 3, 2, 2), np.array([list(inside) + [0.0]], F32), degenerate_records()])


INSIDE = 12  # index of the interior probe in contract_probes()


def mesh_winding(desc, mesh, point, dirs, reach=20.0):
    """Per direction, how many more front faces of `mesh` a ray from `point` crosses going out than going in, by the oracle's mesh
    walk (which culls back faces): the crossings going out are the front-face hits of the ray that comes back from `reach` away.
    1 in every direction for a point inside a closed, outward-facing mesh; 0 outside."""
    import oracle_lib

    def crossings(o, d):
        o, left, n, live = o.astype(np.float64), np.full(len(o), reach), np.zeros(len(o), int), np.ones(len(o), bool)
        for _ in range(64):
            if not live.any():
                break
            r = oracle_lib.mesh_query(desc, mesh, oracle_lib.MESH_REF_TREE, np.concatenate([o, d, np.zeros((len(o), 1))], 1).astype(F32))
            live = live & (r[:, 0] > 0) & (r[:, 1] < left)
            step = r[:, 1].astype(np.float64) + 1e-4  # past the face just counted
            n, o, left = n + live, np.where(live[:, None], o + step[:, None] * d, o), np.where(live, left - step, left)
        return n

    o = np.tile(np.asarray(point, np.float64), (len(dirs), 1))
    return crossings(o + reach * dirs, -dirs) - crossings(o, dirs)
