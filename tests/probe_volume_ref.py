"""THE RULE of probe volumes (include/hrt.h "Probe volumes") in NumPy: the cell of a point (`cell`), the eight probes and their
final weights (`weights`), and the evaluation (`evaluate`).

Everything is fp32 in the order the header writes (NumPy neither fuses nor reassociates), over whole batches of point records
(n, 8) = {P, time, N, bias}.  fminf and fmaxf drop a NaN operand, so they are np.fmin and np.fmax here, not np.minimum and
np.maximum.  The basis is probe_ref.basis: the constants and expressions of "Light probes".  `dtype=np.float64` in `evaluate`
evaluates the same expressions in double, the yardstick of tests/test_probe_volume_ref.py."""
import os
import re

import numpy as np

import probe_ref

F32, U32 = np.float32, np.uint32
RADIANCE, FACING = 1, 2
COEFFS = probe_ref.COEFFS
# F per band, as the header writes them
F_BAND0, F_BAND1, F_BAND2 = F32(12.566371), F32(8.3775804), F32(3.1415927)

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hrt.h")


def header_text():
    with open(_HEADER) as f:
        return f.read()


def header_band_literals():
    """The three F literals of step 6 as the header's rule writes them: (4 pi, 8 pi / 3, pi) as fp32."""
    m = re.search(r"irradiance \(default\):\s+([0-9.]+)f \(4 pi\) for k = 0, ([0-9.]+)f \(8 pi / 3\) for k = 1\.\.3, ([0-9.]+)f \(pi\) for k = 4\.\.8", header_text())
    return tuple(F32(x) for x in m.groups())


def factors(radiance, T=F32):
    return np.array([F_BAND0] + [F_BAND0 if radiance else F_BAND1] * 3 + [F_BAND0 if radiance else F_BAND2] * 5, F32).astype(T)


def _grid(lo, hi, counts):
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    n = np.asarray(counts, np.int64)
    assert lo.shape == (3,) and hi.shape == (3,) and n.shape == (3,) and (n >= 1).all()
    with np.errstate(all="ignore"):
        e = hi - lo
        s = np.where(n > 1, n.astype(F32) / np.where(n > 1, e, F32(1)), F32(0)).astype(F32)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(s).all() and not ((n > 1) & (e == 0)).any(), "create refuses this grid"
    return lo, hi, n, s


def normals(points):
    """(Nn (n, 3) fp32, degenerate (n,) bool) of point records."""
    pts = np.asarray(points, F32).reshape(-1, 8)
    P, N = pts[:, 0:3], pts[:, 4:7]
    with np.errstate(all="ignore"):
        L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        Nn = (N / L[:, None]).astype(F32)
    deg = ~np.isfinite(P).all(axis=1) | ~np.isfinite(N).all(axis=1) | (N == 0).all(axis=1) | ~np.isfinite(Nn).all(axis=1)
    return Nn, deg


def cell(lo, hi, counts, points):
    """Step 1: (i0, i1 (n, 3) uint32, f (n, 3) fp32)."""
    lo, hi, n, s = _grid(lo, hi, counts)
    P = np.asarray(points, F32).reshape(-1, 8)[:, 0:3]
    top = (n - 1).astype(F32)
    with np.errstate(all="ignore"):
        g = np.fmin(np.fmax((P - lo[None, :]) * s[None, :] - F32(.5), F32(0)), top[None, :]).astype(F32)
    g = np.where(n[None, :] > 1, g, F32(0)).astype(F32)
    i0 = np.floor(g).astype(U32)
    f = (g - i0.astype(F32)).astype(F32)
    i1 = np.minimum(i0.astype(np.int64) + 1, (n - 1)[None, :]).astype(U32)
    return i0, i1, f


def centres(lo, hi, counts, c):
    """The grid formula for probe coordinates c (..., 3)."""
    lo, hi, n, _ = _grid(lo, hi, counts)
    return (lo + ((c.astype(F32) + F32(.5)) / n.astype(F32)) * (hi - lo)).astype(F32)


def weights(lo, hi, counts, points, facing=False):
    """Steps 1-3: (index (n, 8) uint32, weight (n, 8) fp32, Nn (n, 3), degenerate (n,)); index and weight are zero for a
    degenerate point."""
    lo, hi, n, _ = _grid(lo, hi, counts)
    pts = np.asarray(points, F32).reshape(-1, 8)
    P = pts[:, 0:3]
    Nn, deg = normals(pts)
    i0, i1, f = cell(lo, hi, n, pts)
    index = np.zeros((len(pts), 8), U32)
    w = np.zeros((len(pts), 8), F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for m in range(8):
            side = [(m >> a) & 1 for a in range(3)]
            c = np.stack([i1[:, a] if side[a] else i0[:, a] for a in range(3)], axis=1)
            wa = [f[:, a] if side[a] else one - f[:, a] for a in range(3)]
            index[:, m] = ((c[:, 2].astype(np.int64) * n[1] + c[:, 1]) * n[0] + c[:, 0]).astype(U32)
            wm = (wa[0] * wa[1]) * wa[2]
            if facing:
                v = centres(lo, hi, n, c) - P
                l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
                dot = (v[:, 0] * Nn[:, 0] + v[:, 1] * Nn[:, 1]) + v[:, 2] * Nn[:, 2]
                cs = np.where(l > 0, dot / np.where(l > 0, l, one), F32(0)).astype(F32)
                t = (cs + one) * F32(.5)
                wm = wm * (t * t + F32(.2))
            w[:, m] = wm
        if facing:
            W = w[:, 0]
            for m in range(1, 8):
                W = W + w[:, m]
            w = (w / W[:, None]).astype(F32)
    index[deg] = 0
    w[deg] = 0
    return index, w, Nn, deg


def evaluate(lo, hi, counts, coeffs, points, radiance=False, facing=False, dtype=F32):
    """Steps 1-6: (n, 3) in `dtype`.  coeffs: (nx*ny*nz, 9, 3).  With dtype=np.float64 steps 4-6 run in double from the fp32 weights,
    normals and constants."""
    T = dtype
    coeffs = np.asarray(coeffs, F32).reshape(-1, 3 * COEFFS)
    assert coeffs.shape[0] == int(np.prod(np.asarray(counts, np.int64)))
    index, w, Nn, deg = weights(lo, hi, counts, points, facing)
    with np.errstate(all="ignore"):
        a = np.zeros((len(index), 3 * COEFFS), T)
        for m in range(8):
            a = a + w[:, m].astype(T)[:, None] * coeffs[index[:, m]].astype(T)
        if T is F32:
            Y = probe_ref.basis(Nn)
        else:
            x, y, z = (Nn[:, k].astype(T) for k in range(3))
            c0, c1, c2, c3, c4 = (T(v) for v in (probe_ref.C0, probe_ref.C1, probe_ref.C2, probe_ref.C3, probe_ref.C4))
            Y = np.stack([np.full(len(Nn), c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3 * (z * z) - 1), c2 * (x * z), c4 * (x * x - y * y)], axis=1)
        F = factors(radiance, T)
        out = np.zeros((len(index), 3), T)
        for k in range(COEFFS):
            out = out + (F[k] * a[:, 3 * k:3 * k + 3]) * Y[:, k][:, None]
    out[deg] = 0
    return out.astype(T)
