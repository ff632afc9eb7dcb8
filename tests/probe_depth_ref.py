"""THE RULE of probe visibility (include/hrt.h "Probe visibility") in NumPy: the octahedral map (`direction`, `texel`), the filter
fold over per-sample (d, r) (`fold`), the moments (`moments`), the Chebyshev weight (`visibility`) and the visible look-up
(`weights_visible`, `evaluate_visible`) on top of probe_volume_ref.

Everything is fp32 in the order the header writes (NumPy neither fuses nor reassociates).  fminf and fmaxf drop a NaN operand, so
they are np.fmin and np.fmax here.  `dtype=np.float64` in `fold` evaluates the same sum in double from the fp32 directions."""
import numpy as np

import probe_ref
import probe_volume_ref as pv

F32, U32 = np.float32, np.uint32
RES, TEXELS, FLOATS, BLOCK = 8, 64, 192, 64
MAX_BLOCKS, VOLUME_MAX = 1 << 20, 1 << 22
ONE, HALF, ZERO = F32(1), F32(.5), F32(0)


def sg(v):
    return np.where(v >= 0, ONE, F32(-1)).astype(F32)


def _fold_pair(px, py):
    return ((ONE - np.abs(py)) * sg(px)).astype(F32), ((ONE - np.abs(px)) * sg(py)).astype(F32)


def direction(e):
    """The centre directions c_e of texels e (any shape, < 64): (..., 3) fp32."""
    e = np.asarray(e, np.int64)
    i, j = e % RES, e // RES
    px = (i.astype(F32) + HALF) * F32(.25) - ONE
    py = (j.astype(F32) + HALF) * F32(.25) - ONE
    z = ((ONE - np.abs(px)) - np.abs(py)).astype(F32)
    fx, fy = _fold_pair(px, py)
    px, py = np.where(z < 0, fx, px).astype(F32), np.where(z < 0, fy, py).astype(F32)
    L = np.sqrt((px * px + py * py) + z * z).astype(F32)
    return np.stack([px / L, py / L, z / L], axis=-1).astype(F32)


def _coord(p):
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(np.floor((p * HALF + HALF) * F32(8)), ZERO), F32(7)).astype(U32)


def texel(v):
    """The texels of vectors v (..., 3), which need not be unit: uint32."""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        s = ((np.abs(v[..., 0]) + np.abs(v[..., 1])) + np.abs(v[..., 2])).astype(F32)
        px, py = (v[..., 0] / s).astype(F32), (v[..., 1] / s).astype(F32)
        fx, fy = _fold_pair(px, py)
    low = v[..., 2] < 0
    px, py = np.where(low, fx, px).astype(F32), np.where(low, fy, py).astype(F32)
    return (U32(RES) * _coord(py) + _coord(px)).astype(U32)


def fold(d, r, live, dtype=F32):
    """The sums of ONE probe: d (s, 3) fp32 directions, r (s,) depths, live (s,) bool (False: a degenerate sample), sample j =
    row j.  Returns (64, 3) {W, A, B} in `dtype`: blocks of 64 samples, each from 0, added in ascending order."""
    T = dtype
    c = direction(np.arange(TEXELS)).astype(T)
    d, r = np.asarray(d, F32).astype(T), np.asarray(r, F32).astype(T)
    total = np.zeros((TEXELS, 3), T)
    for b0 in range(0, len(d), BLOCK):
        acc = np.zeros((TEXELS, 3), T)
        for j in range(b0, min(b0 + BLOCK, len(d))):
            if not live[j]:
                continue
            w = np.fmax(T(0), (c[:, 0] * d[j, 0] + c[:, 1] * d[j, 1]) + c[:, 2] * d[j, 2]).astype(T)
            for _ in range(5):
                w = w * w
            acc[:, 0] = acc[:, 0] + w
            acc[:, 1] = acc[:, 1] + w * r[j]
            acc[:, 2] = acc[:, 2] + w * (r[j] * r[j])
        total = total + acc
    return total.astype(T)


def moments(sums):
    """(n, 64, 3) sums -> (n, 64, 2) {m1, m2}."""
    s = np.asarray(sums, F32).reshape(-1, TEXELS, 3)
    W, A, B = s[..., 0], s[..., 1], s[..., 2]
    with np.errstate(all="ignore"):
        safe = np.where(W > 0, W, ONE)
        m1 = np.where(W > 0, A / safe, F32(np.inf))
        m2 = np.where(W > 0, B / safe, ZERO)
    return np.stack([m1, m2], axis=-1).astype(F32)


def visibility(l, m1, m2):
    l, m1, m2 = (np.asarray(x, F32) for x in (l, m1, m2))
    with np.errstate(all="ignore"):
        var = np.fmax(m2 - m1 * m1, ZERO).astype(F32)
        q = (l - m1).astype(F32)
        c = (var / (var + q * q)).astype(F32)
        vis = np.fmax((c * c) * c, F32(.001)).astype(F32)
    return np.where((l > 0) & ~(l <= m1), vis, ONE).astype(F32)


def weights_visible(lo, hi, counts, mom, points, facing=False):
    """Steps 1-3 of the visible look-up: (index (n, 8), weight (n, 8), Nn, degenerate).  mom: (nx*ny*nz, 64, 2)."""
    lo, hi, n, _ = pv._grid(lo, hi, counts)
    mom = np.asarray(mom, F32).reshape(-1, TEXELS, 2)
    pts = np.asarray(points, F32).reshape(-1, 8)
    P, b = pts[:, 0:3], pts[:, 7]
    Nn, deg = pv.normals(pts)
    deg = deg | ~np.isfinite(b)
    i0, i1, f = pv.cell(lo, hi, n, pts)
    index = np.zeros((len(pts), 8), U32)
    w = np.zeros((len(pts), 8), F32)
    with np.errstate(all="ignore"):
        Pb = (P + b[:, None] * Nn).astype(F32)
        for m in range(8):
            side = [(m >> a) & 1 for a in range(3)]
            c = np.stack([i1[:, a] if side[a] else i0[:, a] for a in range(3)], axis=1)
            wa = [f[:, a] if side[a] else ONE - f[:, a] for a in range(3)]
            index[:, m] = ((c[:, 2].astype(np.int64) * n[1] + c[:, 1]) * n[0] + c[:, 0]).astype(U32)
            wm = (wa[0] * wa[1]) * wa[2]
            C = pv.centres(lo, hi, n, c)
            if facing:
                v = C - P
                l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
                dot = (v[:, 0] * Nn[:, 0] + v[:, 1] * Nn[:, 1]) + v[:, 2] * Nn[:, 2]
                cs = np.where(l > 0, dot / np.where(l > 0, l, ONE), ZERO).astype(F32)
                t = (cs + ONE) * HALF
                wm = wm * (t * t + F32(.2))
            v = (Pb - C).astype(F32)
            l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F32)
            tx = np.where(l > 0, texel(v), U32(0))
            mm = mom[index[:, m], tx]
            w[:, m] = wm * visibility(l, mm[:, 0], mm[:, 1])
        W = w[:, 0]
        for m in range(1, 8):
            W = W + w[:, m]
        w = (w / W[:, None]).astype(F32)
    index[deg] = 0
    w[deg] = 0
    Nn = Nn.copy()
    Nn[deg] = 0
    return index, w, Nn, deg


def evaluate_visible(lo, hi, counts, coeffs, mom, points, radiance=False, facing=False):
    """Steps 1-6 of the visible look-up: (n, 3) fp32."""
    coeffs = np.asarray(coeffs, F32).reshape(-1, 3 * pv.COEFFS)
    index, w, Nn, deg = weights_visible(lo, hi, counts, mom, points, facing)
    with np.errstate(all="ignore"):
        a = np.zeros((len(index), 3 * pv.COEFFS), F32)
        for m in range(8):
            a = a + w[:, m][:, None] * coeffs[index[:, m]]
        Y = probe_ref.basis(Nn)
        F = pv.factors(radiance)
        out = np.zeros((len(index), 3), F32)
        for k in range(pv.COEFFS):
            out = out + (F[k] * a[:, 3 * k:3 * k + 3]) * Y[:, k][:, None]
    out[deg] = 0
    return out.astype(F32)
