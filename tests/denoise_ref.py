"""NumPy statement of the denoiser of include/hrt.h (hrt_denoise): demodulate, a-trous iterations, remodulate.

Every step is fp32 in the order the header writes it down (and csrc/hrt_denoise.hip evaluates it), so the device result agrees
with this one to the rounding of expf / pow alone.  Arrays: colour (h, w, 3), features (h, w, 12) float32."""
import numpy as np

F32 = np.float32
H = np.array([1, 4, 6, 4, 1], F32) / F32(16)  # B3-spline taps


def _finite3(v):
    return np.isfinite(v).all(axis=-1)


def _sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _term(num, den):
    """T(num, den): 0 if num == 0 or den == +inf, else num / den."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = (num / den).astype(F32)
    return np.where((num == 0) | (den == np.inf), F32(0), q).astype(F32)


def demodulate(color, feat):
    """(x, d): x = (c - e/6) / d with d = albedo where > 0, else 1; x is NaN on invalid pixels."""
    a, e = feat[..., 0:3], feat[..., 6:9]
    d = np.where(a > 0, a, F32(1)).astype(F32)
    with np.errstate(all="ignore"):
        x = ((color - e / F32(6)) / d).astype(F32)
    ok = _finite3(x) & np.isfinite(feat[..., 0:10]).all(axis=-1)
    x = np.where(ok[..., None], x, F32(np.nan)).astype(F32)
    return x, d


def iterate(x, feat, i, sigma_color, sigma_normal, sigma_albedo, sigma_depth):
    """One a-trous iteration at step 2^i (taps in row-major order, rows outer)."""
    h, w, _ = x.shape
    s = 1 << i
    n, a, z = feat[..., 3:6], feat[..., 0:3], feat[..., 9]
    sc = F32(sigma_color) * F32(2.0 ** -i)
    den_c, den_n, den_a = sc * sc, F32(sigma_normal) * F32(sigma_normal), F32(sigma_albedo) * F32(sigma_albedo)
    sz = F32(sigma_depth)
    valid_p = _finite3(x)
    sw = np.zeros((h, w), F32)
    sx = np.zeros((h, w, 3), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for k in range(-2, 3):
            for j in range(-2, 3):
                qy, qx = ys + k * s, xs + j * s
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                hh = H[j + 2] * H[k + 2]
                if j == 0 and k == 0:
                    wq = np.full((h, w), hh, F32)
                    xq = x
                    use = np.ones((h, w), bool)
                else:
                    xq = x[cy, cx]
                    use = inside & _finite3(xq)
                    zp, zq = z, z[cy, cx]
                    zs = (sz * np.maximum(np.maximum(zp, zq), F32(1e-3))).astype(F32)
                    dz = (zp - zq).astype(F32)
                    e = ((_term(_sq3(x - xq), den_c) + _term(_sq3(n - n[cy, cx]), den_n)) + _term(_sq3(a - a[cy, cx]), den_a)) + \
                        _term(dz * dz, zs * zs)
                    wq = (hh * np.exp(-e.astype(F32))).astype(F32)
                use = use & valid_p
                sw = np.where(use, sw + wq, sw).astype(F32)
                sx = np.where(use[..., None], sx + wq[..., None] * xq, sx).astype(F32)
        y = (sx / sw[..., None]).astype(F32)
    return np.where(valid_p[..., None], y, x).astype(F32)


def denoise(color, feat, iterations=4, sigma_color=8.0, sigma_normal=0.05, sigma_albedo=0.4, sigma_depth=0.05, gamma=False):
    """The whole rule of include/hrt.h: (h, w, 3) float32.  The defaults are those of DenoiseParams."""
    color = np.ascontiguousarray(color, F32)
    feat = np.ascontiguousarray(feat, F32)
    x, d = demodulate(color, feat)
    for i in range(iterations):
        x = iterate(x, feat, i, sigma_color, sigma_normal, sigma_albedo, sigma_depth)
    with np.errstate(all="ignore"):
        r = (d * x + feat[..., 6:9] / F32(6)).astype(F32)
        out = np.where(_finite3(r)[..., None], r, color).astype(F32)
        if gamma:
            out = np.power(out.astype(np.float64), 1.0 / 2.2).astype(F32)
    return out


def synthetic_features(h, w, seed=0):
    """Random guides with hard edges: four regions of different normal, albedo and depth, and a sky strip (all zero)."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w, 12), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    region = (ys * 2 // max(h, 1)) * 2 + (xs * 2 // max(w, 1))
    normals = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [0.6, 0.8, 0]], F32)
    albedo = np.array([[0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.7, 0.7, 0.7], [0.1, 0.1, 0.9]], F32)
    depth = np.array([2.0, 5.0, 9.0, 3.5], F32)
    f[..., 0:3] = albedo[region]
    f[..., 3:6] = normals[region]
    f[..., 9] = depth[region] + rng.uniform(0, 0.05, (h, w)).astype(F32)
    f[..., 10] = 1
    lamp = (region == 2) & (xs % 7 == 0)   # albedo-0 emitters
    f[lamp, 0:3] = 0
    f[lamp, 6:9] = 5.0
    sky = ys == h - 1
    f[sky] = 0
    return f
