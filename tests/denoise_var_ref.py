"""NumPy statement of the variance-guided denoiser of include/hrt.h (hrt_denoise_var): demodulate both frames, variance of the
mean, prefilter, a-trous iterations that carry the variance, remodulate.

Every step is fp32 in the order the header writes it down (and csrc/hrt_denoise.hip evaluates it), so the device result agrees
with this one to the rounding of expf / pow alone.  Arrays: colour and half colour (h, w, 3), features (h, w, 12) float32."""
import numpy as np

from denoise_ref import F32, H, _finite3, _sq3, _term, demodulate, radius


def prepare(color, half, feat):
    """(x, v, d): x NaN on pixels invalid for either frame; v = |x - x_half|^2, 0 on invalid pixels and where it is not finite."""
    x, d = demodulate(color, feat)
    xh, _ = demodulate(half, feat)
    ok = _finite3(x) & _finite3(xh)
    x = np.where(ok[..., None], x, F32(np.nan)).astype(F32)
    with np.errstate(all="ignore"):
        v = _sq3((x - xh).astype(F32)).astype(F32)
    v = np.where(ok & np.isfinite(v), v, F32(0)).astype(F32)
    return x, v, d


def _pad(v, r, fill):
    return np.pad(v, ((r, r), (r, r)) + ((0, 0),) * (v.ndim - 2), constant_values=fill)


def _guides(feat, fq, sigma_normal, sigma_albedo, sigma_depth):
    """G_pq of the header: (T(normal) + T(albedo)) + T(depth) between every pixel and its tap's features fq."""
    den_n, den_a, sz = F32(sigma_normal) * F32(sigma_normal), F32(sigma_albedo) * F32(sigma_albedo), F32(sigma_depth)
    zp, zq = feat[..., 9], fq[..., 9]
    zs = (sz * np.maximum(np.maximum(zp, zq), F32(1e-3))).astype(F32)
    dz = (zp - zq).astype(F32)
    return ((_term(_sq3(feat[..., 3:6] - fq[..., 3:6]), den_n) + _term(_sq3(feat[..., 0:3] - fq[..., 0:3]), den_a)) +
            _term(dz * dz, zs * zs)).astype(F32)


def pass_(x, v, feat, i, sigma_variance, variance_floor, sigma_normal, sigma_albedo, sigma_depth, prefilter, exp=np.exp):
    """One pass at step 2^i (taps in row-major order, rows outer): a prefilter pass (v alone, guide weights) or an iteration
    (x with the colour width of each pair of pixels, v carried as sum w^2 v / (sum w)^2).  Returns (x, v)."""
    h, w, _ = x.shape
    s = 1 << i
    r = 2 * s
    xpad, vpad, fpad = _pad(x, r, np.nan), _pad(v, r, 0), _pad(feat, r, 0)
    valid_p = _finite3(x)
    sv2 = F32(sigma_variance) * F32(sigma_variance)
    with np.errstate(all="ignore"):
        sw = np.zeros((h, w), F32)
        sx = np.zeros((h, w, 3), F32)
        sv = np.zeros((h, w), F32)
        for k in range(-2, 3):
            for j in range(-2, 3):
                hh = H[j + 2] * H[k + 2]
                if j == 0 and k == 0:
                    wq = np.full((h, w), hh, F32)
                    xq, vq = x, v
                    use = np.ones((h, w), bool)
                else:
                    win = (slice(r + k * s, r + k * s + h), slice(r + j * s, r + j * s + w))
                    xq, vq, fq = xpad[win], vpad[win], fpad[win]
                    use = _finite3(xq)
                    e = _guides(feat, fq, sigma_normal, sigma_albedo, sigma_depth)
                    if not prefilter:
                        den_c = np.full((h, w), np.inf, F32) if sv2 == np.inf else (sv2 * ((v + vq) + F32(variance_floor)).astype(F32)).astype(F32)
                        e = (_term(_sq3(x - xq), den_c) + e).astype(F32)
                    wq = (hh * exp(-e.astype(F32)).astype(F32)).astype(F32)
                use = use & valid_p
                sw = np.where(use, sw + wq, sw).astype(F32)
                if prefilter:
                    sv = np.where(use, sv + wq * vq, sv).astype(F32)
                else:
                    sx = np.where(use[..., None], sx + wq[..., None] * xq, sx).astype(F32)
                    sv = np.where(use, sv + (wq * wq).astype(F32) * vq, sv).astype(F32)
        if prefilter:
            return x, np.where(valid_p, sv / sw, v).astype(F32)
        y = (sx / sw[..., None]).astype(F32)
        vy = (sv / (sw * sw).astype(F32)).astype(F32)
    return np.where(valid_p[..., None], y, x).astype(F32), np.where(valid_p, vy, v).astype(F32)


def denoise_var(color, half, feat, iterations=4, prefilter=2, sigma_variance=8.0, sigma_normal=0.05, sigma_albedo=0.4, sigma_depth=0.05,
                variance_floor=1e-8, gamma=False, exp=np.exp):
    """The whole rule of include/hrt.h: (frame (h, w, 3), variance map (h, w)) float32.  The defaults are those of DenoiseVarParams."""
    color = np.ascontiguousarray(color, F32)
    half = np.ascontiguousarray(half, F32)
    feat = np.ascontiguousarray(feat, F32)
    x, v, d = prepare(color, half, feat)
    g = (sigma_normal, sigma_albedo, sigma_depth)
    for i in range(prefilter):
        x, v = pass_(x, v, feat, i, sigma_variance, variance_floor, *g, prefilter=True, exp=exp)
    for i in range(iterations):
        x, v = pass_(x, v, feat, i, sigma_variance, variance_floor, *g, prefilter=False, exp=exp)
    with np.errstate(all="ignore"):
        r = (d * x + feat[..., 6:9] / F32(6)).astype(F32)
        out = np.where(_finite3(r)[..., None], r, color).astype(F32)
        if gamma:
            out = np.power(out.astype(np.float64), 1.0 / 2.2).astype(F32)
    return out, v


def reach(iterations, prefilter):
    """How far the rule reaches: the iterations' radius plus the prefilter passes'."""
    return radius(iterations) + radius(prefilter)


def denoise_var_window(get, h, w, y0, y1, x0, x1, iterations, prefilter, **params):
    """denoise_ref.denoise_window for this rule: the output and variance on rows y0:y1, columns x0:x1 of an h x w frame, computed on
    a crop of reach(iterations, prefilter) pixels more on every side.  get(cy0, cy1, cx0, cx1) -> (colour, half colour, features)."""
    r = reach(iterations, prefilter)
    cy0, cy1, cx0, cx1 = max(0, y0 - r), min(h, y1 + r), max(0, x0 - r), min(w, x1 + r)
    c, ch, f = get(cy0, cy1, cx0, cx1)
    out, v = denoise_var(c, ch, f, iterations=iterations, prefilter=prefilter, **params)
    return out[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0], v[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]
