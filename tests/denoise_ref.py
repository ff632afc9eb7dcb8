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


def iterate(x, feat, i, sigma_color, sigma_normal, sigma_albedo, sigma_depth, exp=np.exp):
    """One a-trous iteration at step 2^i (taps in row-major order, rows outer).  A tap outside the frame is read from a NaN
    border, so it is skipped exactly as a non-finite neighbour is.  `exp`: the exponential of the weights (tests perturb it)."""
    h, w, _ = x.shape
    s = 1 << i
    r = 2 * s
    sc = F32(sigma_color) * F32(2.0 ** -i)
    den_c, den_n, den_a = sc * sc, F32(sigma_normal) * F32(sigma_normal), F32(sigma_albedo) * F32(sigma_albedo)
    sz = F32(sigma_depth)
    pad = lambda v, fill: np.pad(v, ((r, r), (r, r)) + ((0, 0),) * (v.ndim - 2), constant_values=fill)
    xpad, fpad = pad(x, np.nan), pad(feat, 0)
    n, a, z = feat[..., 3:6], feat[..., 0:3], feat[..., 9]
    valid_p = _finite3(x)
    sw = np.zeros((h, w), F32)
    sx = np.zeros((h, w, 3), F32)
    with np.errstate(all="ignore"):
        for k in range(-2, 3):
            for j in range(-2, 3):
                hh = H[j + 2] * H[k + 2]
                if j == 0 and k == 0:
                    wq = np.full((h, w), hh, F32)
                    xq = x
                    use = np.ones((h, w), bool)
                else:
                    win = (slice(r + k * s, r + k * s + h), slice(r + j * s, r + j * s + w))
                    xq, fq = xpad[win], fpad[win]
                    use = _finite3(xq)
                    zp, zq = z, fq[..., 9]
                    zs = (sz * np.maximum(np.maximum(zp, zq), F32(1e-3))).astype(F32)
                    dz = (zp - zq).astype(F32)
                    e = ((_term(_sq3(x - xq), den_c) + _term(_sq3(n - fq[..., 3:6]), den_n)) + _term(_sq3(a - fq[..., 0:3]), den_a)) + \
                        _term(dz * dz, zs * zs)
                    wq = (hh * exp(-e.astype(F32)).astype(F32)).astype(F32)
                use = use & valid_p
                sw = np.where(use, sw + wq, sw).astype(F32)
                sx = np.where(use[..., None], sx + wq[..., None] * xq, sx).astype(F32)
        y = (sx / sw[..., None]).astype(F32)
    return np.where(valid_p[..., None], y, x).astype(F32)


def denoise(color, feat, iterations=4, sigma_color=8.0, sigma_normal=0.05, sigma_albedo=0.4, sigma_depth=0.05, gamma=False, exp=np.exp):
    """The whole rule of include/hrt.h: (h, w, 3) float32.  The defaults are those of DenoiseParams."""
    color = np.ascontiguousarray(color, F32)
    feat = np.ascontiguousarray(feat, F32)
    x, d = demodulate(color, feat)
    for i in range(iterations):
        x = iterate(x, feat, i, sigma_color, sigma_normal, sigma_albedo, sigma_depth, exp)
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


# ------------------------------------------------------------------------------------------------------------ the exact regime
# With sigma_color = +inf the colour term is off (T = 0), and with the guide sigmas at 1e-30 their squares underflow to 0, so each
# guide term is 0 (equal guides) or +inf (different guides): E is 0 or +inf and every weight is exactly h_j h_k or exactly 0.  No
# transcendental is left, so a device that follows the rule must equal this statement bit for bit.
EXACT = dict(sigma_color=np.inf, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=1e-30)


def radius(iterations):
    """How far the rule reaches: the taps of iteration i lie within 2 * 2^i, so `iterations` reach 2 (2^iterations - 1)."""
    return 2 * ((1 << iterations) - 1)


MASK = 0xFFFFFFFF


def coord_hash(a, b, salt):
    """A 32-bit integer hash of integer coordinate arrays (numpy or torch int64).  Every product stays below 2^63 for
    coordinates below 2^31, so numpy and torch compute the same bits."""
    v = ((a * 73856093) ^ (b * 19349663) ^ (salt * 83492791)) & MASK
    v = ((v ^ (v >> 16)) * 0x45D9F3B) & MASK
    v = ((v ^ (v >> 16)) * 0x45D9F3B) & MASK
    return v ^ (v >> 16)


def coord_unit(a, b, salt):
    """fp32 in [0, 1) from the hash: a 24-bit integer times 2^-24, exact in fp32 on either side."""
    v = coord_hash(a, b, salt) >> 8
    if isinstance(v, np.ndarray):
        return v.astype(F32) * F32(2.0 ** -24)
    import torch
    return v.to(torch.float32) * (2.0 ** -24)


# Region tables of coord_frame: (albedo rgb, normal xyz, emission rgb, depth, coverage).  Rows 0-7: surfaces (one emitter with
# albedo > 0 among them, row 7), row 8: a miss (all 0), row 9: an albedo-0 emitter.  Depths stay small enough that
# (1e-30 * z)^2 underflows to 0.
REGIONS = np.array([
    [0.8, 0.2, 0.2, 0.0, 1.0, 0.0, 0, 0, 0, 2.0, 1],
    [0.2, 0.8, 0.2, 1.0, 0.0, 0.0, 0, 0, 0, 5.0, 1],
    [0.7, 0.7, 0.7, 0.0, 0.0, 1.0, 0, 0, 0, 9.0, 1],
    [0.1, 0.1, 0.9, 0.6, 0.8, 0.0, 0, 0, 0, 3.5, 1],
    [0.8, 0.2, 0.2, 0.0, 1.0, 0.0, 0, 0, 0, 2.5, 1],    # row 0's albedo and normal at another depth
    [0.8, 0.2, 0.2, 1.0, 0.0, 0.0, 0, 0, 0, 2.0, 1],    # row 0's albedo and depth with another normal
    [0.3, 0.2, 0.2, 0.0, 1.0, 0.0, 0, 0, 0, 2.0, 0.5],  # row 0 but for one albedo channel
    [0.9, 0.9, 0.9, 0.0, -1.0, 0.0, 4, 4, 4, 1.5, 1],   # an emitter with albedo
    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0.0, 0],    # a miss
    [0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 6, 5, 4, 1.0, 1],   # an albedo-0 emitter
], F32)
REGIONS_E6 = (REGIONS[:, 6:9] / F32(6)).astype(F32)  # e/6 of each region, divided here once (torch on the GPU divides by a
                                                     # scalar as a multiplication by its reciprocal, which rounds differently)


def coord_frame(ys, xs, seed=0, block=(5, 7)):
    """Colour (..., 3) and hard-edge features (..., 12) of the pixels at integer coordinates (ys, xs), numpy or torch int64
    arrays: the guides are piecewise constant over blocks of block[0] x block[1] pixels (a region of REGIONS picked by a hash
    of the block), the colour is a hash of the pixel in [0, 1) plus e/6.  numpy and torch give the same bits,
    so a frame built on the device can be checked window by window on the host."""
    by, bx = block
    region = coord_hash(ys // by, xs // bx, 1000 + seed) % len(REGIONS)
    if isinstance(ys, np.ndarray):
        stack, table, e6 = (lambda v: np.stack(v, -1)), REGIONS, REGIONS_E6
        feat = np.zeros(ys.shape + (12,), F32)
    else:
        import torch
        stack, table, e6 = (lambda v: torch.stack(v, -1)), torch.from_numpy(REGIONS).to(ys.device), torch.from_numpy(REGIONS_E6).to(ys.device)
        feat = torch.zeros(tuple(ys.shape) + (12,), dtype=torch.float32, device=ys.device)
    feat[..., 0:11] = table[region]
    color = stack([coord_unit(ys, xs, 3 * seed + k) for k in range(3)])
    color = color + e6[region]  # one fp32 addition, the same in numpy and torch
    return color, feat


def coord_window(y0, y1, x0, x1, seed=0, block=(5, 7)):
    """coord_frame over rows y0:y1 and columns x0:x1 (numpy)."""
    ys, xs = np.mgrid[y0:y1, x0:x1].astype(np.int64)
    return coord_frame(ys, xs, seed, block)


def hard_edge_frame(h, w, seed=0, block=(5, 7)):
    """A whole h x w frame of coord_frame (numpy): the exact regime's input."""
    return coord_window(0, h, 0, w, seed, block)


def denoise_window(get, h, w, y0, y1, x0, x1, iterations, **params):
    """The rule's output on rows y0:y1, columns x0:x1 of an h x w frame, computed on a crop of radius(iterations) pixels more on
    every side (clipped at the frame).  Pixels farther than that from the crop's cut edges see exactly the taps they see in the
    full frame, so the result equals the full frame's bit for bit.  get(cy0, cy1, cx0, cx1) -> (colour, features) of the crop."""
    r = radius(iterations)
    cy0, cy1, cx0, cx1 = max(0, y0 - r), min(h, y1 + r), max(0, x0 - r), min(w, x1 + r)
    c, f = get(cy0, cy1, cx0, cx1)
    out = denoise(c, f, iterations=iterations, **params)
    return out[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]


# ------------------------------------------------------------------------------------------------------------ the expf regime
U = 2.0 ** -24       # unit roundoff of fp32
EXP_ULP = 4          # each side's fp32 exponential is taken to be within 4 ulp of exp (OCML expf and numpy claim 1 to 3)


def expf_bound(color, feat, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth, exp_ulp=EXP_ULP):
    """Per value (h, w, 3): a bound on |device - statement| of the LINEAR output when the guide sigmas are finite, so the weights
    go through exp and the two sides may round it differently.  Valid for one iteration, or for any number with the colour term
    off (sigma_color = +inf).

    One iteration.  Both sides compute the same E (fp32 operations without a transcendental), so the weights differ only through
    exp: w' = w (1 + eps_q) with |eps_q| <= eps = (4 exp_ulp + 2) u (an ulp is at most 2u relative; both exponentials, both
    products h_j h_k * exp), plus an
    absolute 2^-126 for weights that go subnormal.  In exact arithmetic
        y' - y = sum_q w_q eps_q (x_q - y) / sum_q w_q (1 + eps_q),   so   |y' - y| <= eps / (1 - eps) * M,  M = max_q |x_q - y|
    over the taps used (the centre tap always has w = 9/64, so sum_q w_q >= 9/64 and the subnormal slack adds at most
    25 * 2^-126 * 64/9 * M < 200 * 2^-126 * M).  Each side's fp32 evaluation of its own quotient is within
    (2 n + 1) u X of its exact value, n = 25 taps, X = max_q |x_q| (recursive sums of n terms: gamma_n sum |w x| <= n u X sum w for
    the numerator, gamma_(n-1) for the denominator, one rounding of the quotient).  So per iteration
        |dy_p| <= 2 eps M_p + 2 (2 n + 1) u X_p.
    Several iterations with the colour term off.  The weights then do not depend on x, so the device applies the same weights to
    its own previous iterate: y'_i+1 = A'_i y'_i.  Every row of A'_i is a convex combination, so the error carried in is at most the
    largest error among the taps p used, B_i+1(p) = max_q B_i(q) + (the one-iteration term of p): the bound adds up linearly over
    iterations, taking the maximum over each pixel's taps.  (M and X are taken from the statement's iterate; the device's differs
    by the bound itself, a second-order change.)
    Remodulation r = d y + e/6 scales it by |d| and adds the two sides' roundings, 4 u (|d y| + |e/6|).
    Invalid pixels are exact on both sides (their bound is 0); non-finite results are compared for identity elsewhere."""
    if iterations > 1 and sigma_color != np.inf:
        raise ValueError("the bound covers one iteration, or any number with the colour term off")
    eps = (4 * exp_ulp + 2) * U
    coef = 2 * eps / (1 - eps) + 200 * 2.0 ** -126
    n = 25
    x, d = demodulate(np.ascontiguousarray(color, F32), np.ascontiguousarray(feat, F32))
    h, w, _ = x.shape
    bound = np.zeros((h, w, 3), np.float64)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            y = iterate(x, feat, i, sigma_color, sigma_normal, sigma_albedo, sigma_depth)
            s, r = 1 << i, 2 << i
            valid = _finite3(x)
            xpad = np.pad(x.astype(np.float64), ((r, r), (r, r), (0, 0)), constant_values=np.nan)
            bpad = np.pad(bound, ((r, r), (r, r), (0, 0)))
            m = np.zeros((h, w, 3)); big = np.zeros((h, w, 3)); carry = np.zeros((h, w, 3))
            y64 = y.astype(np.float64)
            for k in range(-2, 3):
                for j in range(-2, 3):
                    win = (slice(r + k * s, r + k * s + h), slice(r + j * s, r + j * s + w))
                    xq = xpad[win]
                    use = (np.isfinite(xq).all(axis=-1) & valid)[..., None]
                    m = np.where(use, np.maximum(m, np.abs(xq - y64)), m)
                    big = np.where(use, np.maximum(big, np.abs(xq)), big)
                    carry = np.where(use, np.maximum(carry, bpad[win]), carry)
            bound = np.where(valid[..., None], carry + coef * m + 2 * (2 * n + 1) * U * big, 0.0)
            x = y
        e6 = (feat[..., 6:9] / F32(6)).astype(np.float64)
        dy = np.abs(d.astype(np.float64) * x.astype(np.float64))
        out = np.abs(d.astype(np.float64)) * bound * (1 + 2 * U) + 4 * U * (dy + np.abs(e6))
    return np.where(np.isfinite(out), out, np.inf)
