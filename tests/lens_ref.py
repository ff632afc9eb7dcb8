"""THE RULE of the lens cameras (include/hrt.h "Lens cameras") in NumPy, and the counter-based RNG stream it draws from.

`rays(lens, w, h, sample, seed)` gives the records hrt_lens_rays writes and the mask of degenerate samples, in fp32 in the order the
header writes (NumPy neither fuses nor reassociates); `dtype=np.float64` evaluates the same expressions, from the same fp32 draws,
constants and pinhole rays, in double -- the yardstick RAY_TOL below comes from.  The pinhole ray of PERSPECTIVE is the render's
camera ray, which tests/oracle_lib.py already restates (camera_rays); everything else is here."""
from dataclasses import dataclass

import numpy as np

import oracle_lib

F32 = np.float32
U32 = np.uint32
LENS_DRAW = 0x80000000
PI = F32(3.1415927)
TWO_PI = F32(6.2831855)

# Tolerance per ray component between the device's rays and rays() for the lenses and frames of tests/test_gpu_lens.py (CASES x
# FRAMES x DRAWS below): 4 x the largest difference, over every component of every non-degenerate ray of those inputs, between the
# rule evaluated in fp32 and in fp64 from the same draws (fp_gap(): 2.360012e-07, reached on the orthographic origins, which are a
# few units from the world origin; 1.9e-07 .. 2.2e-07 on the equirect and fisheye directions, 1.0e-07 on the thin lens).  That gap is
# the rounding the rule itself allows an fp32 evaluation; the factor leaves room for what NumPy and the device do not share -- sinf
# and cosf, each within a few ulp of the true value on either side -- while sqrtf and the divisions are correctly rounded on both.
# A CPU-side measurement: nothing of the code under test enters it.  tests/test_lens_ref.py holds the constant to the measurement.
RAY_TOL = 4 * 2.360012e-07

CASES = {  # name -> (projection, aperture, focus, extent)
    "thin": ("perspective", 0.2, 4.0, 0.0),
    "ortho": ("ortho", 0.0, 1.0, 3.0),
    "equirect": ("equirect", 0.0, 1.0, 0.0),
    "fisheye180": ("fisheye", 0.0, 1.0, 180.0),
    "fisheye220": ("fisheye", 0.0, 1.0, 220.0),
}
FRAMES = ((37, 23), (8, 17))
DRAWS = ((0, 1), (5, 2 ** 63 + 12345))  # (sample, seed)


@dataclass
class Lens:
    cam: object            # a Camera of the package (ctypes)
    projection: str = "perspective"
    aperture: float = 0.0
    focus: float = 1.0
    extent: float = 0.0


# ------------------------------------------------------------------------------------------------------------------------ RNG
def mix32(x):
    x = np.asarray(x, U32).copy()
    x ^= x >> U32(16); x *= U32(0x7feb352d); x ^= x >> U32(15); x *= U32(0x846ca68b); x ^= x >> U32(16)
    return x


def draws(seed, pixel, sample, index):
    """Draw `index` (broadcast against `pixel`) of stream (seed, pixel, sample): csrc/hrt_kernels.hip Rng, in uint32 arithmetic."""
    with np.errstate(over="ignore"):
        pixel = np.asarray(pixel, np.uint64).astype(U32)
        index = np.asarray(index, np.uint64).astype(U32)
        lo, hi = U32(seed & 0xFFFFFFFF), U32((seed >> 32) & 0xFFFFFFFF)
        k0 = mix32(lo ^ (pixel * U32(0x9E3779B1) + U32(0x7F4A7C15)))
        k1 = mix32(np.asarray(hi + U32(sample & 0xFFFFFFFF) * U32(0x85EBCA77) + U32(0xC2B2AE3D), U32))
        x = np.asarray(k0 + index * U32(0x9E3779B9), U32).copy()
        x ^= x >> U32(16); x *= U32(0x7feb352d); x ^= x >> U32(15); x ^= k1; x *= U32(0x846ca68b); x ^= x >> U32(16)
    return (x >> U32(8)).astype(F32) * F32(1.0 / 16777216.0)


def film(w, h, sample, seed):
    """u, v, time, l0, l1 of every pixel of a w x h frame (fp32), as the rule draws them."""
    p = np.arange(w * h)
    y, x = np.divmod(p, w)
    u = (x.astype(F32) + draws(seed, p, sample, 0)) / F32(w)
    v = (y.astype(F32) + draws(seed, p, sample, 1)) / F32(h)
    return u, v, draws(seed, p, sample, 2), draws(seed, p, sample, LENS_DRAW), draws(seed, p, sample, LENS_DRAW + 1)


def centres(w, h):
    """The film positions of hrt_render_lens_features with n_samples == 0: pixel centres, time 0, l0 = l1 = 0."""
    y, x = np.divmod(np.arange(w * h), w)
    z = np.zeros(w * h, F32)
    return (x.astype(F32) + F32(0.5)) / F32(w), (y.astype(F32) + F32(0.5)) / F32(h), z, z, z


# ----------------------------------------------------------------------------------------------------------------------- rule
def _dot(a, b):
    return (a[:, 0] * b[0] + a[:, 1] * b[1]) + a[:, 2] * b[2]


def _normalize(a):
    L = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a / L[:, None]


def project(lens, u, v, time, l0, l1, dtype=F32):
    """(o, d, degenerate) of the rule for film positions (u, v) and lens draws (l0, l1), every expression in `dtype`."""
    T = dtype
    cam = lens.cam
    R, U, Fw, E = (np.array(list(a), F32).astype(T) for a in (cam.right, cam.up, cam.forward, cam.eye))
    n = len(u)
    uu, vv = u.astype(T), v.astype(T)
    one, two, half = T(1), T(2), T(0.5)
    o = np.tile(E, (n, 1))
    d = np.zeros((n, 3), T)
    deg = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if lens.projection == "perspective":
            cr = oracle_lib.camera_rays(cam, np.stack([u, v], axis=1))  # the render's camera ray, fp32 bits
            ro, rd = cr[:, 0:3].astype(T), cr[:, 3:6].astype(T)
            if lens.aperture == 0:
                return ro, rd, deg
            rad = T(F32(lens.aperture)) * np.sqrt(l0.astype(T))
            phi = T(TWO_PI) * l1.astype(T)
            a, b = rad * np.cos(phi), rad * np.sin(phi)
            c = _dot(rd, Fw)
            deg = ~(c > 0)
            tf = T(F32(lens.focus)) / c
            P = ro + tf[:, None] * rd
            o = ro + (a[:, None] * R + b[:, None] * U)
            d = _normalize(P - o)
        elif lens.projection == "ortho":
            ext, asp = T(F32(lens.extent)), T(F32(cam.aspect))
            sx = (two * uu - one) * ((half * ext) * asp)
            sy = (one - two * vv) * (half * ext)
            o = E + (sx[:, None] * R + sy[:, None] * U)
            d = np.tile(_normalize(Fw[None])[0], (n, 1))
        elif lens.projection == "equirect":
            phi = (two * uu - one) * T(PI)
            th = (half - vv) * T(PI)
            ct, st = np.cos(th), np.sin(th)
            d = _normalize(((ct * np.sin(phi))[:, None] * R + st[:, None] * U) + (ct * np.cos(phi))[:, None] * Fw)
        elif lens.projection == "fisheye":
            qx = (two * uu - one) * T(F32(cam.aspect))
            qy = one - two * vv
            rr = np.sqrt(qx * qx + qy * qy)
            deg = rr > one
            th = rr * (T(F32(lens.extent)) * half * T(PI / F32(180)))
            k = np.sin(th) / rr
            d = _normalize(((k * qx)[:, None] * R + (k * qy)[:, None] * U) + np.cos(th)[:, None] * Fw)
            d[rr == 0] = _normalize(Fw[None])[0]
        else:
            raise ValueError(lens.projection)
    o = np.where(deg[:, None], E, o)
    d = np.where(deg[:, None], T(0), d)
    return o, d, deg


def records(o, d, time):
    r = np.empty((len(o), 8), F32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, time, d, np.inf
    return r


def rays(lens, w, h, sample, seed, dtype=F32):
    """The records of hrt_lens_rays(lens, w, h, sample, seed) -- (w*h, 8) in `dtype` -- and the mask of degenerate samples."""
    u, v, tm, l0, l1 = film(w, h, sample, seed)
    o, d, deg = project(lens, u, v, tm, l0, l1, dtype)
    if dtype is F32:
        return records(o, d, tm), deg
    r = np.empty((w * h, 8), dtype)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tm, d, np.inf
    return r, deg


def fisheye_radius(lens, w, h, sample, seed):
    """rr of every sample of a fisheye frame (fp32): a sample within RAY_TOL of 1 may fall on either side of the rim on the device."""
    u, v, _, _, _ = film(w, h, sample, seed)
    qx = (F32(2) * u - F32(1)) * F32(lens.cam.aspect)
    qy = F32(1) - F32(2) * v
    return np.sqrt(qx * qx + qy * qy)


def make(hrt, name, w, h):
    """The Lens of CASES[name] behind the default camera of a w x h frame, here and as the package's ctypes struct."""
    proj, ap, fo, ex = CASES[name]
    cam = hrt.default_camera(w / h)
    return Lens(cam, proj, ap, fo, ex), hrt.Lens(cam, proj, aperture=ap, focus=fo, extent=ex)


def fp_gap(hrt):
    """Largest |fp32 - fp64| over every component of every non-degenerate ray of CASES x FRAMES x DRAWS."""
    gap = 0.0
    for name in CASES:
        for w, h in FRAMES:
            ref, _ = make(hrt, name, w, h)
            for sample, seed in DRAWS:
                r32, deg = rays(ref, w, h, sample, seed)
                r64, deg64 = rays(ref, w, h, sample, seed, np.float64)
                ok = ~(deg | deg64)
                gap = max(gap, float(np.abs(r32[ok][:, [0, 1, 2, 4, 5, 6]].astype(np.float64) - r64[ok][:, [0, 1, 2, 4, 5, 6]]).max()))
    return gap
