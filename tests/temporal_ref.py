"""NumPy statement of temporal accumulation (include/hrt.h hrt_temporal_accumulate): demodulate, world point, projection into the
previous camera, four bilinear taps with their tests, blend, remodulate.

Every step is fp32 in the order the header writes it down (and csrc/hrt_temporal.hip evaluates it); nothing transcendental is in
it, so the device result equals this one bit for bit.  Arrays: colours (h, w, 3), features (h, w, 12), history (h, w), float32.
Cameras: anything with the fields of hrt_camera (eye, right, up, forward, fovy_deg, aspect, znear, zfar), the ctypes Camera included.
The pixel-centre rays of the current camera come from the caller -- (origins, directions), each (h, w, 3), on the GPU the
output of hrt_debug_kat(HRT_KAT_CAMERA) at u = (x + 0.5) / w, v = (y + 0.5) / h: camera_ray is fp64 arithmetic pinned elsewhere."""
import math

import numpy as np

from denoise_ref import F32, _finite3, _sq3, demodulate

DEFAULTS = dict(alpha_min=0.02, max_history=64.0, depth_tol=0.05, normal_tol=0.1, albedo_tol=0.05)  # those of TemporalParams


def camera_floats(cam):
    """The 16 floats of an hrt_camera, in its layout."""
    return np.array(list(cam.eye) + list(cam.right) + list(cam.up) + list(cam.forward) + [cam.fovy_deg, cam.aspect, cam.znear, cam.zfar], F32)


def same_camera(a, b):
    """memcmp(a, b, sizeof(hrt_camera)) == 0."""
    return camera_floats(a).tobytes() == camera_floats(b).tobytes()


def projection_constants(cam):
    """(kx, ky) = ((float)(cot / aspect), (float)cot), cot in fp64 as hrt_render's projection has it."""
    rad = float(F32(cam.fovy_deg)) / 2.0 * math.pi / 180.0
    cot = math.cos(rad) / math.sin(rad)
    with np.errstate(all="ignore"):
        return F32(np.float64(cot) / np.float64(F32(cam.aspect))), F32(cot)


def pixel_uv(w, h):
    """(u, v) of the pixel centres, (h, w) each: ((float)x + 0.5f) / (float)w as the kernel forms them."""
    ys, xs = np.mgrid[0:h, 0:w]
    return ((xs.astype(F32) + F32(0.5)) / F32(w)).astype(F32), ((ys.astype(F32) + F32(0.5)) / F32(h)).astype(F32)


def project(rays, zbar, prev_cam, w, h):
    """Steps 2 and 3: (px, py, zexp, zc) of every pixel's world point in the previous camera."""
    o, d = (np.ascontiguousarray(v, F32) for v in rays)
    eye, R, U, Fw = (np.array(list(v), F32) for v in (prev_cam.eye, prev_cam.right, prev_cam.up, prev_cam.forward))
    kx, ky = projection_constants(prev_cam)
    with np.errstate(all="ignore"):
        s = [((o[..., k] + (zbar * d[..., k]).astype(F32)).astype(F32) - eye[k]).astype(F32) for k in range(3)]
        dot = lambda v: ((s[0] * v[0]).astype(F32) + (s[1] * v[1]).astype(F32)).astype(F32) + (s[2] * v[2]).astype(F32)
        xc, yc, zc = dot(R).astype(F32), dot(U).astype(F32), dot(Fw).astype(F32)
        px = (((((kx * xc).astype(F32) / zc).astype(F32) + F32(1)).astype(F32) * F32(0.5)).astype(F32) * F32(w)).astype(F32) - F32(0.5)
        py = ((((F32(1) - ((ky * yc).astype(F32) / zc).astype(F32)).astype(F32)) * F32(0.5)).astype(F32) * F32(h)).astype(F32) - F32(0.5)
        zexp = np.sqrt(((s[0] * s[0]).astype(F32) + (s[1] * s[1]).astype(F32)).astype(F32) + (s[2] * s[2]).astype(F32)).astype(F32)
    return px.astype(F32), py.astype(F32), zexp, zc


def _within(v, bound, tol):
    return np.full(v.shape, True) if tol == np.inf else (v <= bound)


def temporal_accumulate(color, half, feat, prev=None, cam=None, prev_cam=None, rays=None, alpha_min=DEFAULTS["alpha_min"],
                        max_history=DEFAULTS["max_history"], depth_tol=DEFAULTS["depth_tol"], normal_tol=DEFAULTS["normal_tol"],
                        albedo_tol=DEFAULTS["albedo_tol"]):
    """The whole rule: (out, out_half, history).  half may be None (then out_half is None).  prev: None on the first frame, else a
    dict with the previous call's color, half (None iff half is), history and the features feat it was accumulated with; then cam
    and prev_cam are wanted, and rays unless the two cameras are the same bytes."""
    color = np.ascontiguousarray(color, F32)
    feat = np.ascontiguousarray(feat, F32)
    use_half = half is not None
    half = np.ascontiguousarray(half, F32) if use_half else color
    h, w, _ = color.shape
    alpha_min, max_history, depth_tol, normal_tol, albedo_tol = (F32(v) for v in (alpha_min, max_history, depth_tol, normal_tol, albedo_tol))
    x, d = demodulate(color, feat)
    xh, _ = demodulate(half, feat)
    cov = feat[..., 10]
    out, out_half, hist = color.copy(), half.copy(), np.ones((h, w), F32)
    if prev is None:
        return out, (out_half if use_half else None), hist
    go = _finite3(x) & _finite3(xh) & ~(cov == 0)
    pc, pf, ph = np.ascontiguousarray(prev["color"], F32), np.ascontiguousarray(prev["feat"], F32), np.ascontiguousarray(prev["history"], F32)
    pch = np.ascontiguousarray(prev["half"], F32) if use_half else pc
    with np.errstate(all="ignore"):
        zbar = (feat[..., 9] / cov).astype(F32)
        if same_camera(cam, prev_cam):
            ys, xs = np.mgrid[0:h, 0:w]
            px, py, zexp = xs.astype(F32), ys.astype(F32), zbar
        else:
            px, py, zexp, zc = project(rays, zbar, prev_cam, w, h)
            go = go & (zc > 0)
        # what every pixel of the previous frame offers as a tap
        xq_all, _ = demodulate(pc, pf)
        xhq_all, _ = demodulate(pch, pf)
        tap_ok = _finite3(xq_all) & _finite3(xhq_all) & np.isfinite(pf[..., 10]) & (pf[..., 10] > 0) & (ph >= 1)
        zq_all = (pf[..., 9] / pf[..., 10]).astype(F32)
        ix, iy = np.floor(px).astype(F32), np.floor(py).astype(F32)
        fx, fy = (px - ix).astype(F32), (py - iy).astype(F32)
        gx, gy = (F32(1) - fx).astype(F32), (F32(1) - fy).astype(F32)
        weights = [(gx * gy).astype(F32), (fx * gy).astype(F32), (gx * fy).astype(F32), (fx * fy).astype(F32)]
        zlim = (depth_tol * np.fmax(zexp, F32(1e-3))).astype(F32)
        sw, sn = np.zeros((h, w), F32), np.zeros((h, w), F32)
        sx, sxh = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
        for t in range(4):
            qx, qy = (ix + F32(t & 1)).astype(F32), (iy + F32(t >> 1)).astype(F32)
            inside = (qx >= 0) & (qx < F32(w)) & (qy >= 0) & (qy < F32(h))
            jx, jy = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
            g, hq = pf[jy, jx], ph[jy, jx]
            use = go & inside & tap_ok[jy, jx]
            use &= _within(np.abs(zexp - zq_all[jy, jx]).astype(F32), zlim, depth_tol)
            use &= _within(_sq3((feat[..., 3:6] - g[..., 3:6]).astype(F32)).astype(F32), normal_tol, normal_tol)
            use &= _within(_sq3((feat[..., 0:3] - g[..., 0:3]).astype(F32)).astype(F32), albedo_tol, albedo_tol)
            wq = weights[t]
            sw = np.where(use, sw + wq, sw).astype(F32)
            sx = np.where(use[..., None], sx + (wq[..., None] * xq_all[jy, jx]).astype(F32), sx).astype(F32)
            sxh = np.where(use[..., None], sxh + (wq[..., None] * xhq_all[jy, jx]).astype(F32), sxh).astype(F32)
            sn = np.where(use, sn + (wq * hq).astype(F32), sn).astype(F32)
        go = go & (sw > 0)
        n_new = np.fmin(((sn / sw).astype(F32) + F32(1)).astype(F32), max_history).astype(F32)
        alpha = np.fmax((F32(1) / n_new).astype(F32), alpha_min).astype(F32)[..., None]
        e6 = (feat[..., 6:9] / F32(6)).astype(F32)

        def blend(xp, s):
            xhist = (s / sw[..., None]).astype(F32)
            y = (xhist + (alpha * (xp - xhist).astype(F32)).astype(F32)).astype(F32)
            return ((d * y).astype(F32) + e6).astype(F32)

        r, rh = blend(x, sx), blend(xh, sxh)
        go = go & _finite3(r) & _finite3(rh)
    out = np.where(go[..., None], r, color).astype(F32)
    out_half = np.where(go[..., None], rh, half).astype(F32)
    hist = np.where(go, n_new, F32(1)).astype(F32)
    return out, (out_half if use_half else None), hist
