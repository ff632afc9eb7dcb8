"""Denoising entry points without a GPU: they are exported, and every bad parameter is refused with HRT_ERR_INVALID and a message
that names it, before any device call (include/hrt.h hrt_denoise)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

HRT_ERR_INVALID = -1
NAMES = ["hrt_render_features", "hrt_denoise_scratch_bytes", "hrt_denoise", "hrt_render_denoised"]
DUMMY = 0x1000  # a device pointer that is never dereferenced: every call below fails validation first


def test_libhrt_exports_the_denoising_entry_points(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for n in NAMES:
        assert hasattr(dev, n) and n in exported


def test_scratch_size(hrt):
    assert hrt.denoise_scratch_bytes(1920, 1080) == 64 * 1920 * 1080
    assert hrt.denoise_scratch_bytes(1, 1) == 64


def default(hrt, **kw):
    p = hrt.DenoiseParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [
    (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"),
    (dict(sigma_color=0.0), "sigma_color"), (dict(sigma_color=-1.0), "sigma_color"), (dict(sigma_color=math.nan), "sigma_color"),
    (dict(sigma_normal=0.0), "sigma_normal"), (dict(sigma_normal=math.nan), "sigma_normal"), (dict(sigma_normal=-math.inf), "sigma_normal"),
    (dict(sigma_albedo=-0.5), "sigma_albedo"), (dict(sigma_albedo=math.nan), "sigma_albedo"),
    (dict(sigma_depth=0.0), "sigma_depth"), (dict(sigma_depth=math.nan), "sigma_depth"),
]


def denoise_call(hrt, p, w=64, h=36, flags=0, color=DUMMY, feat=DUMMY, scratch=DUMMY, out=DUMMY):
    dev = hrt.device_lib()
    rc = dev.hrt_denoise(C.c_void_p(color), C.c_void_p(feat), w, h, None if p is None else C.byref(p), flags, C.c_void_p(scratch),
                         C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def denoised_call(hrt, p, w=64, h=36, spp=4, feature_spp=1, cam=True, out=True):
    dev = hrt.device_lib()
    camera = hrt.default_camera(64 / 36) if cam else None
    buf = np.empty((max(h, 1), max(w, 1), 3), np.float32)
    rc = dev.hrt_render_denoised(None, None if camera is None else C.byref(camera), w, h, spp, feature_spp, 1, 0,
                                 None if p is None else C.byref(p), buf.ctypes.data if out else None, None)
    return rc, dev.hrt_last_error().decode()


@pytest.mark.parametrize("kw,field", BAD_PARAMS)
def test_bad_filter_parameters_are_refused_and_named(hrt, kw, field):
    for entry, call in (("hrt_denoise", denoise_call), ("hrt_render_denoised", denoised_call)):
        rc, msg = call(hrt, default(hrt, **kw))
        assert rc == HRT_ERR_INVALID
        assert field in msg and entry in msg, msg


def test_bad_denoise_arguments_are_refused_and_named(hrt):
    p = default(hrt)
    for kw, word in ((dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(flags=2), "flags"), (dict(color=0), "d_color"),
                     (dict(feat=0), "d_features"), (dict(scratch=0), "d_scratch"), (dict(out=0), "d_out")):
        rc, msg = denoise_call(hrt, p, **kw)
        assert rc == HRT_ERR_INVALID and word in msg and "hrt_denoise" in msg, (kw, msg)
    rc, msg = denoise_call(hrt, None)
    assert rc == HRT_ERR_INVALID and "params" in msg, msg


def test_bad_render_denoised_arguments_are_refused_and_named(hrt):
    p = default(hrt)
    for kw, word in ((dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(spp=0), "spp"), (dict(spp=4, feature_spp=5), "feature_spp"),
                     (dict(cam=False), "camera"), (dict(out=False), "out_rgb")):
        rc, msg = denoised_call(hrt, p, **kw)
        assert rc == HRT_ERR_INVALID and word in msg and "hrt_render_denoised" in msg, (kw, msg)
    rc, msg = denoised_call(hrt, None)
    assert rc == HRT_ERR_INVALID and "params" in msg, msg
    # valid arguments get past validation: the call then fails on the NULL scene, and says so
    for p in (default(hrt), default(hrt, iterations=8, sigma_color=math.inf, sigma_normal=math.inf, sigma_albedo=math.inf, sigma_depth=math.inf)):
        rc, msg = denoised_call(hrt, p, spp=4, feature_spp=4)
        assert rc == HRT_ERR_INVALID and "scene" in msg, msg


def test_bad_render_features_arguments_are_refused_and_named(hrt):
    dev = hrt.device_lib()
    cam = hrt.default_camera(64 / 36)

    def call(camera=True, w=64, h=36, first=0, n=1, out=DUMMY):
        rc = dev.hrt_render_features(None, C.byref(cam) if camera else None, w, h, first, n, 1, C.c_void_p(out), None)
        return rc, dev.hrt_last_error().decode()

    for kw, word in ((dict(camera=False), "camera"), (dict(w=0), "w and h"), (dict(h=0), "w and h"),
                     (dict(first=0xFFFFFFFF, n=2), "first_sample"), (dict(out=0), "d_features"), (dict(), "scene")):
        rc, msg = call(**kw)
        assert rc == HRT_ERR_INVALID and word in msg and "hrt_render_features" in msg, (kw, msg)
