"""The variance-guided denoiser's entry points without a GPU: they are exported, and every bad parameter is refused with
HRT_ERR_INVALID and a message that names it, before the library state is looked at (include/hrt.h hrt_denoise_var)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

HRT_ERR_INVALID = -1
NAMES = ["hrt_denoise_var_scratch_bytes", "hrt_denoise_var", "hrt_render_denoised_var"]
DUMMY = 0x1000  # a device pointer that is never dereferenced: every call below fails validation first


def test_libhrt_exports_the_entry_points(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for n in NAMES:
        assert hasattr(dev, n) and n in exported


def test_scratch_size_and_the_structs_layout(hrt):
    assert hrt.denoise_var_scratch_bytes(1920, 1080) == 64 * 1920 * 1080
    assert hrt.denoise_var_scratch_bytes(1, 1) == 64
    assert C.sizeof(hrt.DenoiseVarParams) == 28
    p = hrt.DenoiseVarParams()
    assert 1 <= p.iterations <= 8 and p.prefilter <= 4 and p.sigma_variance > 0 and p.variance_floor >= 0


def default(hrt, **kw):
    p = hrt.DenoiseVarParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [
    (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(prefilter=5), "prefilter"),
    (dict(sigma_variance=0.0), "sigma_variance"), (dict(sigma_variance=-1.0), "sigma_variance"), (dict(sigma_variance=math.nan), "sigma_variance"),
    (dict(sigma_normal=0.0), "sigma_normal"), (dict(sigma_normal=math.nan), "sigma_normal"), (dict(sigma_normal=-math.inf), "sigma_normal"),
    (dict(sigma_albedo=-0.5), "sigma_albedo"), (dict(sigma_albedo=math.nan), "sigma_albedo"),
    (dict(sigma_depth=0.0), "sigma_depth"), (dict(sigma_depth=math.nan), "sigma_depth"),
    (dict(variance_floor=-1e-9), "variance_floor"), (dict(variance_floor=math.inf), "variance_floor"), (dict(variance_floor=math.nan), "variance_floor"),
]


def filter_call(hrt, p, w=64, h=36, flags=0, color=DUMMY, half=DUMMY, feat=DUMMY, scratch=DUMMY, out=DUMMY, var=0):
    dev = hrt.device_lib()
    rc = dev.hrt_denoise_var(C.c_void_p(color), C.c_void_p(half), C.c_void_p(feat), w, h, None if p is None else C.byref(p), flags,
                             C.c_void_p(scratch), C.c_void_p(out), C.c_void_p(var), None)
    return rc, dev.hrt_last_error().decode()


def render_call(hrt, p, w=64, h=36, spp=4, feature_spp=1, flags=0, cam=True, out=True):
    dev = hrt.device_lib()
    camera = hrt.default_camera(64 / 36) if cam else None
    buf = np.empty((max(h, 1), max(w, 1), 3), np.float32)
    rc = dev.hrt_render_denoised_var(None, None if camera is None else C.byref(camera), w, h, spp, feature_spp, 1, flags,
                                     None if p is None else C.byref(p), buf.ctypes.data if out else None, None, None)
    return rc, dev.hrt_last_error().decode()


@pytest.mark.parametrize("kw,field", BAD_PARAMS)
def test_bad_filter_parameters_are_refused_and_named(hrt, kw, field):
    for entry, call in (("hrt_denoise_var", filter_call), ("hrt_render_denoised_var", render_call)):
        rc, msg = call(hrt, default(hrt, **kw))
        assert rc == HRT_ERR_INVALID
        assert field in msg and entry in msg, msg


def test_bad_denoise_var_arguments_are_refused_and_named(hrt):
    p = default(hrt)
    for kw, word in ((dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(flags=2), "flags"), (dict(flags=1 << 20), "flags"),
                     (dict(color=0), "d_color"), (dict(half=0), "d_color_half"), (dict(feat=0), "d_features"), (dict(scratch=0), "d_scratch"),
                     (dict(out=0), "d_out")):
        rc, msg = filter_call(hrt, p, **kw)
        assert rc == HRT_ERR_INVALID and word in msg and "hrt_denoise_var" in msg, (kw, msg)
    rc, msg = filter_call(hrt, None)
    assert rc == HRT_ERR_INVALID and "params" in msg, msg


def test_bad_render_denoised_var_arguments_are_refused_and_named(hrt):
    p = default(hrt)
    for kw, word in ((dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(spp=0), "spp"), (dict(spp=1), "spp"), (dict(spp=7), "spp"),
                     (dict(spp=4, feature_spp=5), "feature_spp"), (dict(cam=False), "camera"), (dict(out=False), "out_rgb")):
        rc, msg = render_call(hrt, p, **kw)
        assert rc == HRT_ERR_INVALID and word in msg and "hrt_render_denoised_var" in msg, (kw, msg)
    rc, msg = render_call(hrt, None)
    assert rc == HRT_ERR_INVALID and "params" in msg, msg
    # valid arguments get past validation: the call then fails on the NULL scene, and says so
    for q in (default(hrt), default(hrt, iterations=8, prefilter=0, sigma_variance=math.inf, sigma_normal=math.inf, sigma_albedo=math.inf,
                                    sigma_depth=math.inf, variance_floor=0.0),
              default(hrt, prefilter=4)):
        rc, msg = render_call(hrt, q, spp=4, feature_spp=4)
        assert rc == HRT_ERR_INVALID and "scene" in msg, msg
