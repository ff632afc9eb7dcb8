"""Temporal accumulation's entry points without a GPU (include/hrt.h hrt_temporal_accumulate, hrt_history_*, hrt_render_temporal):
they are exported, and every bad argument is refused with HRT_ERR_INVALID and a message that names the entry point and the culprit,
before any device state exists."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

HRT_ERR_INVALID = -1
NAMES = ["hrt_temporal_accumulate", "hrt_history_create", "hrt_history_reset", "hrt_history_destroy", "hrt_render_temporal"]
DUMMY = 0x1000  # device pointers that are never dereferenced: every call below fails validation first
PTRS = dict(color=DUMMY, half=2 * DUMMY, feat=3 * DUMMY, pcolor=4 * DUMMY, phalf=5 * DUMMY, pfeat=6 * DUMMY, phist=7 * DUMMY,
            out=8 * DUMMY, out_half=9 * DUMMY, hist_out=10 * DUMMY)


def test_libhrt_exports_the_entry_points(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for n in NAMES:
        assert hasattr(dev, n) and n in exported


def test_the_params_layout_and_defaults(hrt):
    assert C.sizeof(hrt.TemporalParams) == 20
    p = hrt.TemporalParams()
    assert 0 < p.alpha_min <= 1 and p.max_history >= 1 and p.depth_tol > 0 and p.normal_tol > 0 and p.albedo_tol > 0
    import temporal_ref as tr
    for k, v in tr.DEFAULTS.items():
        assert np.float32(getattr(p, k)) == np.float32(v), k


def default(hrt, **kw):
    p = hrt.TemporalParams()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def accumulate_call(hrt, p, w=64, h=36, cam=True, prev_cam=True, **ptrs):
    dev = hrt.device_lib()
    a = dict(PTRS, **ptrs)
    c = (hrt.default_camera(64 / 36) if cam is True else cam) if cam else None
    pc = (hrt.default_camera(64 / 36) if prev_cam is True else prev_cam) if prev_cam else None
    v = lambda k: C.c_void_p(a[k]) if a[k] else None
    rc = dev.hrt_temporal_accumulate(None if c is None else C.byref(c), None if pc is None else C.byref(pc), w, h, v("color"), v("half"),
                                     v("feat"), v("pcolor"), v("phalf"), v("pfeat"), v("phist"), None if p is None else C.byref(p),
                                     v("out"), v("out_half"), v("hist_out"), None)
    return rc, dev.hrt_last_error().decode()


def render_call(hrt, p, w=64, h=36, spp=4, feature_spp=1, cam=True, out=True, dp=None, hist=DUMMY):
    dev = hrt.device_lib()
    camera = hrt.default_camera(64 / 36) if cam else None
    buf = np.empty((max(h, 1), max(w, 1), 3), np.float32)
    rc = dev.hrt_render_temporal(None, C.c_void_p(hist) if hist else None, None if camera is None else C.byref(camera), w, h, spp, feature_spp, 1, 0,
                                 None if p is None else C.byref(p), None if dp is None else C.byref(dp),
                                 buf.ctypes.data if out else None, None, None)
    return rc, dev.hrt_last_error().decode()


BAD_PARAMS = [
    (dict(alpha_min=0.0), "alpha_min"), (dict(alpha_min=-0.5), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=math.nan), "alpha_min"),
    (dict(alpha_min=math.inf), "alpha_min"),
    (dict(max_history=0.5), "max_history"), (dict(max_history=math.nan), "max_history"), (dict(max_history=math.inf), "max_history"),
    (dict(max_history=-math.inf), "max_history"),
    (dict(depth_tol=0.0), "depth_tol"), (dict(depth_tol=-1.0), "depth_tol"), (dict(depth_tol=math.nan), "depth_tol"),
    (dict(normal_tol=0.0), "normal_tol"), (dict(normal_tol=math.nan), "normal_tol"), (dict(normal_tol=-math.inf), "normal_tol"),
    (dict(albedo_tol=-0.5), "albedo_tol"), (dict(albedo_tol=0.0), "albedo_tol"), (dict(albedo_tol=math.nan), "albedo_tol"),
]


@pytest.mark.parametrize("kw,field", BAD_PARAMS)
def test_bad_parameters_are_refused_and_named(hrt, kw, field):
    for entry, call in (("hrt_temporal_accumulate", accumulate_call), ("hrt_render_temporal", render_call)):
        rc, msg = call(hrt, default(hrt, **kw))
        assert rc == HRT_ERR_INVALID
        assert field in msg and entry in msg, msg


BAD_POINTERS = [
    (dict(color=0), "d_color"), (dict(feat=0), "d_features"), (dict(out=0), "d_out"), (dict(hist_out=0), "d_history_out"),
    (dict(out_half=0), "d_out_half"), (dict(half=0), "d_out_half"),                    # one of the pair without the other
    (dict(half=0, out_half=0), "d_prev_color_half"),                                   # a previous half frame without a current one
    (dict(phalf=0), "d_prev_color_half"), (dict(pcolor=0), "d_prev_color"), (dict(pfeat=0), "d_prev_features"),
    (dict(phist=0), "d_prev_history"), (dict(prev_cam=None), "prev_cam"),
    (dict(prev_cam=None, pcolor=0, phalf=0, pfeat=0), "prev_cam"),                     # one stray d_prev_ pointer on a first frame
    (dict(cam=None), "cam"),
    (dict(out=PTRS["color"]), "alias"), (dict(out_half=PTRS["pfeat"]), "alias"), (dict(hist_out=PTRS["phist"]), "alias"),
    (dict(hist_out=PTRS["out"]), "alias"),
    (dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(w=65536, h=65536), "too large"),
]


@pytest.mark.parametrize("kw,word", BAD_POINTERS)
def test_bad_accumulate_arguments_are_refused_and_named(hrt, kw, word):
    rc, msg = accumulate_call(hrt, default(hrt), **kw)
    assert rc == HRT_ERR_INVALID and word in msg and "hrt_temporal_accumulate" in msg, (kw, msg)


def test_null_params_and_the_frame_limit_of_the_denoisers(hrt):
    rc, msg = accumulate_call(hrt, None)
    assert rc == HRT_ERR_INVALID and "params" in msg and "hrt_temporal_accumulate" in msg, msg
    lim = 0x7fffffff // 16
    rc, msg = accumulate_call(hrt, default(hrt), w=lim + 1, h=1)
    assert rc == HRT_ERR_INVALID and "too large" in msg, msg
    rc, msg = accumulate_call(hrt, default(hrt), w=lim, h=1, hist_out=0)  # the largest frame passes: the call gets to its last check
    assert rc == HRT_ERR_INVALID and "d_history_out" in msg, msg


def bad_cameras(hrt):
    out = []
    c = hrt.default_camera(16 / 9); c.fovy_deg = 0.0; out.append(("fovy 0", c))
    c = hrt.default_camera(16 / 9); c.aspect = float("inf"); out.append(("infinite aspect", c))
    c = hrt.default_camera(16 / 9); c.eye[0] = float("nan"); out.append(("NaN eye", c))
    c = hrt.default_camera(16 / 9); c.right[:] = (0, 0, 0); out.append(("zero right", c))
    c = hrt.default_camera(16 / 9); c.znear = c.zfar = 1.0; out.append(("znear == zfar", c))
    return out


@pytest.mark.parametrize("which", ["cam", "prev_cam"])
def test_a_camera_render_refuses_is_refused_and_named(hrt, which):
    for what, cam in bad_cameras(hrt):
        rc, msg = accumulate_call(hrt, default(hrt), **{which: cam})
        assert rc == HRT_ERR_INVALID and "hrt_temporal_accumulate" in msg and which + ":" in msg, (what, msg)


def test_valid_arguments_get_past_validation(hrt):
    # with and without the half frame, on a first frame and on a later one, every tolerance off: the call then gets to its last
    # check, the history output, which is NULL here (nothing is ever launched on these pointers)
    wide = default(hrt, alpha_min=1.0, max_history=1.0, depth_tol=math.inf, normal_tol=math.inf, albedo_tol=math.inf)
    first = dict(prev_cam=None, pcolor=0, phalf=0, pfeat=0, phist=0)
    for p in (default(hrt), wide):
        for kw in ({}, dict(half=0, out_half=0, phalf=0), first, dict(first, half=0, out_half=0)):
            rc, msg = accumulate_call(hrt, p, hist_out=0, **kw)
            assert rc == HRT_ERR_INVALID and "d_history_out is NULL" in msg, (kw, msg)


def test_bad_render_temporal_arguments_are_refused_and_named(hrt):
    p = default(hrt)
    for kw, word in ((dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(spp=0), "spp"), (dict(spp=1), "spp"), (dict(spp=7), "spp"),
                     (dict(spp=4, feature_spp=5), "feature_spp"), (dict(cam=False), "camera"), (dict(out=False), "out_rgb"),
                     (dict(hist=0), "history"), (dict(dp=hrt.DenoiseVarParams(iterations=9)), "iterations"),
                     (dict(dp=hrt.DenoiseVarParams(sigma_variance=math.nan)), "sigma_variance")):
        rc, msg = render_call(hrt, p, **kw)
        assert rc == HRT_ERR_INVALID and word in msg and "hrt_render_temporal" in msg, (kw, msg)
    rc, msg = render_call(hrt, None)
    assert rc == HRT_ERR_INVALID and "params" in msg, msg
    for dp in (None, hrt.DenoiseVarParams()):  # valid arguments: the call then fails on the NULL scene, and says so
        rc, msg = render_call(hrt, p, spp=4, feature_spp=4, dp=dp)
        assert rc == HRT_ERR_INVALID and "scene" in msg, msg


def test_history_entry_points_refuse_null(hrt):
    dev = hrt.device_lib()
    h = C.c_void_p()
    assert dev.hrt_history_create(None, C.byref(h)) == HRT_ERR_INVALID and "scene" in dev.hrt_last_error().decode()
    assert not h
    assert dev.hrt_history_create(None, None) == HRT_ERR_INVALID and "out" in dev.hrt_last_error().decode()
    dev.hrt_history_reset(None)    # both accept NULL, as hrt_scene_destroy does
    dev.hrt_history_destroy(None)
