"""Path features without a GPU (include/hrt.h "Path features"): the six entry points are exported and declared and the constants are
the header's; every bad argument that can be reached without a device is refused with HRT_ERR_INVALID and a message that names the
entry point and the culprit, in the header's order -- n_samples == 0, a bad `guides` value and feature_spp == 0 with
HRT_GUIDES_FIRST_DIFFUSE among them; an empty batch launches nothing; the Python wrappers and the command-line tool refuse before
they touch a device.  The device pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import probe_volume_ref as pv
from conftest import PKG, ROOT

HRT_OK, HRT_ERR_INVALID, HRT_ERR_STATE = 0, -1, -2
RAYS, KEYS, OUT = 0x1000, 0x3000, 0x2000
EXACT, BRUTE, NO_LDS, NORMALIZE, ACCUMULATE = 64, 128, 2, 256, 512
NAMES = ["hrt_path_features", "hrt_render_path_features", "hrt_render_lens_path_features", "hrt_render_lens_views_path_features",
         "hrt_render_denoised_guides", "hrt_render_denoised_var_guides"]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
NO_STREAM = "n_samples must be positive (a pixel-centre path has no stream)"


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_headers_constants_and_scope(hrt):
    text = pv.header_text()
    assert re.search(r"#define HRT_GUIDES_FIRST_HIT +0u(\s|$)", text) and hrt.GUIDES_FIRST_HIT == 0
    assert re.search(r"#define HRT_GUIDES_FIRST_DIFFUSE +1u(\s|$)", text) and hrt.GUIDES_FIRST_DIFFUSE == 1
    assert re.search(r"#define HRT_FEATURE_FLOATS +12(\s|$)", text) and hrt.FEATURE_FLOATS == 12
    assert text.index("/* ---- Lit paths:") < text.index("/* ---- Path features:"), "the section comes after \"Lit paths\""
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Path features\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("pixel-centre paths", "temporal accumulation", "hrt_render_temporal", "virtual (mirrored) normal", "K > 1"):
        assert item in scope, item
    assert "n_samples == 0 is REFUSED" in text


# ------------------------------------------------------------------------------------------------------------ hrt_path_features
def query(hrt, scene=None, rays=RAYS, keys=None, n=5, sample=0, seed=1, flags=0, out=OUT):
    dev = hrt.device_lib()
    k = None if keys is None else C.c_void_p(keys)
    rc = dev.hrt_path_features(scene, C.c_void_p(rays), k, n, sample, seed, flags, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


EVERY = dict(rays=0, keys=KEYS + 2, n=2 ** 31, out=0)  # everything after the flags wrong at once


@pytest.mark.parametrize("bit", range(32))
def test_the_flags_of_a_query_are_checked_first(hrt, bit):
    entry, flag = "hrt_path_features", 1 << bit
    rc, msg = query(hrt, flags=flag | (EXACT if flag == BRUTE else 0), **EVERY)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": "), msg
    if flag in (EXACT, BRUTE, NO_LDS, NORMALIZE):
        assert msg == entry + ": d_rays is NULL", (bit, msg)
    else:
        assert msg == f"{entry}: unknown flags bits {flag}", (bit, msg)
    rc, msg = query(hrt, flags=BRUTE, **EVERY)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg


def test_path_features_refuses_in_the_headers_order(hrt):
    entry = "hrt_path_features"
    assert query(hrt, **dict(EVERY, n=0)) [0] == HRT_OK, "an empty batch launches nothing"
    assert query(hrt, flags=ACCUMULATE, **dict(EVERY, n=0))[0] == HRT_ERR_INVALID, "the flags are checked for an empty batch, too"
    fixed = dict(EVERY)
    assert query(hrt, **fixed) == (HRT_ERR_INVALID, entry + ": d_rays is NULL")
    fixed["rays"] = RAYS + 8
    assert query(hrt, **fixed) == (HRT_ERR_INVALID, entry + ": d_rays is not 16-byte aligned")
    fixed["rays"] = RAYS
    assert query(hrt, **fixed) == (HRT_ERR_INVALID, entry + ": d_keys is not 4-byte aligned")
    fixed["keys"] = KEYS
    assert query(hrt, **fixed) == (HRT_ERR_INVALID, entry + ": d_out is NULL")
    for off in (1, 2, 3):
        fixed["out"] = OUT + off
        assert query(hrt, **fixed) == (HRT_ERR_INVALID, entry + ": d_out is not 4-byte aligned"), off
    fixed["out"] = OUT + 4  # a record is 48 bytes: 4-byte alignment is all it needs
    assert query(hrt, **fixed)[1].startswith(entry + ": n must be at most 2^31 - 1")
    fixed["n"] = 5
    assert query(hrt, **fixed) == (HRT_ERR_INVALID, entry + ": scene is NULL")


# ------------------------------------------------------------------------------------------------------------ the frame forms
def good_lens(hrt, **kw):
    return hrt.Lens(hrt.default_camera(19 / 11), **kw)


def lens_frame(hrt, lens, scene=None, w=19, h=11, first=0, n=5, seed=1, out=OUT):
    dev = hrt.device_lib()
    rc = dev.hrt_render_lens_path_features(scene, None if lens is None else C.byref(lens), w, h, first, n, seed, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def test_the_lens_frame_refuses_in_the_order_of_its_first_hit_sibling(hrt):
    entry = "hrt_render_lens_path_features"
    late = dict(w=0, n=0, first=2 ** 32 - 1, out=0)  # everything after the lens wrong at once
    assert lens_frame(hrt, None, **late) == (HRT_ERR_INVALID, entry + ": lens is NULL")
    bad = good_lens(hrt, projection="fisheye", extent=400.0)
    assert lens_frame(hrt, bad, **late)[1].startswith(entry + ": extent must be in (0, 360]")
    bad = good_lens(hrt)
    bad.projection = 9
    assert lens_frame(hrt, bad, **late)[1].startswith(entry + ": projection must be")
    lens = good_lens(hrt)
    rc, msg = lens_frame(hrt, lens, **late)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": ") and "n_samples" not in msg, ("the frame comes before the samples", msg)
    late["w"] = 19
    assert lens_frame(hrt, lens, **late) == (HRT_ERR_INVALID, f"{entry}: {NO_STREAM}")
    late["n"] = 1
    assert lens_frame(hrt, lens, **late) == (HRT_ERR_INVALID, entry + ": first_sample + n_samples overflows 32 bits")
    late["first"] = 2 ** 32 - 2
    assert lens_frame(hrt, lens, **late) == (HRT_ERR_INVALID, entry + ": d_features is NULL")
    late["out"] = OUT + 2
    assert lens_frame(hrt, lens, **late) == (HRT_ERR_INVALID, entry + ": d_features is not 4-byte aligned")
    late["out"] = OUT
    assert lens_frame(hrt, lens, **late) == (HRT_ERR_INVALID, entry + ": scene is NULL")
    # the first-hit sibling takes n_samples == 0 (the pixel centres) and goes on to the scene
    dev = hrt.device_lib()
    assert dev.hrt_render_lens_features(None, C.byref(lens), 19, 11, 0, 0, 1, C.c_void_p(OUT), None) == HRT_ERR_INVALID
    assert dev.hrt_last_error().decode() == "hrt_render_lens_features: scene is NULL"


def camera_frame(hrt, cam, scene=None, w=19, h=11, first=0, n=5, seed=1, out=OUT):
    dev = hrt.device_lib()
    rc = dev.hrt_render_path_features(scene, None if cam is None else C.byref(cam), w, h, first, n, seed, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def test_the_camera_frame_refuses_in_the_order_of_its_first_hit_sibling(hrt):
    entry = "hrt_render_path_features"
    late = dict(w=0, n=0, first=2 ** 32 - 1, out=0)
    assert camera_frame(hrt, None, **late) == (HRT_ERR_INVALID, entry + ": camera is NULL")
    cam = hrt.default_camera(19 / 11)
    rc, msg = camera_frame(hrt, cam, **late)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": ") and "n_samples" not in msg, msg
    late["w"] = 19
    assert camera_frame(hrt, cam, **late) == (HRT_ERR_INVALID, f"{entry}: {NO_STREAM}")
    late["n"] = 1
    assert camera_frame(hrt, cam, **late) == (HRT_ERR_INVALID, entry + ": first_sample + n_samples overflows 32 bits")
    late["first"] = 0
    assert camera_frame(hrt, cam, **late) == (HRT_ERR_INVALID, entry + ": d_features is NULL")
    late["out"] = OUT
    assert camera_frame(hrt, cam, **late) == (HRT_ERR_INVALID, entry + ": scene is NULL")


def views_frame(hrt, views, n_views, scene=None, w=19, h=11, first=0, n=5, out=OUT):
    dev = hrt.device_lib()
    rc = dev.hrt_render_lens_views_path_features(scene, views, n_views, w, h, first, n, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def test_the_batch_refuses_in_the_order_of_its_first_hit_sibling(hrt):
    entry = "hrt_render_lens_views_path_features"
    late = dict(w=0, n=0, first=2 ** 32 - 1, out=0)
    assert views_frame(hrt, None, 0, **late)[0] == HRT_OK, "an empty batch launches nothing, whatever else is wrong"
    assert views_frame(hrt, None, 2, **late) == (HRT_ERR_INVALID, entry + ": views is NULL")
    views = (hrt.LensView * 2)()
    views[0].lens, views[0].seed = good_lens(hrt), 1
    views[1].lens, views[1].seed = good_lens(hrt, projection="ortho", extent=-1.0), 2
    rc, msg = views_frame(hrt, views, 2, **late)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": views[1].lens: extent must be finite and > 0"), msg
    views[1].lens = good_lens(hrt, projection="equirect")
    rc, msg = views_frame(hrt, views, 2, **late)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": ") and "n_samples" not in msg and "views[" not in msg, msg
    late["w"] = 19
    assert views_frame(hrt, views, 2, **late) == (HRT_ERR_INVALID, f"{entry}: {NO_STREAM}")
    late["n"] = 1
    assert views_frame(hrt, views, 2, **late) == (HRT_ERR_INVALID, entry + ": first_sample + n_samples overflows 32 bits")
    late["first"] = 3
    assert views_frame(hrt, views, 2, **late) == (HRT_ERR_INVALID, entry + ": d_features is NULL")
    late["out"] = OUT + 1
    assert views_frame(hrt, views, 2, **late) == (HRT_ERR_INVALID, entry + ": d_features is not 4-byte aligned")
    late["out"] = OUT
    rc, msg = views_frame(hrt, views, 2, **dict(late, w=2 ** 14, h=2 ** 12))  # 2 x 2^26 items, above 2^31 / 16
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": n_views * w * h is 134217728, above the"), msg
    assert views_frame(hrt, views, 2, **late) == (HRT_ERR_INVALID, entry + ": scene is NULL")


# ---------------------------------------------------------------------------------------------------------- the guided renders
def guided(hrt, var, guides, cam="default", params="default", scene=None, w=19, h=11, spp=4, feature_spp=2, out=OUT):
    dev = hrt.device_lib()
    cam = hrt.default_camera(19 / 11) if cam == "default" else cam
    p = (hrt.DenoiseVarParams() if var else hrt.DenoiseParams()) if params == "default" else params
    c, pp = (None if cam is None else C.byref(cam)), (None if p is None else C.byref(p))
    if var:
        rc = dev.hrt_render_denoised_var_guides(scene, c, w, h, spp, feature_spp, 1, 0, guides, pp, C.c_void_p(out), None, None)
    else:
        rc = dev.hrt_render_denoised_guides(scene, c, w, h, spp, feature_spp, 1, 0, guides, pp, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


@pytest.mark.parametrize("var", [False, True])
def test_the_guided_renders_refuse_guides_and_feature_spp_by_name(hrt, var):
    entry = "hrt_render_denoised_var_guides" if var else "hrt_render_denoised_guides"
    late = dict(cam=None, out=0, feature_spp=9)  # what the existing functions check after their parameters, frame and spp
    for bad in (2, 3, 255, 2 ** 32 - 1):
        assert guided(hrt, var, bad, **late) == (HRT_ERR_INVALID, f"{entry}: guides must be HRT_GUIDES_FIRST_HIT or HRT_GUIDES_FIRST_DIFFUSE (got {bad})")
    want = f"{entry}: feature_spp must be at least 1 with HRT_GUIDES_FIRST_DIFFUSE (a pixel-centre path has no stream)"
    assert guided(hrt, var, hrt.GUIDES_FIRST_DIFFUSE, **dict(late, feature_spp=0)) == (HRT_ERR_INVALID, want)
    # the existing functions' checks around them, under the new names: the parameters, the frame and spp before, the rest after
    assert guided(hrt, var, 7, params=None, **late) == (HRT_ERR_INVALID, entry + ": params is NULL")
    assert guided(hrt, var, 7, w=0, **late) == (HRT_ERR_INVALID, entry + ": w and h must be positive (got 0 x 11)")
    rc, msg = guided(hrt, var, 7, spp=0, **late)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": spp must be") , msg
    for g in (hrt.GUIDES_FIRST_HIT, hrt.GUIDES_FIRST_DIFFUSE):
        assert guided(hrt, var, g, **late)[1].startswith(entry + ": feature_spp must be at most spp (got 9 > 4)"), g
        assert guided(hrt, var, g, **dict(late, feature_spp=1)) == (HRT_ERR_INVALID, entry + ": camera is NULL"), g
        assert guided(hrt, var, g, out=0) == (HRT_ERR_INVALID, entry + ": out_rgb is NULL"), g
        assert guided(hrt, var, g) == (HRT_ERR_INVALID, entry + ": scene is NULL"), g
    assert guided(hrt, var, hrt.GUIDES_FIRST_HIT, feature_spp=0) == (HRT_ERR_INVALID, entry + ": scene is NULL"), "pixel centres stay with first-hit guides"


# -------------------------------------------------------------------------------------------------------- Python and the tool
def test_python_wrappers_check_their_arguments_before_any_library(hrt):
    S = hrt.DeviceScene

    class Fake:  # stands in for a scene: no method may reach its handle before the arguments are right
        @property
        def _h(self):
            raise AssertionError("the library was reached")

    cam = hrt.default_camera(1.0)
    for bad in ("second", "", None, 1, "Diffuse"):
        with pytest.raises(ValueError, match=r"render_denoised: guides must be \"first\" or \"diffuse\""):
            S.render_denoised(Fake(), cam, 8, 8, 4, 2, guides=bad)
        with pytest.raises(ValueError, match=r"render_denoised_var: guides must be \"first\" or \"diffuse\""):
            S.render_denoised_var(Fake(), cam, 8, 8, 4, 2, guides=bad)
    rays = np.zeros((4, 8), F32)
    with pytest.raises(ValueError, match=r"path_features: rays must have shape \(n, 8\)"):
        S.path_features(Fake(), np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match=r"path_features: keys must be \(n,\) uint32"):
        S.path_features(Fake(), rays, keys=np.zeros(3, U32))
    with pytest.raises(ValueError, match=r"path_features: out must be \(n, 12\) float32"):
        S.path_features(Fake(), rays, out=np.zeros((4, 16), F32))


def test_the_cli_refuses_guides_it_cannot_use_before_it_touches_a_device():
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8", "--spp", "4"]
    for bad in ("second", "1", "Diffuse"):
        r = subprocess.run(base + ["--denoise", "2", "--denoise-guides", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--denoise-guides takes first or diffuse" in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + ["--denoise-guides", "diffuse"], capture_output=True, text=True)
    assert r.returncode == 2 and "--denoise-guides" in r.stderr and "--denoise" in r.stderr and "--denoise-var" in r.stderr, r.stderr
    for filt in ("--denoise", "--denoise-var"):
        r = subprocess.run(base + [filt, "0", "--denoise-guides", "diffuse"], capture_output=True, text=True)
        assert r.returncode == 2 and "--denoise-guides diffuse" in r.stderr and "at least 1" in r.stderr, (filt, r.stderr)
    r = subprocess.run(base + ["--temporal", "2", "--denoise-var", "2", "--denoise-guides", "diffuse"], capture_output=True, text=True)
    assert r.returncode == 2 and "--denoise-guides" in r.stderr and "--temporal" in r.stderr, r.stderr
