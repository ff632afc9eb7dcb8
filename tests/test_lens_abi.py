"""Lens cameras without a GPU (include/hrt.h hrt_lens_rays, hrt_render_lens_device, hrt_render_lens, hrt_render_lens_features): the
four entry points are exported, and every bad argument -- lens, camera, projection, aperture, focus, extent, frame, samples, flags,
pointers -- is refused with HRT_ERR_INVALID and a message that names the entry point and the culprit, in the header's order and
before the scene and the library state are looked at; a NULL scene is refused after those checks.  The device pointers below are
never dereferenced: every call fails validation first."""
import ctypes as C
import subprocess

import pytest

HRT_ERR_INVALID = -1
RAYS, OUT = 0x1000, 0x2000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ["hrt_lens_rays", "hrt_render_lens_device", "hrt_render_lens", "hrt_render_lens_features"]
NAN, INF = float("nan"), float("inf")


def lens(hrt, projection="perspective", aperture=0.0, focus=1.0, extent=0.0, cam=None):
    return hrt.Lens(hrt.default_camera(16 / 9) if cam is None else cam, projection, aperture=aperture, focus=focus, extent=extent)


def call(hrt, entry, L=None, null_lens=False, w=16, h=9, first=0, ns=1, seed=1, flags=0, out=None):
    """One call of `entry` with a NULL scene.  out: the ray / frame / feature pointer.  By default a valid one where a NULL scene
    stops the call afterwards, and NULL for hrt_lens_rays, which takes no scene: its pointer check is its last, so a call that got
    past the check under test still stops there and never launches."""
    dev = hrt.device_lib()
    lp = None if null_lens else C.byref(lens(hrt) if L is None else L)
    if out is None:
        out = 0 if entry == "hrt_lens_rays" else OUT
    if entry == "hrt_lens_rays":
        rc = dev.hrt_lens_rays(lp, w, h, first, seed, C.c_void_p(out), None)
    elif entry == "hrt_render_lens_device":
        rc = dev.hrt_render_lens_device(None, lp, w, h, first, ns, seed, flags, C.c_void_p(out), None)
    elif entry == "hrt_render_lens":
        rc = dev.hrt_render_lens(None, lp, w, h, ns, seed, flags, C.c_void_p(out), None)
    else:
        rc = dev.hrt_render_lens_features(None, lp, w, h, first, ns, seed, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def passes(hrt, entry, **kw):
    """The arguments get past every check before the last: hrt_lens_rays stops at its NULL pointer, the others at the NULL scene."""
    rc, msg = call(hrt, entry, **kw)
    return (rc == HRT_ERR_INVALID and ("d_rays is NULL" if entry == "hrt_lens_rays" else "scene is NULL") in msg), msg


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_four_symbols(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported


def test_libhrt_exports_exactly_the_functions_of_the_header(hrt):
    import os
    import re
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip() and line.split()[-2] in "TtWw"}
    header = open(os.path.join(hrt.REPO_ROOT, "include", "hrt.h")).read()
    declared = set(re.findall(r"^HRT_API [^;(]*?[ *](hrt_[a-z_0-9]+)\(", header, re.M))
    assert set(NAMES) <= declared
    assert {e for e in exported if e.startswith("hrt_")} == declared


def test_the_struct_has_the_headers_layout(hrt):
    L = hrt.Lens
    assert C.sizeof(L) == C.sizeof(hrt.Camera) + 16
    assert [L.cam.offset, L.projection.offset, L.aperture_radius.offset, L.focus_distance.offset, L.extent.offset] == [0, 64, 68, 72, 76]
    assert (hrt.LENS_PERSPECTIVE, hrt.LENS_ORTHOGRAPHIC, hrt.LENS_EQUIRECT, hrt.LENS_FISHEYE, hrt.LENS_DRAW) == (0, 1, 2, 3, 2 ** 31)
    with pytest.raises(ValueError, match="projection"):
        lens(hrt, "pinhole")


# ------------------------------------------------------------------------------------------------------------- the lens checks
@pytest.mark.parametrize("entry", NAMES)
def test_a_null_lens_is_refused_and_named(hrt, entry):
    rc, msg = call(hrt, entry, null_lens=True)
    assert rc == HRT_ERR_INVALID and entry in msg and "lens is NULL" in msg, msg


def bad_cameras(hrt):
    out = []
    c = hrt.default_camera(16 / 9); c.fovy_deg = 0.0; out.append(("fovy 0", c))
    c = hrt.default_camera(16 / 9); c.right[:] = (0, 0, 0); out.append(("zero right", c))
    c = hrt.default_camera(16 / 9); c.znear = c.zfar = 1.0; out.append(("znear == zfar", c))
    c = hrt.default_camera(16 / 9); c.eye[0] = NAN; out.append(("NaN eye", c))
    c = hrt.default_camera(16 / 9); c.aspect = INF; out.append(("infinite aspect", c))
    return out


@pytest.mark.parametrize("entry", NAMES)
def test_the_cameras_render_refuses_are_refused_with_its_message(hrt, entry):
    for what, cam in bad_cameras(hrt):
        for proj, extent in (("perspective", 0.0), ("equirect", 0.0), ("ortho", 2.0)):  # whatever the projection reads of it
            rc, msg = call(hrt, entry, L=lens(hrt, proj, extent=extent, cam=cam))
            assert rc == HRT_ERR_INVALID and msg.startswith("render:") and ("camera" in msg or "inverse" in msg), (what, proj, msg)


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("projection", [4, 5, 2 ** 31, 2 ** 32 - 1])
def test_an_unknown_projection_is_refused_and_named(hrt, entry, projection):
    rc, msg = call(hrt, entry, L=lens(hrt, projection))
    assert rc == HRT_ERR_INVALID and entry in msg and "projection" in msg and str(projection) in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_aperture_radius(hrt, entry):
    for a in (-1e-3, -1.0, NAN, INF, -INF):
        rc, msg = call(hrt, entry, L=lens(hrt, aperture=a, focus=2.0))
        assert rc == HRT_ERR_INVALID and entry in msg and "aperture_radius" in msg, (a, msg)
    for proj, extent in (("ortho", 2.0), ("equirect", 0.0), ("fisheye", 180.0)):  # a thin lens is PERSPECTIVE's
        rc, msg = call(hrt, entry, L=lens(hrt, proj, aperture=0.1, focus=2.0, extent=extent))
        assert rc == HRT_ERR_INVALID and entry in msg and "aperture_radius" in msg and "PERSPECTIVE" in msg, (proj, msg)
    for a in (0.0, -0.0, 1e-30, 0.2, 1e6):
        ok, msg = passes(hrt, entry, L=lens(hrt, aperture=a, focus=2.0))
        assert ok, (a, msg)


@pytest.mark.parametrize("entry", NAMES)
def test_focus_distance(hrt, entry):
    for f in (0.0, -1.0, NAN, INF, -INF):
        rc, msg = call(hrt, entry, L=lens(hrt, aperture=0.1, focus=f))
        assert rc == HRT_ERR_INVALID and entry in msg and "focus_distance" in msg, (f, msg)
        ok, msg = passes(hrt, entry, L=lens(hrt, aperture=0.0, focus=f))  # ignored, any value, without an aperture
        assert ok, (f, msg)
        ok, msg = passes(hrt, entry, L=lens(hrt, "equirect", focus=f))
        assert ok, (f, msg)


@pytest.mark.parametrize("entry", NAMES)
def test_extent(hrt, entry):
    for e in (0.0, -1.0, NAN, INF, -INF):
        rc, msg = call(hrt, entry, L=lens(hrt, "ortho", extent=e))
        assert rc == HRT_ERR_INVALID and entry in msg and "extent" in msg, ("ortho", e, msg)
    for e in (0.0, -1.0, NAN, INF, 360.001, 720.0):
        rc, msg = call(hrt, entry, L=lens(hrt, "fisheye", extent=e))
        assert rc == HRT_ERR_INVALID and entry in msg and "extent" in msg and "360" in msg, ("fisheye", e, msg)
    for proj in ("perspective", "equirect"):
        for e in (1.0, -1.0, NAN, 1e-30):
            rc, msg = call(hrt, entry, L=lens(hrt, proj, extent=e))
            assert rc == HRT_ERR_INVALID and entry in msg and "extent" in msg, (proj, e, msg)
    for proj, e in (("ortho", 1e-3), ("ortho", 1e9), ("fisheye", 1e-3), ("fisheye", 180.0), ("fisheye", 360.0), ("perspective", -0.0)):
        ok, msg = passes(hrt, entry, L=lens(hrt, proj, extent=e))
        assert ok, (proj, e, msg)


@pytest.mark.parametrize("entry", NAMES)
def test_the_lens_fields_are_checked_in_the_headers_order(hrt, entry):
    cam = bad_cameras(hrt)[3][1]
    # everything wrong at once: the camera speaks first, then projection, aperture, focus, extent, frame, pointer
    L = lens(hrt, 7, aperture=-1.0, focus=-1.0, extent=-1.0, cam=cam)
    assert call(hrt, entry, L=L, w=0, out=0)[1].startswith("render:")
    L = lens(hrt, 7, aperture=-1.0, focus=-1.0, extent=-1.0)
    assert "projection" in call(hrt, entry, L=L, w=0, out=0)[1]
    L = lens(hrt, "perspective", aperture=-1.0, focus=-1.0, extent=-1.0)
    assert "aperture_radius" in call(hrt, entry, L=L, w=0, out=0)[1]
    L = lens(hrt, "perspective", aperture=1.0, focus=-1.0, extent=-1.0)
    assert "focus_distance" in call(hrt, entry, L=L, w=0, out=0)[1]
    L = lens(hrt, "perspective", aperture=1.0, focus=1.0, extent=-1.0)
    assert "extent" in call(hrt, entry, L=L, w=0, out=0)[1]
    L = lens(hrt, "perspective", aperture=1.0, focus=1.0)
    assert "w and h" in call(hrt, entry, L=L, w=0, out=0)[1]


# ------------------------------------------------------------------------------------------------------------ frame, samples
@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("w,h", [(0, 9), (16, 0), (0, 0)])
def test_an_empty_frame_is_refused_and_named(hrt, entry, w, h):
    rc, msg = call(hrt, entry, w=w, h=h)
    assert rc == HRT_ERR_INVALID and entry in msg and "w and h" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("w,h", [(2 ** 31, 1), (1, 2 ** 31), (46341, 46341), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_an_oversize_frame_is_refused_and_named(hrt, entry, w, h):
    rc, msg = call(hrt, entry, w=w, h=h)
    assert rc == HRT_ERR_INVALID and entry in msg and "w * h" in msg, msg


@pytest.mark.parametrize("entry", ["hrt_render_lens_device", "hrt_render_lens"])
def test_zero_samples_are_refused_and_named(hrt, entry):
    for first in (0, 5, 2 ** 32 - 1):
        rc, msg = call(hrt, entry, first=first, ns=0)
        assert rc == HRT_ERR_INVALID and entry in msg and "n_samples" in msg, msg


@pytest.mark.parametrize("first,ns", [(2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1), (2 ** 32 - 8, 9)])
def test_sample_indices_that_would_wrap_are_refused_and_named(hrt, first, ns):
    rc, msg = call(hrt, "hrt_render_lens_device", first=first, ns=ns)
    assert rc == HRT_ERR_INVALID and "hrt_render_lens_device" in msg and "first_sample" in msg and "wrap" in msg, msg
    rc, msg = call(hrt, "hrt_render_lens_features", first=first, ns=ns)
    assert rc == HRT_ERR_INVALID and "hrt_render_lens_features" in msg and "first_sample" in msg, msg


@pytest.mark.parametrize("first,ns", [(2 ** 32 - 1, 1), (0, 2 ** 32 - 1), (1, 2 ** 32 - 1), (2 ** 31, 2 ** 31), (7, 2 ** 32 - 7)])
def test_the_last_sample_index_is_allowed(hrt, first, ns):
    ok, msg = passes(hrt, "hrt_render_lens_device", first=first, ns=ns)
    assert ok, msg
    ok, msg = passes(hrt, "hrt_lens_rays", first=2 ** 32 - 1)
    assert ok, msg


# --------------------------------------------------------------------------------------------------------------------- flags
KNOWN = (GAMMA, NO_LDS, EXACT, BRUTE, ACCUMULATE)
BY_NAME = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
           NORMALIZE: "HRT_RAYS_NORMALIZE"}


@pytest.mark.parametrize("entry", ["hrt_render_lens_device", "hrt_render_lens"])
@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in KNOWN])
def test_every_other_flag_bit_is_refused_and_named(hrt, entry, bit):
    rc, msg = call(hrt, entry, flags=1 << bit)
    assert rc == HRT_ERR_INVALID and entry in msg and "flags" in msg, (bit, msg)
    assert BY_NAME.get(1 << bit, str(1 << bit)) in msg, (bit, msg)


@pytest.mark.parametrize("entry", ["hrt_render_lens_device", "hrt_render_lens"])
def test_flag_combinations(hrt, entry):
    for extra in (0, NO_LDS, GAMMA):
        rc, msg = call(hrt, entry, flags=BRUTE | extra)
        assert rc == HRT_ERR_INVALID and "flags" in msg and "EXACT_ONLY" in msg, msg
    rc, msg = call(hrt, entry, flags=GAMMA | ACCUMULATE)
    assert rc == HRT_ERR_INVALID and entry in msg and "ACCUMULATE" in msg, msg
    assert "HRT_FLAG_GAMMA" in msg or entry == "hrt_render_lens", msg  # the host form refuses ACCUMULATE whatever comes with it
    for flags in (0, EXACT, EXACT | BRUTE, NO_LDS, GAMMA, EXACT | BRUTE | NO_LDS | GAMMA):
        ok, msg = passes(hrt, entry, flags=flags)
        assert ok, (flags, msg)
    ok, msg = passes(hrt, "hrt_render_lens_device", flags=ACCUMULATE | EXACT | BRUTE | NO_LDS)
    assert ok, msg
    rc, msg = call(hrt, "hrt_render_lens", flags=ACCUMULATE)  # the host form has no running sums to add to
    assert rc == HRT_ERR_INVALID and "hrt_render_lens" in msg and "ACCUMULATE" in msg, msg


# ------------------------------------------------------------------------------------------------------------------ pointers
@pytest.mark.parametrize("out", [0, RAYS + 4, RAYS + 8])
def test_lens_rays_refuse_a_null_or_misaligned_output(hrt, out):
    rc, msg = call(hrt, "hrt_lens_rays", out=out)  # a misaligned pointer is refused whatever else holds: nothing is launched
    assert rc == HRT_ERR_INVALID and "hrt_lens_rays" in msg and "d_rays" in msg, msg


@pytest.mark.parametrize("entry,word", [("hrt_render_lens_device", "d_frame"), ("hrt_render_lens", "out_rgb")])
def test_frames_refuse_a_null_or_misaligned_output(hrt, entry, word):
    for out in (0, OUT + 1, OUT + 2):
        rc, msg = call(hrt, entry, out=out)
        assert rc == HRT_ERR_INVALID and entry in msg and word in msg, (out, msg)
    for out in (OUT + 4, OUT + 12):
        ok, msg = passes(hrt, entry, out=out)
        assert ok, (out, msg)


def test_features_refuse_a_null_output(hrt):
    rc, msg = call(hrt, "hrt_render_lens_features", out=0)
    assert rc == HRT_ERR_INVALID and "hrt_render_lens_features" in msg and "d_features" in msg, msg


@pytest.mark.parametrize("entry", NAMES[1:])
def test_argument_checks_come_before_the_null_scene(hrt, entry):
    cases = [dict(null_lens=True), dict(L=lens(hrt, 9)), dict(L=lens(hrt, aperture=-1.0)), dict(L=lens(hrt, "ortho")), dict(w=0), dict(out=0)]
    if entry != "hrt_render_lens_features":
        cases += [dict(ns=0), dict(flags=WAVE), dict(flags=1 << 20), dict(out=OUT + 2)]
    if entry == "hrt_render_lens_device":
        cases += [dict(first=2 ** 32 - 1, ns=2)]
    for kw in cases:
        rc, msg = call(hrt, entry, **kw)
        assert rc == HRT_ERR_INVALID and "scene" not in msg, (kw, msg)
    ok, msg = passes(hrt, entry)
    assert ok, msg


def test_the_frame_checks_of_the_render_come_in_the_headers_order(hrt):
    e = "hrt_render_lens_device"
    assert "w and h" in call(hrt, e, w=0, ns=0, first=2 ** 32 - 1, out=0)[1]
    assert "n_samples" in call(hrt, e, ns=0, first=2 ** 32 - 1, out=0)[1]
    assert "first_sample" in call(hrt, e, ns=2, first=2 ** 32 - 1, out=0)[1]
    assert "d_frame is NULL" in call(hrt, e, out=0)[1]
    assert "aligned" in call(hrt, e, out=OUT + 2)[1]
    assert "scene is NULL" in call(hrt, e)[1]


def test_python_binding_checks_the_output(hrt):
    import numpy as np
    with pytest.raises(ValueError, match="out"):
        hrt.DeviceScene.render_lens(None, lens(hrt), 16, 9, 1, out=np.zeros((9, 16, 4), np.float32))
    with pytest.raises(ValueError, match="accumulate"):
        hrt.DeviceScene.render_lens(None, lens(hrt), 16, 9, 1, first_sample=3, accumulate=True)
