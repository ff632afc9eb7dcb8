"""Adaptive lens frames without a GPU (include/hrt.h hrt_render_lens_adaptive_device, hrt_render_lens_adaptive): the two entry points
are exported, and every bad argument -- flags, params, lens, frame, the tile limit, pointers -- is refused with HRT_ERR_INVALID and a
message that names the entry point and the culprit, in the header's order and before the scene and the library state are looked
at; a NULL scene is refused after those checks.  The device pointers below are never dereferenced: every call fails validation
first.  The driver takes --lens with --adaptive."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

HRT_ERR_INVALID = -1
OUT, SPP = 0x2000, 0x4000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ["hrt_render_lens_adaptive_device", "hrt_render_lens_adaptive"]
NAN, INF = float("nan"), float("inf")
OUT_WORD = {"hrt_render_lens_adaptive_device": ("d_frame", "d_tile_spp"), "hrt_render_lens_adaptive": ("out_rgb", "out_tile_spp")}
UNSET = object()


def lens(hrt, projection="perspective", aperture=0.0, focus=1.0, extent=0.0, cam=None):
    return hrt.Lens(hrt.default_camera(16 / 9) if cam is None else cam, projection, aperture=aperture, focus=focus, extent=extent)


def call(hrt, entry, L=None, null_lens=False, w=16, h=9, params=UNSET, seed=1, flags=0, out=OUT, spp=SPP):
    """One call of `entry` with a NULL scene: a call that gets past every argument check stops there."""
    dev = hrt.device_lib()
    lp = None if null_lens else C.byref(lens(hrt) if L is None else L)
    p = hrt.Adaptive(4, 16, 0.5) if params is UNSET else params
    pp = None if p is None else C.byref(p)
    if entry == "hrt_render_lens_adaptive_device":
        rc = dev.hrt_render_lens_adaptive_device(None, lp, w, h, pp, seed, flags, C.c_void_p(out), C.c_void_p(spp), None)
    else:
        rc = dev.hrt_render_lens_adaptive(None, lp, w, h, pp, seed, flags, C.c_void_p(out), C.c_void_p(spp), None)
    return rc, dev.hrt_last_error().decode()


def passes(hrt, entry, **kw):
    rc, msg = call(hrt, entry, **kw)
    return (rc == HRT_ERR_INVALID and "scene is NULL" in msg and entry in msg), msg


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_two_symbols(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported


def test_libhrt_exports_exactly_the_functions_of_the_header(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip() and line.split()[-2] in "TtWw"}
    header = open(os.path.join(hrt.REPO_ROOT, "include", "hrt.h")).read()
    declared = set(re.findall(r"^HRT_API [^;(]*?[ *](hrt_[a-z_0-9]+)\(", header, re.M))
    assert set(NAMES) <= declared
    assert {e for e in exported if e.startswith("hrt_")} == declared


def test_the_header_no_longer_lists_the_adaptive_sampler_as_not_lens_aware(hrt):
    header = open(os.path.join(hrt.REPO_ROOT, "include", "hrt.h")).read()
    sentence = header[header.index("Not lens-aware"):]
    sentence = sentence[:sentence.index(".")]
    assert "adaptive" not in sentence, sentence


def test_the_structs_have_the_headers_layout(hrt):
    L, A = hrt.Lens, hrt.Adaptive
    assert C.sizeof(L) == C.sizeof(hrt.Camera) + 16
    assert [L.cam.offset, L.projection.offset, L.aperture_radius.offset, L.focus_distance.offset, L.extent.offset] == [0, 64, 68, 72, 76]
    assert C.sizeof(A) == 12 and [A.min_spp.offset, A.max_spp.offset, A.threshold.offset] == [0, 4, 8]
    header = open(os.path.join(hrt.REPO_ROOT, "include", "hrt.h")).read()
    body = re.search(r"typedef struct hrt_adaptive \{(.*?)\} hrt_adaptive;", header, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint32_t min_spp, max_spp; float threshold;"
    body = re.search(r"typedef struct hrt_lens \{(.*?)\} hrt_lens;", header, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    assert fields == [("hrt_camera", "cam"), ("uint32_t", "projection"), ("float", "aperture_radius"), ("float", "focus_distance"), ("float", "extent")]


# --------------------------------------------------------------------------------------------------------------------- flags
KNOWN = (GAMMA, NO_LDS, EXACT, BRUTE)
BY_NAME = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
           NORMALIZE: "HRT_RAYS_NORMALIZE", ACCUMULATE: "HRT_RADIANCE_ACCUMULATE"}


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in KNOWN])
def test_every_other_flag_bit_is_refused_and_named(hrt, entry, bit):
    rc, msg = call(hrt, entry, flags=1 << bit)
    assert rc == HRT_ERR_INVALID and entry in msg and "flags" in msg, (bit, msg)
    assert BY_NAME.get(1 << bit, str(1 << bit)) in msg, (bit, msg)


@pytest.mark.parametrize("entry", NAMES)
def test_the_refusals_carry_the_texts_of_the_lens_frames(hrt, entry):
    """The same words hrt_render_lens_device uses for the same bit."""
    dev = hrt.device_lib()
    for bit in (WAVE, STREAM, DUAL, NO_SHADOW_CULL, NORMALIZE, 1 << 20, BRUTE):
        rc, msg = call(hrt, entry, flags=bit)
        L = lens(hrt)
        rc2 = dev.hrt_render_lens_device(None, C.byref(L), 16, 9, 0, 1, 1, bit, C.c_void_p(OUT), None)
        want = dev.hrt_last_error().decode()
        assert rc == rc2 == HRT_ERR_INVALID and msg == want.replace("hrt_render_lens_device", entry), (bit, msg, want)


@pytest.mark.parametrize("entry", NAMES)
def test_flag_combinations(hrt, entry):
    for extra in (0, NO_LDS, GAMMA):
        rc, msg = call(hrt, entry, flags=BRUTE | extra)
        assert rc == HRT_ERR_INVALID and "flags" in msg and "EXACT_ONLY" in msg, msg
    for extra in (0, GAMMA, EXACT):
        rc, msg = call(hrt, entry, flags=ACCUMULATE | extra)
        assert rc == HRT_ERR_INVALID and entry in msg and "HRT_RADIANCE_ACCUMULATE" in msg, msg
    for flags in (0, EXACT, EXACT | BRUTE, NO_LDS, GAMMA, EXACT | BRUTE | NO_LDS | GAMMA):
        ok, msg = passes(hrt, entry, flags=flags)
        assert ok, (flags, msg)


# -------------------------------------------------------------------------------------------------------------------- params
@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("mn,mx,thr,field", [
    (0, 8, 1.0, "min_spp"), (3, 8, 1.0, "min_spp"), (7, 8, 1.0, "min_spp"), (1, 8, 1.0, "min_spp"),
    (8, 4, 1.0, "max_spp"), (4, 2, 0.0, "max_spp"),
    (4, 8, math.nan, "threshold"), (4, 8, -1e-3, "threshold"), (4, 8, -math.inf, "threshold"),
])
def test_bad_parameters_are_refused_and_named(hrt, entry, mn, mx, thr, field):
    rc, msg = call(hrt, entry, params=hrt.Adaptive(mn, mx, thr))
    assert rc == HRT_ERR_INVALID and field in msg and entry in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_null_params_are_refused_and_named(hrt, entry):
    rc, msg = call(hrt, entry, params=None)
    assert rc == HRT_ERR_INVALID and "params" in msg and entry in msg, msg


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("mn,mx,thr", [(2, 2, 0.0), (4, 64, math.inf), (16, 256, 0.05), (2, 3, 1e30), (4, 22, 0.0)])
def test_good_parameters_pass_to_the_scene_check(hrt, entry, mn, mx, thr):
    ok, msg = passes(hrt, entry, params=hrt.Adaptive(mn, mx, thr))
    assert ok, msg


# ---------------------------------------------------------------------------------------------------------------------- lens
def bad_camera(hrt):
    c = hrt.default_camera(16 / 9)
    c.eye[0] = NAN
    return c


@pytest.mark.parametrize("entry", NAMES)
def test_every_lens_field_is_refused_and_named(hrt, entry):
    rc, msg = call(hrt, entry, null_lens=True)
    assert rc == HRT_ERR_INVALID and entry in msg and "lens is NULL" in msg, msg
    rc, msg = call(hrt, entry, L=lens(hrt, cam=bad_camera(hrt)))
    assert rc == HRT_ERR_INVALID and msg.startswith("render:") and ("camera" in msg or "inverse" in msg), msg  # as hrt_render refuses it
    for projection in (4, 2 ** 31, 2 ** 32 - 1):
        rc, msg = call(hrt, entry, L=lens(hrt, projection))
        assert rc == HRT_ERR_INVALID and entry in msg and "projection" in msg and str(projection) in msg, msg
    for a in (-1e-3, NAN, INF):
        rc, msg = call(hrt, entry, L=lens(hrt, aperture=a, focus=2.0))
        assert rc == HRT_ERR_INVALID and entry in msg and "aperture_radius" in msg, (a, msg)
    for proj, extent in (("ortho", 2.0), ("equirect", 0.0), ("fisheye", 180.0)):
        rc, msg = call(hrt, entry, L=lens(hrt, proj, aperture=0.1, focus=2.0, extent=extent))
        assert rc == HRT_ERR_INVALID and entry in msg and "aperture_radius" in msg and "PERSPECTIVE" in msg, (proj, msg)
    for f in (0.0, -1.0, NAN, INF):
        rc, msg = call(hrt, entry, L=lens(hrt, aperture=0.1, focus=f))
        assert rc == HRT_ERR_INVALID and entry in msg and "focus_distance" in msg, (f, msg)
    for proj, e in (("ortho", 0.0), ("ortho", INF), ("fisheye", 0.0), ("fisheye", 360.5), ("perspective", 1.0), ("equirect", NAN)):
        rc, msg = call(hrt, entry, L=lens(hrt, proj, extent=e))
        assert rc == HRT_ERR_INVALID and entry in msg and "extent" in msg, (proj, e, msg)
    for L in (lens(hrt), lens(hrt, aperture=0.2, focus=3.0), lens(hrt, "ortho", extent=4.0), lens(hrt, "equirect"), lens(hrt, "fisheye", extent=180.0),
              lens(hrt, focus=NAN)):
        ok, msg = passes(hrt, entry, L=L)
        assert ok, msg


# --------------------------------------------------------------------------------------------------------- frame and pointers
@pytest.mark.parametrize("entry", NAMES)
def test_the_frame_is_refused_and_named(hrt, entry):
    for w, h in ((0, 9), (16, 0), (0, 0)):
        rc, msg = call(hrt, entry, w=w, h=h)
        assert rc == HRT_ERR_INVALID and entry in msg and "w and h" in msg, msg
    for w, h in ((2 ** 31, 1), (46341, 46341), (2 ** 32 - 1, 2 ** 32 - 1)):
        rc, msg = call(hrt, entry, w=w, h=h)
        assert rc == HRT_ERR_INVALID and entry in msg and "w * h" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_the_tile_limit(hrt, entry):
    """tiles * 64 <= 2^31 - 1: frames of few pixels per tile pass the pixel limit and miss this one."""
    for w, h in ((2 ** 31 - 1, 1), (2 ** 28, 1), (2 ** 27 - 7, 9), (1, 2 ** 28)):  # 2^28, 2^25, 2 x 2^24, 2^25 tiles
        assert w * h <= 2 ** 31 - 1 and ((w + 7) // 8) * ((h + 7) // 8) * 64 > 2 ** 31 - 1
        rc, msg = call(hrt, entry, w=w, h=h)
        assert rc == HRT_ERR_INVALID and entry in msg and "tiles * 64" in msg, msg
    for w, h in ((2 ** 28 - 8, 1), (2 ** 27 - 8, 9), (46336, 46336), (1, 2 ** 28 - 8)):
        assert ((w + 7) // 8) * ((h + 7) // 8) * 64 <= 2 ** 31 - 1
        ok, msg = passes(hrt, entry, w=w, h=h)
        assert ok, msg


@pytest.mark.parametrize("entry", NAMES)
def test_the_output_pointers(hrt, entry):
    frame, counts = OUT_WORD[entry]
    rc, msg = call(hrt, entry, out=0)
    assert rc == HRT_ERR_INVALID and entry in msg and frame + " is NULL" in msg, msg
    for out in (OUT + 1, OUT + 2):
        rc, msg = call(hrt, entry, out=out)
        assert rc == HRT_ERR_INVALID and entry in msg and frame in msg and "aligned" in msg, msg
    for spp in (SPP + 1, SPP + 2):
        rc, msg = call(hrt, entry, spp=spp)
        assert rc == HRT_ERR_INVALID and entry in msg and counts in msg and "aligned" in msg, msg
    for kw in (dict(spp=0), dict(out=OUT + 4, spp=SPP + 12)):  # the counts may be NULL
        ok, msg = passes(hrt, entry, **kw)
        assert ok, msg


@pytest.mark.parametrize("entry", NAMES)
def test_the_checks_come_in_the_headers_order_and_the_null_scene_last(hrt, entry):
    bad_p, bad_L = hrt.Adaptive(3, 2, NAN), lens(hrt, 7, aperture=-1.0)
    big = dict(w=2 ** 28, h=1)
    assert "flags" in call(hrt, entry, flags=WAVE, params=bad_p, L=bad_L, w=0, out=0)[1]
    assert "HRT_RADIANCE_ACCUMULATE" in call(hrt, entry, flags=ACCUMULATE, params=None, null_lens=True, w=0, out=0)[1]
    assert "params" in call(hrt, entry, params=None, L=bad_L, w=0, out=0)[1]
    assert "min_spp" in call(hrt, entry, params=bad_p, L=bad_L, w=0, out=0)[1]
    assert "max_spp" in call(hrt, entry, params=hrt.Adaptive(4, 2, NAN), L=bad_L, w=0, out=0)[1]
    assert "threshold" in call(hrt, entry, params=hrt.Adaptive(4, 8, NAN), L=bad_L, w=0, out=0)[1]
    assert "lens is NULL" in call(hrt, entry, null_lens=True, w=0, out=0)[1]
    assert call(hrt, entry, L=lens(hrt, 7, cam=bad_camera(hrt)), w=0, out=0)[1].startswith("render:")
    assert "projection" in call(hrt, entry, L=bad_L, w=0, out=0)[1]
    assert "aperture_radius" in call(hrt, entry, L=lens(hrt, aperture=-1.0, focus=-1.0, extent=-1.0), w=0, out=0)[1]
    assert "focus_distance" in call(hrt, entry, L=lens(hrt, aperture=1.0, focus=-1.0, extent=-1.0), w=0, out=0)[1]
    assert "extent" in call(hrt, entry, L=lens(hrt, aperture=1.0, focus=1.0, extent=-1.0), w=0, out=0)[1]
    assert "w and h" in call(hrt, entry, w=0, out=0)[1]
    assert "tiles * 64" in call(hrt, entry, out=0, **big)[1]
    assert "is NULL" in call(hrt, entry, out=0, spp=SPP + 2)[1] and "scene" not in call(hrt, entry, out=0, spp=SPP + 2)[1]
    assert OUT_WORD[entry][0] in call(hrt, entry, out=OUT + 2, spp=SPP + 2)[1]
    assert OUT_WORD[entry][1] in call(hrt, entry, spp=SPP + 2)[1]
    assert "scene is NULL" in call(hrt, entry)[1]


def test_python_binding_checks_the_output(hrt):
    import numpy as np
    with pytest.raises(ValueError, match="out"):
        hrt.DeviceScene.render_lens_adaptive(None, lens(hrt), 16, 9, 4, 16, 0.5, out=np.zeros((9, 16, 3), np.float32))


# ----------------------------------------------------------------------------------------------------------------- the driver
def raytracer(*args):
    from conftest import PKG
    return subprocess.run([os.path.join(PKG, "raytracer"), *args], capture_output=True, text=True, timeout=120)


def test_the_driver_takes_a_lens_with_adaptive(tmp_path):
    """--lens fisheye --adaptive gets past argument parsing: without a device the run may stop only for lack of one."""
    r = raytracer("--lens", "fisheye", "--lens-extent", "180", "--adaptive", "0.05", "--spp-min", "4", "--spp", "8", "--w", "32", "--h", "16",
                  "--out", str(tmp_path / "rendu.ppm"))
    text = r.stdout + r.stderr
    assert "cannot be combined" not in text and "unknown option" not in text, text
    if r.returncode != 0:
        assert "hrt_render_lens_adaptive failed" not in text, text
        assert re.search(r"hip|device|gpu", text, re.I), text
    else:
        assert "mean" in r.stdout and "spp" in r.stdout, r.stdout


def test_the_driver_still_refuses_what_a_lens_cannot_do():
    for extra in (("--denoise", "0"), ("--denoise-var", "0"), ("--temporal", "2"), ("--gpus", "1")):
        r = raytracer("--lens", "equirect", *extra)
        assert r.returncode == 2 and "--lens" in r.stderr and "cannot be combined" in r.stderr, (extra, r.stderr)
    r = raytracer("--lens", "equirect", "--views", "2", "--adaptive", "0.1")
    assert r.returncode == 2 and "--views" in r.stderr and "--adaptive" in r.stderr, r.stderr
