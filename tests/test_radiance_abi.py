"""Radiance queries and camera rays without a GPU (include/hrt.h hrt_trace_radiance, hrt_camera_rays): both entry points are
exported, and every bad argument -- flag bit, NULL or misaligned pointer, oversize n, zero samples, sample indices that would wrap,
bad camera or frame size -- is refused with HRT_ERR_INVALID and a message that names it, before the scene and the library state
are looked at; a NULL scene is refused after those checks."""
import ctypes as C
import subprocess

import pytest

HRT_ERR_INVALID = -1
RAYS, KEYS, OUT = 0x1000, 0x3000, 0x2000  # device pointers that are never dereferenced: every call below fails validation first
EXACT, BRUTE, NO_LDS, NORMALIZE, ACCUMULATE = 64, 128, 2, 256, 512


def call(hrt, flags=0, rays=RAYS, keys=None, out=OUT, n=64, first=0, ns=1, seed=1):
    dev = hrt.device_lib()
    rc = dev.hrt_trace_radiance(None, C.c_void_p(rays), None if keys is None else C.c_void_p(keys), n, first, ns, seed, flags,
                                C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def cam_call(hrt, cam=None, w=16, h=9, sample=0, seed=1, rays=0, null_cam=False):
    # rays = NULL by default: hrt_camera_rays checks the camera, then the frame size, then the pointer, so a call that got past
    # the check under test still stops at the NULL pointer and never launches
    dev = hrt.device_lib()
    if cam is None:
        cam = hrt.default_camera(16 / 9)
    rc = dev.hrt_camera_rays(None if null_cam else C.byref(cam), w, h, sample, seed, C.c_void_p(rays), None)
    return rc, dev.hrt_last_error().decode()


@pytest.mark.parametrize("name", ["hrt_trace_radiance", "hrt_camera_rays"])
def test_libhrt_exports_both_symbols(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported


@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in (EXACT, BRUTE, NO_LDS, NORMALIZE, ACCUMULATE)])
def test_every_unknown_flag_bit_is_refused_and_named(hrt, bit):
    rc, msg = call(hrt, flags=1 << bit)
    assert rc == HRT_ERR_INVALID and "flags" in msg and "hrt_trace_radiance" in msg, (bit, msg)


@pytest.mark.parametrize("extra", [0, NO_LDS, NORMALIZE | ACCUMULATE])
def test_mesh_brute_needs_exact_only(hrt, extra):
    rc, msg = call(hrt, flags=BRUTE | extra)
    assert rc == HRT_ERR_INVALID and "flags" in msg and "EXACT_ONLY" in msg, msg


@pytest.mark.parametrize("kw,word", [(dict(rays=0), "d_rays"), (dict(rays=RAYS + 4), "d_rays"), (dict(rays=RAYS + 8), "d_rays"),
                                     (dict(keys=KEYS + 2), "d_keys"), (dict(keys=KEYS + 1), "d_keys"),
                                     (dict(out=0), "d_out"), (dict(out=OUT + 2), "d_out"), (dict(out=OUT + 1), "d_out")])
def test_null_and_misaligned_pointers_are_refused_and_named(hrt, kw, word):
    rc, msg = call(hrt, **kw)
    assert rc == HRT_ERR_INVALID and word in msg, (kw, msg)


def test_four_byte_aligned_keys_and_out_are_enough(hrt):
    rc, msg = call(hrt, keys=KEYS + 4, out=OUT + 4)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg
    rc, msg = call(hrt, out=OUT + 12)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg


@pytest.mark.parametrize("n", [2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1])
def test_oversize_n_is_refused_and_named(hrt, n):
    rc, msg = call(hrt, n=n)
    assert rc == HRT_ERR_INVALID and "n must be" in msg, msg


@pytest.mark.parametrize("first", [0, 5, 2 ** 32 - 1])
def test_zero_samples_are_refused_and_named(hrt, first):
    rc, msg = call(hrt, first=first, ns=0)
    assert rc == HRT_ERR_INVALID and "n_samples" in msg, msg


@pytest.mark.parametrize("first,ns", [(2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1), (2 ** 32 - 8, 9)])
def test_sample_indices_that_would_wrap_are_refused_and_named(hrt, first, ns):
    rc, msg = call(hrt, first=first, ns=ns)
    assert rc == HRT_ERR_INVALID and "first_sample" in msg and "wrap" in msg, msg


@pytest.mark.parametrize("first,ns", [(2 ** 32 - 1, 1), (0, 2 ** 32 - 1), (1, 2 ** 32 - 1), (2 ** 31, 2 ** 31), (7, 2 ** 32 - 7)])
def test_the_last_sample_index_is_allowed(hrt, first, ns):
    rc, msg = call(hrt, first=first, ns=ns)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg


def test_argument_checks_come_before_the_null_scene(hrt):
    for kw in (dict(flags=1 << 20), dict(rays=0), dict(out=OUT + 2), dict(keys=KEYS + 2), dict(n=2 ** 31), dict(ns=0),
               dict(first=2 ** 32 - 1, ns=2)):
        rc, msg = call(hrt, **kw)
        assert rc == HRT_ERR_INVALID and "scene" not in msg, (kw, msg)


def test_pointers_are_not_checked_when_n_is_zero(hrt):
    rc, msg = call(hrt, rays=0, out=0, keys=KEYS + 1, n=0)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg


@pytest.mark.parametrize("flags", [0, EXACT, EXACT | BRUTE, NO_LDS, NORMALIZE, ACCUMULATE, EXACT | BRUTE | NO_LDS | NORMALIZE | ACCUMULATE])
def test_valid_arguments_reach_the_null_scene_check(hrt, flags):
    rc, msg = call(hrt, flags=flags, keys=KEYS, n=2 ** 31 - 1, first=3, ns=100)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg


# ---------------------------------------------------------------------------------------------------------------- camera rays
@pytest.mark.parametrize("w,h", [(0, 9), (16, 0), (0, 0)])
def test_camera_rays_refuse_an_empty_frame(hrt, w, h):
    rc, msg = cam_call(hrt, w=w, h=h)
    assert rc == HRT_ERR_INVALID and "w and h" in msg, msg


@pytest.mark.parametrize("w,h", [(2 ** 16, 2 ** 15), (2 ** 31, 1), (1, 2 ** 31), (46341, 46341), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_camera_rays_refuse_an_oversize_frame(hrt, w, h):
    rc, msg = cam_call(hrt, w=w, h=h)
    assert rc == HRT_ERR_INVALID and "w * h" in msg, msg


@pytest.mark.parametrize("rays", [0, RAYS + 4, RAYS + 8])
def test_camera_rays_refuse_a_null_or_misaligned_output(hrt, rays):
    rc, msg = cam_call(hrt, rays=rays)  # a misaligned pointer is refused whatever else holds: nothing is launched
    assert rc == HRT_ERR_INVALID and "d_rays" in msg, msg


def test_camera_rays_refuse_a_null_camera(hrt):
    rc, msg = cam_call(hrt, null_cam=True)
    assert rc == HRT_ERR_INVALID and "cam" in msg, msg


def bad_cameras(hrt):
    out = []
    c = hrt.default_camera(16 / 9); c.fovy_deg = 0.0; out.append(("fovy 0", c))
    c = hrt.default_camera(16 / 9); c.right[:] = (0, 0, 0); out.append(("zero right", c))
    c = hrt.default_camera(16 / 9); c.znear = c.zfar = 1.0; out.append(("znear == zfar", c))
    c = hrt.default_camera(16 / 9); c.eye[0] = float("nan"); out.append(("NaN eye", c))
    c = hrt.default_camera(16 / 9); c.aspect = float("inf"); out.append(("infinite aspect", c))
    return out


def test_camera_rays_refuse_the_cameras_render_refuses(hrt):
    for what, cam in bad_cameras(hrt):  # the camera check of hrt_render (make_camera), with its message
        rc, msg = cam_call(hrt, cam=cam)
        assert rc == HRT_ERR_INVALID and msg.startswith("render:") and ("camera" in msg or "inverse" in msg), (what, msg)
    rc, msg = cam_call(hrt)  # the default camera passes and reaches the pointer check
    assert rc == HRT_ERR_INVALID and "d_rays is NULL" in msg, msg


def test_python_binding_checks_shapes(hrt):
    with pytest.raises(ValueError, match="shape"):
        hrt.DeviceScene.trace_radiance(None, [[0] * 7])
    with pytest.raises(ValueError, match="keys"):
        hrt.DeviceScene.trace_radiance(None, [[0] * 8] * 2, keys=[1, 2, 3])
