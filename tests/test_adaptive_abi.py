"""Adaptive sampling entry points without a GPU: they are exported, and every bad parameter is refused with HRT_ERR_INVALID and
a message that names it -- before the scene or the library state is looked at (include/hrt.h)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

HRT_ERR_INVALID = -1
NAMES = ["hrt_render_adaptive", "hrt_render_adaptive_tiles"]


def test_libhrt_exports_the_adaptive_entry_points(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for n in NAMES:
        assert hasattr(dev, n) and n in exported


def call(hrt, entry, params, cam=True, out=True, spp_out=True, scene=None):
    dev = hrt.device_lib()
    camera = hrt.default_camera(64 / 36) if cam else None
    p = None if params is None else C.byref(params)
    buf = np.empty((36, 64, 3), dtype=np.float32)
    counts = np.empty(40, dtype=np.uint32)
    if entry == "hrt_render_adaptive":
        rc = dev.hrt_render_adaptive(scene, None if camera is None else C.byref(camera), 64, 36, p, 1, 0,
                                     buf.ctypes.data if out else None, counts.ctypes.data, None)
    else:
        rc = dev.hrt_render_adaptive_tiles(scene, None if camera is None else C.byref(camera), 64, 36, p, 1, 0, 0, 1,
                                           buf.ctypes.data if out else None, counts.ctypes.data if spp_out else None, None)
    return rc, dev.hrt_last_error().decode()


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("mn,mx,thr,field", [
    (0, 8, 1.0, "min_spp"), (3, 8, 1.0, "min_spp"), (7, 8, 1.0, "min_spp"), (1, 8, 1.0, "min_spp"),
    (8, 4, 1.0, "max_spp"), (4, 2, 0.0, "max_spp"),
    (4, 8, math.nan, "threshold"), (4, 8, -1e-3, "threshold"), (4, 8, -math.inf, "threshold"),
])
def test_bad_parameters_are_refused_and_named(hrt, entry, mn, mx, thr, field):
    rc, msg = call(hrt, entry, hrt.Adaptive(mn, mx, thr))
    assert rc == HRT_ERR_INVALID
    assert field in msg and entry in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_null_arguments_are_refused_and_named(hrt, entry):
    ok = hrt.Adaptive(4, 16, 0.5)
    rc, msg = call(hrt, entry, None)
    assert rc == HRT_ERR_INVALID and "params" in msg, msg
    rc, msg = call(hrt, entry, ok, cam=False)
    assert rc == HRT_ERR_INVALID and "camera" in msg, msg
    rc, msg = call(hrt, entry, ok, out=False)
    assert rc == HRT_ERR_INVALID and ("out_rgb" if entry == "hrt_render_adaptive" else "d_tiles") in msg, msg
    if entry == "hrt_render_adaptive_tiles":
        rc, msg = call(hrt, entry, ok, spp_out=False)
        assert rc == HRT_ERR_INVALID and "d_tile_spp" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("mn,mx,thr", [(2, 2, 0.0), (4, 64, math.inf), (16, 256, 0.05), (2, 3, 1e30)])
def test_good_parameters_pass_to_the_scene_check(hrt, entry, mn, mx, thr):
    """Valid parameters (equal bounds, +inf, a max that is no power-of-two multiple of min) get past validation: the call then
    fails on the NULL scene, and says so."""
    rc, msg = call(hrt, entry, hrt.Adaptive(mn, mx, thr))
    assert rc == HRT_ERR_INVALID and "scene" in msg, msg
