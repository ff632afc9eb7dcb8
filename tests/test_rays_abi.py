"""Ray queries without a GPU (include/hrt.h hrt_trace_rays): the entry point is exported, and every bad argument -- mode, flag bit,
NULL or misaligned pointer, oversize n -- is refused with HRT_ERR_INVALID and a message that names it, before the scene and the
library state are looked at; a NULL scene is refused after those checks."""
import ctypes as C
import subprocess

import pytest

HRT_ERR_INVALID = -1
RAYS, OUT = 0x1000, 0x2000  # device pointers that are never dereferenced: every call below fails validation first
EXACT, BRUTE, NO_LDS, NORMALIZE = 64, 128, 2, 256


def call(hrt, mode=0, flags=0, rays=RAYS, out=OUT, n=64):
    dev = hrt.device_lib()
    rc = dev.hrt_trace_rays(None, C.c_void_p(rays), n, mode, flags, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def test_libhrt_exports_hrt_trace_rays(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, "hrt_trace_rays") and "hrt_trace_rays" in exported


@pytest.mark.parametrize("mode", [3, 4, 255, 0xFFFFFFFF])
def test_bad_mode_is_refused_and_named(hrt, mode):
    rc, msg = call(hrt, mode=mode)
    assert rc == HRT_ERR_INVALID and "mode" in msg and "hrt_trace_rays" in msg, msg


@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in (EXACT, BRUTE, NO_LDS, NORMALIZE)])
def test_every_unknown_flag_bit_is_refused_and_named(hrt, bit):
    rc, msg = call(hrt, flags=1 << bit)
    assert rc == HRT_ERR_INVALID and "flags" in msg, (bit, msg)


def test_mesh_brute_needs_exact_only(hrt):
    rc, msg = call(hrt, flags=BRUTE)
    assert rc == HRT_ERR_INVALID and "flags" in msg and "EXACT_ONLY" in msg, msg


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_null_and_misaligned_pointers_are_refused_and_named(hrt, mode):
    align = 4 if mode == 2 else 16
    for kw, word in ((dict(rays=0), "d_rays"), (dict(rays=RAYS + 4), "d_rays"), (dict(rays=RAYS + 8), "d_rays"),
                     (dict(out=0), "d_out"), (dict(out=OUT + align // 2 if align > 4 else OUT + 2), "d_out")):
        rc, msg = call(hrt, mode=mode, **kw)
        assert rc == HRT_ERR_INVALID and word in msg, (mode, kw, msg)
    if mode == 2:  # a 4-byte aligned output is enough for one u32 per ray
        rc, msg = call(hrt, mode=mode, out=OUT + 4)
        assert rc == HRT_ERR_INVALID and "scene" in msg, msg


@pytest.mark.parametrize("n", [2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1])
def test_oversize_n_is_refused_and_named(hrt, n):
    rc, msg = call(hrt, n=n)
    assert rc == HRT_ERR_INVALID and "n must be" in msg, msg


def test_pointers_are_not_checked_when_n_is_zero(hrt):
    rc, msg = call(hrt, rays=0, out=0, n=0)
    assert rc == HRT_ERR_INVALID and "scene" in msg, msg  # got past the argument checks to the NULL scene


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("flags", [0, EXACT, EXACT | BRUTE, NO_LDS, NORMALIZE, EXACT | BRUTE | NO_LDS | NORMALIZE])
def test_valid_arguments_reach_the_null_scene_check(hrt, mode, flags):
    rc, msg = call(hrt, mode=mode, flags=flags, n=2 ** 31 - 1)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg


def test_python_binding_refuses_a_bad_mode(hrt):
    with pytest.raises(ValueError, match="mode"):
        hrt.DeviceScene.trace_rays(None, [[0] * 8], mode="nearest")
