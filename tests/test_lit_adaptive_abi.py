"""Adaptive lit frames without a GPU (include/hrt.h "Adaptive lit frames": hrt_render_lit_adaptive_device, hrt_render_lit_adaptive):
the two entry points are exported and declared; every bad argument that can be reached without a device is refused with
HRT_ERR_INVALID and a message that names the entry point and the culprit, in the header's order -- everything
hrt_render_lens_adaptive checks before the scene, in its order (flags, params, the lens, the frame, the limit, the output pointers),
then tail_after, then the volume checks of "Lit rays".  A volume cannot be created without a device, so "the volume is NULL" is the
last refusal reachable here through the C ABI: what comes after it is in tests/test_gpu_lit_adaptive.py, and the non-finite bias is
refused here where a caller meets it first, in the Python wrapper.  The entry points add no host logic of their own -- they compose
lens_adaptive_check and a LitRule's check and enter -- so there is no sanitized stand-alone program for them.
The pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import probe_volume_ref as pv

HRT_OK, HRT_ERR_INVALID = 0, -1
OUT, SPP = 0x2000, 0x3000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ["hrt_render_lit_adaptive_device", "hrt_render_lit_adaptive"]
NAN, INF = float("nan"), float("inf")
TAIL_RANGE = "tail_after must be in 1 .. HRT_MAXBOUNCES = 6 (got {})"


def lens(hrt, projection="perspective", aperture=0.0, focus=1.0, extent=0.0, cam=None):
    return hrt.Lens(hrt.default_camera(16 / 9) if cam is None else cam, projection, aperture=aperture, focus=focus, extent=extent)


def call(hrt, entry, L=None, null_lens=False, w=16, h=9, params=(4, 32, 0.1), seed=1, flags=0, eval_flags=0, bias=0.0, tail=0, out=OUT, spp=SPP):
    """One call of `entry` with a NULL scene and a NULL volume."""
    dev = hrt.device_lib()
    L = lens(hrt) if L is None else L
    lp = None if null_lens else C.byref(L)
    pp = None if params is None else C.byref(hrt.Adaptive(*params))
    if entry == "hrt_render_lit_adaptive_device":
        rc = dev.hrt_render_lit_adaptive_device(None, None, lp, w, h, pp, seed, flags, eval_flags, bias, tail, C.c_void_p(out), C.c_void_p(spp), None)
    else:
        rc = dev.hrt_render_lit_adaptive(None, None, lp, w, h, pp, seed, flags, eval_flags, bias, tail, C.c_void_p(out), C.c_void_p(spp), None)
    return rc, dev.hrt_last_error().decode()


def names(entry):
    return ("d_frame", "d_tile_spp") if entry.endswith("_device") else ("out_rgb", "out_tile_spp")


LATER = dict(eval_flags=1, bias=NAN, tail=7)  # everything after the lens frame's checks wrong at once


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_two_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_section_its_contract_and_its_scope(hrt):
    text = pv.header_text()
    assert text.index("/* ---- Lit frames:") < text.index("/* ---- Lit bakes:") < text.index("/* ---- Adaptive lit frames:")
    section = text[text.index("/* ---- Adaptive lit frames:"):]
    flat = re.sub(r"\s*\n \* ", " ", section)
    assert "CONTRACT A: every tile of the result is bit-identical to the same tile of hrt_render_lit(volume, lens, w, h, count of that tile" in flat
    assert "may NOT overlap another adaptive call of the same scene" in flat
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Adaptive lit frames\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("batched views", "rank partitions", "denoising of adaptive frames", "streaming kernel", "multi-GPU"):
        assert item in scope, item
    # the older sections still say what they said: their sentences remain true of THEIR entry points
    old = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Lit frames\"\): ([^/]*)\*/", text)
    assert old and "adaptive lit frames" in re.sub(r"\s*\n \* ", " ", old.group(1))


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("bit", range(32))
def test_the_flags_are_those_of_an_adaptive_lens_frame_and_come_first(hrt, entry, bit):
    """An accepted flag bit reaches the next check, a refused one is named -- with every later argument wrong as well."""
    flag = 1 << bit
    rc, msg = call(hrt, entry, flags=flag | (EXACT if flag == BRUTE else 0), params=None, null_lens=True, w=0, out=0, spp=SPP + 2, **LATER)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": "), msg
    if flag in {GAMMA, NO_LDS, EXACT, BRUTE}:
        assert msg == entry + ": params is NULL", (bit, msg)
    else:
        assert "flags" in msg, (bit, msg)
        named = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
                 NORMALIZE: "HRT_RAYS_NORMALIZE", ACCUMULATE: "HRT_RADIANCE_ACCUMULATE"}
        assert named[flag] in msg if flag in named else "unknown bits " + str(flag) in msg, (bit, msg)
        if flag == ACCUMULATE:
            assert "the rounds keep the running sums themselves" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_params_lens_frame_limit_and_outputs_in_the_order_of_an_adaptive_lens_frame(hrt, entry):
    on, sn = names(entry)
    rc, msg = call(hrt, entry, flags=BRUTE, **LATER)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg
    every = dict(params=None, null_lens=True, w=0, h=0, out=0, spp=SPP + 2, **LATER)
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": params is NULL")
    for bad, text in (((3, 32, 0.1), "min_spp must be even and at least 2 (got 3)"), ((0, 32, 0.1), "min_spp must be even and at least 2 (got 0)"),
                      ((8, 4, 0.1), "max_spp must be at least min_spp (got 4 < 8)"), ((4, 32, NAN), "threshold must be a non-negative number"),
                      ((4, 32, -1.0), "threshold must be a non-negative number")):
        rc, msg = call(hrt, entry, **dict(every, params=bad))
        assert rc == HRT_ERR_INVALID and msg.startswith(f"{entry}: {text}"), (bad, msg)
    every["params"] = (4, 32, INF)
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": lens is NULL")
    every["null_lens"] = False
    for proj, e in (("ortho", 0.0), ("fisheye", 360.5)):
        rc, msg = call(hrt, entry, **dict(every, L=lens(hrt, proj, extent=e)))
        assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": extent must be"), (proj, e, msg)
    rc, msg = call(hrt, entry, **every)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "w" in msg and "h" in msg and "NULL" not in msg, msg
    rc, msg = call(hrt, entry, **dict(every, w=65536, h=32768))  # w * h = 2^31, one above the limit
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "NULL" not in msg, msg
    rc, msg = call(hrt, entry, **dict(every, w=2 ** 31 - 1, h=1))  # a frame within the pixel limit whose tiles * 64 are not
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": frame too large: tiles * 64 is"), msg
    every.update(w=16, h=9)
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")
    assert call(hrt, entry, **dict(every, out=OUT + 2)) == (HRT_ERR_INVALID, f"{entry}: {on} is not 4-byte aligned")
    every["out"] = OUT
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {sn} is not 4-byte aligned")
    every["spp"] = SPP
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(7)), "tail_after is next"
    assert call(hrt, entry, **dict(every, spp=0, tail=0, eval_flags=0)) == (HRT_ERR_INVALID, entry + ": volume is NULL"), "the counts may be NULL"


@pytest.mark.parametrize("entry", NAMES)
def test_tail_after_then_eval_flags_then_the_volume(hrt, entry):
    for bad in (7, 8, 2 ** 32 - 1):
        assert call(hrt, entry, eval_flags=1, bias=NAN, tail=bad) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(bad)), bad
    for ok in range(0, 7):  # 0 is the one-segment rule; the next check in the header's order
        rc, msg = call(hrt, entry, eval_flags=1, bias=NAN, tail=ok)
        assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": eval_flags: HRT_PROBE_EVAL_RADIANCE"), (ok, msg)
    for bit in range(3, 32):
        assert call(hrt, entry, eval_flags=(1 << bit) | 2, bias=NAN) == (HRT_ERR_INVALID, f"{entry}: eval_flags: unknown bits {1 << bit}"), bit
    for ef in (0, 2, 4, 6):  # the last refusal reachable without a device
        for L in (lens(hrt), lens(hrt, aperture=0.2, focus=3.0), lens(hrt, "ortho", extent=2.0), lens(hrt, "equirect"), lens(hrt, "fisheye", extent=180.0)):
            assert call(hrt, entry, L=L, eval_flags=ef, bias=NAN) == (HRT_ERR_INVALID, entry + ": volume is NULL"), ef


def test_the_python_wrapper_checks_its_arguments_before_any_library(hrt):
    V, S = hrt.ProbeVolume, hrt.DeviceScene

    class Fake:  # stands in for a scene: no method may reach its handle before the arguments are right
        @property
        def _h(self):
            raise AssertionError("the library was reached")

    class FakeVolume(V):  # a volume that was never created
        def __init__(self):
            pass

        def __del__(self):
            pass

        @property
        def _h(self):
            raise AssertionError("the library was reached")

    vol, L = FakeVolume(), lens(hrt)
    who = "render_lit_adaptive"
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match=who + r": tail_after must be in 1 \.\. 6"):
            S.render_lit_adaptive(Fake(), L, vol, 8, 8, 4, 32, 0.1, tail_after=bad)
    for bad in (NAN, INF, -INF):
        with pytest.raises(ValueError, match=who + ": bias must be finite"):
            S.render_lit_adaptive(Fake(), L, vol, 8, 8, 4, 32, 0.1, bias=bad)
    with pytest.raises(ValueError, match=who + ": eval_flags: PROBE_EVAL_RADIANCE"):
        S.render_lit_adaptive(Fake(), L, vol, 8, 8, 4, 32, 0.1, eval_flags=hrt.PROBE_EVAL_RADIANCE)
    with pytest.raises(ValueError, match=who + ": eval_flags: unknown bits 8"):
        S.render_lit_adaptive(Fake(), L, vol, 8, 8, 4, 32, 0.1, eval_flags=8)
    with pytest.raises(ValueError, match=who + ": volume must be a ProbeVolume"):
        S.render_lit_adaptive(Fake(), L, None, 8, 8, 4, 32, 0.1)
    assert np.float32  # NumPy is the wrapper's own dependency
