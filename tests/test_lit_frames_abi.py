"""Lit frames without a GPU (include/hrt.h "Lit frames": hrt_render_lit_device, hrt_render_lit, hrt_render_lit_views_device,
hrt_render_lit_views): the four entry points are exported and declared; every bad argument that can be reached without a device is
refused with HRT_ERR_INVALID and a message that names the entry point and the culprit, in the header's order -- the checks of
hrt_render_lens*, then tail_after, then the volume checks of "Lit rays", then the scene; an empty batch returns HRT_OK.  A volume
cannot be created without a device, so "the volume is NULL" is the last refusal reachable here through the C ABI: what comes after
it (HRT_LIT_VISIBLE without depth, a non-finite bias at the ABI, a closed volume, the scene) is in tests/test_gpu_lit_frames.py, and
the non-finite bias is refused here where a caller meets it first, in the Python wrapper.  The entry points add no host logic of
their own -- they are hrt_render_lens*'s bodies (lens_render_check / lens_views_check) with a LitRule (check, enter) -- so there is no
sanitized stand-alone program for them.  The device pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import probe_volume_ref as pv

HRT_OK, HRT_ERR_INVALID = 0, -1
OUT = 0x2000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
SINGLE = ["hrt_render_lit_device", "hrt_render_lit"]
BATCH = ["hrt_render_lit_views_device", "hrt_render_lit_views"]
NAMES = SINGLE + BATCH
BLOCKING = ["hrt_render_lit", "hrt_render_lit_views"]
NAN, INF = float("nan"), float("inf")
TAIL_RANGE = "tail_after must be in 1 .. HRT_MAXBOUNCES = 6 (got {})"


def lens(hrt, projection="perspective", aperture=0.0, focus=1.0, extent=0.0, cam=None):
    return hrt.Lens(hrt.default_camera(16 / 9) if cam is None else cam, projection, aperture=aperture, focus=focus, extent=extent)


def call(hrt, entry, L=None, null_lens=False, n_views=2, w=16, h=9, first=0, ns=1, seed=1, flags=0, eval_flags=0, bias=0.0, tail=0, out=OUT):
    """One call of `entry` with a NULL scene and a NULL volume.  A batch holds `n_views` copies of the lens, the bad one last."""
    dev = hrt.device_lib()
    L = lens(hrt) if L is None else L
    if entry in SINGLE:
        lp = None if null_lens else C.byref(L)
        if entry == "hrt_render_lit_device":
            rc = dev.hrt_render_lit_device(None, None, lp, w, h, first, ns, seed, flags, eval_flags, bias, tail, C.c_void_p(out), None)
        else:
            rc = dev.hrt_render_lit(None, None, lp, w, h, ns, seed, flags, eval_flags, bias, tail, C.c_void_p(out), None)
    else:
        views = (hrt.LensView * max(n_views, 1))()
        for v in range(n_views):
            C.memmove(C.byref(views[v].lens), C.byref(L if v == n_views - 1 else lens(hrt)), C.sizeof(hrt.Lens))
            views[v].seed = seed + v
        vp = None if null_lens else views
        if entry == "hrt_render_lit_views_device":
            rc = dev.hrt_render_lit_views_device(None, None, vp, n_views, w, h, first, ns, flags, eval_flags, bias, tail, C.c_void_p(out), None)
        else:
            rc = dev.hrt_render_lit_views(None, None, vp, n_views, w, h, ns, flags, eval_flags, bias, tail, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def reaches_the_volume(hrt, entry, **kw):
    """The arguments get past every check of the lens frame and tail_after: the call stops at the NULL volume."""
    rc, msg = call(hrt, entry, **kw)
    return (rc, msg) == (HRT_ERR_INVALID, entry + ": volume is NULL"), msg


LATER = dict(eval_flags=1, bias=NAN, tail=7)  # everything after the lens frame's checks wrong at once


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_four_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_section_and_its_scope(hrt):
    text = pv.header_text()
    assert text.index("/* ---- Lit paths:") < text.index("/* ---- Lit frames:"), "the section comes after \"Lit paths\""
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Lit frames\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("adaptive lit frames", "lit feature buffers", "cooperative or parked look-up", "probes that move", "streaming kernel", "multi-GPU"):
        assert item in scope, item


# -------------------------------------------------------------------------------------------------- the lens frame's checks, first
@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("bit", range(32))
def test_the_flags_are_those_of_a_lens_frame_and_come_first(hrt, entry, bit):
    """An accepted flag bit reaches the next check, a refused one is named -- with every later argument wrong as well."""
    flag = 1 << bit
    rc, msg = call(hrt, entry, flags=flag | (EXACT if flag == BRUTE else 0), null_lens=True, w=0, ns=0, out=0, **LATER)
    taken = {GAMMA, NO_LDS, EXACT, BRUTE} | (set() if entry in BLOCKING else {ACCUMULATE})
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": "), msg
    if flag in taken:
        assert msg == entry + (": lens is NULL" if entry in SINGLE else ": views is NULL"), (bit, msg)
    else:
        assert "flags" in msg, (bit, msg)
        named = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
                 NORMALIZE: "HRT_RAYS_NORMALIZE", ACCUMULATE: "HRT_RADIANCE_ACCUMULATE"}
        assert named[flag] in msg if flag in named else "unknown bits " + str(flag) in msg, (bit, msg)
        if flag == ACCUMULATE:
            assert entry + "_device" in msg, "the blocking form says where the running sums live"


@pytest.mark.parametrize("entry", NAMES)
def test_flag_combinations_are_refused_as_a_lens_frame_refuses_them(hrt, entry):
    rc, msg = call(hrt, entry, flags=BRUTE, **LATER)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg
    if entry not in BLOCKING:
        rc, msg = call(hrt, entry, flags=GAMMA | ACCUMULATE, **LATER)
        assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "HRT_FLAG_GAMMA cannot be combined with HRT_RADIANCE_ACCUMULATE" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_the_lens_is_checked_as_hrt_lens_rays_checks_it(hrt, entry):
    where = entry + (": " if entry in SINGLE else ": views[1].lens: ")
    rc, msg = call(hrt, entry, null_lens=True, **LATER)
    assert (rc, msg) == (HRT_ERR_INVALID, entry + (": lens is NULL" if entry in SINGLE else ": views is NULL"))
    cam = hrt.default_camera(16 / 9)
    cam.fovy_deg = 0.0
    rc, msg = call(hrt, entry, L=lens(hrt, cam=cam), **LATER)
    assert rc == HRT_ERR_INVALID and "render:" in msg and (entry in SINGLE or msg.startswith(where)), msg
    for projection in (4, 2 ** 32 - 1):
        rc, msg = call(hrt, entry, L=lens(hrt, projection), **LATER)
        assert rc == HRT_ERR_INVALID and msg.startswith(where + "projection must be") and str(projection) in msg, msg
    for a in (-1.0, NAN, INF):
        rc, msg = call(hrt, entry, L=lens(hrt, aperture=a, focus=2.0), **LATER)
        assert rc == HRT_ERR_INVALID and msg.startswith(where + "aperture_radius must be finite and >= 0"), (a, msg)
    rc, msg = call(hrt, entry, L=lens(hrt, "equirect", aperture=0.1, focus=2.0), **LATER)
    assert rc == HRT_ERR_INVALID and msg.startswith(where + "aperture_radius must be 0 unless"), msg
    for f in (0.0, NAN):
        rc, msg = call(hrt, entry, L=lens(hrt, aperture=0.1, focus=f), **LATER)
        assert rc == HRT_ERR_INVALID and msg.startswith(where + "focus_distance"), (f, msg)
    for proj, e in (("ortho", 0.0), ("ortho", INF), ("fisheye", 0.0), ("fisheye", 360.5), ("perspective", 1.0), ("equirect", 90.0)):
        rc, msg = call(hrt, entry, L=lens(hrt, proj, extent=e), **LATER)
        assert rc == HRT_ERR_INVALID and msg.startswith(where + "extent must be"), (proj, e, msg)
    for L in (lens(hrt), lens(hrt, aperture=0.2, focus=3.0), lens(hrt, "ortho", extent=2.0), lens(hrt, "equirect"), lens(hrt, "fisheye", extent=200.0)):
        ok, msg = reaches_the_volume(hrt, entry, L=L)
        assert ok, msg


@pytest.mark.parametrize("entry", NAMES)
def test_frame_samples_and_output_in_the_order_of_a_lens_frame(hrt, entry):
    blocking = entry in BLOCKING
    every = dict(w=0, h=0, ns=0, out=0, **LATER)
    rc, msg = call(hrt, entry, **every)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and ("w" in msg and "h" in msg) and "n_samples" not in msg, msg
    rc, msg = call(hrt, entry, **dict(every, w=65536, h=32768))  # w * h = 2^31, one above the limit
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "n_samples" not in msg and "NULL" not in msg, msg
    every.update(w=16, h=9)
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": n_samples must be positive")
    if not blocking:
        for first, ns in ((2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1)):
            rc, msg = call(hrt, entry, **dict(every, first=first, ns=ns))
            assert (rc, msg) == (HRT_ERR_INVALID, entry + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)"), (first, ns)
        ok, msg = reaches_the_volume(hrt, entry, first=2 ** 32 - 1, ns=1)
        assert ok, msg
    every["ns"] = 4
    name = ("out_rgb" if blocking else "d_frame" if entry in SINGLE else "d_frames")
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {name} is NULL")
    assert call(hrt, entry, **dict(every, out=OUT + 2)) == (HRT_ERR_INVALID, f"{entry}: {name} is not 4-byte aligned")
    every["out"] = OUT
    if entry in BATCH:  # the limit of a batch comes after the output: 2^16 views of 2^15 pixels
        rc, msg = call(hrt, entry, **dict(every, n_views=2 ** 16, w=256, h=128))
        assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": n_views * w * h is 2147483648"), msg
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(7)), "tail_after is next"


# ------------------------------------------------------------------------------------------- tail_after, then the volume's checks
@pytest.mark.parametrize("entry", NAMES)
def test_tail_after_then_eval_flags_then_the_volume(hrt, entry):
    for bad in (7, 8, 2 ** 32 - 1):
        assert call(hrt, entry, eval_flags=1, bias=NAN, tail=bad) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(bad)), bad
    for ok in range(0, 7):  # 0 is the one-segment rule; the next check in the header's order
        rc, msg = call(hrt, entry, eval_flags=1, bias=NAN, tail=ok)
        assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": eval_flags: HRT_PROBE_EVAL_RADIANCE"), (ok, msg)
    for bit in range(3, 32):
        assert call(hrt, entry, eval_flags=(1 << bit) | 2, bias=NAN) == (HRT_ERR_INVALID, f"{entry}: eval_flags: unknown bits {1 << bit}"), bit
    for ef in (0, 2, 4, 6):
        assert call(hrt, entry, eval_flags=ef, bias=NAN) == (HRT_ERR_INVALID, entry + ": volume is NULL"), ef


@pytest.mark.parametrize("entry", BATCH)
def test_an_empty_batch_returns_ok_before_anything_that_needs_a_scene(hrt, entry):
    """Nothing but the flags and tail_after is looked at: no views, no frame, no output, no volume, no scene."""
    assert call(hrt, entry, n_views=0, null_lens=True, w=0, h=0, ns=0, out=0, eval_flags=1, bias=NAN)[0] == HRT_OK
    assert call(hrt, entry, n_views=0, null_lens=True, w=0, h=0, ns=0, out=0, tail=6)[0] == HRT_OK
    rc, msg = call(hrt, entry, n_views=0, flags=WAVE)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_WAVE_KERNEL" in msg, msg
    assert call(hrt, entry, n_views=0, tail=7) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(7))
    if entry == "hrt_render_lit_views":
        stats = hrt.Stats()
        stats.samples = 99
        dev = hrt.device_lib()
        assert dev.hrt_render_lit_views(None, None, None, 0, 4, 4, 1, 0, 0, 0.0, 0, None, C.byref(stats)) == HRT_OK and stats.samples == 0


# ------------------------------------------------------------------------------------------------------------------ the wrappers
def test_python_wrappers_check_their_arguments_before_any_library(hrt):
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
    for who, call_ in (("render_lit", lambda **kw: S.render_lit(Fake(), L, vol, 8, 8, 1, **kw)),
                       ("render_lit_views", lambda **kw: S.render_lit_views(Fake(), [L, L], vol, 8, 8, 1, **kw))):
        for bad in (0, 7, -1):
            with pytest.raises(ValueError, match=who + r": tail_after must be in 1 \.\. 6"):
                call_(tail_after=bad)
        for bad in (NAN, INF, -INF):
            with pytest.raises(ValueError, match=who + ": bias must be finite"):
                call_(bias=bad)
        with pytest.raises(ValueError, match=who + ": eval_flags: PROBE_EVAL_RADIANCE"):
            call_(eval_flags=hrt.PROBE_EVAL_RADIANCE)
        with pytest.raises(ValueError, match=who + ": eval_flags: unknown bits 8"):
            call_(eval_flags=8)
    with pytest.raises(ValueError, match="render_lit: volume must be a ProbeVolume"):
        S.render_lit(Fake(), L, None, 8, 8, 1)
    with pytest.raises(ValueError, match="render_lit_views: 2 lenses but 3 seeds"):
        S.render_lit_views(Fake(), [L, L], vol, 8, 8, 1, seeds=[1, 2, 3])
    assert np.float32  # NumPy is the wrappers' own dependency
