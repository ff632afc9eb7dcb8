"""Batched views without a GPU (include/hrt.h hrt_render_views, hrt_render_views_device): both entry points are exported, and
every bad argument -- a flag bit, a kernel-form flag that has no batched build, NULL views, a bad frame size or sample count, a bad
camera at any index, a NULL or misaligned output, too many items -- is refused with HRT_ERR_INVALID and a message that names the
entry point and the culprit, before the scene and the library state are looked at; a NULL scene is refused after those checks;
no views is HRT_OK."""
import ctypes as C
import subprocess

import pytest

from test_radiance_abi import bad_cameras

HRT_OK, HRT_ERR_INVALID = 0, -1
OUT = 0x2000  # a pointer that is never dereferenced: every call below ends in validation
GAMMA, NO_LDS, WAVE, STREAM, NO_CULL, DUAL, EXACT, BRUTE = 1, 2, 4, 8, 16, 32, 64, 128
ACCEPTED = (GAMMA, NO_LDS, WAVE, STREAM, NO_CULL)
ENTRIES = ["hrt_render_views", "hrt_render_views_device"]
MAX_TILES = 1 << 24  # HRT_VIEWS_MAX_TILES


def make_views(hrt, n, cams=None):
    views = (hrt.View * max(n, 1))()
    for v in range(n):
        views[v].cam = hrt.default_camera(16 / 9) if cams is None else cams[v]
        views[v].seed = 1 + v
    return views


def call(hrt, entry, flags=0, views="default", n=3, w=16, h=9, spp=2, out=OUT):
    dev = hrt.device_lib()
    if isinstance(views, str):
        views = make_views(hrt, n)
    rc = getattr(dev, entry)(None, views, n, w, h, spp, flags, C.c_void_p(out), None)  # (last argument: stats / stream)
    return rc, dev.hrt_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_libhrt_exports_both_symbols(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported


def test_view_is_the_header_struct(hrt):
    assert C.sizeof(hrt.View) == 72 and hrt.View.seed.offset == 64 and hrt.View.cam.offset == 0  # 16 floats, a u64


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in ACCEPTED + (DUAL, EXACT, BRUTE)])
def test_every_unknown_flag_bit_is_refused_and_named(hrt, entry, bit):
    rc, msg = call(hrt, entry, flags=(1 << bit) | GAMMA)
    assert rc == HRT_ERR_INVALID and "flags" in msg and str(1 << bit) in msg and msg.startswith(entry + ":"), (bit, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("flag,name", [(DUAL, "HRT_FLAG_DUAL_KERNEL"), (EXACT, "HRT_FLAG_EXACT_ONLY"), (BRUTE, "HRT_FLAG_MESH_BRUTE"),
                                       (EXACT | BRUTE, "HRT_FLAG_EXACT_ONLY"), (BRUTE | GAMMA, "HRT_FLAG_MESH_BRUTE")])
def test_kernel_forms_without_a_batched_build_are_refused_by_name(hrt, entry, flag, name):
    rc, msg = call(hrt, entry, flags=flag)
    assert rc == HRT_ERR_INVALID and name in msg and msg.startswith(entry + ":"), msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_views_are_refused(hrt, entry):
    rc, msg = call(hrt, entry, views=None, n=2)
    assert rc == HRT_ERR_INVALID and "views is NULL" in msg and msg.startswith(entry + ":"), msg


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,word", [(dict(w=0), "w and h"), (dict(h=0), "w and h"), (dict(spp=0), "spp"),
                                     (dict(w=65536, h=1), "65536"), (dict(w=1, h=65536), "65536"), (dict(w=70000, h=3), "65536"),
                                     (dict(w=65535, h=65535), "w * h")])
def test_bad_frame_sizes_and_sample_counts_are_refused_and_named(hrt, entry, kw, word):
    rc, msg = call(hrt, entry, **kw)
    assert rc == HRT_ERR_INVALID and word in msg and msg.startswith(entry + ":"), (kw, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n,at", [(1, 0), (5, 0), (5, 4), (5, 2)])
def test_a_bad_camera_is_refused_with_its_index(hrt, entry, n, at):
    for what, bad in bad_cameras(hrt):  # the cameras hrt_render refuses (make_camera), with its message behind the index
        cams = [hrt.default_camera(16 / 9) for _ in range(n)]
        cams[at] = bad
        rc, msg = call(hrt, entry, views=make_views(hrt, n, cams), n=n)
        assert rc == HRT_ERR_INVALID and f"views[{at}]" in msg and ("camera" in msg or "inverse" in msg) and msg.startswith(entry + ":"), (what, msg)


@pytest.mark.parametrize("entry,word", [("hrt_render_views", "out_rgb"), ("hrt_render_views_device", "d_frames")])
@pytest.mark.parametrize("out", [0, OUT + 1, OUT + 2, OUT + 3])
def test_a_null_or_misaligned_output_is_refused_and_named(hrt, entry, word, out):
    rc, msg = call(hrt, entry, out=out)
    assert rc == HRT_ERR_INVALID and word in msg and msg.startswith(entry + ":"), msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_item_count_over_the_limit_is_refused_and_named(hrt, entry):
    # 32768 x 32768 pixels are 4096 x 4096 = 2^24 tiles: one view is exactly the limit, two are over it; 2^24 + 1 one-tile views too
    rc, msg = call(hrt, entry, n=2, w=32768, h=32768)
    assert rc == HRT_ERR_INVALID and "HRT_VIEWS_MAX_TILES" in msg and str(2 * MAX_TILES) in msg and msg.startswith(entry + ":"), msg
    rc, msg = call(hrt, entry, n=1, w=32768, h=32768)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg
    rc, msg = call(hrt, entry, n=3, w=32768, h=8 * 1366)  # 3 x 4096 x 1366 = 16 785 408 > 2^24 >= 2 x 4096 x 1366
    assert rc == HRT_ERR_INVALID and "HRT_VIEWS_MAX_TILES" in msg, msg
    rc, msg = call(hrt, entry, n=2, w=32768, h=8 * 1366)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_checks_run_in_the_stated_order(hrt, entry):
    bad = bad_cameras(hrt)[0][1]
    # each call is wrong in everything from its place in the list on: the first wrong thing is the one that is named
    steps = [(dict(flags=1 << 20, views=None, w=0, out=0), "flags"),
             (dict(views=None, w=0, out=0), "views is NULL"),
             (dict(views=make_views(hrt, 3, [bad] * 3), w=0, out=0), "w and h"),
             (dict(views=make_views(hrt, 3, [bad] * 3), spp=0, out=0), "spp"),
             (dict(views=make_views(hrt, 3, [bad] * 3), out=0), "views[0]"),
             (dict(out=0, w=32768, h=32768), "NULL"),
             (dict(w=32768, h=32768), "HRT_VIEWS_MAX_TILES")]
    for kw, word in steps:
        rc, msg = call(hrt, entry, **kw)
        assert rc == HRT_ERR_INVALID and word in msg and "scene" not in msg, (kw, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("flags", [0, GAMMA, WAVE, STREAM, NO_LDS | NO_CULL, GAMMA | NO_LDS | WAVE | STREAM | NO_CULL])
def test_valid_arguments_reach_the_null_scene_check(hrt, entry, flags):
    rc, msg = call(hrt, entry, flags=flags, w=65535, h=9, spp=2 ** 32 - 1)
    assert rc == HRT_ERR_INVALID and "scene is NULL" in msg and msg.startswith(entry + ":"), msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_views_is_ok_and_looks_at_nothing_but_the_flags(hrt, entry):
    assert call(hrt, entry, n=0)[0] == HRT_OK
    assert call(hrt, entry, n=0, views=None, out=0, w=0, h=0, spp=0)[0] == HRT_OK
    rc, msg = call(hrt, entry, n=0, flags=EXACT)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_EXACT_ONLY" in msg, msg


def test_python_binding_checks_seeds_and_out_before_any_call(hrt):
    cams = [hrt.default_camera(1.0)] * 2
    with pytest.raises(ValueError, match="seeds"):
        hrt.DeviceScene.render_views(None, cams, 8, 8, 1, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="out must be"):
        hrt.DeviceScene.render_views(None, cams, 8, 8, 1, out=[[0.0]])
