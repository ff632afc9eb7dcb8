"""Batched lens views without a GPU (include/hrt.h hrt_render_lens_views_device, hrt_render_lens_views,
hrt_render_lens_views_features): the three entry points are exported, hrt_lens_view has the header's layout, and every bad argument
is refused with HRT_ERR_INVALID and a message that names the entry point and the culprit, in the header's order -- flags, (an empty
batch returns HRT_OK,) views, every lens with its index, the frame, the samples, the output pointer, the item limit -- before the
scene and the library state are looked at; a NULL scene is refused after those checks.  The device pointers below are never
dereferenced: every call fails validation first, or has nothing to do."""
import ctypes as C
import os
import re
import subprocess

import pytest

HRT_OK, HRT_ERR_INVALID = 0, -1
OUT = 0x2000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
DEVICE, HOST, FEATURES = "hrt_render_lens_views_device", "hrt_render_lens_views", "hrt_render_lens_views_features"
NAMES = [DEVICE, HOST, FEATURES]
FRAMES = [DEVICE, HOST]
NAN, INF = float("nan"), float("inf")
MAX_PIXELS = 2 ** 31 - 1
MAX_RECORDS = MAX_PIXELS // 16


def lens(hrt, projection="perspective", aperture=0.0, focus=1.0, extent=0.0, cam=None):
    return hrt.Lens(hrt.default_camera(16 / 9) if cam is None else cam, projection, aperture=aperture, focus=focus, extent=extent)


def batch(hrt, lenses, seeds=None):
    views = (hrt.LensView * max(len(lenses), 1))()
    for v, L in enumerate(lenses):
        C.memmove(C.byref(views[v].lens), C.byref(L), C.sizeof(hrt.Lens))
        views[v].seed = v + 1 if seeds is None else seeds[v]
    return views


def call(hrt, entry, lenses=None, views="valid", n=None, w=16, h=9, first=0, ns=1, flags=0, out=OUT):
    """One call of `entry` with a NULL scene.  lenses: the batch (default: three valid ones); views=None passes a NULL array;
    n overrides the view count."""
    dev = hrt.device_lib()
    if lenses is None:
        lenses = [lens(hrt), lens(hrt, "equirect"), lens(hrt, aperture=0.1, focus=2.0)]
    arr = None if views is None else batch(hrt, lenses)
    n = len(lenses) if n is None else n
    if entry == DEVICE:
        rc = dev.hrt_render_lens_views_device(None, arr, n, w, h, first, ns, flags, C.c_void_p(out), None)
    elif entry == HOST:
        rc = dev.hrt_render_lens_views(None, arr, n, w, h, ns, flags, C.c_void_p(out), None)
    else:
        rc = dev.hrt_render_lens_views_features(None, arr, n, w, h, first, ns, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


def big(entry):
    """A frame within the single-frame limit of `entry` of which the default batch of three is above the item limit."""
    side = 2 ** 13 if entry == FEATURES else 2 ** 15
    return dict(w=side, h=side)


def passes(hrt, entry, **kw):
    """The arguments get past every check before the last: the call stops at the NULL scene."""
    rc, msg = call(hrt, entry, **kw)
    return (rc == HRT_ERR_INVALID and entry + ": scene is NULL" in msg), msg


def refused(hrt, entry, word, **kw):
    rc, msg = call(hrt, entry, **kw)
    return (rc == HRT_ERR_INVALID and msg.startswith(entry + ":") and word in msg and "scene" not in msg), msg


# ------------------------------------------------------------------------------------------------------------ symbols, layout
@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_three_symbols(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported


def test_libhrt_still_exports_exactly_the_functions_of_the_header(hrt):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip() and line.split()[-2] in "TtWw"}
    header = open(os.path.join(hrt.REPO_ROOT, "include", "hrt.h")).read()
    declared = set(re.findall(r"^HRT_API [^;(]*?[ *](hrt_[a-z_0-9]+)\(", header, re.M))
    assert set(NAMES) <= declared
    assert {e for e in exported if e.startswith("hrt_")} == declared


def test_the_struct_has_the_headers_layout(hrt):
    V = hrt.LensView
    assert C.sizeof(hrt.Lens) == 80
    assert C.sizeof(V) == C.sizeof(hrt.Lens) + 8 == 88
    assert (V.lens.offset, V.seed.offset) == (0, C.sizeof(hrt.Lens))
    assert V.seed.size == 8
    header = open(os.path.join(hrt.REPO_ROOT, "include", "hrt.h")).read()
    assert re.search(r"typedef struct hrt_lens_view \{\s*hrt_lens lens;\s*uint64_t seed;\s*\} hrt_lens_view;", header)


# ------------------------------------------------------------------------------------------------------------------- 1. flags
KNOWN = (GAMMA, NO_LDS, EXACT, BRUTE, ACCUMULATE)
BY_NAME = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
           NORMALIZE: "HRT_RAYS_NORMALIZE"}


@pytest.mark.parametrize("entry", FRAMES)
@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in KNOWN])
def test_every_other_flag_bit_is_refused_and_named(hrt, entry, bit):
    ok, msg = refused(hrt, entry, "flags", flags=1 << bit)
    assert ok and BY_NAME.get(1 << bit, str(1 << bit)) in msg, (bit, msg)


@pytest.mark.parametrize("entry", FRAMES)
def test_the_flags_are_refused_by_the_single_frames_texts(hrt, entry):
    """The same names and texts as hrt_render_lens_device / hrt_render_lens give, with the new entry point's name in front."""
    dev = hrt.device_lib()
    single = {DEVICE: "hrt_render_lens_device", HOST: "hrt_render_lens"}[entry]
    L = lens(hrt)
    for flags in (WAVE, STREAM, DUAL, NO_SHADOW_CULL, NORMALIZE, 1 << 20, BRUTE, BRUTE | GAMMA, GAMMA | ACCUMULATE, ACCUMULATE | WAVE):
        if single == "hrt_render_lens_device":
            rc1 = dev.hrt_render_lens_device(None, C.byref(L), 16, 9, 0, 1, 1, flags, C.c_void_p(OUT), None)
        else:
            rc1 = dev.hrt_render_lens(None, C.byref(L), 16, 9, 1, 1, flags, C.c_void_p(OUT), None)
        want = dev.hrt_last_error().decode()
        rc, msg = call(hrt, entry, flags=flags)
        assert rc == rc1 == HRT_ERR_INVALID and want.startswith(single + ": "), (flags, want)
        tail = want[len(single):]
        if entry == HOST and flags & ACCUMULATE:  # the text points at the device form, by its name
            tail = tail.replace("hrt_render_lens_device", "hrt_render_lens_views_device")
        assert msg == entry + tail, (flags, msg, want)


@pytest.mark.parametrize("entry", FRAMES)
def test_flag_combinations(hrt, entry):
    for flags in (0, EXACT, EXACT | BRUTE, NO_LDS, GAMMA, EXACT | BRUTE | NO_LDS | GAMMA):
        ok, msg = passes(hrt, entry, flags=flags)
        assert ok, (flags, msg)
    ok, msg = passes(hrt, DEVICE, flags=ACCUMULATE | EXACT | BRUTE | NO_LDS)
    assert ok, msg
    ok, msg = refused(hrt, DEVICE, "HRT_FLAG_GAMMA", flags=GAMMA | ACCUMULATE)
    assert ok and "ACCUMULATE" in msg, msg
    ok, msg = refused(hrt, HOST, "HRT_RADIANCE_ACCUMULATE", flags=ACCUMULATE)  # the host form has no running sums to add to
    assert ok, msg


@pytest.mark.parametrize("entry", FRAMES)
def test_flags_come_first(hrt, entry):
    bad = [lens(hrt), lens(hrt), lens(hrt, 9)]
    for kw in (dict(n=0), dict(views=None), dict(lenses=bad), dict(w=0), dict(ns=0), dict(out=0), dict(w=2 ** 15, h=2 ** 15)):
        ok, msg = refused(hrt, entry, "HRT_FLAG_WAVE_KERNEL", flags=WAVE, **kw)
        assert ok, (kw, msg)


# ------------------------------------------------------------------------------------------------------------ 2. an empty batch
@pytest.mark.parametrize("entry", NAMES)
def test_an_empty_batch_is_ok_whatever_comes_after_it(hrt, entry):
    for kw in (dict(), dict(views=None), dict(w=0, h=0), dict(ns=0, first=2 ** 32 - 1), dict(out=0), dict(out=OUT + 1),
               dict(views=None, w=0, h=0, ns=0, out=0)):
        rc, msg = call(hrt, entry, lenses=[], n=0, **kw)
        assert rc == HRT_OK, (kw, msg)


def test_an_empty_batch_zeroes_the_stats(hrt):
    dev = hrt.device_lib()
    st = hrt.Stats()
    st.samples, st.kernel_ms, st.total_ms = 99, 1.5, 2.5
    assert dev.hrt_render_lens_views(None, None, 0, 16, 9, 1, 0, None, C.byref(st)) == HRT_OK
    assert (st.samples, st.kernel_ms, st.total_ms, st.vgprs, st.lds_bytes, st.waves_launched) == (0, 0.0, 0.0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------- 3. views NULL
@pytest.mark.parametrize("entry", NAMES)
def test_null_views_are_refused_before_everything_behind_them(hrt, entry):
    for kw in (dict(), dict(w=0), dict(ns=0), dict(out=0), big(entry)):
        ok, msg = refused(hrt, entry, "views is NULL", views=None, n=3, **kw)
        assert ok, (kw, msg)


# --------------------------------------------------------------------------------------------------------------- 4. the lenses
def bad_lenses(hrt):
    """(what, lens, word of the message)"""
    out = [("projection", lens(hrt, 7), "projection"), ("aperture", lens(hrt, aperture=-1.0), "aperture_radius"),
           ("aperture off perspective", lens(hrt, "equirect", aperture=0.1), "aperture_radius"),
           ("focus", lens(hrt, aperture=0.1, focus=0.0), "focus_distance"), ("ortho extent", lens(hrt, "ortho"), "extent"),
           ("fisheye extent", lens(hrt, "fisheye", extent=361.0), "extent"), ("perspective extent", lens(hrt, extent=1.0), "extent")]
    c = hrt.default_camera(16 / 9); c.fovy_deg = 0.0; out.append(("fovy 0", lens(hrt, cam=c), "render:"))
    c = hrt.default_camera(16 / 9); c.eye[0] = NAN; out.append(("NaN eye", lens(hrt, "equirect", cam=c), "render:"))
    return out


@pytest.mark.parametrize("entry", NAMES)
def test_a_bad_lens_is_reported_with_the_index_of_its_view(hrt, entry):
    good = lens(hrt, "fisheye", extent=180.0)
    for what, bad, word in bad_lenses(hrt):
        for n, at in ((3, 2), (3, 0), (1, 0), (5, 3)):
            lenses = [good] * n
            lenses[at] = bad
            ok, msg = refused(hrt, entry, f"views[{at}].lens", lenses=lenses)
            assert ok and word in msg, (what, n, at, msg)


@pytest.mark.parametrize("entry", NAMES)
def test_the_first_bad_lens_wins_and_its_fields_keep_their_order(hrt, entry):
    good = lens(hrt)
    ok, msg = refused(hrt, entry, "views[1].lens", lenses=[good, lens(hrt, 7), lens(hrt, aperture=-1.0)])
    assert ok and "projection" in msg, msg
    cam = hrt.default_camera(16 / 9); cam.right[:] = (0, 0, 0)
    everything = lens(hrt, 7, aperture=-1.0, focus=-1.0, extent=-1.0, cam=cam)  # the camera speaks first, then the projection
    ok, msg = refused(hrt, entry, "views[2].lens", lenses=[good, good, everything])
    assert ok and ("camera" in msg or "inverse" in msg), msg
    ok, msg = refused(hrt, entry, "views[2].lens", lenses=[good, good, lens(hrt, 7, aperture=-1.0, focus=-1.0, extent=-1.0)])
    assert ok and "projection" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_a_bad_lens_comes_before_the_frame_the_samples_the_pointer_and_the_limit(hrt, entry):
    lenses = [lens(hrt), lens(hrt), lens(hrt, "ortho")]
    for kw in (dict(w=0), dict(ns=0, first=2 ** 32 - 1), dict(first=2 ** 32 - 1, ns=2), dict(out=0), dict(out=OUT + 2), big(entry)):
        ok, msg = refused(hrt, entry, "views[2].lens", lenses=lenses, **kw)
        assert ok and "extent" in msg, (kw, msg)


@pytest.mark.parametrize("entry", NAMES)
def test_views_may_differ_in_everything(hrt, entry):
    cam = hrt.default_camera(2.0)
    cam.eye[:] = (3.0, -2.0, 5.0)
    lenses = [lens(hrt), lens(hrt, aperture=0.2, focus=4.0), lens(hrt, "ortho", extent=3.0, cam=cam), lens(hrt, "equirect"),
              lens(hrt, "fisheye", extent=220.0), lens(hrt, focus=NAN)]
    ok, msg = passes(hrt, entry, lenses=lenses)
    assert ok, msg


# ---------------------------------------------------------------------------------------------------------------- 5. the frame
@pytest.mark.parametrize("entry", NAMES)
def test_the_frame(hrt, entry):
    for w, h in ((0, 9), (16, 0), (0, 0)):
        ok, msg = refused(hrt, entry, "w and h", w=w, h=h, ns=0, first=2 ** 32 - 1, out=0)  # before the samples and the pointer
        assert ok, (w, h, msg)
    for w, h in ((2 ** 31, 1), (1, 2 ** 31), (46341, 46341), (2 ** 32 - 1, 2 ** 32 - 1)):
        ok, msg = refused(hrt, entry, "w * h", w=w, h=h, out=0)
        assert ok, (w, h, msg)


# -------------------------------------------------------------------------------------------------------------- 6, 7. samples
@pytest.mark.parametrize("entry", FRAMES)
def test_zero_samples_are_refused_and_named(hrt, entry):
    for first in (0, 5, 2 ** 32 - 1):
        ok, msg = refused(hrt, entry, "n_samples", first=first, ns=0, out=0)
        assert ok, msg


def test_zero_samples_of_features_are_the_pixel_centres(hrt):
    ok, msg = passes(hrt, FEATURES, ns=0)
    assert ok, msg


@pytest.mark.parametrize("first,ns", [(2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1), (2 ** 32 - 8, 9)])
def test_sample_indices_that_would_wrap_are_refused_and_named(hrt, first, ns):
    ok, msg = refused(hrt, DEVICE, "first_sample", first=first, ns=ns, out=0)  # before the pointer
    assert ok and "wrap" in msg, msg
    ok, msg = refused(hrt, FEATURES, "first_sample", first=first, ns=ns, out=0)
    assert ok, msg


@pytest.mark.parametrize("first,ns", [(2 ** 32 - 1, 1), (0, 2 ** 32 - 1), (2 ** 31, 2 ** 31), (7, 2 ** 32 - 7)])
def test_the_last_sample_index_is_allowed(hrt, first, ns):
    ok, msg = passes(hrt, DEVICE, first=first, ns=ns)
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------- 8. the pointer
@pytest.mark.parametrize("entry,word", [(DEVICE, "d_frames"), (HOST, "out_rgb"), (FEATURES, "d_features")])
def test_a_null_or_misaligned_output_is_refused_and_named(hrt, entry, word):
    ok, msg = refused(hrt, entry, word + " is NULL", out=0, **big(entry))  # before the limit
    assert ok, msg
    for out in (OUT + 1, OUT + 2, OUT + 3):
        ok, msg = refused(hrt, entry, word + " is not 4-byte aligned", out=out, **big(entry))
        assert ok, (out, msg)
    for out in (OUT + 4, OUT + 12):
        ok, msg = passes(hrt, entry, out=out)
        assert ok, (out, msg)


# --------------------------------------------------------------------------------------------------------------- 9. the limit
@pytest.mark.parametrize("entry", NAMES)
def test_the_item_limit(hrt, entry):
    """n_views * w * h above the pixel limit of the single-frame call is refused, by the product, after every view was checked: the
    array holds exactly n_views entries, so nothing beyond them can have been read; one item fewer passes."""
    limit = MAX_RECORDS if entry == FEATURES else MAX_PIXELS
    side = 2 ** 13 if entry == FEATURES else 2 ** 15          # one frame alone is within the limit ...
    n = limit // (side * side) + 1                            # ... n of them are not
    assert side * side <= limit < n * side * side
    lenses = [lens(hrt, "equirect")] * n
    ok, msg = refused(hrt, entry, "n_views * w * h", lenses=lenses, w=side, h=side)
    assert ok and str(n * side * side) in msg and str(limit) in msg, msg
    ok, msg = passes(hrt, entry, lenses=lenses[:n - 1], w=side, h=side)
    assert ok, msg
    # the largest batches that pass: the limit itself in 1-pixel-high frames
    w = limit // 7
    ok, msg = passes(hrt, entry, lenses=[lens(hrt)] * 7, w=w, h=1)
    assert ok, msg
    ok, msg = refused(hrt, entry, "n_views * w * h", lenses=[lens(hrt)] * 7, w=w + 1, h=1)
    assert ok, msg
    bad = lenses[:n - 1] + [lens(hrt, 9)]                     # the lens of the last view still speaks before the limit
    ok, msg = refused(hrt, entry, f"views[{n - 1}].lens", lenses=bad, w=side, h=side)
    assert ok, msg


# -------------------------------------------------------------------------------------------------------------- 10. the scene
@pytest.mark.parametrize("entry", NAMES)
def test_the_checks_come_in_the_headers_order(hrt, entry):
    frames = entry != FEATURES
    bad = [lens(hrt), lens(hrt), lens(hrt, 9)]
    steps = []
    if frames:
        steps.append(("flags", dict(flags=WAVE, views=None, n=3, w=0, ns=0, out=0)))
    steps += [("views is NULL", dict(views=None, n=3, w=0, ns=0 if frames else 1, out=0)),
              ("views[2].lens", dict(lenses=bad, w=0, ns=0 if frames else 1, out=0)),
              ("w and h", dict(w=0, ns=0 if frames else 1, first=2 ** 32 - 1, out=0))]
    if frames:
        steps.append(("n_samples", dict(ns=0, first=2 ** 32 - 1, out=0, **big(entry))))
    if entry != HOST:  # the blocking form renders samples [0, spp): they cannot wrap
        steps.append(("first_sample", dict(ns=2, first=2 ** 32 - 1, out=0, **big(entry))))
    steps += [("is NULL", dict(out=0, **big(entry))),
              ("aligned", dict(out=OUT + 2, **big(entry))),
              ("n_views * w * h", big(entry))]
    for word, kw in steps:
        ok, msg = refused(hrt, entry, word, **kw)
        assert ok, (word, msg)
    ok, msg = passes(hrt, entry)
    assert ok, msg


# ------------------------------------------------------------------------------------------------------------------- Python
def test_python_binding_checks_its_arguments(hrt):
    import numpy as np
    L = lens(hrt)
    with pytest.raises(ValueError, match="seeds"):
        hrt.DeviceScene.render_lens_views(None, [L, L], 16, 9, 1, seeds=[1])
    with pytest.raises(ValueError, match="out"):
        hrt.DeviceScene.render_lens_views(None, [L, L], 16, 9, 1, out=np.zeros((2, 9, 16, 4), np.float32))
    with pytest.raises(ValueError, match="out"):
        hrt.DeviceScene.render_lens_views(None, [L, L], 16, 9, 1, out=np.zeros((1, 9, 16, 3), np.float32))
    with pytest.raises(ValueError, match="accumulate"):
        hrt.DeviceScene.render_lens_views(None, [L], 16, 9, 1, first_sample=3, accumulate=True)
    with pytest.raises(ValueError, match="seeds"):
        hrt.DeviceScene.render_lens_views_features(None, [L], 16, 9, 0, 1, seeds=[1, 2])
