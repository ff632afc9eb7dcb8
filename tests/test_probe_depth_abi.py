"""Probe visibility without a GPU (include/hrt.h "Probe visibility"): the eight entry points are exported and declared and the
constants are the header's; every bad argument that can be reached without a device is refused with HRT_ERR_INVALID and a message
that names the entry point and the culprit, in the header's order; the shared headers csrc/hrt_probe_depth_oct.h and the visibility
piece of csrc/hrt_probe_volume_cell.h equal tests/probe_depth_ref.py bit for bit in a stand-alone program built with the address and
undefined-behaviour sanitizers (make probe_depth_check); the Python wrapper refuses before it touches a library; the command-line
tool refuses what it cannot combine.  A volume cannot be created without a device, so the checks that come after "the volume is
NULL" are exercised in tests/test_gpu_probe_depth.py.  The device pointers below are never dereferenced: every call fails
validation first."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import probe_depth_ref as pd
import probe_volume_ref as pv
from conftest import PKG, ROOT

HRT_OK, HRT_ERR_INVALID = 0, -1
PROBES, KEYS, OUT, PTS = 0x1000, 0x3000, 0x2000, 0x4000
RADIANCE, FACING = 1, 2
EXACT, BRUTE, NO_LDS, ACCUMULATE = 64, 128, 2, 512
NAMES = ["hrt_probe_depth_device", "hrt_probe_depth", "hrt_probe_volume_update_depth_device", "hrt_probe_volume_update_depth",
         "hrt_probe_eval_visible_device", "hrt_probe_eval_visible", "hrt_probe_depth_texel", "hrt_probe_depth_direction"]
DEPTH = ["hrt_probe_depth_device", "hrt_probe_depth"]
VISIBLE = ["hrt_probe_eval_visible_device", "hrt_probe_eval_visible"]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


# ------------------------------------------------------------------------------------------------------------------- exports
@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_eight_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_headers_constants(hrt):
    text = pv.header_text()
    for name, literal, value in (("RES", "8u", 8), ("TEXELS", "64u", 64), ("FLOATS", "192u", 192), ("MAX_BLOCKS", r"\(1u << 20\)", 1 << 20),
                                 ("VOLUME_MAX", r"\(1u << 22\)", 1 << 22)):
        assert re.search(r"#define HRT_PROBE_DEPTH_" + name + " +" + literal + r"(\s|$)", text), name
        assert getattr(hrt, "PROBE_DEPTH_" + name) == value, name
    assert hrt.PROBE_DEPTH_TEXELS == hrt.PROBE_DEPTH_RES ** 2 and hrt.PROBE_DEPTH_FLOATS == 3 * hrt.PROBE_DEPTH_TEXELS
    assert (pd.RES, pd.TEXELS, pd.FLOATS, pd.MAX_BLOCKS, pd.VOLUME_MAX) == (8, 64, 192, 1 << 20, 1 << 22)
    assert hrt.PROBE_DEPTH_MAX_BLOCKS * hrt.PROBE_DEPTH_FLOATS * 4 == 805306368  # the 805 MB of block values
    assert hrt.PROBE_DEPTH_VOLUME_MAX * hrt.PROBE_DEPTH_TEXELS * 8 == 2 ** 31     # the moments stay at or below 2 GiB
    for gone in (r"Light probes\"\): [^*]*(\* [^*]*)*visibility or depth moments per probe", r"Probe volumes\"\): visibility or depth moments"):
        assert not re.search(gone, text), "the out-of-scope lists have lost this item"
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Probe visibility\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("bilinear texel look-up", "weight crush", "view-dependent bias", "probes that move"):
        assert item in scope, item


# ------------------------------------------------------------------------------------------------------------- the host functions
def test_texel_and_direction_refuse_by_name(hrt):
    dev = hrt.device_lib()
    v, e, out = np.ones(3, F32), C.c_uint32(7), np.zeros(3, F32)
    assert dev.hrt_probe_depth_texel(None, C.byref(e)) == HRT_ERR_INVALID and dev.hrt_last_error() == b"hrt_probe_depth_texel: v is NULL"
    assert dev.hrt_probe_depth_texel(v.ctypes.data, None) == HRT_ERR_INVALID and dev.hrt_last_error() == b"hrt_probe_depth_texel: texel is NULL"
    assert dev.hrt_probe_depth_direction(64, out.ctypes.data) == HRT_ERR_INVALID
    assert dev.hrt_last_error().startswith(b"hrt_probe_depth_direction: texel must be below HRT_PROBE_DEPTH_TEXELS = 64 (got 64)")
    assert dev.hrt_probe_depth_direction(2 ** 32 - 1, out.ctypes.data) == HRT_ERR_INVALID and not out.any()
    assert dev.hrt_probe_depth_direction(3, None) == HRT_ERR_INVALID and dev.hrt_last_error() == b"hrt_probe_depth_direction: out is NULL"
    assert dev.hrt_probe_depth_texel(v.ctypes.data, C.byref(e)) == HRT_OK and e.value == int(pd.texel(v))
    with pytest.raises(ValueError, match="probe_depth_texel: v must have 3 components"):
        hrt.probe_depth_texel([1, 2])
    with pytest.raises(hrt.HrtError, match="hrt_probe_depth_direction"):
        hrt.probe_depth_direction(64)


# ------------------------------------------------------------------------------------------------------------------- refusals
def depth(hrt, entry, scene=None, probes=PROBES, keys=None, n=5, first=0, spp=8, seed=1, r_max=1.0, flags=0, out=OUT, stats=None):
    dev = hrt.device_lib()
    k = None if keys is None else C.c_void_p(keys)
    if entry == "hrt_probe_depth_device":
        rc = dev.hrt_probe_depth_device(scene, C.c_void_p(probes), k, n, first, spp, seed, r_max, flags, C.c_void_p(out), None)
    else:
        rc = dev.hrt_probe_depth(scene, C.c_void_p(probes), k, n, spp, seed, r_max, flags, C.c_void_p(out), stats)
    return rc, dev.hrt_last_error().decode()


REFUSED = {1: "HRT_FLAG_GAMMA", 4: "HRT_FLAG_WAVE_KERNEL", 8: "HRT_FLAG_STREAM_KERNEL", 16: "HRT_FLAG_NO_SHADOW_CULL", 32: "HRT_FLAG_DUAL_KERNEL",
           256: "HRT_RAYS_NORMALIZE"}


@pytest.mark.parametrize("entry", DEPTH)
@pytest.mark.parametrize("bit", range(32))
def test_depth_takes_its_four_flags_and_refuses_every_other_bit_by_name(hrt, entry, bit):
    flag = 1 << bit
    rc, msg = depth(hrt, entry, flags=flag | (EXACT if flag == BRUTE else 0), n=0)
    if flag in (EXACT, BRUTE, NO_LDS) or (flag == ACCUMULATE and entry == "hrt_probe_depth_device"):
        assert rc == HRT_OK, msg
        return
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": flags"), (bit, msg)
    assert ("HRT_RADIANCE_ACCUMULATE" if flag == ACCUMULATE else REFUSED.get(flag, str(flag))) in msg, (bit, msg)


@pytest.mark.parametrize("entry", DEPTH)
def test_depth_checks_come_in_the_headers_order(hrt, entry):
    dev_form = entry == "hrt_probe_depth_device"
    pn, kn, on, align = ("d_probes", "d_keys", "d_out", 16) if dev_form else ("probes", "keys", "out", 4)
    every = dict(probes=0, keys=KEYS + 2, n=2 ** 31, spp=0, r_max=NAN, out=0)  # everything wrong at once
    rc, msg = depth(hrt, entry, flags=BRUTE, **every)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg
    assert depth(hrt, entry, **dict(every, n=0))[0] == HRT_OK, "an empty batch launches nothing"
    fixed = dict(every)
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: {pn} is NULL")
    fixed["probes"] = PROBES + align // 2
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: {pn} is not {align}-byte aligned")
    fixed["probes"] = PROBES
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: {kn} is not 4-byte aligned")
    fixed["keys"] = KEYS
    assert depth(hrt, entry, **fixed)[1].startswith(f"{entry}: n must be at most 2^31 - 1")
    fixed["n"] = 2 ** 20 + 1
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: n_samples must be positive")
    if dev_form:
        rc, msg = depth(hrt, entry, **dict(fixed, first=2 ** 32 - 3, spp=4))
        assert rc == HRT_ERR_INVALID and "first_sample + n_samples must be at most 2^32" in msg, msg
    fixed["spp"] = 64
    rc, msg = depth(hrt, entry, **fixed)
    assert rc == HRT_ERR_INVALID and "HRT_PROBE_DEPTH_MAX_BLOCKS = 1048576 (got 1048577)" in msg, msg
    rc, msg = depth(hrt, entry, **dict(fixed, n=2 ** 19, spp=129))
    assert rc == HRT_ERR_INVALID and "(got 1572864)" in msg, msg
    fixed["n"] = 2 ** 20  # exactly the limit
    for bad in (NAN, INF, -INF, 0.0, -0.0, -1.0):
        rc, msg = depth(hrt, entry, **dict(fixed, r_max=bad))
        assert rc == HRT_ERR_INVALID and msg.startswith(f"{entry}: r_max must be finite and positive"), (bad, msg)
    fixed["r_max"] = 1e-30
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")
    fixed["out"] = OUT + 2
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: {on} is not 4-byte aligned")
    fixed["out"] = OUT
    assert depth(hrt, entry, **fixed) == (HRT_ERR_INVALID, f"{entry}: scene is NULL")
    assert depth(hrt, entry, **dict(fixed, keys=None)) == (HRT_ERR_INVALID, f"{entry}: scene is NULL"), "keys may be NULL"
    if not dev_form:
        st = hrt.Stats(kernel_ms=1.0, samples=7)
        assert depth(hrt, entry, n=0, stats=C.byref(st))[0] == HRT_OK and st.samples == 0 and st.kernel_ms == 0 and st.total_ms == 0
        rc, msg = depth(hrt, entry, flags=ACCUMULATE, n=0)
        assert rc == HRT_ERR_INVALID and "hrt_probe_depth_device" in msg, msg


def visible(hrt, entry, vol=None, pts=PTS, n=5, flags=0, out=OUT, stats=None):
    dev = hrt.device_lib()
    if entry == "hrt_probe_eval_visible_device":
        rc = dev.hrt_probe_eval_visible_device(vol, C.c_void_p(pts), n, flags, C.c_void_p(out), None)
    else:
        rc = dev.hrt_probe_eval_visible(vol, C.c_void_p(pts), n, flags, C.c_void_p(out), stats)
    return rc, dev.hrt_last_error().decode()


BY_NAME = {4: "HRT_FLAG_WAVE_KERNEL", 8: "HRT_FLAG_STREAM_KERNEL", 16: "HRT_FLAG_NO_SHADOW_CULL", 32: "HRT_FLAG_DUAL_KERNEL", 64: "HRT_FLAG_EXACT_ONLY",
           128: "HRT_FLAG_MESH_BRUTE", 256: "HRT_RAYS_NORMALIZE", 512: "HRT_RADIANCE_ACCUMULATE"}


@pytest.mark.parametrize("entry", VISIBLE)
@pytest.mark.parametrize("bit", range(2, 32))
def test_the_visible_lookup_refuses_every_other_flag_bit_by_name(hrt, entry, bit):
    rc, msg = visible(hrt, entry, flags=(1 << bit) | FACING)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": flags"), (bit, msg)
    assert BY_NAME.get(1 << bit, str(1 << bit)) in msg, (bit, msg)


@pytest.mark.parametrize("entry", VISIBLE)
def test_the_visible_lookup_checks_flags_then_an_empty_batch_then_the_volume(hrt, entry):
    wrong = dict(vol=None, pts=PTS + 2, out=0)
    rc, msg = visible(hrt, entry, flags=4, n=0, **wrong)
    assert rc == HRT_ERR_INVALID and "flags" in msg, msg
    for flags in (0, RADIANCE, FACING, RADIANCE | FACING):
        assert visible(hrt, entry, flags=flags, n=0, **wrong)[0] == HRT_OK
        assert visible(hrt, entry, flags=flags, n=2 ** 31, **wrong) == (HRT_ERR_INVALID, entry + ": volume is NULL")
    if entry == "hrt_probe_eval_visible":
        st = hrt.Stats(kernel_ms=1.0, samples=7)
        assert visible(hrt, entry, n=0, stats=C.byref(st))[0] == HRT_OK and st.samples == 0 and st.kernel_ms == 0 and st.total_ms == 0


def test_the_depth_updates_refuse_a_null_volume(hrt):
    dev = hrt.device_lib()
    for entry, args in (("hrt_probe_volume_update_depth_device", (None, C.c_void_p(PTS), None)), ("hrt_probe_volume_update_depth", (None, C.c_void_p(PTS)))):
        assert getattr(dev, entry)(*args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == entry + ": volume is NULL"


def test_python_binding_checks_its_arguments_before_any_library(hrt):
    V, S = hrt.ProbeVolume, hrt.DeviceScene

    class Fake:  # stands in for a volume or a scene: no method may reach its handle before the arguments are right
        count = 4

        @property
        def _h(self):
            raise AssertionError("the library was reached")

    with pytest.raises(ValueError, match=r"ProbeVolume.eval_visible: points must have shape \(n, 8\)"):
        V.eval_visible(Fake(), np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match=r"ProbeVolume.eval_visible: out must be a contiguous \(n, 3\) float32 array"):
        V.eval_visible(Fake(), np.zeros((4, 8), F32), out=np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match=r"ProbeVolume.update_depth: sums must have shape \(n, 64, 3\)"):
        V.update_depth(Fake(), np.zeros((4, 27), F32))
    with pytest.raises(ValueError, match="the volume has 4 probes"):
        V.update_depth(Fake(), np.zeros((5, 64, 3), F32))
    with pytest.raises(ValueError, match=r"probe_depth: points must be probe records of shape \(n, 4\)"):
        S.probe_depth(Fake(), np.zeros((4, 8), F32))
    with pytest.raises(ValueError, match=r"probe_depth: out must be \(n, 64, 3\) float32"):
        S.probe_depth(Fake(), np.zeros((4, 4), F32), out=np.zeros((4, 9, 3), F32))
    with pytest.raises(ValueError, match="probe_depth: accumulate after sample 0 needs the running sums"):
        S.probe_depth(Fake(), np.zeros((4, 4), F32), first_sample=5, accumulate=True)


# ------------------------------------------------------------------------------------------------- the sanitized program
@pytest.fixture(scope="module")
def depth_check():
    """What the stand-alone program prints: the shared headers under the address and undefined-behaviour sanitizers."""
    subprocess.run(["make", "-s", "-C", PKG, "probe_depth_check"], check=True)
    r = subprocess.run([os.path.join(PKG, "probe_depth_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"probe_depth_check: exit {r.returncode}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout)


def test_the_sanitized_program_gives_the_octahedral_map_bit_for_bit(depth_check):
    d = np.array(depth_check["direction"], U32).view(F32).reshape(64, 3)
    assert np.array_equal(bits(d), bits(pd.direction(np.arange(64)))) and depth_check["centre_texel"] == list(range(64))
    v = np.array(depth_check["vectors"], U32).view(F32).reshape(-1, 3)
    got = np.array(depth_check["texel"], U32)
    assert len(v) > 4000 and np.isnan(v).any() and np.isinf(v).any() and (v == 0).all(axis=1).any()
    bad = np.flatnonzero(got != pd.texel(v))
    assert bad.size == 0, (bad[:5].tolist(), v[bad[:3]].tolist())
    assert len(set(got.tolist())) == 64


def test_the_sanitized_program_gives_the_visible_weights_bit_for_bit(depth_check):
    box, counts = ((-1.7, 0.3, 2.1), (2.9, 1.1, 7.6)), (3, 2, 2)  # tests/test_gpu_probe_depth.py's grid_3x2x2
    pts = np.array(depth_check["points"], U32).view(F32).reshape(-1, 8)
    mom = np.array(depth_check["moments"], U32).view(F32).reshape(-1, 64, 2)
    assert len(pts) == 8 ** 3 + 10 and mom.shape[0] == 12 and np.isinf(mom[..., 0]).any()
    for facing, suffix in ((False, ""), (True, "_facing")):
        index, weight, _, deg = pd.weights_visible(*box, counts, mom, pts, facing)
        assert deg.sum() == 7 and deg[8 ** 3:8 ** 3 + 7].all()
        assert np.array_equal(np.array(depth_check["index" + suffix], U32).reshape(-1, 8), index), facing
        gw = np.array(depth_check["weight" + suffix], U32).reshape(-1, 8)
        bad = np.flatnonzero((gw != bits(weight)).any(axis=1))
        assert bad.size == 0, (facing, bad[:5].tolist(), pts[bad[:1]].tolist())
        live = ~deg & np.isfinite(weight).all(axis=1)
        assert live.sum() >= 8 ** 3 and np.allclose(weight[live].sum(axis=1), 1, atol=1e-6) and (weight[live] >= 0).all()
        plain = pv.weights(*box, counts, pts, True)[1]
        assert not np.array_equal(bits(weight), bits(plain)), "visibility changes the weights"


# --------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_cli_refuses_what_it_cannot_combine_before_it_touches_a_device():
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8"]
    grid = ["--probe-grid", "2,2,1", "--probe-box", "-1,-1,-1,1,1,1"]
    for alone in (["--probe-visible"], ["--probe-visible", "--probe-rmax", "2"]):
        r = subprocess.run(base + grid + alone, capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-quad" in r.stderr and "--probe-visible" in r.stderr, (alone, r.stderr)
    r = subprocess.run(base + ["--probe-quad", "0", "--probe-visible"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-grid" in r.stderr, r.stderr
    r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-rmax", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-rmax" in r.stderr and "--probe-visible" in r.stderr, r.stderr
    for bad in ("0", "-1", "nan", "inf"):
        r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-visible", "--probe-rmax", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-rmax takes a finite positive distance" in r.stderr, (bad, r.stderr)
