"""Light probes without a GPU (include/hrt.h "Light probes"): the four entry points are exported and declared; every bad argument
-- flags, pointers, counts, samples, the block limit -- is refused with HRT_ERR_INVALID and a message that names the entry point and
the culprit, in the header's order and before the scene and the library state are looked at, a NULL scene after those checks, and
an empty batch returns HRT_OK; the host grid generator equals tests/probe_ref.py bit for bit, through libhrt.so and through a
stand-alone program built with the address and undefined-behaviour sanitizers (make probe_check); the command-line tool refuses
what it cannot combine.  The device pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import probe_ref
from conftest import PKG, ROOT

HRT_OK, HRT_ERR_INVALID = 0, -1
PTS, KEYS, OUT = 0x1000, 0x3000, 0x2000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ["hrt_probe_rays", "hrt_probes_device", "hrt_probes", "hrt_probe_grid_points"]
TRACED = NAMES[:3]
FUSED = NAMES[1:3]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
BLOCK = probe_ref.BLOCK
MAX_BLOCKS = 1 << 22


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def call(hrt, entry, pts=PTS, keys=0, n=5, first=0, ns=1, seed=1, flags=0, out=OUT):
    """One call of `entry` with a NULL scene and pointers that are never followed."""
    dev = hrt.device_lib()
    p, k, o = C.c_void_p(pts), C.c_void_p(keys), C.c_void_p(out)
    if entry == "hrt_probe_rays":
        rc = dev.hrt_probe_rays(p, k, n, first, seed, o, None)
    elif entry == "hrt_probes_device":
        rc = dev.hrt_probes_device(None, p, k, n, first, ns, seed, flags, o, None)
    else:
        rc = dev.hrt_probes(None, p, k, n, ns, seed, flags, o, None)
    return rc, dev.hrt_last_error().decode()


def passes(hrt, entry, **kw):
    """The arguments get past every check before the last: hrt_probe_rays stops at its NULL output, the others at the NULL scene."""
    if entry == "hrt_probe_rays":
        kw["out"] = 0
    rc, msg = call(hrt, entry, **kw)
    return (rc == HRT_ERR_INVALID and ("d_rays is NULL" if entry == "hrt_probe_rays" else "scene is NULL") in msg), msg


# ------------------------------------------------------------------------------------------------------------------- exports
@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_four_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    with open(os.path.join(ROOT, "include", "hrt.h")) as f:
        assert re.search(r"^HRT_API int " + name + r"\(", f.read(), re.M)


def test_the_headers_constants(hrt):
    with open(os.path.join(ROOT, "include", "hrt.h")) as f:
        text = f.read()
    assert re.search(r"#define HRT_PROBE_FLOATS 4\b", text) and re.search(r"#define HRT_PROBE_COEFFS 9\b", text)
    assert re.search(r"#define HRT_PROBE_MAX_BLOCKS \(1u << 22\)", text)
    assert hrt.PROBE_BLOCK == BLOCK and hrt.PROBE_FLOATS == 4 and hrt.PROBE_COEFFS == 9


# --------------------------------------------------------------------------------------------------------------------- flags
KNOWN = (NO_LDS, EXACT, BRUTE, ACCUMULATE)
BY_NAME = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
           NORMALIZE: "HRT_RAYS_NORMALIZE", GAMMA: "HRT_FLAG_GAMMA"}
WHY = {WAVE: "a probe launch has one kernel form", STREAM: "a probe launch has one kernel form", DUAL: "a probe launch has one kernel form",
       NORMALIZE: "a probe has no direction to normalise", GAMMA: "probes are linear radiance, not a frame"}


@pytest.mark.parametrize("entry", FUSED)
@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in KNOWN])
def test_every_other_flag_bit_is_refused_by_name(hrt, entry, bit):
    rc, msg = call(hrt, entry, flags=1 << bit)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": flags") , (bit, msg)
    assert BY_NAME.get(1 << bit, str(1 << bit)) in msg and WHY.get(1 << bit, "") in msg, (bit, msg)


@pytest.mark.parametrize("entry", FUSED)
def test_flag_combinations(hrt, entry):
    for extra in (0, NO_LDS):
        rc, msg = call(hrt, entry, flags=BRUTE | extra)
        assert rc == HRT_ERR_INVALID and "EXACT_ONLY" in msg, msg
    for flags in (0, EXACT, EXACT | BRUTE, NO_LDS, EXACT | BRUTE | NO_LDS):
        ok, msg = passes(hrt, entry, flags=flags)
        assert ok, (flags, msg)
    ok, msg = passes(hrt, "hrt_probes_device", flags=ACCUMULATE | EXACT | BRUTE | NO_LDS)
    assert ok, msg
    rc, msg = call(hrt, "hrt_probes", flags=ACCUMULATE)  # the host form has no running sums to add to: hrt_bake's wording
    assert rc == HRT_ERR_INVALID and msg == "hrt_probes: flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device (hrt_probes_device)", msg


# ------------------------------------------------------------------------------------------------------- counts and pointers
@pytest.mark.parametrize("entry", TRACED)
def test_an_empty_batch_returns_ok_whatever_else_is_passed(hrt, entry):
    rc, msg = call(hrt, entry, n=0, pts=0, keys=KEYS + 1, ns=0, first=2 ** 32 - 1, out=0)
    assert rc == HRT_OK, msg
    if entry != "hrt_probe_rays":  # but the flags are checked first
        rc, msg = call(hrt, entry, n=0, flags=WAVE)
        assert rc == HRT_ERR_INVALID and "HRT_FLAG_WAVE_KERNEL" in msg, msg
    if entry == "hrt_probes":
        st = hrt.Stats(kernel_ms=1.0, samples=7)
        assert hrt.device_lib().hrt_probes(None, None, None, 0, 1, 1, 0, None, C.byref(st)) == HRT_OK and st.samples == 0 and st.kernel_ms == 0


@pytest.mark.parametrize("entry", TRACED)
def test_probes_and_keys(hrt, entry):
    name = "probes" if entry == "hrt_probes" else "d_probes"
    rc, msg = call(hrt, entry, pts=0)
    assert rc == HRT_ERR_INVALID and entry in msg and f"{name} is NULL" in msg, msg
    for off in ((1, 2) if entry == "hrt_probes" else (4, 8, 12)):  # device records are read with 16-byte loads, host ones copied
        rc, msg = call(hrt, entry, pts=PTS + off)
        assert rc == HRT_ERR_INVALID and entry in msg and name in msg and "aligned" in msg, (off, msg)
    for off in (1, 2, 3):
        rc, msg = call(hrt, entry, keys=KEYS + off)
        assert rc == HRT_ERR_INVALID and entry in msg and "keys is not 4-byte aligned" in msg, (off, msg)
    for keys in (0, KEYS, KEYS + 4):
        ok, msg = passes(hrt, entry, keys=keys)
        assert ok, (keys, msg)


@pytest.mark.parametrize("entry", TRACED)
@pytest.mark.parametrize("n", [2 ** 31, 2 ** 32 - 1])
def test_too_many_probes_are_refused_and_named(hrt, entry, n):
    rc, msg = call(hrt, entry, n=n)
    assert rc == HRT_ERR_INVALID and entry in msg and "2^31 - 1" in msg and str(n) in msg, msg
    ok, msg = passes(hrt, "hrt_probe_rays", n=2 ** 31 - 1)
    assert ok, msg


@pytest.mark.parametrize("entry", FUSED)
def test_samples_and_the_block_limit(hrt, entry):
    for first in (0, 5, 2 ** 32 - 1):
        rc, msg = call(hrt, entry, first=first, ns=0)
        assert rc == HRT_ERR_INVALID and entry in msg and "n_samples must be positive" in msg, msg
    for first, ns in ((2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1)):
        rc, msg = call(hrt, "hrt_probes_device", first=first, ns=ns)
        assert rc == HRT_ERR_INVALID and "hrt_probes_device" in msg and "first_sample + n_samples must be at most 2^32" in msg and "wrap" in msg, msg
    ok, msg = passes(hrt, "hrt_probes_device", n=1, first=2 ** 32 - 1, ns=1)
    assert ok, msg
    # n * ceil(n_samples / BLOCK) <= 2^22, at the edge on both factors
    for n, ns in ((MAX_BLOCKS, BLOCK), (MAX_BLOCKS // 2, 2 * BLOCK), (1, MAX_BLOCKS * BLOCK), (MAX_BLOCKS, 1)):
        ok, msg = passes(hrt, entry, n=n, ns=ns)
        assert ok, (n, ns, msg)
    for n, ns, items in ((MAX_BLOCKS + 1, 1, MAX_BLOCKS + 1), (MAX_BLOCKS, BLOCK + 1, 2 * MAX_BLOCKS), (1, MAX_BLOCKS * BLOCK + 1, MAX_BLOCKS + 1),
                         (2 ** 31 - 1, 2 ** 32 - 1, (2 ** 31 - 1) * -(-(2 ** 32 - 1) // BLOCK))):
        rc, msg = call(hrt, entry, n=n, ns=ns)
        assert rc == HRT_ERR_INVALID and entry in msg and "HRT_PROBE_MAX_BLOCKS" in msg and str(MAX_BLOCKS) in msg and f"got {items}" in msg, (n, ns, msg)


def test_outputs(hrt):
    for out in (0, OUT + 4, OUT + 8):
        rc, msg = call(hrt, "hrt_probe_rays", out=out)
        assert rc == HRT_ERR_INVALID and "hrt_probe_rays" in msg and "d_rays" in msg, msg
    for entry, word in (("hrt_probes_device", "d_out"), ("hrt_probes", "out")):
        for out in (0, OUT + 1, OUT + 2):
            rc, msg = call(hrt, entry, out=out)
            assert rc == HRT_ERR_INVALID and entry in msg and f": {word} is " in msg, (out, msg)
        for out in (OUT + 4, OUT + 12):
            ok, msg = passes(hrt, entry, out=out)
            assert ok, (out, msg)


def test_the_checks_come_in_the_headers_order_and_before_the_scene(hrt):
    e = "hrt_probes_device"
    wrong = dict(pts=PTS + 4, keys=KEYS + 2, n=2 ** 31, ns=0, first=2 ** 32 - 1, out=0)
    assert "flags" in call(hrt, e, flags=WAVE, **wrong)[1]
    assert "d_probes is not 16-byte aligned" in call(hrt, e, **wrong)[1]
    wrong["pts"] = 0
    assert "d_probes is NULL" in call(hrt, e, **wrong)[1]
    wrong["pts"] = PTS
    assert "d_keys" in call(hrt, e, **wrong)[1]
    wrong["keys"] = KEYS
    assert "n must be at most" in call(hrt, e, **wrong)[1]
    wrong["n"] = MAX_BLOCKS + 1
    assert "n_samples must be positive" in call(hrt, e, **wrong)[1]
    wrong["ns"] = 2
    assert "first_sample" in call(hrt, e, **wrong)[1]
    wrong["first"] = 0
    assert "HRT_PROBE_MAX_BLOCKS" in call(hrt, e, **wrong)[1]
    wrong["n"] = 5
    assert "d_out is NULL" in call(hrt, e, **wrong)[1]
    wrong["out"] = OUT + 2
    assert "d_out is not 4-byte aligned" in call(hrt, e, **wrong)[1]
    wrong["out"] = OUT
    assert "scene is NULL" in call(hrt, e, **wrong)[1]
    r = "hrt_probe_rays"
    assert "d_probes" in call(hrt, r, pts=0, keys=KEYS + 2, n=2 ** 31, out=0)[1]
    assert "d_keys" in call(hrt, r, keys=KEYS + 2, n=2 ** 31, out=0)[1]
    assert "n must be at most" in call(hrt, r, n=2 ** 31, out=0)[1]
    assert "d_rays is NULL" in call(hrt, r, out=0)[1]
    for entry in FUSED:
        for kw in (dict(flags=GAMMA), dict(pts=0), dict(keys=KEYS + 1), dict(n=2 ** 31), dict(ns=0), dict(n=MAX_BLOCKS + 1), dict(out=0)):
            rc, msg = call(hrt, entry, **kw)
            assert rc == HRT_ERR_INVALID and "scene" not in msg, (kw, msg)


def test_python_binding_checks_its_arguments(hrt):
    pts = np.zeros((4, 4), F32)
    with pytest.raises(ValueError, match="probes: points must be probe records"):
        hrt.DeviceScene.probes(None, np.zeros((4, 8), F32))
    with pytest.raises(ValueError, match="keys"):
        hrt.DeviceScene.probes(None, pts, keys=np.zeros(3, U32))
    with pytest.raises(ValueError, match=r"out must be \(n, 9, 3\) float32"):
        hrt.DeviceScene.probes(None, pts, out=np.zeros((4, 3), F32))
    with pytest.raises(ValueError, match="accumulate"):
        hrt.DeviceScene.probes(None, pts, first_sample=3, accumulate=True)
    with pytest.raises(ValueError, match="points"):
        hrt.probe_rays(pts)  # the rays of a sample are made on the device: a torch tensor there
    with pytest.raises(ValueError, match="probe_grid: lo and hi"):
        hrt.probe_grid((0, 0), (1, 1, 1), 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- the generator
BOX = ((-1.7, 0.3, 2.1), (2.9, 1.1, 7.6))
BACK = ((3.0, -2.0, 5.0), (-1.0, -2.0, 0.5))  # lo > hi on two axes, lo == hi on one
SIZES = [(1, 1, 1), (3, 2, 2), (1, 7, 1), (16, 8, 4)]


@pytest.mark.parametrize("size", SIZES)
def test_grid_points_equal_the_numpy_rule_bit_for_bit(hrt, size):
    for (lo, hi), time in ((BOX, 0.25), (BACK, 0.0)):
        got = hrt.probe_grid(lo, hi, *size, time)
        want = probe_ref.grid(lo, hi, *size, time)
        assert got.shape == (size[0] * size[1] * size[2], 4) and np.array_equal(bits(got), bits(want)), (size, lo)
    one = hrt.probe_grid(*BOX, 1, 1, 1)[0]
    assert np.allclose(one[0:3], (np.array(BOX[0]) + np.array(BOX[1])) / 2, atol=1e-6) and one[3] == 0  # a single probe sits in the middle
    g = hrt.probe_grid((0, 0, 0), (3, 2, 2), 3, 2, 2)
    assert g[1, 0:3].tolist() == [1.5, 0.5, 0.5] and g[3, 0:3].tolist() == [0.5, 1.5, 0.5] and g[6, 0:3].tolist() == [0.5, 0.5, 1.5]  # x fastest, z slowest


def test_the_generator_refuses_by_name(hrt):
    for kw, word in ((dict(nx=0), "nx, ny and nz"), (dict(ny=0), "nx, ny and nz"), (dict(nz=0), "nx, ny and nz"),
                     (dict(nx=65536, ny=32768), "2^31 - 1"), (dict(nx=2 ** 32 - 1, ny=2 ** 32 - 1, nz=2 ** 32 - 1), "2^31 - 1"),
                     (dict(lo=(0, NAN, 0)), "lo must be finite"), (dict(hi=(1, 1, INF)), "hi must be finite"), (dict(time=NAN), "time"),
                     (dict(time=-INF), "time")):
        args = dict(lo=BOX[0], hi=BOX[1], nx=2, ny=2, nz=2, time=0.0)
        args.update(kw)
        with pytest.raises(hrt.HrtError, match="hrt_probe_grid_points") as e:
            hrt.probe_grid(**args)
        assert word in str(e.value), (kw, str(e.value))
    dev = hrt.device_lib()
    lo, hi, buf = np.array(BOX[0], F32), np.array(BOX[1], F32), np.zeros(4, F32)
    for args, word in (((None, hi.ctypes.data, 1, 1, 1, 0.0, buf.ctypes.data), b"lo is NULL"), ((lo.ctypes.data, None, 1, 1, 1, 0.0, buf.ctypes.data), b"hi is NULL"),
                       ((lo.ctypes.data, hi.ctypes.data, 1, 1, 1, 0.0, None), b"out_probes is NULL")):
        assert dev.hrt_probe_grid_points(*args) == HRT_ERR_INVALID and word in dev.hrt_last_error()


# ------------------------------------------------------------------------------------------------- the sanitized program
@pytest.fixture(scope="module")
def probe_check():
    """What the stand-alone program prints: the generator's header under the address and undefined-behaviour sanitizers."""
    subprocess.run(["make", "-s", "-C", PKG, "probe_check"], check=True)
    r = subprocess.run([os.path.join(PKG, "probe_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"probe_check: exit {r.returncode}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout)


def test_the_sanitized_program_gives_the_numpy_rule_bit_for_bit(probe_check):
    seen = 0
    for bname, (lo, hi), time in (("box", BOX, 0.25), ("back", BACK, 0.0)):
        for size in SIZES:
            got = probe_check[f"{bname}_{size[0]}x{size[1]}x{size[2]}"]
            want = probe_ref.grid(lo, hi, *size, time)
            assert got["rc"] == HRT_OK and np.array_equal(np.array(got["records"], U32).reshape(-1, 4), bits(want)), (bname, size)
            seen += 1
    assert seen == 8


def test_the_sanitized_program_refuses_before_it_writes(probe_check):
    words = {"null_lo": "lo is NULL", "null_hi": "hi is NULL", "null_out": "out_probes is NULL", "nx_zero": "nx, ny and nz", "ny_zero": "nx, ny and nz",
             "nz_zero": "nx, ny and nz", "too_many": "2^31 - 1", "too_many_wrapping": "2^31 - 1", "lo_nan": "lo must be finite",
             "hi_inf": "hi must be finite", "time_nan": "time", "time_inf": "time"}
    assert set(words) == {k for k, v in probe_check.items() if v["rc"] != HRT_OK}
    for case, word in words.items():
        got = probe_check[case]
        assert got["rc"] == HRT_ERR_INVALID and got["error"].startswith("hrt_probe_grid_points: ") and word in got["error"] and got["records"] == [], (case, got)


# --------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_cli_refuses_what_it_cannot_combine_before_it_touches_a_device():
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8"]
    grid, box = ["--probe-grid", "2,2,1"], ["--probe-box", "-1,-1,-1,1,1,1"]
    r = subprocess.run(base + grid, capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-grid" in r.stderr and "--probe-box" in r.stderr, r.stderr
    r = subprocess.run(base + box, capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-box" in r.stderr and "--probe-grid" in r.stderr, r.stderr
    for other in (["--lens", "ortho"], ["--bake-quad", "0"], ["--views", "2"], ["--adaptive", "0.05"]):
        r = subprocess.run(base + grid + box + other, capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-grid" in r.stderr and other[0] in r.stderr, (other, r.returncode, r.stderr)
    for bad in (["--probe-grid", "2,2"], ["--probe-grid", "0,1,1"], ["--probe-grid", "a,b,c"], ["--probe-grid", "65536,32768,1"],
                ["--probe-grid", "4294967295,4294967295,4294967295"], ["--probe-grid", "4294967296,1,1"]):
        r = subprocess.run(base + bad + box, capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-grid" in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + grid + ["--probe-box", "0,0,0,1,1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-box" in r.stderr, r.stderr
