"""Lit rays without a GPU (include/hrt.h "Lit rays"): the five entry points are exported and declared and the constant is the
header's; every bad argument that can be reached without a device is refused with HRT_ERR_INVALID and a message that names the entry
point and the culprit, in the header's order; the shared cell header gives the NumPy rule's weights bit for bit on the point records
a lit kernel makes of its hits, in a stand-alone program built with the address and undefined-behaviour sanitizers (make
probe_lit_check); the Python wrappers refuse before they touch a library; the command-line tool refuses what it cannot combine.  A
volume cannot be created without a device, so the checks that come after "the volume is NULL" are exercised in
tests/test_gpu_probe_lit.py.  The device pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import probe_depth_ref as pd
import probe_lit_ref as pl
import probe_volume_ref as pv
from conftest import PKG, ROOT

HRT_OK, HRT_ERR_INVALID = 0, -1
RAYS, KEYS, OUT = 0x1000, 0x3000, 0x2000
EXACT, BRUTE, NO_LDS, NORMALIZE, ACCUMULATE = 64, 128, 2, 256, 512
NAMES = ["hrt_trace_lit", "hrt_probes_lit_device", "hrt_probes_lit", "hrt_probe_volume_blend_device", "hrt_probe_volume_blend"]
LIT = NAMES[:3]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_five_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_headers_constant_and_scope(hrt):
    text = pv.header_text()
    assert re.search(r"#define HRT_LIT_VISIBLE +4u(\s|$)", text) and hrt.LIT_VISIBLE == 4 == pl.LIT_VISIBLE
    assert hrt.LIT_VISIBLE & (hrt.PROBE_EVAL_RADIANCE | hrt.PROBE_EVAL_FACING) == 0
    assert "a probe-lit frame mode of the renderer" not in text, "the out-of-scope list of \"Probe volumes\" has lost this item"
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Lit rays and probe relighting\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("mirror and glass", "more than one segment", "cooperative", "probes that move", "multi-GPU"):
        assert item in scope, item
    assert "CONCURRENCY: a call only READS the volume" in text


# ------------------------------------------------------------------------------------------------------------------- refusals
def lit(hrt, entry, scene=None, vol=None, rays=RAYS, keys=None, n=5, first=0, spp=8, seed=1, flags=0, eval_flags=0, bias=0.0, out=OUT, stats=None):
    dev = hrt.device_lib()
    k = None if keys is None else C.c_void_p(keys)
    if entry == "hrt_probes_lit":
        rc = dev.hrt_probes_lit(scene, vol, C.c_void_p(rays), k, n, spp, seed, flags, eval_flags, bias, C.c_void_p(out), stats)
    else:
        rc = getattr(dev, entry)(scene, vol, C.c_void_p(rays), k, n, first, spp, seed, flags, eval_flags, bias, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


EVERY = dict(rays=0, keys=KEYS + 2, n=2 ** 31, spp=0, out=0)  # everything after the volume wrong at once


@pytest.mark.parametrize("entry", LIT)
@pytest.mark.parametrize("bit", range(32))
def test_the_trace_flags_are_checked_first(hrt, entry, bit):
    """flags come before eval_flags, the volume and everything else: an accepted bit reaches "eval_flags", a refused one is named."""
    flag = 1 << bit
    rc, msg = lit(hrt, entry, flags=flag | (EXACT if flag == BRUTE else 0), eval_flags=1, bias=NAN, **EVERY)
    taken = {EXACT, BRUTE, NO_LDS} | ({ACCUMULATE} if entry != "hrt_probes_lit" else set()) | ({NORMALIZE} if entry == "hrt_trace_lit" else set())
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": "), msg
    if flag in taken:
        assert "eval_flags: HRT_PROBE_EVAL_RADIANCE" in msg, (bit, msg)
    else:
        assert "flags" in msg and "eval_flags" not in msg, (bit, msg)
        if flag == ACCUMULATE:
            assert "hrt_probes_lit_device" in msg
    rc, msg = lit(hrt, entry, flags=BRUTE, eval_flags=1, **EVERY)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg


@pytest.mark.parametrize("entry", LIT)
def test_eval_flags_then_the_volume_come_before_an_empty_batch(hrt, entry):
    for ef in (1, 1 | 2, 1 | 4):
        rc, msg = lit(hrt, entry, eval_flags=ef, bias=NAN, **EVERY)
        assert (rc, msg) == (HRT_ERR_INVALID, entry + ": eval_flags: HRT_PROBE_EVAL_RADIANCE: the tail of a lit ray is the irradiance about the hit's normal")
    for bit in range(3, 32):
        rc, msg = lit(hrt, entry, eval_flags=(1 << bit) | 2, bias=NAN, **EVERY)
        assert (rc, msg) == (HRT_ERR_INVALID, f"{entry}: eval_flags: unknown bits {1 << bit}"), bit
    for ef in (0, 2, 4, 6):
        for n in (0, 5, 2 ** 31):
            assert lit(hrt, entry, eval_flags=ef, bias=NAN, **dict(EVERY, n=n)) == (HRT_ERR_INVALID, entry + ": volume is NULL"), (ef, n)


@pytest.mark.parametrize("entry", NAMES[3:])
def test_blend_refuses_a_null_volume_first(hrt, entry):
    dev = hrt.device_lib()
    args = (None, None, C.c_float(NAN)) + ((None,) if entry.endswith("_device") else ())
    assert getattr(dev, entry)(*args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == entry + ": volume is NULL"


def test_python_wrappers_check_their_arguments_before_any_library(hrt):
    V, S = hrt.ProbeVolume, hrt.DeviceScene

    class Fake:  # stands in for a scene: no method may reach its handle before the arguments are right
        @property
        def _h(self):
            raise AssertionError("the library was reached")

    class FakeVolume(V):  # a volume that was never created
        count, loaded, lo, hi, shape = 4, False, (0, 0, 0), (1, 1, 1), (2, 2, 1)

        def __init__(self):
            pass

        def __del__(self):
            pass

        @property
        def _h(self):
            raise AssertionError("the library was reached")

    vol = FakeVolume()
    rays, probes = np.zeros((4, 8), F32), np.zeros((4, 4), F32)
    for who, fn, batch in (("trace_lit", S.trace_lit, rays), ("probes_lit", S.probes_lit, probes)):
        with pytest.raises(ValueError, match=who + ": volume must be a ProbeVolume"):
            fn(Fake(), batch, object())
        with pytest.raises(ValueError, match=who + ": eval_flags: PROBE_EVAL_RADIANCE"):
            fn(Fake(), batch, vol, eval_flags=hrt.PROBE_EVAL_RADIANCE | hrt.LIT_VISIBLE)
        with pytest.raises(ValueError, match=who + ": eval_flags: unknown bits 8"):
            fn(Fake(), batch, vol, eval_flags=8 | hrt.PROBE_EVAL_FACING)
        for bad in (NAN, INF, -INF):
            with pytest.raises(ValueError, match=who + ": bias must be finite"):
                fn(Fake(), batch, vol, bias=bad)
        with pytest.raises(ValueError, match=who + ": accumulate after sample 0 needs the running sums"):
            fn(Fake(), batch, vol, first_sample=5, accumulate=True)
    with pytest.raises(ValueError, match=r"trace_lit: rays must have shape \(n, 8\)"):
        S.trace_lit(Fake(), probes, vol)
    with pytest.raises(ValueError, match=r"probes_lit: points must be probe records of shape \(n, 4\)"):
        S.probes_lit(Fake(), rays, vol)
    with pytest.raises(ValueError, match=r"probes_lit: out must be \(n, 9, 3\) float32"):
        S.probes_lit(Fake(), probes, vol, out=np.zeros((4, 3), F32))
    with pytest.raises(ValueError, match=r"trace_lit: out must be \(n, 3\) float32"):
        S.trace_lit(Fake(), rays, vol, out=np.zeros((4, 9, 3), F32))
    for bad in (1.0, -0.25, NAN, 2.0):
        with pytest.raises(ValueError, match=r"ProbeVolume.blend: keep must be in \[0, 1\)"):
            V.blend(vol, np.zeros((4, 9, 3), F32), bad)
        with pytest.raises(ValueError, match=r"ProbeVolume.relight: keep must be in \[0, 1\)"):
            V.relight(vol, Fake(), 4, 1, keep=bad)
    with pytest.raises(ValueError, match=r"ProbeVolume.blend: coeffs must have shape \(n, 9, 3\)"):
        V.blend(vol, np.zeros((4, 27), F32), 0.5)
    with pytest.raises(ValueError, match="the volume has 4 probes"):
        V.blend(vol, np.zeros((5, 9, 3), F32), 0.5)
    with pytest.raises(ValueError, match="ProbeVolume.relight: spp must be positive and rounds non-negative"):
        V.relight(vol, Fake(), 0, 1)
    with pytest.raises(ValueError, match="ProbeVolume.relight: eval_flags: PROBE_EVAL_RADIANCE"):
        V.relight(vol, Fake(), 4, 1, eval_flags=1)
    with pytest.raises(ValueError, match="ProbeVolume.relight: depth_rmax must be finite and positive"):
        V.relight(vol, Fake(), 4, 1, depth_rmax=0.0)


# ------------------------------------------------------------------------------------------------- the sanitized program
@pytest.fixture(scope="module")
def lit_check():
    """What the stand-alone program prints: the shared cell header under the address and undefined-behaviour sanitizers."""
    subprocess.run(["make", "-s", "-C", PKG, "probe_lit_check"], check=True)
    r = subprocess.run([os.path.join(PKG, "probe_lit_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"probe_lit_check: exit {r.returncode}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout)


def test_the_sanitized_program_gives_the_tails_weights_bit_for_bit(lit_check):
    box, counts = ((-1.7, 0.3, 2.1), (2.9, 1.1, 7.6)), (3, 2, 2)  # tests/test_gpu_probe_depth.py's grid_3x2x2
    pts = np.array(lit_check["points"], U32).view(F32).reshape(-1, 8)
    mom = np.array(lit_check["moments"], U32).view(F32).reshape(-1, 64, 2)
    assert len(pts) == 606 and mom.shape[0] == 12 and (pts[:, 7] == F32(1e-3)).all()
    lo, hi = np.asarray(box[0], F32), np.asarray(box[1], F32)
    outside = ((pts[:600, 0:3] < lo) | (pts[:600, 0:3] > hi)).any(axis=1)
    assert 50 < outside.sum() < 550, "hit points inside and outside the box"
    seen = []
    for ef in (0, pl.FACING, pl.LIT_VISIBLE, pl.FACING | pl.LIT_VISIBLE):
        facing = bool(ef & pl.FACING)
        index, weight, _, deg = pd.weights_visible(*box, counts, mom, pts, facing) if ef & pl.LIT_VISIBLE else pv.weights(*box, counts, pts, facing)
        assert deg.tolist() == [False] * 601 + [True] * 5, ef
        assert np.array_equal(np.array(lit_check[f"index_{ef}"], U32).reshape(-1, 8), index), ef
        gw = np.array(lit_check[f"weight_{ef}"], U32).reshape(-1, 8)
        bad = np.flatnonzero((gw != bits(weight)).any(axis=1))
        assert bad.size == 0, (ef, bad[:5].tolist(), pts[bad[:1]].tolist())
        assert np.allclose(weight[~deg].sum(axis=1), 1, atol=1e-5) and (weight[~deg] >= 0).all(), ef
        seen.append(gw.tobytes())
    assert len(set(seen)) == 4, "facing and visibility each change the weights"


# --------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_cli_refuses_what_it_cannot_combine_before_it_touches_a_device():
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8"]
    grid = ["--probe-grid", "2,2,1", "--probe-box", "-1,-1,-1,1,1,1"]
    r = subprocess.run(base + grid + ["--probe-bounces", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-quad" in r.stderr and "--probe-bounces" in r.stderr, r.stderr
    r = subprocess.run(base + ["--probe-lit"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-grid" in r.stderr and "--probe-lit" in r.stderr, r.stderr
    r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-keep", "0.5"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-keep" in r.stderr and "--probe-bounces" in r.stderr, r.stderr
    r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-lit"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-quad" in r.stderr and "--probe-lit" in r.stderr, r.stderr
    for bad in ("0", "-1", "x"):
        r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-bounces", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-bounces takes a positive number of rounds" in r.stderr, (bad, r.stderr)
    for bad in ("1", "-0.5", "nan", "2"):
        r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-bounces", "2", "--probe-keep", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-keep takes a fraction in [0, 1)" in r.stderr, (bad, r.stderr)
