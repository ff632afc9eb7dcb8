"""Lit paths without a GPU (include/hrt.h "Lit paths"): the four entry points are exported and declared and the constants are the
header's; every bad argument that can be reached without a device is refused with HRT_ERR_INVALID and a message that names the entry
point and the culprit, in the header's order -- tail_after right after the flags; the NumPy statement of the rule does what the
header says with a path's surfaces; the Python wrappers refuse before they touch a library; the command-line tool refuses what it
cannot combine.  A volume cannot be created without a device, so the checks that come after "the volume is NULL" are exercised in
tests/test_gpu_lit_paths.py.  The device pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lit_paths_ref as lp
import probe_volume_ref as pv
from conftest import PKG, ROOT

HRT_OK, HRT_ERR_INVALID, HRT_ERR_STATE = 0, -1, -2
RAYS, KEYS, OUT = 0x1000, 0x3000, 0x2000
EXACT, BRUTE, NO_LDS, NORMALIZE, ACCUMULATE = 64, 128, 2, 256, 512
NAMES = ["hrt_trace_lit_paths", "hrt_path_tails", "hrt_probes_lit_paths_device", "hrt_probes_lit_paths"]
WITH_VOLUME = [NAMES[0]] + NAMES[2:]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
TAIL_RANGE = "tail_after must be in 1 .. HRT_MAXBOUNCES = 6 (got {})"


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_four_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_headers_constants_and_scope(hrt):
    text = pv.header_text()
    assert re.search(r"#define HRT_TAIL_FLOATS +16u(\s|$)", text) and hrt.TAIL_FLOATS == 16 == lp.TAIL_FLOATS
    assert re.search(r"#define HRT_TAIL_REACHED +0x80000000u(\s|$)", text) and hrt.TAIL_REACHED == 0x80000000 == lp.REACHED
    assert re.search(r"#define HRT_MAXBOUNCES +6(\s|$)", text) and hrt.MAXBOUNCES == 6 == lp.MAXBOUNCES
    assert hrt.TAIL_WORD == 11 == lp.TAIL_WORD
    assert text.index("/* ---- Lit rays:") < text.index("/* ---- Lit paths:"), "the section comes after \"Lit rays\""
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Lit paths\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("lens-camera sources", "cooperative", "probes that move", "multi-GPU"):
        assert item in scope, item
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Lit rays and probe relighting\"\): ([^/]*)\*/", text)
    assert m and "\"Lit paths\" below" in re.sub(r"\s*\n \* ", " ", m.group(1)), "\"Lit rays\" says where its two open items went"


# ------------------------------------------------------------------------------------------------------------------- refusals
def lit(hrt, entry, scene=None, vol=None, rays=RAYS, keys=None, n=5, first=0, spp=8, seed=1, flags=0, eval_flags=0, bias=0.0, tail=1, out=OUT):
    dev = hrt.device_lib()
    k = None if keys is None else C.c_void_p(keys)
    if entry == "hrt_probes_lit_paths":
        rc = dev.hrt_probes_lit_paths(scene, vol, C.c_void_p(rays), k, n, spp, seed, flags, eval_flags, bias, tail, C.c_void_p(out), None)
    elif entry == "hrt_path_tails":
        rc = dev.hrt_path_tails(scene, C.c_void_p(rays), k, n, first, seed, flags, bias, tail, C.c_void_p(out), None)
    else:
        rc = getattr(dev, entry)(scene, vol, C.c_void_p(rays), k, n, first, spp, seed, flags, eval_flags, bias, tail, C.c_void_p(out), None)
    return rc, dev.hrt_last_error().decode()


EVERY = dict(rays=0, keys=KEYS + 2, n=2 ** 31, spp=0, out=0)  # everything after the volume wrong at once


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("bit", range(32))
def test_the_trace_flags_are_checked_first_and_tail_after_next(hrt, entry, bit):
    """An accepted flag bit reaches "tail_after", a refused one is named -- with every later argument wrong as well."""
    flag = 1 << bit
    rc, msg = lit(hrt, entry, flags=flag | (EXACT if flag == BRUTE else 0), eval_flags=1, bias=NAN, tail=0, **EVERY)
    taken = {EXACT, BRUTE, NO_LDS}
    taken |= {ACCUMULATE} if entry in ("hrt_trace_lit_paths", "hrt_probes_lit_paths_device") else set()
    taken |= {NORMALIZE} if entry in ("hrt_trace_lit_paths", "hrt_path_tails") else set()
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": "), msg
    if flag in taken:
        assert msg == entry + ": " + TAIL_RANGE.format(0), (bit, msg)
    else:
        assert "flags" in msg and "tail_after" not in msg, (bit, msg)
        if flag == ACCUMULATE and entry == "hrt_probes_lit_paths":
            assert "hrt_probes_lit_paths_device" in msg
    rc, msg = lit(hrt, entry, flags=BRUTE, tail=0, **EVERY)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_tail_after_is_refused_by_name_outside_1_to_6(hrt, entry):
    for bad in (0, 7, 8, 2 ** 32 - 1):
        assert lit(hrt, entry, eval_flags=1, bias=NAN, tail=bad, **EVERY) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(bad)), bad
    for ok in range(1, 7):  # the next check in the header's order
        rc, msg = lit(hrt, entry, eval_flags=1, bias=NAN, tail=ok, **EVERY)
        assert rc == HRT_ERR_INVALID and msg.startswith(entry + (": bias must be finite" if entry == "hrt_path_tails" else ": eval_flags: HRT_PROBE_EVAL_RADIANCE")), (ok, msg)


@pytest.mark.parametrize("entry", WITH_VOLUME)
def test_eval_flags_then_the_volume_come_before_an_empty_batch(hrt, entry):
    for bit in range(3, 32):
        assert lit(hrt, entry, eval_flags=(1 << bit) | 2, bias=NAN, **EVERY) == (HRT_ERR_INVALID, f"{entry}: eval_flags: unknown bits {1 << bit}"), bit
    for ef in (0, 2, 4, 6):
        for n in (0, 5, 2 ** 31):
            assert lit(hrt, entry, eval_flags=ef, bias=NAN, **dict(EVERY, n=n)) == (HRT_ERR_INVALID, entry + ": volume is NULL"), (ef, n)


def test_path_tails_refuses_in_the_headers_order(hrt):
    entry = "hrt_path_tails"
    for bad in (NAN, INF, -INF):
        rc, msg = lit(hrt, entry, bias=bad, **EVERY)
        assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": bias must be finite"), (bad, msg)
    assert lit(hrt, entry, **dict(EVERY, n=0))[0] == HRT_OK, "an empty batch launches nothing"
    fixed = dict(EVERY)
    assert lit(hrt, entry, **fixed) == (HRT_ERR_INVALID, entry + ": d_rays is NULL")
    fixed["rays"] = RAYS + 8
    assert lit(hrt, entry, **fixed) == (HRT_ERR_INVALID, entry + ": d_rays is not 16-byte aligned")
    fixed["rays"] = RAYS
    assert lit(hrt, entry, **fixed) == (HRT_ERR_INVALID, entry + ": d_keys is not 4-byte aligned")
    fixed["keys"] = KEYS
    assert lit(hrt, entry, **fixed) == (HRT_ERR_INVALID, entry + ": d_out is NULL")
    for off in (4, 8, 12):  # a tail record is stored as four 16-byte pieces
        fixed["out"] = OUT + off
        assert lit(hrt, entry, **fixed) == (HRT_ERR_INVALID, entry + ": d_out is not 16-byte aligned"), off
    fixed["out"] = OUT
    assert lit(hrt, entry, **fixed)[1].startswith(entry + ": n must be at most 2^31 - 1")
    fixed["n"] = 5
    assert lit(hrt, entry, **fixed) == (HRT_ERR_INVALID, entry + ": scene is NULL")


# ------------------------------------------------------------------------------------------------------ the rule's bookkeeping
def test_the_numpy_rule_counts_segments_and_diffuse_hits_as_the_header_writes():
    D, G, M = lp.DIFFUSE, 1, 2
    assert lp.walk([D, D, D, D, D, D], 1) == (1, True) and lp.walk([D, D, D, D, D, D], 6) == (6, True)
    assert lp.walk([M, G, D, D, M, D], 1) == (3, True), "mirror and glass cost a bounce and do not count"
    assert lp.walk([M, G, D, D, M, D], 2) == (4, True) and lp.walk([M, G, D, D, M, D], 3) == (6, True)
    assert lp.walk([M, G, D, D, M, D], 4) == (6, False), "the bounces ran out"
    assert lp.walk([M, M, M, M, M, M], 1) == (6, False)
    assert lp.walk([None], 1) == (1, False) and lp.walk([D, M, None], 2) == (3, False), "a miss ends the path without a tail"
    assert lp.walk([D, None], 1) == (1, True)
    T = np.zeros((3, 16), F32)
    T[:, 8:11], T[:, 12:15] = (0.5, 0.25, 2.0), (1.0, 2.0, 3.0)
    T.view(U32)[:, 11] = (2, 0x80000003, 0)
    G3 = np.full((3, 3), 4.0, F32)
    G3[0] = NAN  # not read where the tail was not reached
    assert np.array_equal(lp.sample_value(T, G3), np.array([[1, 2, 3], [3, 3, 11], [1, 2, 3]], F32))
    _, thr, seg, reached, a = lp.split(T)
    assert seg.tolist() == [2, 3, 0] and reached.tolist() == [False, True, False]
    bad = T.copy()
    bad.view(U32)[0, 11] = 0x100
    with pytest.raises(AssertionError):
        lp.split(bad)


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
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match=r"trace_lit: tail_after must be in 1 \.\. 6"):
            S.trace_lit(Fake(), rays, vol, tail_after=bad)
        with pytest.raises(ValueError, match=r"probes_lit: tail_after must be in 1 \.\. 6"):
            S.probes_lit(Fake(), probes, vol, tail_after=bad)
        with pytest.raises(ValueError, match=r"ProbeVolume.relight: tail_after must be in 1 \.\. 6"):
            V.relight(vol, Fake(), 4, 1, tail_after=bad)
        with pytest.raises(ValueError, match=r"path_tails: tail_after must be in 1 \.\. 6"):
            S.path_tails(Fake(), rays, bad)
    with pytest.raises(ValueError, match=r"path_tails: tail_after must be in 1 \.\. 6"):
        S.path_tails(Fake(), rays, None)
    for bad in (NAN, INF):
        with pytest.raises(ValueError, match="path_tails: bias must be finite"):
            S.path_tails(Fake(), rays, 1, bias=bad)
    with pytest.raises(ValueError, match=r"path_tails: rays must have shape \(n, 8\)"):
        S.path_tails(Fake(), probes, 1)
    with pytest.raises(ValueError, match=r"path_tails: keys must be \(n,\) uint32"):
        S.path_tails(Fake(), rays, 1, keys=np.zeros(3, U32))
    with pytest.raises(ValueError, match=r"path_tails: out must be \(n, 16\) float32"):
        S.path_tails(Fake(), rays, 1, out=np.zeros((4, 3), F32))
    # the arguments of the one-segment forms are still checked first, with the tail given
    with pytest.raises(ValueError, match="trace_lit: eval_flags: PROBE_EVAL_RADIANCE"):
        S.trace_lit(Fake(), rays, vol, eval_flags=hrt.PROBE_EVAL_RADIANCE, tail_after=9)


# --------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_cli_refuses_a_tail_it_cannot_use_before_it_touches_a_device():
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8"]
    grid = ["--probe-grid", "2,2,1", "--probe-box", "-1,-1,-1,1,1,1"]
    for bad in ("0", "7", "-1", "x", "2.5"):
        r = subprocess.run(base + grid + ["--probe-lit", "--probe-tail", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-tail takes a number of diffuse hits in 1 .. 6" in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + grid + ["--probe-quad", "0", "--probe-tail", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-tail" in r.stderr and "--probe-lit" in r.stderr and "--probe-bounces" in r.stderr, r.stderr
