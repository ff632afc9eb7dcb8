"""Lit bakes without a GPU (include/hrt.h "Lit bakes": hrt_bake_lit_device, hrt_bake_lit): the two entry points are exported and
declared; every bad argument that can be reached without a device is refused with HRT_ERR_INVALID and a message that names the
entry point and the culprit, in the header's order -- (the blocking form: HRT_RADIANCE_ACCUMULATE,) the flags of a bake, n == 0,
the points, keys and n as hrt_bake* checks them, the samples and the output, tail_after, then the volume checks of "Lit rays".  A
volume cannot be created without a device, so "the volume is NULL" is the last refusal reachable here through the C ABI: what comes
after it is in tests/test_gpu_bake_lit.py, and the non-finite bias is refused here where a caller meets it first, in the Python
wrapper.  The entry points add no host logic of their own -- they are hrt_bake*'s body (bake_call: bake_flags_check,
bake_points_check, samples_out_check) with a LitRule (check, enter) -- so there is no sanitized stand-alone program for them.  The
pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import probe_volume_ref as pv

HRT_OK, HRT_ERR_INVALID = 0, -1
PTS, OUT, KEYS = 0x1000, 0x2000, 0x3000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ["hrt_bake_lit_device", "hrt_bake_lit"]
NAN, INF = float("nan"), float("inf")
TAIL_RANGE = "tail_after must be in 1 .. HRT_MAXBOUNCES = 6 (got {})"


def call(hrt, entry, points=PTS, keys=0, n=4, first=0, ns=1, seed=1, flags=0, eval_flags=0, bias=0.0, tail=0, out=OUT, stats=None):
    """One call of `entry` with a NULL scene and a NULL volume."""
    dev = hrt.device_lib()
    p, k, o = C.c_void_p(points), C.c_void_p(keys), C.c_void_p(out)
    if entry == "hrt_bake_lit_device":
        rc = dev.hrt_bake_lit_device(None, None, p, k, n, first, ns, seed, flags, eval_flags, bias, tail, o, None)
    else:
        rc = dev.hrt_bake_lit(None, None, p, k, n, ns, seed, flags, eval_flags, bias, tail, o, stats)
    return rc, dev.hrt_last_error().decode()


def names(entry):
    return ("d_points", "d_keys", "d_out") if entry.endswith("_device") else ("points", "keys", "out")


LATER = dict(eval_flags=1, bias=NAN, tail=7)  # everything after the bake's own checks wrong at once


@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_two_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API int " + name + r"\(", pv.header_text(), re.M)


def test_the_section_its_rule_and_its_scope(hrt):
    text = pv.header_text()
    assert text.index("/* ---- Lit frames:") < text.index("/* ---- Lit bakes:") < text.index("/* ---- Adaptive lit frames:")
    section = text[text.index("/* ---- Lit bakes:"):text.index("/* ---- Adaptive lit frames:")]
    flat = re.sub(r"\s*\n \* ", " ", section)
    assert "hrt_bake_rays(d_points, d_keys, n, s, seed)" in flat and "the same d_keys, first_sample = s, n_samples = 1" in flat
    assert "NOT the point record's own bias" in flat, "the two biases are told apart"
    m = re.search(r"OUT OF SCOPE \(DESIGN.md section 5 \"Lit bakes\"\): ([^/]*)\*/", text)
    assert m
    scope = re.sub(r"\s*\n \* ", " ", m.group(1))
    for item in ("cooperative or parked look-up", "batched point sets over several volumes", "multi-GPU"):
        assert item in scope, item


@pytest.mark.parametrize("entry", NAMES)
@pytest.mark.parametrize("bit", range(32))
def test_the_flags_are_those_of_a_bake_and_come_first(hrt, entry, bit):
    """An accepted flag bit reaches the next check, a refused one is named -- with every later argument wrong as well."""
    flag = 1 << bit
    rc, msg = call(hrt, entry, flags=flag | (EXACT if flag == BRUTE else 0), points=0, keys=2, n=2 ** 31, ns=0, out=0, **LATER)
    taken = {NO_LDS, EXACT, BRUTE} | (set() if entry == "hrt_bake_lit" else {ACCUMULATE})
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": "), msg
    if flag in taken:
        assert msg == f"{entry}: {names(entry)[0]} is NULL", (bit, msg)
    else:
        assert "flags" in msg, (bit, msg)
        named = {GAMMA: "HRT_FLAG_GAMMA", WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL",
                 NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL", NORMALIZE: "HRT_RAYS_NORMALIZE", ACCUMULATE: "HRT_RADIANCE_ACCUMULATE"}
        assert named[flag] in msg if flag in named else "unknown bits " + str(flag) in msg, (bit, msg)
        if flag == ACCUMULATE:
            assert "hrt_bake_lit_device" in msg, "the blocking form says where the running sums live"


@pytest.mark.parametrize("entry", NAMES)
def test_flag_combinations_are_refused_as_a_bake_refuses_them(hrt, entry):
    rc, msg = call(hrt, entry, flags=BRUTE, **LATER)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry) and "HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY" in msg, msg
    if entry == "hrt_bake_lit":  # ACCUMULATE comes before the other flags in the blocking form
        rc, msg = call(hrt, entry, flags=ACCUMULATE | WAVE, **LATER)
        assert rc == HRT_ERR_INVALID and "HRT_RADIANCE_ACCUMULATE" in msg and "WAVE" not in msg, msg


@pytest.mark.parametrize("entry", NAMES)
def test_an_empty_batch_returns_ok_after_the_flags(hrt, entry):
    """Nothing but the flags is looked at: no points, no output, no tail_after, no volume, no scene."""
    assert call(hrt, entry, n=0, points=0, keys=2, ns=0, out=0, **LATER)[0] == HRT_OK
    rc, msg = call(hrt, entry, n=0, flags=WAVE)
    assert rc == HRT_ERR_INVALID and "HRT_FLAG_WAVE_KERNEL" in msg, msg
    if entry == "hrt_bake_lit":
        stats = hrt.Stats()
        stats.samples = 99
        assert call(hrt, entry, n=0, stats=C.byref(stats))[0] == HRT_OK and stats.samples == 0


@pytest.mark.parametrize("entry", NAMES)
def test_points_keys_n_samples_and_output_in_the_order_of_a_bake(hrt, entry):
    pn, kn, on = names(entry)
    dev_form = entry.endswith("_device")
    every = dict(points=0, keys=2, n=2 ** 31, ns=0, out=0, **LATER)
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {pn} is NULL")
    align = 16 if dev_form else 4
    every["points"] = PTS + (8 if dev_form else 2)
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {pn} is not {align}-byte aligned")
    every["points"] = PTS
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {kn} is not 4-byte aligned")
    every["keys"] = KEYS
    rc, msg = call(hrt, entry, **every)
    assert rc == HRT_ERR_INVALID and msg.startswith(f"{entry}: n must be at most 2^31 - 1"), msg
    every["n"] = 2 ** 31 - 1
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": n_samples must be positive")
    if dev_form:
        for first, ns in ((2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1)):
            rc, msg = call(hrt, entry, **dict(every, first=first, ns=ns))
            assert (rc, msg) == (HRT_ERR_INVALID, entry + ": first_sample + n_samples must be at most 2^32 (sample indices do not wrap)"), (first, ns)
        assert call(hrt, entry, first=2 ** 32 - 1, ns=1) == (HRT_ERR_INVALID, entry + ": volume is NULL")
    every["ns"] = 4
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")
    assert call(hrt, entry, **dict(every, out=OUT + 2)) == (HRT_ERR_INVALID, f"{entry}: {on} is not 4-byte aligned")
    every["out"] = OUT
    assert call(hrt, entry, **every) == (HRT_ERR_INVALID, entry + ": " + TAIL_RANGE.format(7)), "tail_after is next"


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
        assert call(hrt, entry, eval_flags=ef, bias=NAN) == (HRT_ERR_INVALID, entry + ": volume is NULL"), ef


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

    vol, pts = FakeVolume(), np.zeros((3, 8), dtype=np.float32)
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match=r"bake_lit: tail_after must be in 1 \.\. 6"):
            S.bake_lit(Fake(), pts, vol, tail_after=bad)
    for bad in (NAN, INF, -INF):
        with pytest.raises(ValueError, match="bake_lit: bias must be finite"):
            S.bake_lit(Fake(), pts, vol, bias=bad)
    with pytest.raises(ValueError, match="bake_lit: eval_flags: PROBE_EVAL_RADIANCE"):
        S.bake_lit(Fake(), pts, vol, eval_flags=hrt.PROBE_EVAL_RADIANCE)
    with pytest.raises(ValueError, match="bake_lit: eval_flags: unknown bits 8"):
        S.bake_lit(Fake(), pts, vol, eval_flags=8)
    with pytest.raises(ValueError, match="bake_lit: volume must be a ProbeVolume"):
        S.bake_lit(Fake(), pts, None)
    with pytest.raises(ValueError, match="bake_lit: "):
        S.bake_lit(Fake(), np.zeros((3, 7), dtype=np.float32), vol)
    with pytest.raises(ValueError, match="bake_lit: keys must be"):
        S.bake_lit(Fake(), pts, vol, keys=np.zeros(2, dtype=np.uint32))
    with pytest.raises(ValueError, match="bake_lit: accumulate after sample 0 needs the running sums"):
        S.bake_lit(Fake(), pts, vol, first_sample=2, accumulate=True)
    doc = S.bake_lit.__doc__
    assert "not the point record's own bias" in doc and "LOOK-UP" in doc
