"""Baking without a GPU (include/hrt.h "Baking"): the five entry points are exported and Python's Quad has the header's layout;
every bad argument -- flags, pointers, counts, samples -- is refused with HRT_ERR_INVALID and a message that names the entry point
and the culprit, in the header's order and before the scene and the library state are looked at, a NULL scene after those checks,
and an empty batch returns HRT_OK; the two host point generators equal tests/bake_ref.py bit for bit, through libhrt.so and through
a stand-alone program built with the address and undefined-behaviour sanitizers (make bake_check).  The device pointers below are
never dereferenced: every call fails validation first."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bake_ref
from conftest import PKG

HRT_OK, HRT_ERR_INVALID = 0, -1
PTS, KEYS, OUT = 0x1000, 0x3000, 0x2000
GAMMA, NO_LDS, WAVE, STREAM, NO_SHADOW_CULL, DUAL, EXACT, BRUTE, NORMALIZE, ACCUMULATE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ["hrt_bake_rays", "hrt_bake_device", "hrt_bake", "hrt_bake_quad_points", "hrt_bake_mesh_points"]
TRACED = NAMES[:3]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def call(hrt, entry, pts=PTS, keys=0, n=5, first=0, ns=1, seed=1, flags=0, out=OUT):
    """One call of `entry` with a NULL scene and pointers that are never followed."""
    dev = hrt.device_lib()
    p, k, o = C.c_void_p(pts), C.c_void_p(keys), C.c_void_p(out)
    if entry == "hrt_bake_rays":
        rc = dev.hrt_bake_rays(p, k, n, first, seed, o, None)
    elif entry == "hrt_bake_device":
        rc = dev.hrt_bake_device(None, p, k, n, first, ns, seed, flags, o, None)
    else:
        rc = dev.hrt_bake(None, p, k, n, ns, seed, flags, o, None)
    return rc, dev.hrt_last_error().decode()


def passes(hrt, entry, **kw):
    """The arguments get past every check before the last: hrt_bake_rays stops at its NULL output, the others at the NULL scene."""
    if entry == "hrt_bake_rays":
        kw["out"] = 0
    rc, msg = call(hrt, entry, **kw)
    return (rc == HRT_ERR_INVALID and ("d_rays is NULL" if entry == "hrt_bake_rays" else "scene is NULL") in msg), msg


# ------------------------------------------------------------------------------------------------------------------- exports
@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_five_symbols(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported


def test_the_quad_has_the_headers_layout(hrt):
    Q = hrt.Quad
    assert C.sizeof(Q) == 64
    assert [Q.v0.offset, Q.v1.offset, Q.v3.offset, Q.tangent.offset, Q.bitangent.offset, Q.material.offset] == [0, 12, 24, 36, 48, 60]
    host = hrt.HostScene().setup("cornell_mesh", 1.0, 1)
    quads = hrt.scene_quads(host.flatten())
    assert len(quads) >= 5 and all(np.isfinite(list(q.v0) + list(q.v1) + list(q.v3)).all() for q in quads)
    assert all(0 <= q.material < 64 for q in quads)  # the field after the five vectors is where the header puts it


# --------------------------------------------------------------------------------------------------------------------- flags
KNOWN = (NO_LDS, EXACT, BRUTE, ACCUMULATE)
BY_NAME = {WAVE: "HRT_FLAG_WAVE_KERNEL", STREAM: "HRT_FLAG_STREAM_KERNEL", DUAL: "HRT_FLAG_DUAL_KERNEL", NO_SHADOW_CULL: "HRT_FLAG_NO_SHADOW_CULL",
           NORMALIZE: "HRT_RAYS_NORMALIZE", GAMMA: "HRT_FLAG_GAMMA"}


@pytest.mark.parametrize("entry", ["hrt_bake_device", "hrt_bake"])
@pytest.mark.parametrize("bit", [b for b in range(32) if (1 << b) not in KNOWN])
def test_every_other_flag_bit_is_refused_by_name(hrt, entry, bit):
    rc, msg = call(hrt, entry, flags=1 << bit)
    assert rc == HRT_ERR_INVALID and entry in msg and "flags" in msg, (bit, msg)
    assert BY_NAME.get(1 << bit, str(1 << bit)) in msg, (bit, msg)


@pytest.mark.parametrize("entry", ["hrt_bake_device", "hrt_bake"])
def test_flag_combinations(hrt, entry):
    for extra in (0, NO_LDS):
        rc, msg = call(hrt, entry, flags=BRUTE | extra)
        assert rc == HRT_ERR_INVALID and "EXACT_ONLY" in msg, msg
    for flags in (0, EXACT, EXACT | BRUTE, NO_LDS, EXACT | BRUTE | NO_LDS):
        ok, msg = passes(hrt, entry, flags=flags)
        assert ok, (flags, msg)
    ok, msg = passes(hrt, "hrt_bake_device", flags=ACCUMULATE | EXACT | BRUTE | NO_LDS)
    assert ok, msg
    rc, msg = call(hrt, "hrt_bake", flags=ACCUMULATE)  # the host form has no running sums to add to
    assert rc == HRT_ERR_INVALID and "hrt_bake" in msg and "ACCUMULATE" in msg and "hrt_bake_device" in msg, msg


# ------------------------------------------------------------------------------------------------------- counts and pointers
@pytest.mark.parametrize("entry", TRACED)
def test_an_empty_batch_returns_ok_whatever_else_is_passed(hrt, entry):
    rc, msg = call(hrt, entry, n=0, pts=0, keys=KEYS + 1, ns=0, first=2 ** 32 - 1, out=0)
    assert rc == HRT_OK, msg
    if entry != "hrt_bake_rays":  # but the flags are checked first
        rc, msg = call(hrt, entry, n=0, flags=WAVE)
        assert rc == HRT_ERR_INVALID and "HRT_FLAG_WAVE_KERNEL" in msg, msg
    if entry == "hrt_bake":
        st = hrt.Stats(kernel_ms=1.0, samples=7)
        assert hrt.device_lib().hrt_bake(None, None, None, 0, 1, 1, 0, None, C.byref(st)) == HRT_OK and st.samples == 0 and st.kernel_ms == 0


@pytest.mark.parametrize("entry", TRACED)
def test_points_and_keys(hrt, entry):
    name = "points" if entry == "hrt_bake" else "d_points"
    rc, msg = call(hrt, entry, pts=0)
    assert rc == HRT_ERR_INVALID and entry in msg and f"{name} is NULL" in msg, msg
    for off in ((1, 2) if entry == "hrt_bake" else (4, 8, 12)):  # device records are read with 16-byte loads, host ones copied
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
def test_too_many_points_are_refused_and_named(hrt, entry, n):
    rc, msg = call(hrt, entry, n=n)
    assert rc == HRT_ERR_INVALID and entry in msg and "2^31 - 1" in msg and str(n) in msg, msg
    ok, msg = passes(hrt, entry, n=2 ** 31 - 1)
    assert ok, msg


@pytest.mark.parametrize("entry", ["hrt_bake_device", "hrt_bake"])
def test_samples(hrt, entry):
    for first in (0, 5, 2 ** 32 - 1):
        rc, msg = call(hrt, entry, first=first, ns=0)
        assert rc == HRT_ERR_INVALID and entry in msg and "n_samples must be positive" in msg, msg
    for first, ns in ((2 ** 32 - 1, 2), (2, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 1)):
        rc, msg = call(hrt, "hrt_bake_device", first=first, ns=ns)
        assert rc == HRT_ERR_INVALID and "hrt_bake_device" in msg and "first_sample + n_samples must be at most 2^32" in msg and "wrap" in msg, msg
    for first, ns in ((2 ** 32 - 1, 1), (0, 2 ** 32 - 1), (2 ** 31, 2 ** 31)):
        ok, msg = passes(hrt, "hrt_bake_device", first=first, ns=ns)
        assert ok, msg
    ok, msg = passes(hrt, "hrt_bake_rays", first=2 ** 32 - 1)
    assert ok, msg


def test_outputs(hrt):
    for out in (0, OUT + 4, OUT + 8):
        rc, msg = call(hrt, "hrt_bake_rays", out=out)
        assert rc == HRT_ERR_INVALID and "hrt_bake_rays" in msg and "d_rays" in msg, msg
    for entry, word in (("hrt_bake_device", "d_out"), ("hrt_bake", "out")):
        for out in (0, OUT + 1, OUT + 2):
            rc, msg = call(hrt, entry, out=out)
            assert rc == HRT_ERR_INVALID and entry in msg and f": {word} is " in msg, (out, msg)
        for out in (OUT + 4, OUT + 12):
            ok, msg = passes(hrt, entry, out=out)
            assert ok, (out, msg)


def test_the_checks_come_in_the_headers_order_and_before_the_scene(hrt):
    e = "hrt_bake_device"
    wrong = dict(pts=PTS + 4, keys=KEYS + 2, n=2 ** 31, ns=0, first=2 ** 32 - 1, out=0)
    assert "flags" in call(hrt, e, flags=WAVE, **wrong)[1]
    assert "d_points is not 16-byte aligned" in call(hrt, e, **wrong)[1]
    wrong["pts"] = 0
    assert "d_points is NULL" in call(hrt, e, **wrong)[1]
    wrong["pts"] = PTS
    assert "d_keys" in call(hrt, e, **wrong)[1]
    wrong["keys"] = KEYS
    assert "n must be at most" in call(hrt, e, **wrong)[1]
    wrong["n"] = 5
    assert "n_samples must be positive" in call(hrt, e, **wrong)[1]
    wrong["ns"] = 2
    assert "first_sample" in call(hrt, e, **wrong)[1]
    wrong["first"] = 0
    assert "d_out is NULL" in call(hrt, e, **wrong)[1]
    wrong["out"] = OUT + 2
    assert "d_out is not 4-byte aligned" in call(hrt, e, **wrong)[1]
    wrong["out"] = OUT
    assert "scene is NULL" in call(hrt, e, **wrong)[1]
    r = "hrt_bake_rays"
    assert "d_points" in call(hrt, r, pts=0, keys=KEYS + 2, n=2 ** 31, out=0)[1]
    assert "d_keys" in call(hrt, r, keys=KEYS + 2, n=2 ** 31, out=0)[1]
    assert "n must be at most" in call(hrt, r, n=2 ** 31, out=0)[1]
    assert "d_rays is NULL" in call(hrt, r, out=0)[1]
    for entry in ("hrt_bake_device", "hrt_bake"):
        for kw in (dict(flags=GAMMA), dict(pts=0), dict(keys=KEYS + 1), dict(n=2 ** 31), dict(ns=0), dict(out=0)):
            rc, msg = call(hrt, entry, **kw)
            assert rc == HRT_ERR_INVALID and "scene" not in msg, (kw, msg)


def test_python_binding_checks_its_arguments(hrt):
    pts = np.zeros((4, 8), F32)
    with pytest.raises(ValueError, match="points"):
        hrt.DeviceScene.bake(None, np.zeros((4, 7), F32))
    with pytest.raises(ValueError, match="keys"):
        hrt.DeviceScene.bake(None, pts, keys=np.zeros(3, U32))
    with pytest.raises(ValueError, match="out"):
        hrt.DeviceScene.bake(None, pts, out=np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match="accumulate"):
        hrt.DeviceScene.bake(None, pts, first_sample=3, accumulate=True)
    with pytest.raises(ValueError, match="points"):
        hrt.bake_rays(pts)  # the rays of a sample are made on the device: a torch tensor there


# --------------------------------------------------------------------------------------------------------------- generators
TILTED = ((0.3, -1.7, 2.1), (2.9, -1.1, 2.6), (-0.2, 0.8, 3.3))
FLOOR = ((-2.0, -2.0, 2.0), (2.0, -2.0, 2.0), (-2.0, -2.0, -2.0))
MESH_POS = np.array([[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0.3], [-1, 0.4, 0.5], [0.3, -1, 0.25], [7, 8, 9]], F32)
MESH_IDX = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [4, 4, 1]], U32)  # vertex 0 shared by three, 5 unused, 4 named twice by one


@pytest.mark.parametrize("tw", [1, 3, 8])
@pytest.mark.parametrize("th", [1, 3, 8])
@pytest.mark.parametrize("side", [1, -1])
def test_quad_points_equal_the_numpy_rule_bit_for_bit(hrt, tw, th, side):
    for (v0, v1, v3), time, bias in ((TILTED, 0.25, 1e-4), (FLOOR, 0.0, 0.0)):
        got = hrt.quad_points(hrt.Quad.make(v0, v1, v3), tw, th, side, time, bias)
        want = bake_ref.quad_points(v0, v1, v3, tw, th, side, time, bias)
        assert got.shape == (tw * th, 8) and np.array_equal(bits(got), bits(want)), (tw, th, side)
        Nn = want[0, 4:7].astype(np.float64)
        assert abs(Nn @ Nn - 1) < 1e-6 and np.array_equal(bits(got[:, 4:7]), bits(np.tile(want[0, 4:7], (tw * th, 1))))
    # +1 is the side the trace path lights: the floor's normal points up into the box
    assert hrt.quad_points(hrt.Quad.make(*FLOOR), 1, 1, 1)[0, 4:7].tolist() == [0, 1, 0]


def test_mesh_points_equal_the_numpy_rule_bit_for_bit(hrt):
    got = hrt.mesh_points(MESH_POS, MESH_IDX, 0.5, 1e-3)
    want = bake_ref.mesh_points(MESH_POS, MESH_IDX, 0.5, 1e-3)
    assert got.shape == (6, 8) and np.array_equal(bits(got), bits(want))
    assert (got[5, 4:7] == 0).all() and bake_ref.point_degenerate(got).tolist() == [False] * 5 + [True]  # the unused vertex
    one = bake_ref.mesh_points(MESH_POS, MESH_IDX[:1], 0.5, 1e-3)
    assert not np.array_equal(got[0, 4:7], one[0, 4:7]) and np.array_equal(got[1, 0:4], one[1, 0:4])  # the shared vertex sums
    none = hrt.mesh_points(MESH_POS, np.zeros((0, 3), U32))
    assert np.array_equal(none[:, 0:3], MESH_POS) and (none[:, 4:7] == 0).all()
    assert hrt.mesh_points(np.zeros((0, 3), F32), np.zeros((0, 3), U32)).shape == (0, 8)


def test_the_generators_refuse_by_name(hrt):
    q = hrt.Quad.make(*TILTED)
    for kw, word in ((dict(tw=0), "tw and th"), (dict(th=0), "tw and th"), (dict(tw=65536, th=32768), "2^31 - 1"), (dict(side=0), "side"),
                     (dict(side=2), "side"), (dict(side=-2), "side"), (dict(time=NAN), "time"), (dict(time=INF), "time"),
                     (dict(bias=-INF), "bias"), (dict(bias=NAN), "bias")):
        args = dict(tw=2, th=2, side=1, time=0.0, bias=0.0)
        args.update(kw)
        with pytest.raises(hrt.HrtError, match="hrt_bake_quad_points") as e:
            hrt.quad_points(q, **args)
        assert word in str(e.value), (kw, str(e.value))
    dev = hrt.device_lib()
    buf = np.zeros(8, F32)
    assert dev.hrt_bake_quad_points(None, 1, 1, 1, 0.0, 0.0, buf.ctypes.data) == HRT_ERR_INVALID and b"quad is NULL" in dev.hrt_last_error()
    assert dev.hrt_bake_quad_points(C.byref(q), 1, 1, 1, 0.0, 0.0, None) == HRT_ERR_INVALID and b"out_points is NULL" in dev.hrt_last_error()
    for bad in ([[0, 1, 6]], [[0, 1, 2], [2 ** 32 - 1, 0, 1]]):
        with pytest.raises(hrt.HrtError, match="hrt_bake_mesh_points.*n_vertices"):
            hrt.mesh_points(MESH_POS, np.array(bad, U32))
    for kw, word in ((dict(time=NAN), "time"), (dict(bias=INF), "bias")):
        with pytest.raises(hrt.HrtError, match="hrt_bake_mesh_points") as e:
            hrt.mesh_points(MESH_POS, MESH_IDX, **kw)
        assert word in str(e.value)
    p, ix, out = MESH_POS.ctypes.data, MESH_IDX.ctypes.data, np.zeros((6, 8), F32).ctypes.data
    for args, word in (((None, 6, ix, 4, 0.0, 0.0, out), b"positions is NULL"), ((p, 6, None, 4, 0.0, 0.0, out), b"indices is NULL"),
                       ((p, 6, ix, 4, 0.0, 0.0, None), b"out_points is NULL")):
        assert dev.hrt_bake_mesh_points(*args) == HRT_ERR_INVALID and word in dev.hrt_last_error()


# ------------------------------------------------------------------------------------------------- the sanitized program
@pytest.fixture(scope="module")
def bake_check():
    """What the stand-alone program prints: the generators' header under the address and undefined-behaviour sanitizers."""
    subprocess.run(["make", "-s", "-C", PKG, "bake_check"], check=True)
    r = subprocess.run([os.path.join(PKG, "bake_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"bake_check: exit {r.returncode}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout)


def test_the_sanitized_program_gives_the_numpy_rule_bit_for_bit(bake_check):
    seen = 0
    for qname, (v0, v1, v3), time, bias in (("tilted", TILTED, 0.25, 1e-4), ("floor", FLOOR, 0.0, 0.0)):
        for tw in (1, 3, 8):
            for th in (1, 3, 8):
                for side, sname in ((1, "front"), (-1, "back")):
                    got = bake_check[f"{qname}_{tw}x{th}_{sname}"]
                    want = bake_ref.quad_points(v0, v1, v3, tw, th, side, time, bias)
                    assert got["rc"] == HRT_OK and np.array_equal(np.array(got["records"], U32).reshape(-1, 8), bits(want)), (qname, tw, th, side)
                    seen += 1
    assert seen == 36
    got = bake_check["mesh_fan"]
    assert got["rc"] == HRT_OK and np.array_equal(np.array(got["records"], U32).reshape(-1, 8), bits(bake_ref.mesh_points(MESH_POS, MESH_IDX, 0.5, 1e-3)))
    got = bake_check["mesh_no_triangles"]
    assert got["rc"] == HRT_OK and np.array_equal(np.array(got["records"], U32).reshape(-1, 8), bits(bake_ref.mesh_points(MESH_POS, [], 0.0, 0.0)))
    assert bake_check["mesh_empty"] == {"rc": HRT_OK, "error": "", "records": []}


def test_the_sanitized_program_refuses_before_it_follows_a_bad_index(bake_check):
    words = {"quad_null": "quad is NULL", "quad_null_out": "out_points is NULL", "quad_tw_zero": "tw and th", "quad_th_zero": "tw and th",
             "quad_too_many": "2^31 - 1", "quad_side_zero": "side", "quad_side_two": "side", "quad_time_nan": "time", "quad_bias_inf": "bias",
             "mesh_bad_index": "vertex index 6 >= n_vertices 6", "mesh_huge_index": "vertex index 4294967295", "mesh_null_positions": "positions is NULL",
             "mesh_null_indices": "indices is NULL", "mesh_null_out": "out_points is NULL", "mesh_time_inf": "time", "mesh_bias_nan": "bias"}
    assert set(words) == {k for k, v in bake_check.items() if v["rc"] != HRT_OK}
    for case, word in words.items():
        got = bake_check[case]
        entry = "hrt_bake_quad_points" if case.startswith("quad") else "hrt_bake_mesh_points"
        assert got["rc"] == HRT_ERR_INVALID and got["error"].startswith(entry + ": ") and word in got["error"] and got["records"] == [], (case, got)


# --------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_cli_refuses_a_quad_past_the_scenes_before_it_touches_a_device(hrt):
    from conftest import ROOT
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8"]
    n = len(hrt.scene_quads(hrt.HostScene().setup("cornell_box", 1.0, 1).flatten()))
    for index in (str(n), "99", "-2"):
        r = subprocess.run(base + ["--bake-quad", index], capture_output=True, text=True)
        assert r.returncode == 2 and f"--bake-quad {index}" in r.stderr and f"{n} quads" in r.stderr, (index, r.returncode, r.stderr)
    r = subprocess.run(base + ["--bake-quad", "0", "--lens", "ortho"], capture_output=True, text=True)
    assert r.returncode == 2 and "--bake-quad" in r.stderr
    r = subprocess.run(base + ["--bake-side", "-1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--bake-quad INDEX" in r.stderr
