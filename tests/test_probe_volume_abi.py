"""Probe volumes without a GPU (include/hrt.h "Probe volumes"): the seven entry points are exported and declared and the constants
are the header's; hrt_probe_volume_weights -- the shared header csrc/hrt_probe_volume_cell.h, as the kernel runs it -- equals
tests/probe_volume_ref.py bit for bit, through libhrt.so and through a stand-alone program built with the address and
undefined-behaviour sanitizers (make probe_volume_check); every bad argument that can be reached without a device is refused with
HRT_ERR_INVALID and a message that names the entry point and the culprit, in the header's order; the Python wrapper refuses before
it touches a library; the command-line tool refuses what it cannot combine.  A volume cannot be created without a device (create
allocates), so the checks that come after "the volume is NULL" are exercised in tests/test_gpu_probe_volume.py.  The device
pointers below are never dereferenced: every call fails validation first."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import probe_volume_ref as pv
from conftest import PKG, ROOT

HRT_OK, HRT_ERR_INVALID, HRT_ERR_STATE = 0, -1, -2
PTS, OUT = 0x1000, 0x2000
RADIANCE, FACING = 1, 2
NAMES = ["hrt_probe_volume_create", "hrt_probe_volume_update_device", "hrt_probe_volume_update", "hrt_probe_volume_destroy",
         "hrt_probe_eval_device", "hrt_probe_eval", "hrt_probe_volume_weights"]
EVAL = ["hrt_probe_eval_device", "hrt_probe_eval"]
F32, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")

# The grids of tests/test_gpu_probe_volume.py (and of tests/probe_volume/probe_volume_check.cpp).
BOX = ((-1.7, 0.3, 2.1), (2.9, 1.1, 7.6))
BACK = ((-1.0, 2.0, 0.0), (1.0, -0.5, 3.0))  # lo > hi on y
GRIDS = {"grid_3x2x4": (BOX, (3, 2, 4)), "grid_1x1x1": (BOX, (1, 1, 1)), "grid_4x1x1": (BOX, (4, 1, 1)), "grid_2x2x2_back": (BACK, (2, 2, 2))}


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def rule_points(box, counts, seed=5):
    """The point records of the rule's tests for one grid: random inside, exactly at probe centres, exactly on cell faces, outside
    past every face and corner, huge but finite positions, and the degenerate records; normals of every length and direction."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(box[0], F32), np.asarray(box[1], F32)
    n = np.asarray(counts)
    e = hi - lo
    P = [lo + rng.random((40, 3)).astype(F32) * e]
    ijk = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), -1).reshape(-1, 3)
    P.append(pv.centres(lo, hi, counts, ijk))                                                       # probe centres
    P.append((lo + (ijk.astype(F32) / n.astype(F32)) * e).astype(F32))                              # cell faces, the box's own included
    P.append((lo + ((ijk + 1).astype(F32) / n.astype(F32)) * e).astype(F32))
    t = np.stack(np.meshgrid(*[np.array([-0.6, 0.37, 1.8], F32)] * 3, indexing="ij"), -1).reshape(-1, 3)  # past every face, edge and corner
    P.append((lo + t * e).astype(F32))
    P.append(np.array([[1e18, -1e18, 1e18], [-1e18, 0.5, 3e18], [lo[0], 1e18, hi[2]]], F32))        # huge but finite
    P = np.concatenate(P).astype(F32)
    N = rng.standard_normal((len(P), 3)).astype(F32) * F32(10.0) ** rng.integers(-3, 4, (len(P), 1)).astype(F32)
    N[::7] = np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0], [0, 0, -1]], F32)[np.arange(len(N[::7])) % 4]
    pts = np.zeros((len(P), 8), F32)
    pts[:, 0:3], pts[:, 3], pts[:, 4:7], pts[:, 7] = P, 0.25, N, 1e-4
    mid = (lo + F32(0.4) * e).astype(F32)
    deg = np.zeros((7, 8), F32)
    deg[:, 0:3], deg[:, 6] = mid, 1.0
    deg[0, 0] = NAN          # NaN in P
    deg[1, 1] = -INF
    deg[2, 5] = INF          # inf in N
    deg[3, 4] = NAN
    deg[4, 4:7] = 0          # N == 0
    deg[5, 4:7] = (-0.0, 0.0, 0.0)
    deg[6, 4:7] = (1e-30, 0, 0)  # a squared length that underflows
    ok = np.zeros((1, 8), F32)   # time and bias are not read
    ok[0, 0:3], ok[0, 3], ok[0, 4:7], ok[0, 7] = mid, NAN, (0, 1, 0), INF
    return np.concatenate([pts, deg, ok]).astype(F32), len(pts), len(pts) + len(deg)


# ------------------------------------------------------------------------------------------------------------------- exports
@pytest.mark.parametrize("name", NAMES)
def test_libhrt_exports_the_seven_symbols_and_the_header_declares_them(hrt, name):
    dev = hrt.device_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dev._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert hasattr(dev, name) and name in exported
    assert re.search(r"^HRT_API (?:int|void) " + name + r"\(", pv.header_text(), re.M)


def test_the_headers_constants(hrt):
    text = pv.header_text()
    assert re.search(r"#define HRT_PROBE_VOLUME_MAX \(1u << 24\)", text) and re.search(r"#define HRT_PROBE_RECORD_FLOATS 32\b", text)
    assert re.search(r"#define HRT_PROBE_EVAL_RADIANCE 1u\b", text) and re.search(r"#define HRT_PROBE_EVAL_FACING +2u\b", text)
    assert (hrt.PROBE_VOLUME_MAX, hrt.PROBE_RECORD_FLOATS, hrt.PROBE_EVAL_RADIANCE, hrt.PROBE_EVAL_FACING) == (1 << 24, 32, RADIANCE, FACING)
    assert hrt.PROBE_RECORD_FLOATS * 4 == 128 and hrt.PROBE_RECORD_FLOATS >= 3 * hrt.PROBE_COEFFS
    assert hrt.PROBE_VOLUME_MAX * hrt.PROBE_RECORD_FLOATS * 4 == 2 ** 31  # the packed copy stays at or below 2 GiB


# ----------------------------------------------------------------------------------------------------------------- the weights
@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("facing", [False, True])
def test_weights_equal_the_numpy_rule_bit_for_bit(hrt, grid, facing):
    box, counts = GRIDS[grid]
    pts, n_plain, n_deg_end = rule_points(box, counts)
    index, weight, _, deg = pv.weights(*box, counts, pts, facing)
    assert np.array_equal(np.flatnonzero(deg), np.arange(n_plain, n_deg_end)), "the degenerate records, and only they"
    assert np.isfinite(weight).all() and (index < np.prod(counts)).all()
    for i, p in enumerate(pts):
        gi, gw = hrt.probe_volume_weights(*box, *counts, p, facing)
        assert gi.dtype == U32 and gw.dtype == F32
        assert np.array_equal(gi, index[i]) and np.array_equal(bits(gw), bits(weight[i])), (grid, facing, i, p.tolist(), gw.tolist(), weight[i].tolist())
    live = ~deg
    assert np.allclose(weight[live].sum(axis=1), 1, atol=1e-6) and (weight[live] >= 0).all()
    assert not weight[deg].any() and not index[deg].any()


def test_index_order_and_clamping(hrt):
    box, counts = ((0, 0, 0), (3, 2, 4)), (3, 2, 4)
    up = [0, 0, 0, 0, 0, 0, 1, 0]
    i, w = hrt.probe_volume_weights(*box, *counts, [1.0, 1.0, 2.0] + up[3:])  # between probes 0|1 in x, 0|1 in y, 1|2 in z, half way each
    assert i.tolist() == [(k * 2 + j) * 3 + x for k in (1, 2) for j in (0, 1) for x in (0, 1)] and w.tolist() == [0.125] * 8
    i, w = hrt.probe_volume_weights(*box, *counts, [2.5, 0.5, 3.5] + up[3:])  # exactly at probe (2, 0, 3)
    assert i[0] == (3 * 2 + 0) * 3 + 2 and w.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    i, w = hrt.probe_volume_weights(*box, *counts, [-9.0, 0.5, 99.0] + up[3:])  # outside: the clamped point's probe
    assert i[0] == (3 * 2 + 0) * 3 + 0 and w[0] == 1
    i, w = hrt.probe_volume_weights((0, 0, 0), (1, 1, 1), 1, 1, 1, [5, 5, 5] + up[3:], facing=True)  # one probe: all eight corners are it
    assert i.tolist() == [0] * 8 and w.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_the_grid_and_the_weights_refuse_by_name(hrt):
    p = [0.5, 0.5, 0.5, 0, 0, 0, 1, 0]
    for kw, word in ((dict(nx=0), "nx, ny and nz"), (dict(ny=0), "nx, ny and nz"), (dict(nz=0), "nx, ny and nz"),
                     (dict(nx=4096, ny=4096, nz=2), "HRT_PROBE_VOLUME_MAX = 16777216"), (dict(nx=2 ** 32 - 1, ny=2 ** 32 - 1, nz=2 ** 32 - 1), "HRT_PROBE_VOLUME_MAX"),
                     (dict(lo=(0, NAN, 0)), "lo must be finite"), (dict(hi=(1, 1, INF)), "hi must be finite"),
                     (dict(lo=(0, 1, 0)), "lo == hi on axis y"), (dict(hi=(1, 1e-44, 1)), "axis y: n / (hi - lo) is not finite")):
        args = dict(lo=(0, 0, 0), hi=(1, 1, 1), nx=2, ny=2, nz=2)
        args.update(kw)
        with pytest.raises(hrt.HrtError, match="hrt_probe_volume_weights") as e:
            hrt.probe_volume_weights(point=p, **args)
        assert word in str(e.value), (kw, str(e.value))
    assert hrt.probe_volume_weights((0, 1, 0), (1, 1, 1), 2, 1, 2, p)[1].sum() == 1  # lo == hi is fine where the axis has one probe
    assert hrt.probe_volume_weights((0, 0, 0), (1, 1, 1), 256, 256, 256, p)[1].sum() == pytest.approx(1)  # exactly HRT_PROBE_VOLUME_MAX
    dev = hrt.device_lib()
    lo, hi, pt = np.zeros(3, F32), np.ones(3, F32), np.array(p, F32)
    ix, w = np.zeros(8, U32), np.zeros(8, F32)
    a = dict(lo=lo.ctypes.data, hi=hi.ctypes.data, pt=pt.ctypes.data, ix=ix.ctypes.data, w=w.ctypes.data)
    for null, word in (("lo", b"lo is NULL"), ("hi", b"hi is NULL"), ("pt", b"point is NULL"), ("ix", b"index is NULL"), ("w", b"weight is NULL")):
        b = dict(a)
        b[null] = None
        assert dev.hrt_probe_volume_weights(b["lo"], b["hi"], 2, 2, 2, b["pt"], 0, b["ix"], b["w"]) == HRT_ERR_INVALID
        assert dev.hrt_last_error().startswith(b"hrt_probe_volume_weights: ") and word in dev.hrt_last_error()
    assert dev.hrt_probe_volume_weights(a["lo"], a["hi"], 2, 2, 2, a["pt"], 4, a["ix"], a["w"]) == HRT_ERR_INVALID and b"flags" in dev.hrt_last_error()
    with pytest.raises(ValueError, match="probe_volume_weights: point"):
        hrt.probe_volume_weights(lo, hi, 2, 2, 2, p[:7])
    with pytest.raises(ValueError, match="probe_volume_weights: lo and hi"):
        hrt.probe_volume_weights((0, 0), hi, 2, 2, 2, p)


# ------------------------------------------------------------------------------------------------------------------- refusals
def call(hrt, entry, vol=None, pts=PTS, n=5, flags=0, out=OUT, stats=None):
    dev = hrt.device_lib()
    if entry == "hrt_probe_eval_device":
        rc = dev.hrt_probe_eval_device(vol, C.c_void_p(pts), n, flags, C.c_void_p(out), None)
    else:
        rc = dev.hrt_probe_eval(vol, C.c_void_p(pts), n, flags, C.c_void_p(out), stats)
    return rc, dev.hrt_last_error().decode()


BY_NAME = {4: "HRT_FLAG_WAVE_KERNEL", 8: "HRT_FLAG_STREAM_KERNEL", 16: "HRT_FLAG_NO_SHADOW_CULL", 32: "HRT_FLAG_DUAL_KERNEL", 64: "HRT_FLAG_EXACT_ONLY",
           128: "HRT_FLAG_MESH_BRUTE", 256: "HRT_RAYS_NORMALIZE", 512: "HRT_RADIANCE_ACCUMULATE"}


@pytest.mark.parametrize("entry", EVAL)
@pytest.mark.parametrize("bit", range(2, 32))
def test_every_other_flag_bit_is_refused_by_name(hrt, entry, bit):
    rc, msg = call(hrt, entry, flags=(1 << bit) | RADIANCE)
    assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": flags"), (bit, msg)
    assert BY_NAME.get(1 << bit, str(1 << bit)) in msg, (bit, msg)


@pytest.mark.parametrize("entry", EVAL)
def test_flags_come_first_then_an_empty_batch_then_the_volume(hrt, entry):
    wrong = dict(vol=None, pts=PTS + 2, out=0)
    rc, msg = call(hrt, entry, flags=4, n=0, **wrong)
    assert rc == HRT_ERR_INVALID and "flags" in msg, msg
    for flags in (0, RADIANCE, FACING, RADIANCE | FACING):
        rc, msg = call(hrt, entry, flags=flags, n=0, **wrong)
        assert rc == HRT_OK, msg
        rc, msg = call(hrt, entry, flags=flags, n=2 ** 31, **wrong)
        assert rc == HRT_ERR_INVALID and msg == entry + ": volume is NULL", msg
    if entry == "hrt_probe_eval":
        st = hrt.Stats(kernel_ms=1.0, samples=7)
        assert call(hrt, entry, n=0, stats=C.byref(st))[0] == HRT_OK and st.samples == 0 and st.kernel_ms == 0 and st.total_ms == 0


def test_updates_and_create_refuse_by_name(hrt):
    dev = hrt.device_lib()
    for entry, args in (("hrt_probe_volume_update_device", (None, C.c_void_p(PTS), None)), ("hrt_probe_volume_update", (None, C.c_void_p(PTS)))):
        assert getattr(dev, entry)(*args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == entry + ": volume is NULL"
    dev.hrt_probe_volume_destroy(None)  # nothing to do
    lo, hi = np.zeros(3, F32), np.ones(3, F32)
    h = C.c_void_p(0x77)
    who = "hrt_probe_volume_create: "
    assert dev.hrt_probe_volume_create(lo.ctypes.data, hi.ctypes.data, 2, 2, 2, None) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == who + "out is NULL"
    for args, word in (((None, hi.ctypes.data, 2, 2, 2), "lo is NULL"), ((lo.ctypes.data, None, 2, 2, 2), "hi is NULL"),
                       ((lo.ctypes.data, hi.ctypes.data, 0, 2, 2), "nx, ny and nz must be positive"),
                       ((lo.ctypes.data, hi.ctypes.data, 257, 256, 256), "nx * ny * nz must be at most HRT_PROBE_VOLUME_MAX"),
                       ((lo.ctypes.data, lo.ctypes.data, 1, 2, 1), "lo == hi on axis y")):
        assert dev.hrt_probe_volume_create(*args, C.byref(h)) == HRT_ERR_INVALID and dev.hrt_last_error().decode().startswith(who + word), (word, dev.hrt_last_error())
        assert h.value is None, "a refused create hands back NULL"


def test_python_binding_checks_its_arguments_before_any_library(hrt):
    V = hrt.ProbeVolume
    with pytest.raises(ValueError, match=r"ProbeVolume.eval: points must have shape \(n, 8\)"):
        V.eval(None, np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match="ProbeVolume.update: coeffs must have shape"):
        V.update(None, np.zeros((4, 27), F32))
    with pytest.raises(ValueError, match="ProbeVolume: lo and hi"):
        V((0, 0), (1, 1, 1), 1, 1, 1)

    class Fake:  # stands in for a volume: neither method may reach its handle before the arguments are right
        count = 4

        @property
        def _h(self):
            raise AssertionError("the library was reached")

    with pytest.raises(ValueError, match="the volume has 4 probes"):
        V.update(Fake(), np.zeros((5, 9, 3), F32))
    with pytest.raises(ValueError, match=r"ProbeVolume.eval: out must be a contiguous \(n, 3\) float32 array"):
        V.eval(Fake(), np.zeros((4, 8), F32), out=np.zeros((4, 4), F32))
    with pytest.raises(ValueError, match="ProbeVolume.eval: out"):
        V.eval(Fake(), np.zeros((4, 8), F32), out=np.zeros((4, 3), np.float64))


# ------------------------------------------------------------------------------------------------- the sanitized program
@pytest.fixture(scope="module")
def volume_check():
    """What the stand-alone program prints: the shared header under the address and undefined-behaviour sanitizers."""
    subprocess.run(["make", "-s", "-C", PKG, "probe_volume_check"], check=True)
    r = subprocess.run([os.path.join(PKG, "probe_volume_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"probe_volume_check: exit {r.returncode}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout)


def test_the_sanitized_program_gives_the_numpy_rule_bit_for_bit(volume_check):
    grids = dict(GRIDS, grid_3x1x2_flat=((BOX[0], (2.9, 0.3, 7.6)), (3, 1, 2)))  # lo == hi on an axis with one probe
    for name, (box, counts) in grids.items():
        got = volume_check[name]
        assert got["rc"] == HRT_OK
        pts = np.array(got["points"], U32).view(F32).reshape(-1, 8)
        assert len(pts) == 8 ** 3 + 10
        for facing, suffix in ((False, ""), (True, "_facing")):
            index, weight, _, deg = pv.weights(*box, counts, pts, facing)
            assert deg.sum() == 7 and deg[8 ** 3:8 ** 3 + 7].all()
            assert np.array_equal(np.array(got["index" + suffix], U32).reshape(-1, 8), index), (name, facing)
            gw = np.array(got["weight" + suffix], U32).reshape(-1, 8)
            bad = np.flatnonzero((gw != bits(weight)).any(axis=1))
            assert bad.size == 0, (name, facing, bad[:5].tolist(), pts[bad[:1]].tolist())


def test_the_sanitized_program_refuses_by_name(volume_check):
    words = {"null_lo": "lo is NULL", "null_hi": "hi is NULL", "nx_zero": "nx, ny and nz", "ny_zero": "nx, ny and nz", "nz_zero": "nx, ny and nz",
             "too_many": "HRT_PROBE_VOLUME_MAX", "too_many_wrapping": "HRT_PROBE_VOLUME_MAX", "lo_nan": "lo must be finite", "hi_inf": "hi must be finite",
             "flat_axis": "lo == hi on axis y", "thin_axis": "axis y: n / (hi - lo) is not finite"}
    assert set(words) == {k for k, v in volume_check.items() if v["rc"] != HRT_OK}
    for case, word in words.items():
        got = volume_check[case]
        assert got["rc"] == HRT_ERR_INVALID and got["error"].startswith("hrt_probe_volume_create: ") and word in got["error"] and "points" not in got, (case, got)


# --------------------------------------------------------------------------------------------------------------------- the CLI
def test_the_cli_refuses_what_it_cannot_combine_before_it_touches_a_device():
    exe = os.path.join(PKG, "raytracer")
    base = [exe, "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8"]
    grid, box = ["--probe-grid", "2,2,1"], ["--probe-box", "-1,-1,-1,1,1,1"]
    for extra in ([], ["--probe-side", "-1"], ["--probe-facing"]):  # a look-up needs the grid it looks up
        r = subprocess.run(base + ["--probe-quad", "0"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-quad" in r.stderr and "--probe-grid" in r.stderr, (extra, r.stderr)
    for alone in (["--probe-side", "-1"], ["--probe-facing"]):
        r = subprocess.run(base + grid + box + alone, capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-quad" in r.stderr and alone[0] in r.stderr, (alone, r.stderr)
    r = subprocess.run(base + grid + box + ["--probe-quad", "0", "--probe-side", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--probe-side" in r.stderr, r.stderr
    for index in ("11", "999", "-1"):  # cornell_box has 11 quads; worded as --bake-quad words it
        r = subprocess.run(base + grid + box + ["--probe-quad", index], capture_output=True, text=True)
        assert r.returncode == 2 and f"--probe-quad {index}: the scene has 11 quads" in r.stderr, (index, r.stderr)
    for index in ("11", "999"):
        r = subprocess.run(base + grid + box + ["--probe-quad", index], capture_output=True, text=True)
        b = subprocess.run(base + ["--bake-quad", index], capture_output=True, text=True)
        assert b.returncode == 2 and b.stderr == r.stderr.replace("--probe-quad", "--bake-quad"), (index, b.stderr, r.stderr)
    for other in (["--lens", "ortho"], ["--bake-quad", "0"], ["--views", "2"], ["--adaptive", "0.05"]):  # as --probe-grid alone refuses them
        r = subprocess.run(base + grid + box + ["--probe-quad", "0"] + other, capture_output=True, text=True)
        assert r.returncode == 2 and "--probe-grid" in r.stderr and other[0] in r.stderr, (other, r.returncode, r.stderr)
