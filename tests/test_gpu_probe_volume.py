"""Probe volumes on the GPU (include/hrt.h "Probe volumes").  Every comparison but the statistical one is on bits.

1. the rule: hrt_probe_eval_device equals tests/probe_volume_ref.py bit for bit over grids, flag combinations, batch sizes and point
   kinds -- for libhrt.so and for the A/B build with the other mapping of points to lanes (libhrt_var_probe_eval.so, Makefile);
2. plumbing: update from a traced grid and eval on a non-default torch stream, `out=`, the NumPy path and its stats, a second
   update, coefficients with NaN neighbours; and the refusals that need a real volume, in the header's order;
3. units, end to end: a traced 1 x 1 x 1 volume over the square emitter of tests/test_gpu_probes.py against the SH9 reconstruction
   from the emitter's analytic coefficients;
4. resources: create / update / evaluate / destroy leave hrt_debug_live_resources where it was;
5. the command-line tool writes the file the Python composition gives."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import probe_volume_ref as pv
import probe_volume_run as run
import test_gpu_rays as qr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
HRT_ERR_INVALID = -1
bits = qr.bits


def on_gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
@pytest.fixture(scope="module")
def want():
    """The NumPy rule over the whole matrix, once: {grid: {(radiance, facing): (1000, 3)}}."""
    out = {}
    for name, (box, counts, coeffs, pts) in run.matrix().items():
        out[name] = {f: pv.evaluate(*box, counts, coeffs, pts, *f) for f in run.FLAGS}
        for f, w in out[name].items():
            assert np.isfinite(w).all() and w.any(), (name, f)
    return out


@pytest.fixture(scope="module")
def shipped(gpu):
    return run.run(gpu)


@pytest.fixture(scope="module")
def ab_build(gpu, tmp_path_factory):
    """The same matrix from a process of its own that loads the A/B library."""
    path = str(tmp_path_factory.mktemp("probe_volume") / "ab.npz")
    env = dict(os.environ, HRT_LIBNAME="libhrt_var_probe_eval.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "probe_volume_run.py"), path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "libhrt_var_probe_eval.so" in r.stdout, r.stdout + r.stderr
    return dict(np.load(path))


def check_matrix(got, want, who):
    seen = 0
    for name, by_flags in want.items():
        for (radiance, facing), w in by_flags.items():
            for n in run.BATCHES:
                g = got[f"{name}__{int(radiance)}{int(facing)}__{n}"]
                assert g.shape == (n, 3) and g.dtype == F32
                bad = np.flatnonzero((bits(g) != bits(w[:n])).any(axis=1))
                assert bad.size == 0, (who, name, radiance, facing, n, bad[:8].tolist(), g[bad[:2]].tolist(), w[bad[:2]].tolist())
                seen += 1
    assert seen == 4 * 4 * len(run.BATCHES) == len(got)


def test_eval_is_the_numpy_rule_bit_for_bit(shipped, want):
    check_matrix(shipped, want, "libhrt.so")


def test_the_other_mapping_of_points_to_lanes_gives_the_same_bits(ab_build, want):
    check_matrix(ab_build, want, "libhrt_var_probe_eval.so")


def test_the_matrix_holds_every_kind_of_point():
    import test_probe_volume_abi as abi
    for name, (box, counts, coeffs, pts) in run.matrix().items():
        _, deg = pv.normals(pts)
        lo, hi = np.minimum(*np.asarray(box, F32)), np.maximum(*np.asarray(box, F32))
        outside = ((pts[:, 0:3] < lo) | (pts[:, 0:3] > hi)).any(axis=1)
        assert deg[:63].any() and (~deg[:7]).any() and outside[:63].any() and (np.abs(pts[:, 0:3]) >= 1e18).any() and (coeffs < 0).any(), name
        i0, i1, f = pv.cell(*box, counts, pts[~deg])
        assert len(pts) == 1000 and ((f == 0).any() and (f > 0).any() or max(counts) == 1)


# ----------------------------------------------------------------------------------------------------------------- 2. plumbing
CORNELL_BOX = ((-1.6, -0.4, -1.2), (1.6, 1.6, 1.6))  # probe_ref.BOXES["cornell_mesh"]
FLOOR = 8  # of the flattened scene's quads: the one in the plane y = -2


@pytest.fixture(scope="module")
def cornell(gpu):
    host, desc, dev, cam = qr.build(gpu, "cornell_mesh", 19, 11)
    floor = gpu.scene_quads(desc)[FLOOR]
    assert abs(floor.v0[1] + 2) < 1e-5 and abs(floor.v1[1] + 2) < 1e-5 and abs(floor.v3[1] + 2) < 1e-5
    pts = gpu.quad_points(floor, 8, 8)
    return host, desc, dev, pts


def test_update_from_a_traced_grid_and_eval_on_a_second_stream(gpu, cornell):
    import torch
    _, _, dev, pts = cornell
    counts = (3, 2, 2)
    grid = gpu.probe_grid(*CORNELL_BOX, *counts)
    stream = torch.cuda.Stream()
    with gpu.ProbeVolume(*CORNELL_BOX, *counts) as vol, torch.cuda.stream(stream):
        d_pts = on_gpu(pts)
        coeffs = dev.probes(on_gpu(grid), spp=64)
        assert vol.update(coeffs) is vol
        got = vol.eval(d_pts)
        out = torch.empty((len(pts), 3), dtype=torch.float32, device="cuda")
        assert vol.eval(d_pts, facing=True, out=out) is out
        stream.synchronize()
        h_coeffs = coeffs.cpu().numpy()
        assert h_coeffs.shape == (12, 9, 3) and h_coeffs.any()
        want = pv.evaluate(*CORNELL_BOX, counts, h_coeffs, pts)
        assert want.any() and np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert np.array_equal(bits(out.cpu().numpy()), bits(pv.evaluate(*CORNELL_BOX, counts, h_coeffs, pts, facing=True)))
        # the NumPy path: blocking, with stats
        st = gpu.Stats()
        host = vol.eval(pts, stats=st)
        assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(want))
        assert st.samples == len(pts) and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
        mine = np.zeros((len(pts), 3), F32)
        assert vol.eval(pts, radiance=True, out=mine) is mine and np.array_equal(bits(mine), bits(pv.evaluate(*CORNELL_BOX, counts, h_coeffs, pts, radiance=True)))
        assert vol.eval(np.zeros((0, 8), F32)).shape == (0, 3) and vol.eval(on_gpu(np.zeros((0, 8), F32))).shape == (0, 3)
        # a second update, from the host this time
        other = np.random.default_rng(3).standard_normal((12, 9, 3)).astype(F32)
        vol.update(other)
        want2 = pv.evaluate(*CORNELL_BOX, counts, other, pts)
        got2 = vol.eval(d_pts)
        stream.synchronize()
        assert np.array_equal(bits(got2.cpu().numpy()), bits(want2)) and not np.array_equal(bits(want2), bits(want))
        # the five floats of padding in a record are zeros, not the next probe's or whatever lies round the caller's buffer
        big = torch.full((12 + 8, 9, 3), float("nan"), dtype=torch.float32, device="cuda")
        big[4:16] = on_gpu(other)
        vol.update(big[4:16])
        got3 = vol.eval(d_pts)
        stream.synchronize()
        assert np.array_equal(bits(got3.cpu().numpy()), bits(want2))
        with pytest.raises(ValueError, match="the volume has 12 probes"):
            vol.update(big)
        with pytest.raises(ValueError, match="out must be a contiguous"):
            vol.eval(d_pts, out=torch.empty((len(pts), 4), device="cuda"))


def test_the_refusals_that_need_a_volume_come_in_the_headers_order(gpu):
    dev = gpu.device_lib()
    PTS, OUT = 0x1000, 0x2000
    with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as vol:
        for entry, pn, on, offs in (("hrt_probe_eval_device", "d_points", "d_out", (4, 8)), ("hrt_probe_eval", "points", "out", (1, 2))):
            def call(pts=PTS, n=5, flags=0, out=OUT):
                args = (vol._h, C.c_void_p(pts), n, flags, C.c_void_p(out), None)
                return getattr(dev, entry)(*args), dev.hrt_last_error().decode()
            wrong = dict(pts=PTS + offs[0], n=2 ** 31, out=0)
            rc, msg = call(**wrong)
            assert rc == HRT_ERR_INVALID and msg == entry + ": the volume has no coefficients yet (hrt_probe_volume_update)", msg
            assert "flags" in call(flags=8, **wrong)[1]
        vol.update(np.zeros((2, 9, 3), F32))
        for entry, pn, on, offs in (("hrt_probe_eval_device", "d_points", "d_out", (4, 8)), ("hrt_probe_eval", "points", "out", (1, 2))):
            def call(pts=PTS, n=5, flags=0, out=OUT):
                args = (vol._h, C.c_void_p(pts), n, flags, C.c_void_p(out), None)
                return getattr(dev, entry)(*args), dev.hrt_last_error().decode()
            wrong = dict(pts=0, n=2 ** 31, out=0)
            assert call(**wrong) == (HRT_ERR_INVALID, f"{entry}: {pn} is NULL")
            for off in offs:
                wrong["pts"] = PTS + off
                rc, msg = call(**wrong)
                assert rc == HRT_ERR_INVALID and msg.startswith(f"{entry}: {pn} is not ") and "-byte aligned" in msg, msg
            wrong["pts"] = PTS
            rc, msg = call(**wrong)
            assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": n must be at most 2^31 - 1") and str(2 ** 31) in msg, msg
            wrong["n"] = 2 ** 31 - 1
            assert call(**wrong) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")
            wrong["out"] = OUT + 2
            assert call(**wrong) == (HRT_ERR_INVALID, f"{entry}: {on} is not 4-byte aligned")
        for entry, name, args in (("hrt_probe_volume_update_device", "d_coeffs", (None,)), ("hrt_probe_volume_update", "coeffs", ())):
            assert getattr(dev, entry)(vol._h, None, *args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == f"{entry}: {name} is NULL"
            assert getattr(dev, entry)(vol._h, C.c_void_p(PTS + 2), *args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == f"{entry}: {name} is not 4-byte aligned"


# -------------------------------------------------------------------------------------------------------------------- 3. units
def emitter_coefficients():
    """(1 / 4 pi) x the integral of Y_k over the solid angle of the 2 x 2 quad in the plane z = 0, seen from (0, 0, 1), in fp64:
    Gauss-Legendre over the quad with d omega = dx dy / r^3.  The integrand is smooth (r >= 1), so 64 x 64 nodes are exact to
    rounding; bands 0 and 1 are held to the closed forms of tests/test_gpu_probes.py below."""
    t, wt = np.polynomial.legendre.leggauss(64)
    x, y = np.meshgrid(t, t, indexing="ij")
    w = np.outer(wt, wt)
    r = np.sqrt(x * x + y * y + 1)
    dx, dy, dz = x / r, y / r, -1 / r
    dw = w / r ** 3
    k = [np.sqrt(1 / (4 * np.pi)), np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi)), np.sqrt(5 / (16 * np.pi)), np.sqrt(15 / (16 * np.pi))]
    Y = [k[0] + 0 * x, k[1] * dy, k[1] * dz, k[1] * dx, k[2] * dx * dy, k[2] * dy * dz, k[3] * (3 * dz * dz - 1), k[2] * dx * dz, k[4] * (dx * dx - dy * dy)]
    return np.array([(f * dw).sum() for f in Y]) / (4 * np.pi), k


def basis64(n, k):
    x, y, z = n
    return np.array([k[0], k[1] * y, k[1] * z, k[1] * x, k[2] * x * y, k[2] * y * z, k[3] * (3 * z * z - 1), k[2] * x * z, k[4] * (x * x - y * y)])


def test_a_traced_volume_reconstructs_the_square_emitter(gpu):
    """The scene and the statistics of test_coefficients_over_a_square_emitter_are_the_analytic_ones (tests/test_gpu_probes.py): a
    2 x 2 emitter in z = 0 lit towards +z, a dark sky, the probe at (0, 0, 1); a sample returns Le / 6 where its direction hits
    (p = 1/6) and 0 elsewhere, n = 4096 samples.  That test bounds the error of the traced mean of `hit` by 5 sqrt(p (1 - p) / n)
    and of `q hit` for a polynomial |q| <= 1 (x, y, z there) by 5 sqrt(p / n), since the variance of q hit is at most E[hit] = p.
    The band-2 polynomials obey the same bound: |xy|, |yz|, |xz| <= 1/2 and |x^2 - y^2| <= 1 on the sphere; |3 z^2 - 1| <= 2, so its
    standard error is at most 2 sqrt(p / n).  A coefficient is constant_k x Le/6 x such a mean, and the radiance-mode output is
    sum_k 4 pi c_k Y_k(N): its error is at most sum_k 4 pi |Y_k(N)| constant_k (Le/6) 5 se_k, which is the tolerance below.  fp32
    rounding (1e-6 relative) is far below it."""
    n, seed, key = 4096, 7, 0
    p = 1 / 6
    se0, se1 = np.sqrt(p * (1 - p) / n), np.sqrt(p / n)
    s = gpu.HostScene()
    s.set_sky(True)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0,
               gpu.Material.make(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=6.0))
    dev = gpu.DeviceScene(s.flatten())
    rec = dev.trace_rays(qr.make_rays([(0.0, 0.0, 1.0)], [(0.0, 0.0, -1.0)]), "shade")
    assert bits(rec)[0, gpu.HIT_KIND] == gpu.KIND_SQUARE
    Le = rec[0, gpu.SHADE_EMISSION].astype(np.float64)
    assert (Le > 0).all()
    c, k = emitter_coefficients()
    F = 2 * (2 / np.pi) * (1 / np.sqrt(2)) * np.arctan(1 / np.sqrt(2))
    assert abs(c[0] - k[0] * p) < 1e-12 and abs(c[2] + k[1] * F / 4) < 1e-12 and np.abs(c[[1, 3, 4, 5, 7, 8]]).max() < 1e-15  # that test's closed forms
    box = ((-1, -1, 0), (1, 1, 2))  # one probe, at the centre (0, 0, 1)
    grid = gpu.probe_grid(*box, 1, 1, 1)
    assert grid[0].tolist() == [0, 0, 1, 0]
    coeffs = dev.probes(grid, n, seed=seed, keys=np.array([key], U32))
    const = np.array([k[0], k[1], k[1], k[1], k[2], k[2], k[3], k[2], k[4]])
    se = np.array([se0, se1, se1, se1, se1, se1, 2 * se1, se1, se1])
    normals = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    pts = np.zeros((6, 8), F32)
    pts[:, 0:3], pts[:, 4:7] = (0.3, -0.2, 5.0), normals  # anywhere: one probe serves every point
    with gpu.ProbeVolume(*box, 1, 1, 1) as vol:
        got = vol.update(coeffs).eval(pts, radiance=True).astype(np.float64)
    for i, nrm in enumerate(normals.astype(np.float64)):
        Y = basis64(nrm, k)
        want = 4 * np.pi * (c * Y).sum() * Le / 6
        tol = (4 * np.pi * np.abs(Y) * const * 5 * se).sum() * Le / 6
        print(f"N = {nrm.tolist()}: got {got[i].tolist()}, want {want.tolist()}, tolerance {tol.tolist()}")
        assert (np.abs(got[i] - want) <= tol).all(), (nrm.tolist(), got[i].tolist(), want.tolist(), tol.tolist())
    # the reconstruction looks at the emitter: brighter towards -z than towards +z by more than both tolerances
    assert (got[5] > got[4]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. resources
def test_a_volume_gives_back_what_it_took(gpu):
    import torch
    torch.cuda.synchronize()
    before = gpu.live_resources()
    vol = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 4, 4, 4)
    assert gpu.live_resources()[0] == before[0] + 1
    vol.update(np.ones((64, 9, 3), F32))
    pts = np.zeros((10, 8), F32)
    pts[:, 6] = 1
    assert np.isfinite(vol.eval(pts)).all() and vol.eval(on_gpu(pts)).shape == (10, 3)
    vol.close()
    vol.close()  # twice is fine
    assert gpu.live_resources() == before
    gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 2, 2).close()  # never updated
    assert gpu.live_resources() == before


# ---------------------------------------------------------------------------------------------------------------------- 5. CLI
@pytest.mark.parametrize("facing", [False, True])
def test_the_cli_writes_the_lightmap_the_library_computes(gpu, tmp_path, facing):
    lo, hi, spp = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 65
    path, mine = tmp_path / "probe_map.ppm", tmp_path / "mine.ppm"
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8",
                        "--probe-grid", "2,2,1", "--probe-box", ",".join(str(x) for x in lo + hi), "--probe-quad", "0", "--spp", str(spp),
                        "--out", str(path)] + (["--probe-facing"] if facing else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    _, desc, dev, _ = qr.build(gpu, "cornell_box", 8, 8)
    coeffs = dev.probes(gpu.probe_grid(lo, hi, 2, 2, 1), spp)  # the tool's seed is the library's default
    pts = gpu.quad_points(gpu.scene_quads(desc)[0], 8, 8, 1, 0.0, 0.0)
    with gpu.ProbeVolume(lo, hi, 2, 2, 1) as vol:
        lightmap = vol.update(coeffs).eval(pts, facing=facing)
    assert lightmap.any()
    gpu.write_ppm(str(mine), lightmap.reshape(8, 8, 3))
    assert path.read_bytes() == mine.read_bytes()
