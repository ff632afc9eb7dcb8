"""Lit bakes on the GPU (include/hrt.h "Lit bakes"), every comparison but the furnace on bits: (A) the fused bake is the fold of
hrt_bake_rays and hrt_trace_lit[_paths] over its samples, for every tail, look-up, bias and with keys, degenerate points giving exact
zeros; (B) the same under the proof builds; (C) running sums and a sentinel row; (D) lanes take further points by grid stride; (E) the
blocking form is the device form and fills its stats; (F) the furnace: a final gather against a relit volume follows the geometric
series; (G) the refusals that need a volume, in "Lit rays"' order; (H) repeated calls leave no device buffer behind; (I) the
command-line tool writes the bytes the library computes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import probe_lit_ref as pl
import test_gpu_lit_frames as tf
import test_gpu_live_resources as tlr
import test_gpu_probe_lit as tl
import test_gpu_rays as qr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT, BRUTE, NO_LDS, ACCUMULATE = 64, 128, 2, 512
HRT_ERR_INVALID = -1
NAN, INF = float("nan"), float("inf")
FACING, VISIBLE = tl.FACING, tl.VISIBLE
SCENES = tf.SCENES  # cornell_mesh, random_spheres
TAILS = (None, 1, 2, 6)
FIRST, S, SEED = 3, 5, 11
bits = qr.bits
on_gpu = tl.on_gpu

_points = {}


def points(gpu, name):
    """(records, degenerate mask) of a scene, made once: the 9 x 7 texel centres of one wall (the scene's first quad; a hand-made
    quad inside the probe box where the scene has none), the vertices of a small hand-made mesh in the middle of the box with their
    unnormalised area-weighted normals (its last vertex is used by no triangle: N = 0), and one point each with N = 0, a NaN
    coordinate and a negative record bias."""
    if name not in _points:
        lo, hi = (np.array(v, F32) for v in tl.TAIL_SCENES[name])
        quads = gpu.scene_quads(gpu.HostScene().setup(name, tf.W / tf.H, 1).flatten())
        mid, ext = (lo + hi) / 2, (hi - lo)
        quad = quads[0] if quads else gpu.Quad.make(mid - 0.3 * ext, mid + np.array([0.3, -0.3, -0.3], F32) * ext, mid + np.array([-0.3, -0.3, 0.3], F32) * ext)
        wall = gpu.quad_points(quad, 9, 7, 1, 0.0, 1e-4)
        pos = (mid + 0.2 * ext * np.array([[-1, -1, -1], [1, -1, -1], [1, -1, 1], [-1, -1, 1], [0, 1, 0], [0.5, 0.5, 0.5]], F32)).astype(F32)
        tri = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], U32)
        mesh = gpu.mesh_points(pos, tri, 0.0, 1e-3)
        odd = np.zeros((3, 8), F32)
        odd[:, 0:3] = mid
        odd[:, 4:7] = (0.0, 1.0, 0.0)
        odd[0, 4:7] = 0.0          # N = 0
        odd[1, 1] = NAN            # a NaN coordinate
        odd[2, 7] = -1e-3          # a negative record bias
        pts = np.ascontiguousarray(np.concatenate([wall, mesh, odd]), F32)
        deg = np.zeros(len(pts), bool)
        deg[len(wall) + 5] = True  # the unused vertex
        deg[-3:] = True
        _points[name] = (pts, deg)
    return _points[name]


def keys_for(n):
    return (np.arange(n, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(U32)


def folded(gpu, dev, vol, d_pts, d_keys, first, n, seed=SEED, flags=0, **lit):
    """The running sums of the composition: per sample hrt_bake_rays, then hrt_trace_lit[_paths] of one sample, accumulated."""
    import torch
    acc = torch.zeros((d_pts.shape[0], 3), dtype=torch.float32, device="cuda")
    for s in range(first, first + n):
        dev.trace_lit(gpu.bake_rays(d_pts, s, seed, d_keys), vol, 1, first_sample=s, seed=seed, keys=d_keys, out=acc, accumulate=True, flags=flags, **lit)
    return acc.cpu().numpy()


# ------------------------------------------------------------------------------------ A. the fused bake is the fold of the query
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("name", SCENES)
def test_the_fused_bake_is_the_fold_of_bake_rays_and_lit_rays(gpu, name, tail):
    dev, cam, vol, _ = tf.case(gpu, name)
    pts, deg = points(gpu, name)
    d_pts = on_gpu(pts)
    for keys in (None, keys_for(len(pts))):
        d_keys = None if keys is None else on_gpu(keys)
        for ef in tl.EVAL_FLAGS:
            for bias in (0.0, 1e-3):
                what = (name, tail, keys is not None, ef, bias)
                want = folded(gpu, dev, vol, d_pts, d_keys, FIRST, S, eval_flags=ef, bias=bias, tail_after=tail) / F32(S)
                got = dev.bake_lit(d_pts, vol, S, first_sample=FIRST, seed=SEED, keys=d_keys, eval_flags=ef, bias=bias, tail_after=tail).cpu().numpy()
                assert np.isfinite(want).all() and want[~deg].any(), what
                assert got.shape == (len(pts), 3) and np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).any(axis=1).sum()))
                assert (bits(got[deg]) == 0).all(), (what, "a degenerate point gives exact zeros")


def test_the_look_up_bias_is_not_the_records_bias(gpu):
    """The record's bias moves the ray's origin, the call's bias the look-up at the hit: each changes the result on its own (in
    cornell_mesh, whose walls the volume's box encloses: the visible look-up's bias matters only between its probes)."""
    name = "cornell_mesh"
    dev, cam, vol, _ = tf.case(gpu, name)
    pts, deg = points(gpu, name)
    moved = pts.copy()
    moved[~deg, 7] = 5e-2
    base = dev.bake_lit(on_gpu(pts), vol, 2, seed=SEED, eval_flags=VISIBLE).cpu().numpy()
    by_record = dev.bake_lit(on_gpu(moved), vol, 2, seed=SEED, eval_flags=VISIBLE).cpu().numpy()
    by_lookup = dev.bake_lit(on_gpu(pts), vol, 2, seed=SEED, eval_flags=VISIBLE, bias=5e-2).cpu().numpy()
    assert not np.array_equal(bits(base), bits(by_record)) and not np.array_equal(bits(base), bits(by_lookup))
    assert not np.array_equal(bits(by_record), bits(by_lookup))


# ------------------------------------------------------------------------------------------------------------ B. proof builds
@pytest.mark.parametrize("flags", (EXACT, EXACT | BRUTE, NO_LDS))
@pytest.mark.parametrize("name", SCENES)
def test_the_fold_holds_under_the_proof_builds(gpu, name, flags):
    dev, cam, vol, _ = tf.case(gpu, name)
    pts, deg = points(gpu, name)
    d_pts = on_gpu(pts)
    for tail in (None, 2):
        want = folded(gpu, dev, vol, d_pts, None, FIRST, S, flags=flags, eval_flags=FACING, tail_after=tail) / F32(S)
        got = dev.bake_lit(d_pts, vol, S, first_sample=FIRST, seed=SEED, flags=flags, eval_flags=FACING, tail_after=tail).cpu().numpy()
        assert want[~deg].any() and np.array_equal(bits(got), bits(want)), (name, flags, tail)


# ------------------------------------------------------------------------------------------------------------ C. running sums
@pytest.mark.parametrize("tail", (None, 2))
def test_running_sums_and_a_sentinel_row(gpu, tail):
    import torch
    dev, cam, vol, _ = tf.case(gpu, "cornell_mesh")
    pts, deg = points(gpu, "cornell_mesh")
    n = len(pts)
    d_pts = on_gpu(pts)
    sums = folded(gpu, dev, vol, d_pts, None, 0, 5, tail_after=tail)
    big = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda")  # a sentinel row past n
    acc = big[:n]
    acc.zero_()
    acc[torch.from_numpy(deg).to("cuda")] = 9.0  # the sums of a degenerate point are left as they are
    assert dev.bake_lit(d_pts, vol, 2, first_sample=0, seed=SEED, out=acc, accumulate=True, tail_after=tail) is acc
    dev.bake_lit(d_pts, vol, 3, first_sample=2, seed=SEED, out=acc, accumulate=True, tail_after=tail)
    got = big.cpu().numpy()
    assert np.array_equal(bits(got[:n][~deg]), bits(sums[~deg])), "2 + 3 samples accumulated are the 5 sums"
    assert (got[:n][deg] == 9.0).all() and (got[n] == -7.0).all(), "a degenerate point's sums and the row past n stay untouched"
    once = dev.bake_lit(d_pts, vol, 5, seed=SEED, accumulate=True, tail_after=tail).cpu().numpy()
    assert np.array_equal(bits(once), bits(sums)), "one accumulate call of 5 from zeros"
    assert np.array_equal(bits(dev.bake_lit(d_pts, vol, 5, seed=SEED, tail_after=tail).cpu().numpy()), bits(sums / F32(5)))


# --------------------------------------------------------------------------------------------------------- D. beyond one grid
@pytest.mark.parametrize("tail", (None, 1))
def test_lanes_take_further_points_by_grid_stride(gpu, tail):
    import torch
    dev, cam, vol, _ = tf.case(gpu, "random_spheres")
    pts, _ = points(gpu, "random_spheres")
    m = len(pts)
    # A launch is the workgroups that can be resident at once: at most 8 waves on each of a compute unit's 4 SIMDs.
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4 * 64
    n = resident + 2 * m + 1
    idx = (torch.arange(n, device="cuda") * 7) % m
    many, keys = on_gpu(pts)[idx].contiguous(), (torch.arange(n, device="cuda") % 1000).to(torch.int32)
    got = dev.bake_lit(many, vol, 1, seed=4, keys=keys, tail_after=tail)
    half = n // 2
    a = dev.bake_lit(many[:half].contiguous(), vol, 1, seed=4, keys=keys[:half].contiguous(), tail_after=tail)
    b = dev.bake_lit(many[half:].contiguous(), vol, 1, seed=4, keys=keys[half:].contiguous(), tail_after=tail)
    assert half < resident < n and got.any()
    assert torch.equal(got.view(torch.int32), torch.cat([a, b]).view(torch.int32))


# ------------------------------------------------------------------------------------------------------- E. the blocking form
def test_the_blocking_form_is_the_device_form_and_fills_its_stats(gpu):
    dev, cam, vol, _ = tf.case(gpu, "cornell_mesh")
    pts, deg = points(gpu, "cornell_mesh")
    keys = keys_for(len(pts))
    for tail in (None, 1):
        st = gpu.Stats()
        got = dev.bake_lit(pts, vol, 3, seed=SEED, keys=keys, stats=st, eval_flags=FACING, tail_after=tail)
        assert isinstance(got, np.ndarray) and got.shape == (len(pts), 3) and st.samples == len(pts) * 3 and st.kernel_ms > 0
        want = dev.bake_lit(on_gpu(pts), vol, 3, seed=SEED, keys=on_gpu(keys), eval_flags=FACING, tail_after=tail).cpu().numpy()
        assert want[~deg].any() and np.array_equal(bits(got), bits(want)), tail
        later = dev.bake_lit(pts, vol, 2, first_sample=3, seed=SEED, tail_after=tail)  # NumPy through the device form
        assert np.array_equal(bits(later), bits(dev.bake_lit(on_gpu(pts), vol, 2, first_sample=3, seed=SEED, tail_after=tail).cpu().numpy()))
    empty = dev.bake_lit(np.zeros((0, 8), F32), vol, 3)
    assert empty.shape == (0, 3)
    lib = gpu.device_lib()
    rc = lib.hrt_bake_lit(dev._h, vol._h, pts.ctypes.data, None, len(pts), 1, 1, ACCUMULATE, 0, 0.0, 0, C.c_void_p(0x2000), None)
    assert rc == HRT_ERR_INVALID and "hrt_bake_lit: flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device" in lib.hrt_last_error().decode()


# ----------------------------------------------------------------------------------------------------------------- F. the furnace
def test_a_final_gather_in_the_furnace_follows_the_geometric_series(gpu):
    """A closed diffuse room of albedo rho that emits e, a 2^3 volume relit 7 rounds at 4096 samples: every sample of a lit bake is
    e / 6 + rho x G exactly (the first hit emits e, nothing else is lit directly), so the lightmap is round 8 of the series and the
    only error is the volume's G.  tests/test_gpu_probe_lit.py (test_the_furnace_relit_round_by_round_is_the_geometric_series) bounds
    the relative error of exactly that G at 5 %; here it enters times rho next to the exact e / 6, so the bound on the lightmap is
    rho x 5 % of the series' value, at every texel.  The deviation is printed."""
    rho, e, N = 0.5, 6.0, 4096
    dev = tl.furnace_scene(gpu, rho, e)
    box, counts = ((-1, -1, -1), (1, 1, 1)), (2, 2, 2)
    wall = gpu.Quad.make((-1.0, -1.1, -1.1), (-1.0, 1.1, -1.1), (-1.0, -1.1, 1.1))  # x = -1, its lit side faces +x
    pts = gpu.quad_points(wall, 5, 5, 1, 0.0, 1e-4)
    want = pl.furnace(e, rho, 8)
    with gpu.ProbeVolume(*box, *counts) as vol:
        vol.relight(dev, N, 7)
        for tail in (None, 1):
            got = dev.bake_lit(pts, vol, 256, seed=3, tail_after=tail).astype(np.float64)
            d = (got - want) / want
            print(f"tail_after {tail}: deviation from the series' 8th term {d.min():+.5f} .. {d.max():+.5f} (series {want:.5f})")
            assert got.shape == (25, 3) and np.abs(d).max() <= 0.05 * rho, (tail, float(np.abs(d).max()))
    dev.close()


# ------------------------------------------------------------------------------------------- G. refusals that need a volume
def test_the_refusals_that_need_a_volume_come_in_the_order_of_lit_rays(gpu):
    lib = gpu.device_lib()
    PTS, OUT = 0x1000, 0x2000

    def call(entry, v, ef=0, bias=0.0, tail=0):
        if entry == "hrt_bake_lit_device":
            rc = lib.hrt_bake_lit_device(None, v._h, C.c_void_p(PTS), None, 5, 0, 1, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        else:
            rc = lib.hrt_bake_lit(None, v._h, C.c_void_p(PTS), None, 5, 1, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        return rc, lib.hrt_last_error().decode()

    for entry in ("hrt_bake_lit_device", "hrt_bake_lit"):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as v:
            for tail in (0, 2):
                assert call(entry, v, ef=1 | VISIBLE, bias=NAN, tail=tail)[1].startswith(entry + ": eval_flags: HRT_PROBE_EVAL_RADIANCE"), "by name, first"
                assert call(entry, v, ef=8 | VISIBLE, bias=NAN, tail=tail) == (HRT_ERR_INVALID, entry + ": eval_flags: unknown bits 8")
                assert call(entry, v, ef=VISIBLE, bias=NAN, tail=tail) == (HRT_ERR_INVALID, entry + ": the volume has no coefficients yet (hrt_probe_volume_update)")
            v.update(np.zeros((2, 9, 3), F32))
            for tail in (0, 2):
                assert call(entry, v, ef=VISIBLE | FACING, bias=NAN, tail=tail) == \
                    (HRT_ERR_INVALID, entry + ": eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet (hrt_probe_volume_update_depth)")
                for bad in (NAN, INF, -INF):
                    assert call(entry, v, ef=FACING, bias=bad, tail=tail)[1].startswith(entry + ": bias must be finite"), bad
                assert call(entry, v, ef=FACING, tail=tail) == (HRT_ERR_INVALID, entry + ": scene is NULL")
            v.update_depth(np.zeros((2, 64, 3), F32))
            assert call(entry, v, ef=VISIBLE, bias=NAN)[1].startswith(entry + ": bias must be finite")
            assert call(entry, v, ef=VISIBLE) == (HRT_ERR_INVALID, entry + ": scene is NULL")
            assert call(entry, v, ef=VISIBLE, tail=7)[1].startswith(entry + ": tail_after must be in 1 .. HRT_MAXBOUNCES"), "tail_after before the volume"
        closed = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1)
        closed.close()
        assert call(entry, closed) == (HRT_ERR_INVALID, entry + ": volume is NULL"), "a closed volume has no handle"
    dev, cam, vol, _ = tf.case(gpu, "cornell_mesh")
    pts, _ = points(gpu, "cornell_mesh")
    with pytest.raises(gpu.HrtError, match="hrt_bake_lit_device: eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet"):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as v:
            dev.bake_lit(on_gpu(pts), v.update(np.zeros((2, 9, 3), F32)), 1, eval_flags=VISIBLE)
    closed = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1)
    closed.close()
    for p in (pts, on_gpu(pts)):
        with pytest.raises(gpu.HrtError, match="volume is NULL"):
            dev.bake_lit(p, closed)


# ------------------------------------------------------------------------------------------------------------ H. resources
def test_repeated_calls_leave_no_device_buffers_behind(gpu):
    import torch
    torch.cuda.synchronize()
    see = tlr.Peak(gpu)
    before = see()
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", tf.W, tf.H)
    vol = tl.zero_volume(gpu, tl.TAIL_SCENES["cornell_mesh"])
    pts, _ = points(gpu, "cornell_mesh")
    d_pts = on_gpu(pts)
    out = torch.zeros((len(pts), 3), dtype=torch.float32, device="cuda")

    def round_():
        for tail in (None, 2):
            dev.bake_lit(pts, vol, 2, tail_after=tail)
            dev.bake_lit(pts, vol, 2, keys=keys_for(len(pts)), tail_after=tail)
            dev.bake_lit(d_pts, vol, 2, out=out, tail_after=tail)
        torch.cuda.synchronize()
        return see()

    held = round_()
    for _ in range(3):
        assert round_() == held, "repeated calls leave hrt_debug_live_resources where the first left it"
    peak = see.peak
    round_()
    assert see.peak == peak, "a further round peaks where the earlier ones did"
    vol.close()
    dev.close()
    assert gpu.live_resources() == before


# ------------------------------------------------------------------------------------------------------------------ I. the CLI
def cli(tmp_path, extra, spp, out="out.ppm"):
    path = tmp_path / out
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8",
                        "--bake-quad", "0", "--spp", str(spp), "--out", str(path)] + extra, capture_output=True, text=True)
    return r, path


GRID = ["--probe-grid", "2,2,1", "--probe-box", "-1.0,-1.0,-1.0,1.0,1.0,1.0"]


@pytest.mark.parametrize("extra", ([], ["--probe-tail", "2", "--probe-facing"], ["--probe-bounces", "2", "--probe-visible", "--probe-rmax", "1.25"]))
def test_the_cli_writes_the_lightmap_the_library_computes(gpu, tmp_path, extra):
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 65, (2, 2, 1)
    r, path = cli(tmp_path, GRID + ["--bake-lit"] + extra, spp)
    assert r.returncode == 0, r.stdout + r.stderr
    _, desc, dev, _ = qr.build(gpu, "cornell_box", 8, 8)
    pts = gpu.quad_points(gpu.scene_quads(desc)[0], 8, 8, 1, 0.0, 1e-4)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        if "--probe-bounces" in extra:
            vol.relight(dev, spp, 2, eval_flags=VISIBLE, depth_rmax=1.25)
            lightmap = dev.bake_lit(pts, vol, spp, seed=1, eval_flags=VISIBLE)
        else:
            vol.update(dev.probes(gpu.probe_grid(lo, hi, *counts), spp, seed=1))  # without --probe-bounces the grid is path-traced
            lightmap = dev.bake_lit(pts, vol, spp, seed=1, eval_flags=FACING if extra else 0, tail_after=2 if extra else None)
    assert np.isfinite(lightmap).all() and lightmap.any()
    mine = tmp_path / "mine.ppm"
    gpu.write_ppm(str(mine), lightmap.reshape(8, 8, 3))
    assert path.read_bytes() == mine.read_bytes()
    plain, ppath = cli(tmp_path, [], spp, "plain.ppm")  # --bake-quad alone still writes what it wrote
    assert plain.returncode == 0, plain.stdout + plain.stderr
    gpu.write_ppm(str(mine), dev.bake(pts, spp, seed=1).reshape(8, 8, 3))
    assert ppath.read_bytes() == mine.read_bytes() and ppath.read_bytes() != path.read_bytes()
    dev.close()


def test_the_cli_refuses_half_a_lit_bake_as_it_refused_before(gpu, tmp_path):
    r, _ = cli(tmp_path, GRID, 4)  # --probe-grid with --bake-quad, without --bake-lit: as before
    assert r.returncode == 2 and "--probe-grid traces light probes on one GPU: it cannot be combined with --bake-quad" in r.stderr
    r, _ = cli(tmp_path, ["--bake-lit"], 4)
    assert r.returncode == 2 and r.stderr.startswith("--bake-lit bakes a lightmap whose paths end in a probe grid: give")
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--bake-lit"] + GRID, capture_output=True, text=True)
    assert r.returncode == 2 and r.stderr.startswith("--bake-lit bakes a lightmap whose paths end in a probe grid: give")
