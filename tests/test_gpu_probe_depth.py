"""Probe visibility on the GPU (include/hrt.h "Probe visibility").  Every comparison but the analytic and the end-to-end one is on
bits.

1. CONTRACT A: hrt_probe_depth_device is, bit for bit, the header's fixed-order fold (tests/probe_depth_ref.py) over the per-sample
   outputs of hrt_probe_rays and hrt_trace_rays(HRT_QUERY_CLOSEST) -- at the lane, wave and block edges, from a non-zero first
   sample, with keys, under the proof build and as running sums, for a degenerate probe and for one so far outside the scene
   that the far-origin rule runs;
2. geometry without the query path: one probe over a large quad against the fp64 fold with the analytic depth;
3. the look-up equals the NumPy rule bit for bit over grids, moments crafted to reach every branch, point kinds, batch sizes and
   flag combinations;
4. a depth of all {+inf, 0} makes eval_visible(facing) the bits of eval(facing);
5. the leak test, end to end: a probe behind a wall is weighted out;
6. resources; 7. the command-line tool writes the lightmap the library computes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bake_ref
import probe_depth_ref as pd
import probe_volume_ref as pv
import test_gpu_rays as qr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT = 64
HRT_ERR_INVALID = -1
NAN, INF = float("nan"), float("inf")
bits = qr.bits


def on_gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).to("cuda")


# ---------------------------------------------------------------------------------------------------------------- 1. CONTRACT A
COUNTS = (1, 63, 64, 65, 130)
FIRST = 37                 # a first sample that is no multiple of anything
SMAX = 130
# cornell_mesh: hits everywhere, a mesh for the far-origin rule; single_sphere: most rays miss.  Per scene: two probes inside, a
# degenerate one, one far outside (farther than 16 x (scene bound + 1) from the origin), and r_max between the depths that occur.
CONTRACT = {"cornell_mesh": (np.array([[0.3, 0.2, 0.1, 0.0], [-1.0, 1.1, -0.6, 0.0], [0.0, NAN, 0.0, 0.0], [700.0, 150.0, -400.0, 0.0]], F32), 2.5),
            "single_sphere": (np.array([[0.4, 0.3, 2.5, 0.0], [-3.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, INF], [900.0, -300.0, 500.0, 0.0]], F32), 3.0)}


def series(gpu, dev, d_p, d_keys, first, S, seed, r_max, flags):
    """For samples first .. first + S - 1: the device's own directions (hrt_probe_rays), r = fminf(t, r_max) of the closest-hit
    records of those rays (a miss: r_max), the degenerate mask, and the share of rays that hit."""
    import torch
    ds, rs = [], []
    for s in range(first, first + S):
        rays = gpu.probe_rays(d_p, s, seed, d_keys)
        ds.append(rays[:, 4:7])
        rs.append(dev.trace_rays(rays, "closest", flags))
    d, rec = torch.stack(ds).cpu().numpy(), torch.stack(rs).cpu().numpy()
    hit = bits(rec[..., gpu.HIT_KIND]) != gpu.KIND_MISS
    r = np.where(hit, np.fmin(rec[..., gpu.HIT_T], F32(r_max)), F32(r_max)).astype(F32)
    return d, r, (d == 0).all(axis=2), hit


def fold_all(d, r, deg):
    """(samples, probes, ...) -> (probes, 64, 3)."""
    return np.stack([pd.fold(d[:, i], r[:, i], ~deg[:, i]) for i in range(d.shape[1])])


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_fused_depth_is_the_fixed_order_fold_of_probe_rays_and_closest_hits(gpu, name, exact):
    seed, flags = 5, EXACT if exact else 0
    _, desc, dev, _ = qr.build(gpu, name, 19, 11)
    probes, r_max = CONTRACT[name]
    n = len(probes)
    d_p = on_gpu(probes)
    for keys in (None, bake_ref.keys_for(n)):
        d_keys = None if keys is None else on_gpu(keys)
        for first in (0, FIRST):
            d, r, deg, hit = series(gpu, dev, d_p, d_keys, first, SMAX, seed, r_max, flags)
            assert np.array_equal(deg, np.tile(np.array([False, False, True, False]), (SMAX, 1)))
            live = hit[~deg]
            print(f"{name}: {live.mean():.3f} of the rays hit; {(r[~deg] < F32(r_max)).mean():.3f} are nearer than r_max")
            assert (live.mean() < 0.5) == (name == "single_sphere") and (r[~deg] < F32(r_max)).any() and (r[~deg] == F32(r_max)).any()
            for S in COUNTS:
                what = (name, exact, keys is not None, first, S)
                want = fold_all(d[:S], r[:S], deg[:S])
                got = dev.probe_depth(d_p, S, first_sample=first, seed=seed, keys=d_keys, r_max=r_max, flags=flags).cpu().numpy()
                assert got.shape == (n, 64, 3) and np.array_equal(bits(got), bits(want)), what
                assert (bits(got[2]) == 0).all() and got[[0, 1, 3]].any(), what
            if first:
                continue
            a, b = 65, 64  # running sums over two calls: out + t of each
            base = np.random.default_rng(3).uniform(0, 2, (n, 64, 3)).astype(F32)
            acc = on_gpu(base)
            assert dev.probe_depth(d_p, a, first_sample=0, seed=seed, keys=d_keys, r_max=r_max, flags=flags, out=acc, accumulate=True) is acc
            dev.probe_depth(d_p, b, first_sample=a, seed=seed, keys=d_keys, r_max=r_max, flags=flags, out=acc, accumulate=True)
            want = (base + fold_all(d[:a], r[:a], deg[:a])) + fold_all(d[a:a + b], r[a:a + b], deg[a:a + b])
            assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), (name, exact, keys is not None, "running sums")
    # the NumPy path: blocking, with stats, the same bits
    st = gpu.Stats()
    d, r, deg, _ = series(gpu, dev, d_p, None, 0, 65, seed, r_max, flags)
    host = dev.probe_depth(probes, 65, seed=seed, r_max=r_max, flags=flags, stats=st)
    assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(fold_all(d, r, deg))) and st.samples == n * 65 and st.kernel_ms > 0


def test_waves_take_further_items_by_grid_stride(gpu):
    import torch
    _, desc, dev, _ = qr.build(gpu, "cornell_mesh", 19, 11)
    probes, r_max = CONTRACT["cornell_mesh"]
    m = len(probes)
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 7  # more (probe, block) items than waves can be resident
    want = dev.probe_depth(on_gpu(probes), 65, seed=4, r_max=r_max).cpu().numpy()
    idx = torch.arange(n, device="cuda") % m
    got = dev.probe_depth(on_gpu(probes)[idx].contiguous(), 65, seed=4, keys=idx.to(torch.int32), r_max=r_max)
    assert got.shape == (n, 64, 3) and want.any() and torch.equal(got.view(torch.int32), on_gpu(want)[idx].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 2. analytic
def test_depth_over_a_large_quad_is_the_analytic_one(gpu):
    """One probe at height h over a 200 x 200 quad in z = 0 that faces +z, a dark sky: a direction with d.z < 0 meets the plane at
    h / -d.z (inside the quad wherever that is below r_max), every other one misses.  The sums are compared with the fp64 fold
    over the device's own directions.  Tolerance, relative 1e-5 per texel: the quad intersection's fp32 rounding; the 256 x 2^-24
    of summation error is below it."""
    h, r_max, S, seed = 1.25, 6.0, 256, 9
    s = gpu.HostScene()
    s.set_sky(True)
    s.add_quad((-100.0, -100.0, 0.0), (1, 0, 0), (0, 1, 0), 200.0, 200.0, gpu.Material.make(albedo=(0.5, 0.5, 0.5)))
    dev = gpu.DeviceScene(s.flatten())
    probes = np.array([[0.0, 0.0, h, 0.0]], F32)
    import torch
    d_p = on_gpu(probes)
    d = torch.stack([gpu.probe_rays(d_p, j, seed)[0, 4:7] for j in range(S)]).cpu().numpy().astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.where(d[:, 2] < 0, np.minimum(h / -d[:, 2], r_max), r_max)
    c = pd.direction(np.arange(64)).astype(np.float64)
    w = np.maximum(0, d @ c.T) ** 32  # (S, 64): the fold again, in one expression and with the depths in double
    want = np.stack([w.sum(0), (w * r[:, None]).sum(0), (w * (r * r)[:, None]).sum(0)], axis=1)
    got = dev.probe_depth(probes, S, seed=seed, r_max=r_max)[0].astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print(f"largest relative difference over the 64 x 3 sums: {rel.max():.3e}; {(r < r_max).sum()} of {S} rays hit below r_max")
    assert (want > 0).all() and (r < r_max).sum() > S // 4 and (r == r_max).sum() > S // 4
    assert rel.max() <= 1e-5, float(rel.max())


# ------------------------------------------------------------------------------------------------------------------ 3. the rule
BOX = ((-1.7, 0.3, 2.1), (2.9, 1.1, 7.6))
GRIDS = {"grid_3x2x2": (BOX, (3, 2, 2)), "grid_4x1x2": (BOX, (4, 1, 2))}
BATCHES = (1, 7, 8, 9, 33, 257)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (radiance, facing)


def lookup_case(name):
    """(box, counts, coeffs, sums, points): 257 point records of every kind, the special ones first so that every batch size holds
    some, and depth sums whose moments reach every branch of the visibility factor for some corner of some point."""
    box, counts = GRIDS[name]
    rng = np.random.default_rng(11)
    lo, hi = np.asarray(box[0], F32), np.asarray(box[1], F32)
    e = hi - lo
    count = int(np.prod(counts))
    ijk = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), -1).reshape(-1, 3)
    P = [np.array([lo + F32(0.4) * e, lo - F32(0.6) * e, hi + F32(1.8) * e], F32),       # inside, outside the box twice
         pv.centres(lo, hi, counts, ijk[:4]),                                              # at probe centres: l == 0 with bias 0
         lo + rng.random((250, 3)).astype(F32) * F32(1.4) * e - F32(0.2) * e]
    P = np.concatenate(P).astype(F32)[:257]
    N = rng.standard_normal((257, 3)).astype(F32) * F32(10.0) ** rng.integers(-2, 3, (257, 1)).astype(F32)
    pts = np.zeros((257, 8), F32)
    pts[:, 0:3], pts[:, 3], pts[:, 4:7] = P, 0.25, N
    pts[:, 7] = rng.choice(np.array([0.0, -0.3, 0.05, 0.5, 1e-4], F32), 257)
    pts[3:7, 7] = 0.0                   # the probe centres themselves
    pts[7, 7] = -0.25                   # negative bias
    pts[8, 4:7] = 0                     # degenerate: N == 0
    pts[9, 7] = INF                     # degenerate: a bias that is not finite
    pts[10, 7] = NAN
    pts[11, 4] = NAN
    pts[12, 0] = -INF
    pts[13, 4:7] = (1e-30, 0, 0)        # a squared length that underflows
    coeffs = rng.standard_normal((count, 9, 3)).astype(F32)
    # the moments: random ones round the distances that occur, then crafted ones at the texels some corners look through
    sums = np.zeros((count, 64, 3), F32)
    m1 = rng.uniform(0.2, 3.0, (count, 64)).astype(F32)
    Wt = rng.uniform(0.5, 40.0, (count, 64)).astype(F32)
    sums[..., 0], sums[..., 1], sums[..., 2] = Wt, Wt * m1, Wt * (m1 * m1 + rng.uniform(0, 0.3, (count, 64)).astype(F32))
    sums[rng.random((count, 64)) < 0.15] = 0  # texels nobody looked through: {+inf, 0}
    index, texel, l = corner_geometry(box, counts, pts)
    live = np.isfinite(l) & (l > 0)
    rows = np.flatnonzero(live.all(axis=1))
    for k, i in enumerate(rows[:60]):  # W = 1: the moments are the sums themselves
        m = k % 8
        kind = (k // 8) % 3
        lm = l[i, m]
        val = {0: (lm, lm * lm + F32(0.1)),                          # l == m1 exactly
               1: (lm * F32(0.5), (lm * F32(0.5)) * (lm * F32(0.5))),  # var == 0 with l > m1
               2: (lm * F32(0.75), F32(0.5) * (lm * F32(0.75)) * (lm * F32(0.75)))}[kind]  # m2 < m1^2
        sums[index[i, m], texel[i, m]] = (1.0, val[0], val[1])
    return box, counts, coeffs, sums, pts


def corner_geometry(box, counts, pts):
    """Per point and corner: the probe, the texel it looks at Pb through and l, by the NumPy rule."""
    lo, hi, n, _ = pv._grid(*box, counts)
    Nn, _ = pv.normals(pts)
    i0, i1, _ = pv.cell(lo, hi, n, pts)
    index, texel, l = np.zeros((len(pts), 8), np.int64), np.zeros((len(pts), 8), np.int64), np.zeros((len(pts), 8), F32)
    with np.errstate(all="ignore"):
        Pb = (pts[:, 0:3] + pts[:, 7:8] * Nn).astype(F32)
        for m in range(8):
            c = np.stack([i1[:, a] if (m >> a) & 1 else i0[:, a] for a in range(3)], axis=1)
            index[:, m] = (c[:, 2].astype(np.int64) * n[1] + c[:, 1]) * n[0] + c[:, 0]
            v = (Pb - pv.centres(lo, hi, n, c)).astype(F32)
            l[:, m] = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            texel[:, m] = pd.texel(v)
    return index, texel, l


@pytest.fixture(scope="module")
def lookups():
    """The cases and the NumPy rule over them, once."""
    out = {}
    for name in GRIDS:
        box, counts, coeffs, sums, pts = lookup_case(name)
        mom = pd.moments(sums)
        want = {f: pd.evaluate_visible(*box, counts, coeffs, mom, pts, *f) for f in FLAGS}
        out[name] = (box, counts, coeffs, sums, pts, mom, want)
    return out


def test_the_cases_reach_every_branch(lookups):
    for name, (box, counts, coeffs, sums, pts, mom, want) in lookups.items():
        index, texel, l = corner_geometry(box, counts, pts)
        _, _, _, deg = pd.weights_visible(*box, counts, mom, pts)
        assert deg[8:14].all() and not deg[:8].any() and deg.sum() == 6, name
        ok = ~deg
        m1, m2 = mom[index, texel, 0], mom[index, texel, 1]
        with np.errstate(all="ignore"):
            var = m2 - m1 * m1
        assert (np.isinf(m1) & ok[:, None]).any() and ((l == m1) & (l > 0) & ok[:, None]).any(), name
        assert ((var == 0) & (l > m1) & ok[:, None]).any() and ((var < 0) & (l > m1) & ok[:, None]).any(), name
        assert ((var > 0) & (l > m1) & ok[:, None]).any() and ((l < m1) & np.isfinite(m1) & ok[:, None]).any(), name
        assert (l[3:7] == 0).any(axis=1).all(), name  # the points at probe centres
        lo, hi = np.minimum(*np.asarray(box, F32)), np.maximum(*np.asarray(box, F32))
        assert ((pts[:3, 0:3] < lo) | (pts[:3, 0:3] > hi)).any(axis=1).sum() == 2 and (pts[ok, 7] < 0).any() and (pts[ok, 7] == 0).any()
        for f, w in want.items():
            assert np.isfinite(w).all() and w[ok].any() and not w[deg].any(), (name, f)
        assert not np.array_equal(bits(want[(False, False)]), bits(pv.evaluate(*box, counts, coeffs, pts))), "visibility changes the result"


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_eval_visible_is_the_numpy_rule_bit_for_bit(gpu, lookups, name):
    import torch
    box, counts, coeffs, sums, pts, mom, want = lookups[name]
    with gpu.ProbeVolume(*box, *counts) as vol:
        vol.update(coeffs)
        assert vol.update_depth(on_gpu(sums)) is vol
        d_pts = on_gpu(pts)
        for (radiance, facing), w in want.items():
            for n in BATCHES:
                sentinel = torch.full((n + 2, 3), 7.0, dtype=torch.float32, device="cuda")
                got = vol.eval_visible(d_pts[:n].contiguous(), radiance, facing, out=sentinel[:n])
                torch.cuda.synchronize()
                assert (sentinel[n:] == 7.0).all(), "results written past the batch"
                g = got.cpu().numpy()
                bad = np.flatnonzero((bits(g) != bits(w[:n])).any(axis=1))
                assert bad.size == 0, (name, radiance, facing, n, bad[:8].tolist(), g[bad[:2]].tolist(), w[bad[:2]].tolist())
        # the NumPy path: blocking, with stats; the depth from the host
        vol.update_depth(sums)
        st = gpu.Stats()
        host = vol.eval_visible(pts, facing=True, stats=st)
        assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(want[(False, True)])) and st.samples == len(pts) and st.kernel_ms > 0
        assert vol.eval_visible(np.zeros((0, 8), F32)).shape == (0, 3)
        with pytest.raises(ValueError, match="the volume has"):
            vol.update_depth(np.zeros((1, 64, 3), F32))


# ---------------------------------------------------------------------------------------------------------------- 4. all visible
def test_a_depth_that_hides_nothing_gives_the_facing_lookup(gpu, lookups):
    box, counts, coeffs, sums, pts, mom, want = lookups["grid_3x2x2"]
    pts = pts.copy()
    pts[9:11, 7] = 0.0  # the plain look-up does not read the bias: keep the degenerate sets equal
    with gpu.ProbeVolume(*box, *counts) as vol:
        vol.update(coeffs).update_depth(np.zeros((int(np.prod(counts)), 64, 3), F32))
        for radiance in (False, True):
            plain = vol.eval(pts, radiance, facing=True)
            assert plain.any() and np.array_equal(bits(vol.eval_visible(pts, radiance, facing=True)), bits(plain))


def test_the_refusals_that_need_a_volume_come_in_the_headers_order(gpu):
    dev = gpu.device_lib()
    PTS, OUT = 0x1000, 0x2000
    entries = (("hrt_probe_eval_visible_device", "d_points", "d_out", 4), ("hrt_probe_eval_visible", "points", "out", 1))
    with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as vol:
        def call(entry, pts=PTS, n=5, flags=0, out=OUT):
            return getattr(dev, entry)(vol._h, C.c_void_p(pts), n, flags, C.c_void_p(out), None), dev.hrt_last_error().decode()
        wrong = dict(pts=0, n=2 ** 31, out=0)
        for entry, *_ in entries:
            assert call(entry, **wrong) == (HRT_ERR_INVALID, entry + ": the volume has no coefficients yet (hrt_probe_volume_update)")
        vol.update(np.zeros((2, 9, 3), F32))
        for entry, *_ in entries:
            assert call(entry, **wrong) == (HRT_ERR_INVALID, entry + ": the volume has no depth moments yet (hrt_probe_volume_update_depth)")
            assert "flags" in call(entry, flags=8, **wrong)[1]
        for entry, name, args in (("hrt_probe_volume_update_depth_device", "d_sums", (None,)), ("hrt_probe_volume_update_depth", "sums", ())):
            assert getattr(dev, entry)(vol._h, None, *args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == f"{entry}: {name} is NULL"
            assert getattr(dev, entry)(vol._h, C.c_void_p(PTS + 2), *args) == HRT_ERR_INVALID and dev.hrt_last_error().decode() == f"{entry}: {name} is not 4-byte aligned"
        vol.update_depth(np.zeros((2, 64, 3), F32))
        for entry, pn, on, off in entries:
            assert call(entry, **wrong) == (HRT_ERR_INVALID, f"{entry}: {pn} is NULL")
            wrong2 = dict(wrong, pts=PTS + off)
            assert "-byte aligned" in call(entry, **wrong2)[1]
            assert call(entry, **dict(wrong, pts=PTS))[1].startswith(entry + ": n must be at most 2^31 - 1")
            assert call(entry, **dict(wrong, pts=PTS, n=5)) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")


# --------------------------------------------------------------------------------------------------------------- 5. the leak test
def test_a_probe_behind_a_wall_is_weighted_out(gpu):
    """A dark sky; a black 40 x 40 wall in the plane x = 0 (two squares back to back: a square is hit from its front only); a 2 x 2
    emitter at x = -3 lit towards +x; a 2 x 1 x 1 grid over (-2, -.5, -.5) .. (2, .5, .5), so the probes sit at x = -1 (lit) and
    x = +1 (dark, behind the wall); 1024 samples, r_max 4.  At (.5, 0, 0) the plain look-up takes a quarter of the lit probe
    through the wall; the rule leaves the lit probe .25 x .001 against .75, about a five-hundredth of that.  The condition is a
    tenth."""
    s = gpu.HostScene()
    s.set_sky(True)
    black = gpu.Material.make(albedo=(0, 0, 0))
    s.add_quad((0.0, -20.0, -20.0), (0, 1, 0), (0, 0, 1), 40.0, 40.0, black)   # faces +x
    s.add_quad((0.0, -20.0, -20.0), (0, 0, 1), (0, 1, 0), 40.0, 40.0, black)   # faces -x
    s.add_quad((-3.0, -1.0, -1.0), (0, 1, 0), (0, 0, 1), 2.0, 2.0,
               gpu.Material.make(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=6.0))
    dev = gpu.DeviceScene(s.flatten())
    for o, d, t in (((-1, 0, 0), (1, 0, 0), 1.0), ((1, 0, 0), (-1, 0, 0), 1.0), ((-1, 0, 0), (-1, 0, 0), 2.0)):  # both faces of the wall, the emitter
        rec = dev.trace_rays(qr.make_rays([o], [d]), "closest")
        assert bits(rec)[0, gpu.HIT_KIND] == gpu.KIND_SQUARE and rec[0, gpu.HIT_T] == F32(t), (o, d, rec)
    lo, hi, counts, spp, r_max = (-2, -.5, -.5), (2, .5, .5), (2, 1, 1), 1024, 4.0
    grid = gpu.probe_grid(lo, hi, *counts)
    assert grid[:, 0].tolist() == [-1, 1]
    coeffs = dev.probes(grid, spp)
    sums = dev.probe_depth(grid, spp, r_max=r_max)
    assert coeffs[0].any() and not coeffs[1].any(), "the probe behind the wall is dark"
    pts = np.zeros((2, 8), F32)
    pts[:, 0:3], pts[:, 4:7] = [(.5, 0, 0), (-.5, 0, 0)], (-1, 0, 0)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        vol.update(coeffs).update_depth(sums)
        plain, visible = vol.eval(pts), vol.eval_visible(pts)
    print(f"behind the wall: plain {plain[0].tolist()}, visible {visible[0].tolist()}, ratio {(visible[0] / plain[0]).tolist()}")
    print(f"before the wall: plain {plain[1].tolist()}, visible {visible[1].tolist()}")
    assert (plain[0] > 0).all()
    assert (visible[0] <= 0.1 * plain[0]).all()
    assert (visible[1] >= plain[1]).all()


# ---------------------------------------------------------------------------------------------------------------- 6. resources
def test_a_volume_with_depth_gives_back_what_it_took(gpu):
    import torch
    torch.cuda.synchronize()
    before = gpu.live_resources()
    vol = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 4, 4, 4)
    vol.update(np.ones((64, 9, 3), F32))
    assert gpu.live_resources()[0] == before[0] + 1
    vol.update_depth(np.ones((64, 64, 3), F32))
    assert gpu.live_resources()[0] == before[0] + 2, "the moments are a second buffer of the volume's"
    vol.update_depth(on_gpu(np.ones((64, 64, 3), F32)))
    assert gpu.live_resources()[0] == before[0] + 2
    pts = np.zeros((10, 8), F32)
    pts[:, 6] = 1
    assert np.isfinite(vol.eval_visible(pts)).all() and vol.eval_visible(on_gpu(pts)).shape == (10, 3)
    vol.close()
    vol.close()
    assert gpu.live_resources() == before
    # a scene's block values go with the scene
    s = gpu.HostScene()
    s.set_sky(True)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0, gpu.Material.make())
    dev = gpu.DeviceScene(s.flatten())
    held = gpu.live_resources()
    dev.probe_depth(np.array([[0, 0, 1, 0]], F32), 65, r_max=2.0)
    assert gpu.live_resources()[0] == held[0] + 1
    dev.close()
    assert gpu.live_resources() == before


# ---------------------------------------------------------------------------------------------------------------------- 7. CLI
@pytest.mark.parametrize("rmax", [None, 0.75])
def test_the_cli_writes_the_visible_lightmap_the_library_computes(gpu, tmp_path, rmax):
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 65, (2, 2, 1)
    path, mine = tmp_path / "probe_map.ppm", tmp_path / "mine.ppm"
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8",
                        "--probe-grid", ",".join(str(c) for c in counts), "--probe-box", ",".join(str(x) for x in lo + hi), "--probe-quad", "0",
                        "--spp", str(spp), "--out", str(path), "--probe-visible"] + ([] if rmax is None else ["--probe-rmax", str(rmax)]),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    if rmax is None:  # 1.5 x the diagonal of a grid cell, in fp32
        e = (np.asarray(hi, F32) - np.asarray(lo, F32)) / np.asarray(counts, F32)
        rmax = float(F32(1.5) * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))
    _, desc, dev, _ = qr.build(gpu, "cornell_box", 8, 8)
    grid = gpu.probe_grid(lo, hi, *counts)
    coeffs, sums = dev.probes(grid, spp), dev.probe_depth(grid, spp, r_max=rmax)  # the tool's seed is the library's default
    pts = gpu.quad_points(gpu.scene_quads(desc)[0], 8, 8, 1, 0.0, 0.0)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        vol.update(coeffs).update_depth(sums)
        lightmap, plain = vol.eval_visible(pts), vol.eval(pts)
    assert lightmap.any() and (rmax < 1 or not np.array_equal(lightmap, plain))
    gpu.write_ppm(str(mine), lightmap.reshape(8, 8, 3))
    assert path.read_bytes() == mine.read_bytes()
