"""Lit rays and probe relighting on the GPU (include/hrt.h "Lit rays").  Every comparison but the furnace is on bits.

A. a ray that cannot continue past its first hit is the integrator's ray: trace_lit against a volume of zeros equals trace_radiance;
B. the tail is the look-up: trace_lit(V) = A + albedo * G, with A from the zero volume, albedo, n, t and the type from
   trace_rays("shade") and G from the volume's own eval / eval_visible on the records {p, time, n, bias};
C. the fused update is the fold of the query: probes_lit equals the fixed-order sum of "Light probes" (tests/probe_ref.py) over
   per-sample probe_rays + trace_lit; with a zero volume where no ray continues it equals probes;
D. blend is the hysteresis expression;
E. the furnace: a closed diffuse room relit round by round follows the geometric series, and meets the path tracer;
F. the refusals that need a volume, resources, and the command-line tool."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bake_ref
import probe_lit_ref as pl
import probe_ref
import probe_volume_ref as pv
import test_gpu_probe_depth as tpd
import test_gpu_rays as qr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT = 64
HRT_ERR_INVALID = -1
NAN, INF = float("nan"), float("inf")
FACING, VISIBLE = pl.FACING, pl.LIT_VISIBLE
EVAL_FLAGS = (0, FACING, VISIBLE, FACING | VISIBLE)
bits = qr.bits
on_gpu = tpd.on_gpu
COUNTS = (3, 2, 2)
SHADE_TYPE = 15  # the Surface::type word of a SHADE record


def unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def zero_volume(gpu, box):
    vol = gpu.ProbeVolume(*box, *COUNTS)
    return vol.update(np.zeros((vol.count, 9, 3), F32))


def random_volume(gpu, box, seed):
    """(volume, coefficients, depth sums): random coefficients; depth moments round the distances that occur in a room of this size,
    a seventh of the texels never looked through ({+inf, 0}), a seventh with no variance, a seventh with m2 < m1^2."""
    rng = np.random.default_rng(seed)
    count = int(np.prod(COUNTS))
    coeffs = rng.standard_normal((count, 9, 3)).astype(F32)
    m1 = rng.uniform(0.2, 3.0, (count, 64)).astype(F32)
    W = rng.uniform(0.5, 40.0, (count, 64)).astype(F32)
    kind = rng.integers(0, 7, (count, 64))
    m2 = np.where(kind == 1, m1 * m1, np.where(kind == 2, F32(0.5) * (m1 * m1), m1 * m1 + rng.uniform(0, 0.3, (count, 64)).astype(F32))).astype(F32)
    sums = np.stack([W, W * m1, W * m2], axis=-1).astype(F32)
    sums[kind == 0] = 0
    vol = gpu.ProbeVolume(*box, *COUNTS)
    vol.update(coeffs).update_depth(sums)
    return vol, coeffs, sums


# ------------------------------------------------------------------------------------- A. a ray that cannot continue
def emitter_scene(gpu, n_lights, dark=True):
    """One diffuse 2 x 2 quad in z = 0 that faces +z and emits, `n_lights` point lights above it: a diffuse scatter off a one-sided
    plane cannot hit it again, and a dark sky adds +0."""
    s = gpu.HostScene()
    s.set_sky(dark)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0,
               gpu.Material.make(albedo=(0.7, 0.5, 0.3), emissive=True, light_color=(0.9, 0.6, 0.2), light_intensity=2.5))
    for pos, col in (((0.3, -0.2, 1.5), (1.0, 0.8, 0.6)), ((-0.8, 0.9, 0.7), (0.2, 0.5, 1.0)))[:n_lights]:
        s.add_light(pos, 0.2, col)
    return gpu.DeviceScene(s.flatten())


def emitter_rays():
    """Rays that hit the quad from its front, rays that miss it (beside it, away from it, from behind it), a degenerate one."""
    rng = np.random.default_rng(5)
    o = np.concatenate([rng.uniform(-1.5, 1.5, (60, 2)), rng.uniform(0.2, 2.0, (60, 1))], axis=1).astype(F32)
    target = np.concatenate([rng.uniform(-1.3, 1.3, (60, 2)), np.zeros((60, 1))], axis=1).astype(F32)
    rays = qr.make_rays(o, unit(target - o))
    rays[50:55, 4:7] *= -1           # away from the plane
    rays[55:59, 2] *= -1             # from behind: a square is hit from its front only
    rays[55:59, 6] *= -1
    rays[59, 4] = NAN
    return rays


@pytest.mark.parametrize("n_lights", [1, 2])
def test_a_ray_that_cannot_continue_is_the_integrators_ray(gpu, n_lights):
    rays = emitter_rays()
    n = len(rays)
    d_rays = on_gpu(rays)
    box = ((-2, -2, -1), (2, 2, 3))
    dev = emitter_scene(gpu, n_lights)
    rec = dev.trace_rays(rays, "closest")
    hit = bits(rec[:, gpu.HIT_KIND]) != gpu.KIND_MISS
    assert hit[:50].sum() > 15 and (~hit[:50]).any() and not hit[50:].any(), "hits, misses and a degenerate ray"
    with zero_volume(gpu, box) as vol:
        for exact in (0, EXACT):
            for keys in (None, bake_ref.keys_for(n)):
                d_keys = None if keys is None else on_gpu(keys)
                for first in (0, 37):
                    want = dev.trace_radiance(d_rays, 1, first_sample=first, seed=7, keys=d_keys, flags=exact).cpu().numpy()
                    for ef in (0, FACING):
                        got = dev.trace_lit(d_rays, vol, 1, first_sample=first, seed=7, keys=d_keys, eval_flags=ef, flags=exact).cpu().numpy()
                        assert np.array_equal(bits(got), bits(want)), (n_lights, exact, keys is not None, first, ef)
                    assert want[hit].all() and not want[~hit].any() and (bits(want[59]) == 0).all()
        # several samples, and the NumPy form
        want = dev.trace_radiance(rays, 3, first_sample=5, seed=7)
        got = dev.trace_lit(rays, vol, 3, first_sample=5, seed=7)
        assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(want))
        # under the gradient sky the rays that miss are still the integrator's
        sky = emitter_scene(gpu, n_lights, dark=False)
        want = sky.trace_radiance(d_rays, 1, first_sample=37, seed=7).cpu().numpy()
        got = sky.trace_lit(d_rays, vol, 1, first_sample=37, seed=7).cpu().numpy()
        miss = ~hit
        miss[59] = False
        assert want[miss].all() and np.array_equal(bits(got[miss]), bits(want[miss])) and (bits(got[59]) == 0).all()


# ----------------------------------------------------------------------------------------------- B. the tail is the look-up
TAIL_SCENES = {"cornell_mesh": probe_ref.BOXES["cornell_mesh"][:2], "random_spheres": probe_ref.BOXES["random_spheres"][:2]}
BATCHES = (1, 63, 64, 65, 257)


def tail_rays(gpu, cam, box, seed):
    """257 rays: camera rays of a 19 x 11 frame interleaved (so that the prefix batches hold all kinds) with rays from
    inside the volume's box in random directions, at the frame's times; one degenerate."""
    rng = np.random.default_rng(seed)
    camera = gpu.camera_rays(cam, 19, 11, 0, 3).cpu().numpy()
    lo, hi = np.asarray(box[0], F32), np.asarray(box[1], F32)
    inside = qr.make_rays(lo + rng.random((257, 3)).astype(F32) * (hi - lo), unit(rng.standard_normal((257, 3))))
    inside[:, 3] = rng.random(257).astype(F32)
    rays = inside.copy()
    rays[0::2] = camera[rng.permutation(len(camera))[:129]]
    rays[[5, 41, 70, 200], 0:3] = (0.0, 50.0, 0.0)   # from far above the scene, upwards: misses in a closed room's scene too
    rays[[5, 41, 70, 200], 4:7] = (0.0, 1.0, 0.0)
    rays[62, 5] = INF
    return np.ascontiguousarray(rays[:257], F32)


@pytest.mark.parametrize("name", sorted(TAIL_SCENES))
def test_the_tail_is_the_lookup(gpu, name):
    import torch
    box = TAIL_SCENES[name]
    _, desc, dev, cam = qr.build(gpu, name, 19, 11)
    rays = tail_rays(gpu, cam, box, 21)
    n = len(rays)
    d_rays = on_gpu(rays)
    rec = dev.trace_rays(rays, "shade")
    ru = bits(rec)
    kind, typ = ru[:, gpu.HIT_KIND], ru[:, SHADE_TYPE]
    hit = kind != gpu.KIND_MISS
    diffuse = hit & (typ == pl.DIFFUSE)
    miss = ~hit
    miss[62] = False  # the degenerate ray
    print(f"{name}: {diffuse.sum()} diffuse hits, {(hit & ~diffuse).sum()} on mirror or glass, {(kind == gpu.KIND_MESH).sum()} on a mesh, {miss.sum()} misses")
    assert diffuse.sum() > 50 and (hit & ~diffuse).any() and miss.sum() >= 4 and not hit[62]
    assert (kind == gpu.KIND_MESH).any() == (name == "cornell_mesh")
    for b in BATCHES[1:]:
        assert diffuse[:b].any() and miss[:b].any(), b
    albedo = np.where(hit[:, None], rec[:, 8:11], F32(0)).astype(F32)
    SMAX = 5
    with zero_volume(gpu, box) as zero:
        A = np.stack([dev.trace_lit(d_rays, zero, 1, first_sample=s, seed=9).cpu().numpy() for s in range(SMAX)])
    assert (A[0][hit] != 0).any()
    vol, coeffs, sums = random_volume(gpu, box, 31)
    with vol:
        for bias in (0.0, 1e-3):
            pts = pl.point_records(rays[:, 0:3], rays[:, 4:7], np.where(hit, rec[:, 0], F32(0)), np.where(hit[:, None], rec[:, 4:7], F32(0)), rays[:, 3], bias)
            for ef in EVAL_FLAGS:
                G = (vol.eval_visible if ef & VISIBLE else vol.eval)(pts, facing=bool(ef & FACING))
                assert np.isfinite(G).all() and G[diffuse].all() and not G[~hit].any()
                v = np.stack([pl.sample_value(A[s], albedo, diffuse, G) for s in range(SMAX)])
                assert not np.array_equal(v[0][diffuse], A[0][diffuse])
                for b in BATCHES:
                    sentinel = torch.full((b + 2, 3), 7.0, dtype=torch.float32, device="cuda")
                    got = dev.trace_lit(d_rays[:b].contiguous(), vol, 1, seed=9, eval_flags=ef, bias=bias, out=sentinel[:b])
                    torch.cuda.synchronize()
                    assert (sentinel[b:] == 7.0).all(), "results written past the batch"
                    g = got.cpu().numpy()
                    bad = np.flatnonzero((bits(g) != bits(v[0][:b])).any(axis=1))
                    assert bad.size == 0, (name, bias, ef, b, bad[:8].tolist(), g[bad[:2]].tolist(), v[0][bad[:2]].tolist())
                # three samples from sample 2, as a mean; then running sums over two calls
                got = dev.trace_lit(d_rays, vol, 3, first_sample=2, seed=9, eval_flags=ef, bias=bias).cpu().numpy()
                assert np.array_equal(bits(got), bits(pl.ray_output(v[2:5]))), (name, bias, ef, "three samples")
                base = np.random.default_rng(2).uniform(0, 2, (n, 3)).astype(F32)
                acc = on_gpu(base)
                assert dev.trace_lit(d_rays, vol, 2, seed=9, eval_flags=ef, bias=bias, out=acc, accumulate=True) is acc
                dev.trace_lit(d_rays, vol, 3, first_sample=2, seed=9, eval_flags=ef, bias=bias, out=acc, accumulate=True)
                want = pl.ray_output(v[2:5], base=pl.ray_output(v[0:2], base=base))
                want[62] = base[62]  # a degenerate ray leaves its sums as they are
                assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), (name, bias, ef, "running sums")
        # the proof build shades the same hits the same way
        plain = dev.trace_lit(d_rays, vol, 1, seed=9, eval_flags=FACING | VISIBLE, bias=1e-3).cpu().numpy()
        exact = dev.trace_lit(d_rays, vol, 1, seed=9, eval_flags=FACING | VISIBLE, bias=1e-3, flags=EXACT).cpu().numpy()
        same = (bits(dev.trace_rays(rays, "shade", EXACT)) == ru).all(axis=1)
        assert same.mean() > 0.9 and np.array_equal(bits(plain[same]), bits(exact[same]))


# --------------------------------------------------------------------------------- C. the fused update is the fold of the query
COUNTS_C = (1, 63, 64, 65, 130)
FIRST, SMAX_C = 37, 130
FOLD_BOXES = {"cornell_mesh": probe_ref.BOXES["cornell_mesh"][:2], "single_sphere": ((-3.5, -1.5, -1.0), (1.5, 1.5, 3.5))}


def lit_series(gpu, dev, vol, d_p, d_keys, first, S, seed, flags, ef, bias):
    """For samples first .. first + S - 1: the basis values of the device's own directions (hrt_probe_rays), the one-sample
    hrt_trace_lit outputs for those records, and the degenerate mask."""
    import torch
    ds, vs = [], []
    for s in range(first, first + S):
        r = gpu.probe_rays(d_p, s, seed, d_keys)
        ds.append(r[:, 4:7])
        vs.append(dev.trace_lit(r, vol, 1, first_sample=s, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags))
    d, v = torch.stack(ds).cpu().numpy(), torch.stack(vs).cpu().numpy()
    return np.stack([probe_ref.basis(x) for x in d]), v, (d == 0).all(axis=2)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", sorted(FOLD_BOXES))
def test_fused_lit_probes_are_the_fixed_order_fold_of_probe_rays_and_lit_rays(gpu, name, exact):
    seed, flags, ef, bias = 5, EXACT if exact else 0, FACING | VISIBLE, 1e-3
    _, desc, dev, _ = qr.build(gpu, name, 19, 11)
    probes, _ = tpd.CONTRACT[name]
    n = len(probes)
    d_p = on_gpu(probes)
    vol, _, _ = random_volume(gpu, FOLD_BOXES[name], 17)
    with vol:
        for keys in (None, bake_ref.keys_for(n)):
            d_keys = None if keys is None else on_gpu(keys)
            for first in (0, FIRST):
                Y, v, deg = lit_series(gpu, dev, vol, d_p, d_keys, first, SMAX_C, seed, flags, ef, bias)
                assert np.array_equal(deg, np.tile(np.array([False, False, True, False]), (SMAX_C, 1)))
                for S in COUNTS_C:
                    what = (name, exact, keys is not None, first, S)
                    want = probe_ref.fold(Y[:S], v[:S], deg[:S]) / F32(S)
                    got = dev.probes_lit(d_p, vol, S, first_sample=first, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags).cpu().numpy()
                    assert got.shape == (n, 9, 3) and np.array_equal(bits(got), bits(want)), what
                    assert (bits(got[2]) == 0).all() and (S < 64 or got[[0, 1, 3]].any()), what  # a few samples may all miss under a dark sky
                if first:
                    continue
                a, b = 65, 64  # running sums over two calls
                base = np.random.default_rng(3).uniform(0, 2, (n, 9, 3)).astype(F32)
                acc = on_gpu(base)
                assert dev.probes_lit(d_p, vol, a, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags, out=acc, accumulate=True) is acc
                dev.probes_lit(d_p, vol, b, first_sample=a, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags, out=acc, accumulate=True)
                want = (base + probe_ref.fold(Y[:a], v[:a], deg[:a])) + probe_ref.fold(Y[a:a + b], v[a:a + b], deg[a:a + b])
                assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), (name, exact, keys is not None, "running sums")
        # the NumPy path: blocking, with stats, the same bits
        st = gpu.Stats()
        Y, v, deg = lit_series(gpu, dev, vol, d_p, None, 0, 65, seed, flags, ef, bias)
        host = dev.probes_lit(probes, vol, 65, seed=seed, eval_flags=ef, bias=bias, flags=flags, stats=st)
        assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(probe_ref.fold(Y, v, deg) / F32(65)))
        assert st.samples == n * 65 and st.kernel_ms > 0
        # the volume changes the result where diffuse surfaces are hit; single_sphere's one sphere is a mirror, which gets no tail
        with zero_volume(gpu, FOLD_BOXES[name]) as zero:
            assert np.array_equal(host, dev.probes_lit(probes, zero, 65, seed=seed, flags=flags)) == (name == "single_sphere")


def test_waves_take_further_items_by_grid_stride(gpu):
    import torch
    _, desc, dev, _ = qr.build(gpu, "cornell_mesh", 19, 11)
    probes, _ = tpd.CONTRACT["cornell_mesh"]
    m = len(probes)
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 7  # more (probe, block) items than waves can be resident
    vol, _, _ = random_volume(gpu, FOLD_BOXES["cornell_mesh"], 17)
    with vol:
        want = dev.probes_lit(on_gpu(probes), vol, 65, seed=4, eval_flags=FACING).cpu().numpy()
        idx = torch.arange(n, device="cuda") % m
        got = dev.probes_lit(on_gpu(probes)[idx].contiguous(), vol, 65, seed=4, keys=idx.to(torch.int32), eval_flags=FACING)
        assert got.shape == (n, 9, 3) and want.any() and torch.equal(got.view(torch.int32), on_gpu(want)[idx].view(torch.int32))


@pytest.mark.parametrize("n_lights", [1, 2])
def test_with_a_zero_volume_where_no_ray_continues_lit_probes_are_probes(gpu, n_lights):
    dev = emitter_scene(gpu, n_lights)
    probes = np.array([[0.2, -0.3, 0.8, 0.0], [-0.9, 0.6, 0.3, 0.0], [0.0, 0.0, -0.5, 0.0], [NAN, 0.0, 1.0, 0.0]], F32)
    with zero_volume(gpu, ((-2, -2, -1), (2, 2, 3))) as vol:
        for S, first in ((65, 0), (130, 37)):
            want = dev.probes(on_gpu(probes), S, first_sample=first, seed=8).cpu().numpy()
            got = dev.probes_lit(on_gpu(probes), vol, S, first_sample=first, seed=8).cpu().numpy()
            assert want[:2].all() and not want[2:].any() and np.array_equal(bits(got), bits(want)), (n_lights, S, first)


# ------------------------------------------------------------------------------------------------------------------- D. blend
def test_blend_is_the_hysteresis_expression(gpu):
    box, counts, _, _, pts = tpd.lookup_case("grid_3x2x2")
    rng = np.random.default_rng(41)
    c0, c1, c2 = (rng.standard_normal((12, 9, 3)).astype(F32) for _ in range(3))
    with gpu.ProbeVolume(*box, *counts) as vol:
        vol.update(c0)
        before = vol.eval(pts, facing=True)
        assert np.array_equal(bits(before), bits(pv.evaluate(*box, counts, c0, pts, False, True)))
        assert vol.blend(c1, 0.7) is vol
        p = pl.blend(c0, c1, 0.7)
        assert not np.array_equal(p, c0) and not np.array_equal(p, c1)
        for radiance, facing in tpd.FLAGS:
            assert np.array_equal(bits(vol.eval(pts, radiance, facing)), bits(pv.evaluate(*box, counts, p, pts, radiance, facing))), (radiance, facing)
        vol.blend(on_gpu(c2), 0.25)  # the device form, on top of the first blend
        p = pl.blend(p, c2, 0.25)
        assert np.array_equal(bits(vol.eval(pts, facing=True)), bits(pv.evaluate(*box, counts, p, pts, False, True)))
        vol.blend(c1, 0.0)  # keep = 0: the bits of an update
        after = vol.eval(pts, facing=True)
        vol.update(c1)
        assert np.array_equal(bits(after), bits(vol.eval(pts, facing=True)))
    dev = gpu.device_lib()
    with gpu.ProbeVolume(*box, *counts) as vol:
        with pytest.raises(gpu.HrtError, match="hrt_probe_volume_blend: the volume has no coefficients yet"):
            vol.blend(c1, 0.5)
        vol.update(c0)
        for entry, name, tail in (("hrt_probe_volume_blend_device", "d_coeffs", (None,)), ("hrt_probe_volume_blend", "coeffs", ())):
            call = lambda ptr, keep: (getattr(dev, entry)(vol._h, ptr, C.c_float(keep), *tail), dev.hrt_last_error().decode())
            assert call(None, NAN) == (HRT_ERR_INVALID, f"{entry}: {name} is NULL")
            assert call(C.c_void_p(0x1002), NAN) == (HRT_ERR_INVALID, f"{entry}: {name} is not 4-byte aligned")
            for bad in (NAN, 1.0, -0.5, INF):
                rc, msg = call(C.c_void_p(0x1000), bad)
                assert rc == HRT_ERR_INVALID and msg.startswith(f"{entry}: keep must be in [0, 1)"), (bad, msg)
        assert np.array_equal(bits(vol.eval(pts)), bits(pv.evaluate(*box, counts, c0, pts))), "a refused blend changes nothing"


# ----------------------------------------------------------------------------------------------------------------- E. the furnace
def furnace_scene(gpu, rho=0.5, e=6.0):
    """Six inward-facing squares of side 2.2 centred on the faces of the cube [-1, 1]^3 (they overlap past the edges: no ray
    leaves), diffuse with albedo rho, emitting e, under a dark sky."""
    s = gpu.HostScene()
    s.set_sky(True)
    m = gpu.Material.make(albedo=(rho, rho, rho), emissive=True, light_color=(1, 1, 1), light_intensity=e)
    for corner, right, up in (((-1.0, -1.1, -1.1), (0, 1, 0), (0, 0, 1)), ((1.0, -1.1, -1.1), (0, 0, 1), (0, 1, 0)),     # x = -1 faces +x, x = +1 faces -x
                              ((-1.1, -1.0, -1.1), (0, 0, 1), (1, 0, 0)), ((-1.1, 1.0, -1.1), (1, 0, 0), (0, 0, 1)),     # y
                              ((-1.1, -1.1, -1.0), (1, 0, 0), (0, 1, 0)), ((-1.1, -1.1, 1.0), (0, 1, 0), (1, 0, 0))):    # z
        s.add_quad(corner, right, up, 2.2, 2.2, m)
    return gpu.DeviceScene(s.flatten())


def test_the_furnace_relit_round_by_round_is_the_geometric_series(gpu):
    """Band 0 over Y0 of every probe.  Round 1: every sample has the value e / 6 exactly, so only the summation rounds -- 1e-5
    relative.  Later rounds, 5 %: a coefficient of band 1 or 2 has sampling noise v x 0.282 / sqrt(N), 0.44 % of v at N = 4096;
    through the factors 8 pi / 3 and pi that is about 2 % of G at one probe; fully correlated over the rounds it accumulates to
    rho x 2 % / (1 - rho) = 2 %; the bound is 2.5 x that worst case (opposite walls cancel most of it).
    Measured on MI355X: round 1 off by 3.4e-7; 8 rounds -0.49 % .. +0.28 % from the series, 1.9825 .. 1.9978 x round 1; 6 rounds
    -0.49 % .. +0.04 % from the path tracer's band 0 (1.96875, the series' own value)."""
    rho, e, N, Y0 = 0.5, 6.0, 4096, 0.2820948
    dev = furnace_scene(gpu, rho, e)
    box, counts = ((-1, -1, -1), (1, 1, 1)), (2, 2, 2)
    grid = gpu.probe_grid(*box, *counts)
    rays = qr.make_rays(grid[:, 0:3], unit(np.random.default_rng(1).standard_normal((8, 3))))
    assert (bits(dev.trace_rays(rays, "closest"))[:, gpu.HIT_KIND] == gpu.KIND_SQUARE).all()
    band0 = {}
    for K in (1, 6, 8):
        with gpu.ProbeVolume(*box, *counts) as vol:
            assert vol.relight(dev, N, K - 1) is vol  # K - 1 rounds into the volume, the K-th gathered here
            c = dev.probes_lit(on_gpu(grid), vol, N, first_sample=(K - 1) * N).cpu().numpy()
            band0[K] = c[:, 0, :].astype(np.float64) / Y0
    d1 = np.abs(band0[1] - e / 6).max() / (e / 6)
    d8 = (band0[8] - pl.furnace(e, rho, 8)) / pl.furnace(e, rho, 8)
    path = dev.probes(grid, N)[:, 0, :].astype(np.float64) / Y0
    d6 = (band0[6] - path) / path
    print(f"round 1: largest relative deviation from e / 6: {d1:.3e}")
    print(f"8 rounds: deviation from the series {d8.min():+.4f} .. {d8.max():+.4f}; ratio to round 1 {(band0[8] / band0[1]).min():.4f} .. {(band0[8] / band0[1]).max():.4f}")
    print(f"6 rounds: deviation from the path tracer's band 0 {d6.min():+.4f} .. {d6.max():+.4f} (series {pl.furnace(e, rho, 6):.5f}, path {path.mean():.5f})")
    assert d1 <= 1e-5
    assert np.abs(d8).max() <= 0.05 and (band0[8] > 1.9 * band0[1]).all()
    assert np.abs(d6).max() <= 0.05


# ------------------------------------------------------------------------------------ F. refusals, resources, the command line
def test_the_refusals_that_need_a_volume_come_in_the_headers_order(gpu):
    dev = gpu.device_lib()
    RAYS, KEYS, OUT = 0x1000, 0x3000, 0x2000

    def call(entry, vol, scene_h=None, rays=RAYS, keys=None, n=5, first=0, spp=8, flags=0, ef=0, bias=0.0, out=OUT):
        k = None if keys is None else C.c_void_p(keys)
        if entry == "hrt_probes_lit":
            rc = dev.hrt_probes_lit(scene_h, vol._h, C.c_void_p(rays), k, n, spp, 1, flags, ef, bias, C.c_void_p(out), None)
        else:
            rc = getattr(dev, entry)(scene_h, vol._h, C.c_void_p(rays), k, n, first, spp, 1, flags, ef, bias, C.c_void_p(out), None)
        return rc, dev.hrt_last_error().decode()

    every = dict(rays=0, keys=KEYS + 2, n=2 ** 31, spp=0, out=0)
    for entry, rn, on, align in (("hrt_trace_lit", "d_rays", "d_out", 16), ("hrt_probes_lit_device", "d_probes", "d_out", 16), ("hrt_probes_lit", "probes", "out", 4)):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as vol:
            assert call(entry, vol, ef=VISIBLE, bias=NAN, **every) == (HRT_ERR_INVALID, entry + ": the volume has no coefficients yet (hrt_probe_volume_update)")
            vol.update(np.zeros((2, 9, 3), F32))
            rc, msg = call(entry, vol, ef=VISIBLE | FACING, bias=NAN, **every)
            assert rc == HRT_ERR_INVALID and msg == entry + ": eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet (hrt_probe_volume_update_depth)"
            for bad in (NAN, INF, -INF):
                rc, msg = call(entry, vol, bias=bad, **every)
                assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": bias must be finite"), (bad, msg)
            vol.update_depth(np.zeros((2, 64, 3), F32))
            assert call(entry, vol, ef=VISIBLE, bias=NAN, **every)[1].startswith(entry + ": bias must be finite")
            assert call(entry, vol, ef=VISIBLE, **dict(every, n=0))[0] == 0, "an empty batch launches nothing"
            fixed = dict(every)
            assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: {rn} is NULL")
            fixed["rays"] = RAYS + align // 2
            assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: {rn} is not {align}-byte aligned")
            fixed["rays"] = RAYS
            assert "keys is not 4-byte aligned" in call(entry, vol, **fixed)[1]
            fixed["keys"] = KEYS
            if entry == "hrt_trace_lit":  # hrt_trace_radiance's order: the output, then the counts
                assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")
                fixed["out"] = OUT
                assert call(entry, vol, **fixed)[1].startswith(f"{entry}: n must be at most 2^31 - 1")
                fixed["n"] = 5
                assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: n_samples must be positive")
                assert "first_sample + n_samples must be at most 2^32" in call(entry, vol, **dict(fixed, first=2 ** 32 - 3, spp=4))[1]
            else:  # hrt_probes*' order: the counts, the limit, then the output
                assert call(entry, vol, **fixed)[1].startswith(f"{entry}: n must be at most 2^31 - 1")
                fixed["n"] = 2 ** 22 + 1
                assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: n_samples must be positive")
                fixed["spp"] = 64
                assert "HRT_PROBE_MAX_BLOCKS = 4194304 (got 4194305)" in call(entry, vol, **fixed)[1]
                fixed["n"] = 5
                assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: {on} is NULL")
                fixed["out"] = OUT + 2
                assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: {on} is not 4-byte aligned")
                fixed["out"] = OUT
            fixed["spp"] = 8
            assert call(entry, vol, **fixed) == (HRT_ERR_INVALID, f"{entry}: scene is NULL")


def test_lit_calls_give_back_what_they_took(gpu):
    import torch
    torch.cuda.synchronize()
    before = gpu.live_resources()
    dev = furnace_scene(gpu)
    held = gpu.live_resources()
    vol = gpu.ProbeVolume((-1, -1, -1), (1, 1, 1), 2, 2, 2)
    assert gpu.live_resources()[0] == held[0] + 1
    grid = gpu.probe_grid((-1, -1, -1), (1, 1, 1), 2, 2, 2)
    vol.relight(dev, 65, 2, keep=0.5, depth_rmax=1.5, eval_flags=VISIBLE)
    torch.cuda.synchronize()
    # the volume's moments, the scene's depth blocks and its lit blocks; relight's own tensors are torch's
    assert gpu.live_resources()[0] == held[0] + 4 and gpu.live_resources()[1:] == held[1:]
    rays = qr.make_rays(grid[:, 0:3], unit(np.ones((8, 3))))
    assert dev.trace_lit(rays, vol, 2, eval_flags=VISIBLE).all() and dev.probes_lit(grid, vol, 65).any()
    vol.blend(np.ones((8, 9, 3), F32), 0.5)
    assert gpu.live_resources()[0] == held[0] + 4, "the blocking forms free what they stage"
    vol.close()
    vol.close()
    dev.close()
    assert gpu.live_resources() == before


def cli(tmp_path, extra, spp):
    path = tmp_path / "out.ppm"
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "8", "--h", "8",
                        "--probe-grid", "2,2,1", "--probe-box", "-1.0,-1.0,-1.0,1.0,1.0,1.0", "--spp", str(spp), "--out", str(path)] + extra,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return path.read_bytes()


@pytest.mark.parametrize("keep", [None, 0.5])
def test_the_cli_writes_the_relit_lightmap_the_library_computes(gpu, tmp_path, keep):
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 65, (2, 2, 1)
    got = cli(tmp_path, ["--probe-quad", "0", "--probe-bounces", "2", "--probe-facing"] + ([] if keep is None else ["--probe-keep", str(keep)]), spp)
    _, desc, dev, _ = qr.build(gpu, "cornell_box", 8, 8)
    pts = gpu.quad_points(gpu.scene_quads(desc)[0], 8, 8, 1, 0.0, 0.0)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        one = vol.relight(dev, spp, 1, keep=keep or 0.0, eval_flags=FACING).eval(pts, facing=True)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        lightmap = vol.relight(dev, spp, 2, keep=keep or 0.0, eval_flags=FACING).eval(pts, facing=True)
    assert lightmap.any() and not np.array_equal(lightmap, one), "the second round adds a bounce"
    mine = tmp_path / "mine.ppm"
    gpu.write_ppm(str(mine), lightmap.reshape(8, 8, 3))
    assert got == mine.read_bytes()


def test_the_cli_writes_the_probe_lit_frame_the_library_computes(gpu, tmp_path):
    import torch
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 5, (2, 2, 1)
    got = cli(tmp_path, ["--probe-lit", "--probe-bounces", "2", "--probe-visible", "--probe-rmax", "1.25"], spp)
    _, desc, dev, cam = qr.build(gpu, "cornell_box", 8, 8)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        vol.relight(dev, spp, 2, eval_flags=VISIBLE, depth_rmax=1.25)
        acc = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
        for s in range(spp):
            dev.trace_lit(gpu.camera_rays(cam, 8, 8, s, 1), vol, 1, first_sample=s, seed=1, eval_flags=VISIBLE, out=acc, accumulate=True)
        unlit = dev.trace_radiance(gpu.camera_rays(cam, 8, 8, 0, 1), 1).cpu().numpy()
    sums = acc.cpu().numpy()  # linear: a volume of five samples per probe rings, and the gamma of a negative mean is NaN, as in a render
    assert np.isfinite(sums).all() and (sums != 0).mean() > 0.5 and not np.array_equal(sums, spp * unlit)
    gpu.finalize_tiles(acc.data_ptr(), 1, spp, gpu.FLAG_GAMMA, acc.data_ptr())
    frame = acc.cpu().numpy()
    mine = tmp_path / "mine.ppm"
    gpu.write_ppm(str(mine), frame.reshape(8, 8, 3))
    assert got == mine.read_bytes()
