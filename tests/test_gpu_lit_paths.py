"""Lit paths on the GPU (include/hrt.h "Lit paths").  Every comparison but the mirror's tail point and the furnace is on bits.

A. tail_after = 1 is today's lit ray where nothing specular is met first, and differs from it behind mirror and glass;
B. every K is its tails plus the volume's own look-up: trace_lit(tail_after=K) = a, or a + thr * G with the record from path_tails
   and G from the volume's eval / eval_visible on the record's first eight floats (tests/lit_paths_ref.py);
C. the tails are the integrator's: a path without a tail is trace_radiance's sample, a first diffuse hit is trace_rays("shade")'s, and
   the segment counts are what the CPU oracle's paths give;
D. a planar mirror, analytically;
E. the fused update is the fold of the query (tests/probe_ref.py);
F. the mirrored furnace: one wall of the closed room a perfect mirror -- with a tail the series is the diffuse room's, without one
   the probes lose exactly the solid angle of the mirror;
G. refusals that need a volume, resources, and the command-line tool."""
import ctypes as C

import numpy as np
import pytest

import bake_ref
import lit_paths_ref as lp
import oracle_lib
import probe_lit_ref as pl
import probe_ref
import radiance_oracle
import test_gpu_probe_depth as tpd
import test_gpu_probe_lit as tl
import test_gpu_rays as qr

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT = 64
HRT_ERR_INVALID = -1
NAN = float("nan")
FACING, VISIBLE = pl.FACING, pl.LIT_VISIBLE
bits = qr.bits
on_gpu = tpd.on_gpu
DEGENERATE = 62  # the degenerate ray of tl.tail_rays
SPECULAR_FIRST = {"cornell_mesh": 21, "random_spheres": 48}  # rays of tl.tail_rays whose first hit is mirror or glass


_cases = {}


def tail_case(gpu, name):
    """(device scene, camera, the 257 rays, their SHADE records as words, description): built once per scene."""
    if name not in _cases:
        _, desc, dev, cam = qr.build(gpu, name, 19, 11)
        rays = tl.tail_rays(gpu, cam, tl.TAIL_SCENES[name], 21)
        _cases[name] = (dev, cam, rays, bits(dev.trace_rays(rays, "shade")), desc)
    return _cases[name]


def first_hits(gpu, ru):
    """(hit, first hit diffuse, first hit mirror or glass) of SHADE records as words."""
    hit = ru[:, gpu.HIT_KIND] != gpu.KIND_MISS
    diffuse = hit & (ru[:, tl.SHADE_TYPE] == pl.DIFFUSE)
    return hit, diffuse, hit & ~diffuse


# --------------------------------------------------------------------------------------------------- A. K = 1 is today's lit ray
@pytest.mark.parametrize("name", sorted(tl.TAIL_SCENES))
def test_one_diffuse_hit_is_todays_lit_ray_where_nothing_specular_is_met_first(gpu, name):
    dev, _, rays, ru, _ = tail_case(gpu, name)
    n = len(rays)
    d_rays = on_gpu(rays)
    hit, diffuse, specular = first_hits(gpu, ru)
    assert specular.sum() == SPECULAR_FIRST[name] and diffuse.sum() > 50 and (~hit).sum() >= 5
    vol, _, _ = tl.random_volume(gpu, tl.TAIL_SCENES[name], 31)
    with vol:
        for ef in tl.EVAL_FLAGS:
            for bias in (0.0, 1e-3):
                for keys in (None, bake_ref.keys_for(n)):
                    d_keys = None if keys is None else on_gpu(keys)
                    what = (name, ef, bias, keys is not None)
                    want = dev.trace_lit(d_rays, vol, 1, first_sample=3, seed=9, keys=d_keys, eval_flags=ef, bias=bias).cpu().numpy()
                    got = dev.trace_lit(d_rays, vol, 1, first_sample=3, seed=9, keys=d_keys, eval_flags=ef, bias=bias, tail_after=1).cpu().numpy()
                    same = (bits(got) == bits(want)).all(axis=1)
                    assert same[~specular].all(), (what, np.flatnonzero(~same & ~specular)[:8].tolist())
                    assert (~same[specular]).any(), (what, "behind mirror and glass the chain is followed")
                    assert want[diffuse].any() and (bits(got[DEGENERATE]) == 0).all()


# ------------------------------------------------------------------------ B. every K is its tails plus the volume's own look-up
@pytest.mark.parametrize("K", [1, 2, 6])
@pytest.mark.parametrize("name", sorted(tl.TAIL_SCENES))
def test_every_tail_count_is_its_tail_records_plus_the_volumes_lookup(gpu, name, K):
    import torch
    dev, _, rays, ru, _ = tail_case(gpu, name)
    n, SMAX, seed = len(rays), 5, 9
    d_rays = on_gpu(rays)
    _, _, specular = first_hits(gpu, ru)
    vol, _, _ = tl.random_volume(gpu, tl.TAIL_SCENES[name], 31)
    with vol:
        for bias in (0.0, 1e-3):
            T = [dev.path_tails(rays, K, s, seed=seed, bias=bias) for s in range(SMAX)]
            pts, thr, seg, reached, a = lp.split(T[0])
            assert (bits(T[0][DEGENERATE]) == 0).all(), "a degenerate ray writes 16 zeros"
            assert (seg[np.arange(n) != DEGENERATE] >= 1).all() and (seg <= 6).all() and (pts[:, 7] == F32(bias))[reached].all()
            assert not bits(T[0][~reached][:, 0:11]).any(), "a path without a tail writes p = 0, n = 0, thr = 0"
            if K == 1:
                assert (reached & specular & (seg >= 2)).any(), "a tail reached after a mirror or glass hit"
            assert (~reached & (np.arange(n) != DEGENERATE)).any(), "a path that ends without a tail"
            for ef in tl.EVAL_FLAGS:
                look = vol.eval_visible if ef & VISIBLE else vol.eval
                v = np.stack([lp.sample_value(T[s], look(T[s][:, 0:8], facing=bool(ef & FACING))) for s in range(SMAX)])
                assert reached.any() or (name, K) == ("random_spheres", 6), "six diffuse hits in a row are rare under an open sky"
                assert np.isfinite(v).all() and (not reached.any() or not np.array_equal(v[0][reached], a[reached])), "the volume is in the value"
                what = (name, K, bias, ef)
                for b in tl.BATCHES:
                    sentinel = torch.full((b + 2, 3), 7.0, dtype=torch.float32, device="cuda")
                    got = dev.trace_lit(d_rays[:b].contiguous(), vol, 1, seed=seed, eval_flags=ef, bias=bias, out=sentinel[:b], tail_after=K)
                    torch.cuda.synchronize()
                    assert (sentinel[b:] == 7.0).all(), "results written past the batch"
                    g = got.cpu().numpy()
                    bad = np.flatnonzero((bits(g) != bits(v[0][:b])).any(axis=1))
                    assert bad.size == 0, (what, b, bad[:8].tolist(), g[bad[:2]].tolist(), v[0][bad[:2]].tolist())
                # three samples from sample 2, as a mean; then running sums over two calls
                got = dev.trace_lit(d_rays, vol, 3, first_sample=2, seed=seed, eval_flags=ef, bias=bias, tail_after=K).cpu().numpy()
                assert np.array_equal(bits(got), bits(pl.ray_output(v[2:5]))), (what, "three samples")
                base = np.random.default_rng(2).uniform(0, 2, (n, 3)).astype(F32)
                acc = on_gpu(base)
                assert dev.trace_lit(d_rays, vol, 2, seed=seed, eval_flags=ef, bias=bias, out=acc, accumulate=True, tail_after=K) is acc
                dev.trace_lit(d_rays, vol, 3, first_sample=2, seed=seed, eval_flags=ef, bias=bias, out=acc, accumulate=True, tail_after=K)
                want = pl.ray_output(v[2:5], base=pl.ray_output(v[0:2], base=base))
                want[DEGENERATE] = base[DEGENERATE]  # a degenerate ray leaves its sums as they are
                assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), (what, "running sums")
        # the proof builds trace the same paths the same way; keys and the torch form of path_tails
        same = (bits(dev.trace_rays(rays, "shade", EXACT)) == ru).all(axis=1)
        plain = dev.trace_lit(d_rays, vol, 1, seed=seed, eval_flags=FACING | VISIBLE, bias=1e-3, tail_after=K).cpu().numpy()
        exact = dev.trace_lit(d_rays, vol, 1, seed=seed, eval_flags=FACING | VISIBLE, bias=1e-3, flags=EXACT, tail_after=K).cpu().numpy()
        assert same.mean() > 0.9 and np.array_equal(bits(plain[same]), bits(exact[same]))
        Tp = dev.path_tails(d_rays, K, 0, seed=seed, bias=1e-3)
        Te = dev.path_tails(d_rays, K, 0, seed=seed, bias=1e-3, flags=EXACT)
        assert isinstance(Tp, torch.Tensor) and np.array_equal(bits(Tp.cpu().numpy()), bits(T[0]))
        assert np.array_equal(bits(Tp.cpu().numpy()[same]), bits(Te.cpu().numpy()[same]))
        keys = bake_ref.keys_for(n)
        Tk = dev.path_tails(rays, K, 1, seed=seed, keys=keys)
        got = dev.trace_lit(rays, vol, 1, first_sample=1, seed=seed, keys=keys, tail_after=K)
        assert np.array_equal(bits(got), bits(lp.sample_value(Tk, vol.eval(Tk[:, 0:8])))) and not np.array_equal(Tk, T[1])


# --------------------------------------------------------------------------------------------- C. the tails are the integrator's
@pytest.mark.parametrize("name", sorted(tl.TAIL_SCENES))
def test_a_path_without_a_tail_is_the_integrators_sample_and_a_first_diffuse_hit_is_the_shade_record(gpu, name):
    dev, _, rays, ru, _ = tail_case(gpu, name)
    n = len(rays)
    hit, diffuse, _ = first_hits(gpu, ru)
    rec = ru.view(F32)
    for K in (1, 2, 6):
        for s in (0, 4):
            T = dev.path_tails(rays, K, s, seed=9)
            _, _, _, reached, a = lp.split(T)
            want = dev.trace_radiance(rays, 1, first_sample=s, seed=9)
            assert (~reached).sum() >= 5 and np.array_equal(bits(a[~reached]), bits(want[~reached])), (name, K, s)
    T = dev.path_tails(rays, 1, 2, seed=9, bias=0.25)
    pts, thr, seg, reached, _ = lp.split(T)
    assert reached[diffuse].all() and (seg[diffuse] == 1).all() and not reached[~hit].any() and (seg[~hit & (np.arange(n) != DEGENERATE)] == 1).all()
    want = pl.point_records(rays[:, 0:3], rays[:, 4:7], rec[:, 0], rec[:, 4:7], rays[:, 3], 0.25)
    assert np.array_equal(bits(pts[diffuse]), bits(want[diffuse])), "p = o + t * d, the time, the shaded normal, the bias"
    assert np.array_equal(bits(thr[diffuse]), bits(rec[diffuse, 8:11])), "thr = 1 * albedo"


@pytest.mark.parametrize("name", ["random_spheres", "cornell_box"])
def test_segments_and_tails_are_those_of_the_oracles_paths(gpu, name):
    """The oracle's path of (ray, key, sample) as closest-hit queries (OracleScene.trace_ray_path), the material type of every hit
    from the scene's materials through trace_rays("shade") on those very segments, and lit_paths_ref.walk for what the rule does with
    them.  Meshless scenes: no triangle ties; the cap allows for a glass branch that flips on the last bit."""
    _, desc, dev, cam = qr.build(gpu, name, 19, 11)
    rays = tl.tail_rays(gpu, cam, tl.TAIL_SCENES.get(name, probe_ref.BOXES["cornell_mesh"][:2]), 21)
    n, seed = len(rays), 9
    oracle = oracle_lib.OracleScene(desc)
    live = [i for i in range(n) if i != DEGENERATE]
    for sample in (0, 3):
        rows = [oracle.trace_ray_path(rays[i], i, sample, seed) for i in live]
        flat = np.concatenate(rows)
        segs = qr.make_rays(flat[:, 0:3], flat[:, 3:6], flat[:, 6])
        su = bits(dev.trace_rays(segs, "shade"))
        agree = su[:, gpu.HIT_KIND] == flat[:, 7].astype(U32)
        types = [None if k == gpu.KIND_MISS else int(t) for k, t in zip(flat[:, 7].astype(U32), su[:, tl.SHADE_TYPE])]
        starts = np.cumsum([0] + [len(r) for r in rows])
        for K in (1, 2, 3, 6):
            _, _, seg, reached, _ = lp.split(dev.path_tails(rays, K, sample, seed=seed))
            bad, specular_tails = 0, 0
            for j, i in enumerate(live):
                path = types[starts[j]:starts[j + 1]]
                want = lp.walk(path, K)
                ok = agree[starts[j]:starts[j + 1]].all() and (int(seg[i]), bool(reached[i])) == want
                bad += not ok
                specular_tails += ok and want[1] and any(t in (1, 2) for t in path[:want[0]])
            print(f"{name}, sample {sample}, K = {K}: {bad} of {len(live)} rays disagree with the oracle's path (cap {radiance_oracle.tie_cap(n)}); "
                  f"{specular_tails} tails behind mirror or glass")
            assert bad <= radiance_oracle.tie_cap(n), (name, sample, K, bad)
            assert specular_tails > 0 or K > 1, (name, sample, K)


# ------------------------------------------------------------------------------------------------ D. a planar mirror, analytically
def test_a_planar_mirror_sends_the_tail_to_the_reflected_point(gpu):
    """A mirror quad in z = 0 (x, y in [-1, 1], facing +z) and a diffuse emitting wall in x = 2 (y in [-3, 3], z in [0, 6], facing
    -x) under a dark sky.  Rays from x <= -1, z > 0 towards points of the mirror: the reflection of direction d is (dx, dy, -dz), and it
    meets x = 2 at m + ((2 - mx) / dx) (dx, dy, -dz).  The tail point is within 1e-4 of that in float64: HRT_EPS = 1e-5 of origin
    offset at the bounce plus a few ulp (2.4e-7 each) of coordinates no larger than 4."""
    s = gpu.HostScene()
    s.set_sky(True)
    mirror, wall = (0.9, 0.8, 0.7), (0.6, 0.5, 0.4)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0, gpu.Material.make(albedo=mirror, type=gpu.MAT_MIRROR))
    s.add_quad((2.0, -3.0, 0.0), (0, 0, 1), (0, 1, 0), 6.0, 6.0,
               gpu.Material.make(albedo=wall, emissive=True, light_color=(1.0, 0.5, 0.25), light_intensity=3.0))
    dev = gpu.DeviceScene(s.flatten())
    rng = np.random.default_rng(4)
    n = 97
    m = np.stack([rng.uniform(0.2, 0.9, n), rng.uniform(-0.5, 0.5, n), np.zeros(n)], axis=1)           # dx >= 1.2, |dy| <= 1, |dz| <= 1:
    o = np.stack([rng.uniform(-1.5, -1.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 1.0, n)], axis=1)  # the wall is met at |y| <= 2, z <= 1.5
    d64 = (m - o) / np.linalg.norm(m - o, axis=1, keepdims=True)
    rays = qr.make_rays(o, d64)
    o32, d32 = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)  # the construction for the rays as the device reads them
    t0 = -o32[:, 2] / d32[:, 2]
    m64 = o32 + t0[:, None] * d32
    r = d32 * np.array([1.0, 1.0, -1.0])
    p64 = m64 + ((2.0 - m64[:, 0]) / r[:, 0])[:, None] * r
    assert (np.abs(p64[:, 1]) < 3).all() and (p64[:, 2] > 0).all() and (p64[:, 2] < 6).all() and np.abs(p64).max() <= 4
    first = bits(dev.trace_rays(rays, "shade"))
    assert (first[:, gpu.HIT_KIND] == gpu.KIND_SQUARE).all() and (first[:, tl.SHADE_TYPE] == gpu.MAT_MIRROR).all()
    for flags in (0, EXACT):
        pts, thr, seg, reached, a = lp.split(dev.path_tails(rays, 1, 5, seed=3, flags=flags))
        assert reached.all() and (seg == 2).all()
        want_thr = (F32(1) * np.asarray(mirror, F32)) * np.asarray(wall, F32)
        assert np.array_equal(bits(thr), bits(np.tile(want_thr, (n, 1)))), "thr = (1 * mirror albedo) * wall albedo in fp32"
        err = np.abs(pts[:, 0:3].astype(np.float64) - p64).max()
        print(f"flags {flags}: the tail point is within {err:.3e} of the reflection construction")
        assert err <= 1e-4
        assert np.array_equal(bits(pts[:, 4:7]), bits(np.tile(np.array([-1, 0, 0], F32), (n, 1)))) and a.all()
    # the one-segment lit ray sees nothing in the mirror; the lit path sees the wall, and the wall's tail
    box = ((-2, -3.5, -0.5), (2.5, 3.5, 6.5))
    vol, _, _ = tl.random_volume(gpu, box, 5)
    with vol:
        assert not dev.trace_lit(rays, vol, 1, first_sample=5, seed=3).any()
        T = dev.path_tails(rays, 1, 5, seed=3)
        got = dev.trace_lit(rays, vol, 1, first_sample=5, seed=3, tail_after=1)
        assert got.all() and np.array_equal(bits(got), bits(lp.sample_value(T, vol.eval(T[:, 0:8]))))


# --------------------------------------------------------------------------------- E. the fused update is the fold of the query
def lit_path_series(gpu, dev, vol, d_p, d_keys, first, S, seed, flags, ef, bias, K):
    """tl.lit_series with a tail: per sample the basis values of the device's own directions, the one-sample trace_lit(tail_after=K)
    outputs for those records, and the degenerate mask."""
    import torch
    ds, vs = [], []
    for s in range(first, first + S):
        r = gpu.probe_rays(d_p, s, seed, d_keys)
        ds.append(r[:, 4:7])
        vs.append(dev.trace_lit(r, vol, 1, first_sample=s, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags, tail_after=K))
    d, v = torch.stack(ds).cpu().numpy(), torch.stack(vs).cpu().numpy()
    return np.stack([probe_ref.basis(x) for x in d]), v, (d == 0).all(axis=2)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", sorted(tl.FOLD_BOXES))
def test_fused_lit_path_probes_are_the_fixed_order_fold_of_probe_rays_and_lit_paths(gpu, name, exact, K):
    seed, flags, ef, bias = 5, EXACT if exact else 0, FACING | VISIBLE, 1e-3
    _, desc, dev, _ = qr.build(gpu, name, 19, 11)
    probes, _ = tpd.CONTRACT[name]
    n = len(probes)
    d_p = on_gpu(probes)
    vol, _, _ = tl.random_volume(gpu, tl.FOLD_BOXES[name], 17)
    with vol:
        for keys in (None, bake_ref.keys_for(n)):
            d_keys = None if keys is None else on_gpu(keys)
            for first in (0, tl.FIRST):
                Y, v, deg = lit_path_series(gpu, dev, vol, d_p, d_keys, first, tl.SMAX_C, seed, flags, ef, bias, K)
                for S in tl.COUNTS_C:
                    what = (name, exact, K, keys is not None, first, S)
                    want = probe_ref.fold(Y[:S], v[:S], deg[:S]) / F32(S)
                    got = dev.probes_lit(d_p, vol, S, first_sample=first, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags, tail_after=K).cpu().numpy()
                    assert got.shape == (n, 9, 3) and np.array_equal(bits(got), bits(want)), what
                    assert (bits(got[2]) == 0).all() and (S < 64 or got[[0, 1, 3]].any()), what
                if first:
                    continue
                a, b = 65, 64  # running sums over two calls
                base = np.random.default_rng(3).uniform(0, 2, (n, 9, 3)).astype(F32)
                acc = on_gpu(base)
                assert dev.probes_lit(d_p, vol, a, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags, out=acc, accumulate=True, tail_after=K) is acc
                dev.probes_lit(d_p, vol, b, first_sample=a, seed=seed, keys=d_keys, eval_flags=ef, bias=bias, flags=flags, out=acc, accumulate=True, tail_after=K)
                want = (base + probe_ref.fold(Y[:a], v[:a], deg[:a])) + probe_ref.fold(Y[a:a + b], v[a:a + b], deg[a:a + b])
                assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), (name, exact, K, keys is not None, "running sums")
        # the NumPy path: blocking, with stats, the same bits; and the tail is in them
        st = gpu.Stats()
        Y, v, deg = lit_path_series(gpu, dev, vol, d_p, None, 0, 65, seed, flags, ef, bias, K)
        host = dev.probes_lit(probes, vol, 65, seed=seed, eval_flags=ef, bias=bias, flags=flags, stats=st, tail_after=K)
        assert isinstance(host, np.ndarray) and np.array_equal(bits(host), bits(probe_ref.fold(Y, v, deg) / F32(65)))
        assert st.samples == n * 65 and st.kernel_ms > 0
        if name == "cornell_mesh":  # single_sphere's probes see a mirror under a dark sky and nothing diffuse
            assert not np.array_equal(host, dev.probes_lit(probes, vol, 65, seed=seed, eval_flags=ef, bias=bias, flags=flags)), "one segment is another sum"


def test_waves_take_further_items_by_grid_stride(gpu):
    import torch
    _, desc, dev, _ = qr.build(gpu, "cornell_mesh", 19, 11)
    probes, _ = tpd.CONTRACT["cornell_mesh"]
    m = len(probes)
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 7  # more (probe, block) items than waves can be resident
    vol, _, _ = tl.random_volume(gpu, tl.FOLD_BOXES["cornell_mesh"], 17)
    with vol:
        want = dev.probes_lit(on_gpu(probes), vol, 65, seed=4, eval_flags=FACING, tail_after=2).cpu().numpy()
        idx = torch.arange(n, device="cuda") % m
        got = dev.probes_lit(on_gpu(probes)[idx].contiguous(), vol, 65, seed=4, keys=idx.to(torch.int32), eval_flags=FACING, tail_after=2)
        assert got.shape == (n, 9, 3) and want.any() and torch.equal(got.view(torch.int32), on_gpu(want)[idx].view(torch.int32))


# --------------------------------------------------------------------------------------------------------- F. the mirrored furnace
def mirrored_furnace(gpu, rho=0.5, e=6.0):
    """tl.furnace_scene with the x = -1 wall a mirror of albedo 1 that does not emit."""
    s = gpu.HostScene()
    s.set_sky(True)
    m = gpu.Material.make(albedo=(rho, rho, rho), emissive=True, light_color=(1, 1, 1), light_intensity=e)
    walls = (((-1.0, -1.1, -1.1), (0, 1, 0), (0, 0, 1)), ((1.0, -1.1, -1.1), (0, 0, 1), (0, 1, 0)),
             ((-1.1, -1.0, -1.1), (0, 0, 1), (1, 0, 0)), ((-1.1, 1.0, -1.1), (1, 0, 0), (0, 0, 1)),
             ((-1.1, -1.1, -1.0), (1, 0, 0), (0, 1, 0)), ((-1.1, -1.1, 1.0), (0, 1, 0), (1, 0, 0)))
    for k, (corner, right, up) in enumerate(walls):
        s.add_quad(corner, right, up, 2.2, 2.2, gpu.Material.make(albedo=(1, 1, 1), type=gpu.MAT_MIRROR) if k == 0 else m)
    return gpu.DeviceScene(s.flatten())


def mirror_fraction(p):
    """The fraction of the sphere that the part of the plane x = -1 inside the room, y and z in [-1, 1], subtends at p, in float64:
    the solid angle of a rectangle at height h over a corner-rectangle [0, a] x [0, b] is atan(a b / (h sqrt(a^2 + b^2 + h^2))),
    and the wall is the signed sum of four of them."""
    h = p[0] + 1.0
    corner = lambda a, b: np.arctan(a * b / (h * np.sqrt(a * a + b * b + h * h)))
    y0, y1, z0, z1 = -1.0 - p[1], 1.0 - p[1], -1.0 - p[2], 1.0 - p[2]
    return (corner(y1, z1) - corner(y0, z1) - corner(y1, z0) + corner(y0, z0)) / (4.0 * np.pi)


def test_the_mirrored_furnace_is_the_diffuse_rooms_series_with_a_tail_and_loses_the_mirror_without(gpu):
    """Band 0 over Y0 of every probe of a 2 x 2 x 2 grid on [-0.5, 0.5]^3 (no probe in a wall's plane), N = 4096.  With
    tail_after = 1 every sample of round 1 is e / 6 exactly -- a wall seen directly or in the mirror, albedo 1 -- so only the summation
    rounds (1e-5); a mirror changes no term of the series, so the bounds of the diffuse furnace carry over: 8 rounds within 5 % of
    (e / 6)(1 - rho^8) / (1 - rho) and above 1.9 x round 1 (tests/test_gpu_probe_lit.py derives them).  The one-segment probes_lit
    gathers nothing in the mirror: its round 1 over e / 6 is 1 - f, f the fraction of the sphere the mirror subtends at the probe
    (0.2111 at the four near probes, 0.0855 at the far ones); a sample sees the mirror or not, so the noise is binomial,
    sqrt(f (1 - f) / N) <= 0.0064, and +-0.02 is 3 sigma of that rounded up.
    Measured on MI355X: with a tail round 1 off by 3.4e-7, 8 rounds -0.24 % .. +0.06 % from the series and 1.9875 .. 1.9933 x round
    1; one segment within 0.0155 of 1 - f at every probe."""
    rho, e, N, Y0 = 0.5, 6.0, 4096, 0.2820948
    dev = mirrored_furnace(gpu, rho, e)
    box, counts = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), (2, 2, 2)
    grid = gpu.probe_grid(*box, *counts)
    band0 = {}
    for K in (1, 8):
        with gpu.ProbeVolume(*box, *counts) as vol:
            assert vol.relight(dev, N, K - 1, tail_after=1) is vol
            c = dev.probes_lit(on_gpu(grid), vol, N, first_sample=(K - 1) * N, tail_after=1).cpu().numpy()
            band0[K] = c[:, 0, :].astype(np.float64) / Y0
    d1 = np.abs(band0[1] - e / 6).max() / (e / 6)
    d8 = (band0[8] - pl.furnace(e, rho, 8)) / pl.furnace(e, rho, 8)
    print(f"with a tail, round 1: largest relative deviation from e / 6: {d1:.3e}")
    print(f"with a tail, 8 rounds: deviation from the series {d8.min():+.4f} .. {d8.max():+.4f}; ratio to round 1 {(band0[8] / band0[1]).min():.4f} .. {(band0[8] / band0[1]).max():.4f}")
    with gpu.ProbeVolume(*box, *counts) as vol:
        vol.update(np.zeros((8, 9, 3), F32))
        one = dev.probes_lit(grid, vol, N)[:, 0, :].astype(np.float64) / Y0 / (e / 6)
    f = np.array([mirror_fraction(p) for p in grid[:, 0:3].astype(np.float64)])
    far = grid[:, 0] > 0
    print(f"one segment, round 1 over e / 6: {one[:, 0].round(4).tolist()}; 1 - f: {(1 - f).round(4).tolist()}; largest difference {np.abs(one - (1 - f)[:, None]).max():.4f}")
    assert d1 <= 1e-5
    assert np.abs(d8).max() <= 0.05 and (band0[8] > 1.9 * band0[1]).all()
    assert far.sum() == 4 and (f[far] >= 0.085).all() and (f[~far] > f[far].max()).all()
    assert (np.abs(one - (1 - f)[:, None]) <= 0.02).all()


# ------------------------------------------------------------------------------------ G. refusals, resources, the command line
def test_the_refusals_that_need_a_volume_come_in_the_headers_order(gpu):
    dev = gpu.device_lib()
    RAYS, OUT = 0x1000, 0x2000

    def call(entry, vol, ef=0, bias=0.0, tail=1, n=5, rays=0):
        if entry == "hrt_probes_lit_paths":
            rc = dev.hrt_probes_lit_paths(None, vol._h, C.c_void_p(rays), None, n, 8, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        else:
            rc = getattr(dev, entry)(None, vol._h, C.c_void_p(rays), None, n, 0, 8, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        return rc, dev.hrt_last_error().decode()

    for entry, rn in (("hrt_trace_lit_paths", "d_rays"), ("hrt_probes_lit_paths_device", "d_probes"), ("hrt_probes_lit_paths", "probes")):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as vol:
            for bad in (0, 7):  # before the volume is looked at
                assert call(entry, vol, ef=1, bias=NAN, tail=bad) == (HRT_ERR_INVALID, f"{entry}: tail_after must be in 1 .. HRT_MAXBOUNCES = 6 (got {bad})")
            rc, msg = call(entry, vol, ef=1 | VISIBLE, bias=NAN)
            assert rc == HRT_ERR_INVALID and msg.startswith(entry + ": eval_flags: HRT_PROBE_EVAL_RADIANCE:"), msg
            assert call(entry, vol, ef=VISIBLE, bias=NAN) == (HRT_ERR_INVALID, entry + ": the volume has no coefficients yet (hrt_probe_volume_update)")
            vol.update(np.zeros((2, 9, 3), F32))
            rc, msg = call(entry, vol, ef=VISIBLE | FACING, bias=NAN)
            assert rc == HRT_ERR_INVALID and msg == entry + ": eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet (hrt_probe_volume_update_depth)"
            assert call(entry, vol, bias=NAN)[1].startswith(entry + ": bias must be finite")
            vol.update_depth(np.zeros((2, 64, 3), F32))
            assert call(entry, vol, ef=VISIBLE, n=0)[0] == 0, "an empty batch launches nothing"
            assert call(entry, vol, ef=VISIBLE) == (HRT_ERR_INVALID, f"{entry}: {rn} is NULL")
            assert call(entry, vol, ef=VISIBLE, rays=RAYS) == (HRT_ERR_INVALID, f"{entry}: scene is NULL")


def test_lit_path_calls_give_back_what_they_took(gpu):
    import torch
    torch.cuda.synchronize()
    before = gpu.live_resources()
    dev = tl.furnace_scene(gpu)
    held = gpu.live_resources()
    vol = gpu.ProbeVolume((-1, -1, -1), (1, 1, 1), 2, 2, 2)
    assert gpu.live_resources()[0] == held[0] + 1
    grid = gpu.probe_grid((-1, -1, -1), (1, 1, 1), 2, 2, 2)
    vol.relight(dev, 65, 2, keep=0.5, depth_rmax=1.5, eval_flags=VISIBLE, tail_after=2)
    torch.cuda.synchronize()
    # the volume's moments, the scene's depth blocks and its lit blocks; relight's own tensors are torch's
    assert gpu.live_resources()[0] == held[0] + 4 and gpu.live_resources()[1:] == held[1:]
    rays = qr.make_rays(grid[:, 0:3], tl.unit(np.ones((8, 3))))
    assert dev.trace_lit(rays, vol, 2, eval_flags=VISIBLE, tail_after=2).all() and dev.probes_lit(grid, vol, 65, tail_after=2).any()
    assert dev.path_tails(rays, 2).any() and dev.path_tails(on_gpu(rays), 2).any()
    assert gpu.live_resources()[0] == held[0] + 4, "the blocking forms free what they stage; a tail record call takes nothing"
    vol.close()
    dev.close()
    assert gpu.live_resources() == before


def test_the_cli_writes_the_lightmap_the_library_relights_with_a_tail(gpu, tmp_path):
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 65, (2, 2, 1)
    got = tl.cli(tmp_path, ["--probe-quad", "0", "--probe-bounces", "2", "--probe-facing", "--probe-tail", "1"], spp)
    plain = tl.cli(tmp_path, ["--probe-quad", "0", "--probe-bounces", "2", "--probe-facing"], spp)
    _, desc, dev, _ = qr.build(gpu, "cornell_box", 8, 8)
    pts = gpu.quad_points(gpu.scene_quads(desc)[0], 8, 8, 1, 0.0, 0.0)
    maps = []
    for tail in (1, None):
        with gpu.ProbeVolume(lo, hi, *counts) as vol:
            maps.append(vol.relight(dev, spp, 2, eval_flags=FACING, tail_after=tail).eval(pts, facing=True))
    assert maps[0].any() and not np.array_equal(maps[0], maps[1]), "cornell_box has a mirror and a glass sphere: the tail follows them"
    for name, lightmap, data in (("tail", maps[0], got), ("plain", maps[1], plain)):
        mine = tmp_path / (name + ".ppm")
        gpu.write_ppm(str(mine), lightmap.reshape(8, 8, 3))
        assert data == mine.read_bytes(), name


def test_the_cli_writes_the_lit_path_frame_the_library_computes(gpu, tmp_path):
    import torch
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 5, (2, 2, 1)
    got = tl.cli(tmp_path, ["--probe-lit", "--probe-tail", "1"], spp)
    _, desc, dev, cam = qr.build(gpu, "cornell_box", 8, 8)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        vol.update(dev.probes(gpu.probe_grid(lo, hi, *counts), spp, seed=1))  # without --probe-bounces the grid is path-traced
        acc, one = (torch.zeros((64, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        for s in range(spp):
            dev.trace_lit(gpu.camera_rays(cam, 8, 8, s, 1), vol, 1, first_sample=s, seed=1, out=acc, accumulate=True, tail_after=1)
            dev.trace_lit(gpu.camera_rays(cam, 8, 8, s, 1), vol, 1, first_sample=s, seed=1, out=one, accumulate=True)
    assert np.isfinite(acc.cpu().numpy()).all() and not torch.equal(acc, one)
    gpu.finalize_tiles(acc.data_ptr(), 1, spp, gpu.FLAG_GAMMA, acc.data_ptr())
    mine = tmp_path / "mine.ppm"
    gpu.write_ppm(str(mine), acc.cpu().numpy().reshape(8, 8, 3))
    assert got == mine.read_bytes()
