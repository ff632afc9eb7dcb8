"""Light probes on the GPU (include/hrt.h "Light probes"): the rays of probes are the NumPy rule's (tests/probe_ref.py) within
PROBE_TOL, degenerate where it says; the fused call is, bit for bit, the header's fixed-order sum over the per-sample outputs of
hrt_probe_rays and hrt_trace_radiance (CONTRACT A) -- at the lane, wave and block edges, at the top of the sample range, with keys,
under the proof builds and as running sums; keys alone decide a probe's random numbers; waves take further items by grid stride;
the coefficients over a square emitter are the analytic ones; per-sample values follow the CPU oracle; a probe launch may run beside
a render of the same scene; the Python binding on torch and NumPy; and the command-line tool writes what the library computes.

The probes, unless said otherwise, are probe_ref.contract_probes(): a 3 x 2 x 2 grid inside the scene, a probe inside its glass
sphere (cornell_mesh, random_spheres) or inside a closed mesh (backrooms_pool's flamingo: tests/test_probe_ref.py shows that it
is), and two degenerate records (a NaN position, an infinite time)."""
import os
import subprocess

import numpy as np
import pytest

import bake_ref
import probe_ref
import radiance_oracle as ro
import test_gpu_radiance_oracle as orc
import test_gpu_rays as qr

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT, NO_LDS, GAMMA, WAVE = 64, 2, 1, 4
BLOCK = probe_ref.BLOCK
COUNTS = tuple(sorted({1, 63, 65, BLOCK, BLOCK + 1, 2 * BLOCK + 1}))
SMAX = max(COUNTS + (65 + BLOCK + 1,))  # the two ranges of the running sums fit too
bits = qr.bits

_built = {}


def scene(gpu, name):
    if name not in _built:
        _, desc, dev, cam = qr.build(gpu, name, 19, 11)
        _built[name] = (desc, dev, cam)
    return _built[name]


def on_gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).to("cuda")


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
def check_rays(got, probes, sample, seed, keys, what):
    tol = F32(probe_ref.PROBE_TOL)
    want, deg = probe_ref.rays(probes, sample, seed, keys)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got[:, 0:4]), bits(want[:, 0:4])), what  # {P, time} as given
    assert np.array_equal(bits(got[:, 7]), bits(want[:, 7])), what      # tmax = +inf
    got_deg = (got[:, 4:7] == 0).all(axis=1)
    assert np.array_equal(got_deg, deg), (what, np.flatnonzero(got_deg != deg)[:8].tolist())
    assert np.array_equal(bits(got[deg]), bits(want[deg])), what        # {P, time, 0, 0, 0, +inf} bit for bit, the NaN of P included
    if (~deg).any():
        err = np.abs(got[~deg][:, 4:7] - want[~deg][:, 4:7])
        print(f"{what}: max component difference {err.max():.3e} (PROBE_TOL {tol:.3e})")
        assert err.max() <= tol, (what, float(err.max()))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_probe_rays_follow_the_rule(gpu, n):
    import ctypes as C
    import torch
    for name in probe_ref.CONTRACT_SCENES:
        base = probe_ref.contract_probes(name)
        probes = np.ascontiguousarray(np.resize(base[::-1], (n, 4)))  # the degenerate records first, so that n = 1 is one of them
        for sample, seed in probe_ref.DRAWS:
            for keys in (None, bake_ref.keys_for(n)):
                sentinel = on_gpu(np.full((n + 2, 8), 7.0, F32))
                d_p, d_keys = on_gpu(probes), None if keys is None else on_gpu(keys)
                rc = gpu.device_lib().hrt_probe_rays(C.c_void_p(d_p.data_ptr()), None if keys is None else C.c_void_p(d_keys.data_ptr()), n, sample,
                                                     seed, C.c_void_p(sentinel.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0
                out = sentinel.cpu().numpy()
                assert (out[n:] == 7.0).all(), f"n = {n}: records written past the batch"
                check_rays(out[:n], probes, sample, seed, keys, (name, n, sample, keys is not None))
                assert np.array_equal(bits(gpu.probe_rays(d_p, sample, seed, d_keys).cpu().numpy()), bits(out[:n]))


# ---------------------------------------------------------------------------------------------------------------- 2. CONTRACT A
def series(gpu, dev, d_p, d_keys, first, S, seed, flags=0):
    """For samples first .. first + S - 1: the basis values of the device's own directions (hrt_probe_rays), the outputs of
    hrt_trace_radiance(first_sample = s, n_samples = 1, the same keys) on those records, and the degenerate mask."""
    import torch
    ds, vs = [], []
    for s in range(first, first + S):
        r = gpu.probe_rays(d_p, s, seed, d_keys)
        ds.append(r[:, 4:7])
        vs.append(dev.trace_radiance(r, spp=1, first_sample=s, seed=seed, keys=d_keys, flags=flags))
    d, v = torch.stack(ds).cpu().numpy(), torch.stack(vs).cpu().numpy()
    Y = np.stack([probe_ref.basis(x) for x in d])
    return Y, v, (d == 0).all(axis=2)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", probe_ref.CONTRACT_SCENES)
def test_fused_probes_are_the_fixed_order_sum_of_probe_rays_and_radiance_queries(gpu, name, exact):
    import torch
    seed, flags = 3, EXACT if exact else 0
    desc, dev, cam = scene(gpu, name)
    probes = probe_ref.contract_probes(name)
    n = len(probes)
    pdeg = probe_ref.probe_degenerate(probes)
    d_p = on_gpu(probes)
    for keys in (None, bake_ref.keys_for(n)):
        d_keys = None if keys is None else on_gpu(keys)
        for high in (False, True):
            start = 2 ** 32 - SMAX if high else 0
            Y, v, deg = series(gpu, dev, d_p, d_keys, start, SMAX, seed, flags)
            assert np.isfinite(v).all() and v.any() and np.array_equal(deg, np.tile(pdeg, (SMAX, 1)))
            for S in COUNTS:
                sl = slice(SMAX - S, SMAX) if high else slice(0, S)  # first_sample = 2^32 - S, or 0
                first = start + sl.start
                what = (name, exact, keys is not None, first, S)
                t = probe_ref.fold(Y[sl], v[sl], deg[sl])
                got = dev.probes(d_p, S, first_sample=first, seed=seed, keys=d_keys, flags=flags).cpu().numpy()
                assert got.shape == (n, 9, 3) and np.array_equal(bits(got), bits(t / F32(S))), what
                assert (bits(got[pdeg]) == 0).all(), what
            if high:
                continue
            # running sums over two ranges: out + t of each
            a, b = 65, BLOCK + 1
            base = np.random.default_rng(3).uniform(0, 2, (n, 9, 3)).astype(F32)
            acc = on_gpu(base)
            assert dev.probes(d_p, a, first_sample=0, seed=seed, keys=d_keys, flags=flags, out=acc, accumulate=True) is acc
            dev.probes(d_p, b, first_sample=a, seed=seed, keys=d_keys, flags=flags, out=acc, accumulate=True)
            want = (base + probe_ref.fold(Y[0:a], v[0:a], deg[0:a])) + probe_ref.fold(Y[a:a + b], v[a:a + b], deg[a:a + b])
            assert np.array_equal(bits(acc.cpu().numpy()), bits(want)), (name, exact, keys is not None, "running sums")
            if not exact:
                whole = dev.probes(d_p, SMAX, seed=seed, keys=d_keys).cpu().numpy()
                assert np.array_equal(bits(dev.probes(d_p, SMAX, seed=seed, keys=d_keys, flags=NO_LDS).cpu().numpy()), bits(whole))


def test_the_contract_scenes_select_both_builds(gpu):
    import ctypes as C
    lights = {}
    for name in probe_ref.CONTRACT_SCENES:
        desc, dev, cam = scene(gpu, name)
        lights[name] = C.cast(desc, C.POINTER(C.c_uint32 * 18)).contents[16] != 0  # hrt_scene_desc::n_lights
    assert any(lights.values()) and not all(lights.values()), lights


# ---------------------------------------------------------------------------------------------------------------------- 3. keys
def test_keys_alone_decide_the_random_numbers_of_a_probe(gpu):
    desc, dev, cam = scene(gpu, "cornell_mesh")
    probes = probe_ref.contract_probes("cornell_mesh")
    n, S = len(probes), BLOCK + 1
    plain = dev.probes(on_gpu(probes), S, seed=11).cpu().numpy()
    perm = np.random.default_rng(5).permutation(n).astype(U32)
    moved = dev.probes(on_gpu(probes[perm]), S, seed=11, keys=on_gpu(perm)).cpu().numpy()
    assert plain.any() and np.array_equal(bits(moved), bits(plain[perm]))
    twice = dev.probes(on_gpu(probes[[0, 0]]), S, seed=11, keys=on_gpu(np.array([0, 1000], U32))).cpu().numpy()
    assert np.array_equal(bits(twice[0]), bits(plain[0])) and not np.array_equal(bits(twice[0]), bits(twice[1]))


# --------------------------------------------------------------------------------------------------------- 4. beyond one grid
@pytest.mark.parametrize("name", ["random_spheres", "backrooms_pool"])
def test_waves_take_further_items_by_grid_stride(gpu, name):
    import torch
    desc, dev, cam = scene(gpu, name)
    probes = probe_ref.contract_probes(name)
    m = len(probes)
    # The launch is the workgroups that can be resident at once: at most 5 waves on each of a compute unit's 4 SIMDs, one item each.
    n = torch.cuda.get_device_properties(0).multi_processor_count * 20 + 7
    want = dev.probes(on_gpu(probes), 64, seed=4).cpu().numpy()
    idx = torch.arange(n, device="cuda") % m
    many = on_gpu(probes)[idx].contiguous()
    got = dev.probes(many, 64, seed=4, keys=idx.to(torch.int32))
    assert got.shape == (n, 9, 3) and torch.equal(got.view(torch.int32), on_gpu(want)[idx].view(torch.int32))
    assert want.any() and want[probe_ref.INSIDE].any()


# ------------------------------------------------------------------------------------------------------------------ 5. analytic
@pytest.mark.parametrize("seed,key", [(7, 0), (2 ** 63 + 5, 12345)])
def test_coefficients_over_a_square_emitter_are_the_analytic_ones(gpu, seed, key):
    """tests/test_gpu_bake.py's scene: a 2 x 2 emissive quad in the plane z = 0 whose lit side faces +z, a dark sky and nothing
    else; the probe is at (0, 0, 1).  A path that hits the emitter returns Le and ends, one that misses returns 0.  Seen from the
    probe the quad subtends 4 asin(1/2) = 2 pi / 3 (a face of the cube round the probe), so a uniform direction hits with
    p = 1/6: out[0] / (Y0 Le/6) is the hit fraction, a Bernoulli mean with standard error sqrt(p (1 - p) / n).  The mean of z over
    the hits: E[z hit] = -(1 / 4 pi) x the integral of cos(theta) over the quad's solid angle = -(pi F) / (4 pi) = -F / 4 with the form
    factor F = 0.554126 of that test; E[x hit] = E[y hit] = 0 by symmetry.  |x|, |y|, |z| <= 1, so the variance of each of those
    three is at most E[hit] = p and sqrt(p / n) bounds their standard errors.  A swapped axis or a wrong coefficient layout moves
    -F/4 = -0.1385 onto another coefficient, 21 standard errors away."""
    n = 4096
    F = 2 * (2 / np.pi) * (1 / np.sqrt(2)) * np.arctan(1 / np.sqrt(2))
    assert abs(F - 0.554126) < 1e-6 and abs(4 * np.arcsin(0.5) - 2 * np.pi / 3) < 1e-12
    p = 1 / 6
    se0, se1 = np.sqrt(p * (1 - p) / n), np.sqrt(p / n)
    s = gpu.HostScene()
    s.set_sky(True)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0,
               gpu.Material.make(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=6.0))
    dev = gpu.DeviceScene(s.flatten())
    P = (0.0, 0.0, 1.0)
    rec = dev.trace_rays(qr.make_rays([P], [(0.0, 0.0, -1.0)]), "shade")
    assert bits(rec)[0, gpu.HIT_KIND] == gpu.KIND_SQUARE and abs(rec[0, gpu.HIT_T] - 1.0) < 1e-5, "the ray straight down must hit the emitter"
    Le = rec[0, gpu.SHADE_EMISSION].astype(np.float64)
    assert (Le > 0).all()
    keys = np.array([key], U32)

    def check(hit_frac, zmean, ymean, xmean, who):
        print(f"{who} (seed, key) = ({seed}, {key}): hit fraction {hit_frac}, E[z hit] {zmean} (-F/4 = {-F / 4:.6f}), E[y hit] {ymean}, E[x hit] {xmean}")
        assert np.all(np.abs(np.asarray(hit_frac) - p) <= 5 * se0), who
        assert np.all(np.abs(np.asarray(zmean) + F / 4) <= 5 * se1), who
        assert np.all(np.abs(np.asarray(ymean)) <= 5 * se1) and np.all(np.abs(np.asarray(xmean)) <= 5 * se1), who

    # the NumPy rule's own directions first, so that a failing device is not blamed on the inputs
    d = np.concatenate([probe_ref.directions(seed, keys, k) for k in range(n)]).astype(np.float64)
    with np.errstate(all="ignore"):
        at = (-P[2] / d[:, 2])[:, None] * d[:, 0:2]
        hit = (np.abs(at) <= 1).all(axis=1) & (d[:, 2] < 0)
    check(hit.mean(), (d[:, 2] * hit).mean(), (d[:, 1] * hit).mean(), (d[:, 0] * hit).mean(), "NumPy")
    got = dev.probes(np.array([list(P) + [0.0]], F32), n, seed=seed, keys=keys)[0].astype(np.float64)
    c0, c1 = float(probe_ref.C0), float(probe_ref.C1)
    check(got[0] / (c0 * Le / 6), got[2] / (c1 * Le / 6), got[1] / (c1 * Le / 6), got[3] / (c1 * Le / 6), "device")


# -------------------------------------------------------------------------------------------------------------------- 6. oracle
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres", "backrooms_pool"])
def test_per_sample_values_on_probe_rays_follow_the_oracle(gpu, name):
    """12 probes x 3 samples on cornell_mesh and random_spheres; on backrooms_pool the probe inside the flamingo as well, whose
    first segments start inside a mesh."""
    sc, dev = orc.device(gpu, name, orc.LW, orc.LH)
    probes = probe_ref.contract_probes(name)[:13 if name == "backrooms_pool" else 12]
    d_p = on_gpu(probes)
    for s in range(3):
        rec = gpu.probe_rays(d_p, s, ro.SEED)
        got = dev.trace_radiance(rec, spp=1, first_sample=s, seed=ro.SEED).cpu().numpy()
        want, tie = ro.expected(sc, rec.cpu().numpy(), keys=None, first_sample=s, n_samples=1, seed=ro.SEED)
        orc.agree(got, want, f"{name} probe rays, sample {s} ({int(tie.sum())} tie rays)")


# ---------------------------------------------------------------------------------------------------------------- 7. concurrency
def test_probes_on_a_second_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    w, h, spp, seed = 480, 270, 8, 3
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", w, h)
    d_p = on_gpu(np.resize(probe_ref.contract_probes("cornell_mesh"), (64, 4)))
    S = BLOCK + 1
    tiles = gpu.tiles_total(w, h)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    want = dev.probes(d_p, S, seed=seed)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    got = torch.empty_like(want)
    torch.cuda.synchronize()
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        dev.probes(d_p, S, seed=seed, out=got)
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert want.any()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the probes beside a render"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside a probe launch"


# ------------------------------------------------------------------------------------------------------------------- 8. Python
def test_torch_and_numpy_paths_agree(gpu):
    import torch
    spp, seed = BLOCK + 3, 8
    desc, dev, cam = scene(gpu, "random_spheres")
    probes = probe_ref.contract_probes("random_spheres")
    n = len(probes)
    keys = bake_ref.keys_for(n)
    st = gpu.Stats()
    want = dev.probes(probes, spp, seed=seed, keys=keys, stats=st)
    assert isinstance(want, np.ndarray) and want.shape == (n, 9, 3) and want.dtype == F32 and want.any()
    assert st.samples == n * spp and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
    d_p, d_keys = on_gpu(probes), on_gpu(keys)
    out = torch.empty((n, 9, 3), dtype=torch.float32, device="cuda")
    got = dev.probes(d_p, spp, seed=seed, keys=d_keys, out=out)
    assert got is out and np.array_equal(bits(got.cpu().numpy()), bits(want))
    sums = np.zeros((n, 9, 3), F32)  # NumPy out: running sums through the host
    assert dev.probes(probes, spp, seed=seed, keys=keys, out=sums, accumulate=True) is sums
    assert np.array_equal(bits(sums / F32(spp)), bits(want))
    assert dev.probes(np.zeros((0, 4), F32), spp).shape == (0, 9, 3) and dev.probes(on_gpu(np.zeros((0, 4), F32)), spp).shape == (0, 9, 3)
    with pytest.raises(ValueError):
        dev.probes(d_p, spp, out=torch.empty((n, 27), device="cuda"))
    for flag, word in ((WAVE, "HRT_FLAG_WAVE_KERNEL"), (GAMMA, "HRT_FLAG_GAMMA"), (256, "HRT_RAYS_NORMALIZE")):
        with pytest.raises(gpu.HrtError, match=word):
            dev.probes(d_p, spp, flags=flag)


# ---------------------------------------------------------------------------------------------------------------------- 9. CLI
def test_the_cli_writes_the_file_the_library_computes(gpu, tmp_path):
    from conftest import PKG, ROOT
    lo, hi, spp = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 65
    path = tmp_path / "probes.txt"
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", "16", "--h", "16",
                        "--probe-grid", "2,2,1", "--probe-box", ",".join(str(x) for x in lo + hi), "--spp", str(spp), "--out", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = np.array([[float(x) for x in line.split()] for line in path.read_text().splitlines()])
    assert rows.shape == (4, 3 + 27)
    probes = gpu.probe_grid(lo, hi, 2, 2, 1)
    _, desc, dev, cam = qr.build(gpu, "cornell_box", 16, 16)
    want = dev.probes(probes, spp)  # the tool's seed is the library's default
    assert want.any()
    assert np.array_equal(bits(rows[:, 0:3].astype(F32)), bits(probes[:, 0:3]))  # %.9g round-trips fp32
    assert np.array_equal(bits(rows[:, 3:].astype(F32)), bits(want.reshape(4, 27)))
