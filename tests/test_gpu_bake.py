"""Baking on the GPU (include/hrt.h "Baking"): the rays of bake points are the NumPy rule's (tests/bake_ref.py) within BAKE_TOL,
degenerate where it says; the fused bake is the composition of hrt_bake_rays and hrt_trace_radiance bit for bit (CONTRACT A), in mean
and in accumulate mode, under the proof builds and with keys; keys alone decide a point's random numbers; lanes take further points
by grid stride; the irradiance under a square emitter is the analytic form factor; a lightmap end to end; a bake may run beside a
render of the same scene; and the Python binding on torch and NumPy.

The points, unless said otherwise, are bake_ref.contract_points(): the 19 x 11 SHADE hit points of the default camera's pixel-centre
rays with the SHADE normal, bias 1e-4, time 0 (computed by the CPU oracle and checked against the device here), and four hand-made
records after them (a NaN position, N = 0, N = (1e-20, 0, 0),
bias = -1)."""
import numpy as np
import pytest

import bake_ref
import test_gpu_rays as qr

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT, NO_LDS, GAMMA, WAVE = 64, 2, 1, 4
bits = qr.bits
W, H = bake_ref.W, bake_ref.H

_built = {}


def scene(gpu, name):
    """(desc, device scene, default camera) of a named scene at the contract frame, built once."""
    if name not in _built:
        _, desc, dev, cam = qr.build(gpu, name, W, H)
        _built[name] = (desc, dev, cam)
    return _built[name]


def hit_points(gpu, dev, cam, w, h):
    rays = qr.pixel_centre_rays(cam, w, h)
    return bake_ref.hit_points(rays, dev.trace_rays(rays, "shade"))


def on_gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).to("cuda")


@pytest.mark.parametrize("name", bake_ref.CONTRACT_SCENES)
def test_the_contract_points_are_the_devices_shade_hit_points(gpu, name):
    """bake_ref.contract_points(), which BAKE_TOL is derived from on the CPU, takes its hits from the oracle: they are the hit points
    and normals of hrt_trace_rays' SHADE records -- by value (a zero may differ in sign), but for an exact tie between two
    triangles of a mesh, which tests/test_gpu_rays.py allows the two walks to settle differently and holds to 1 in 100."""
    desc, dev, cam = scene(gpu, name)
    got = hit_points(gpu, dev, cam, W, H)
    want = bake_ref.contract_points(gpu, name)[:-4]
    same = (got == want).all(axis=1)
    print(f"{name}: {int((~same).sum())} of {len(want)} points differ")
    assert same.sum() >= len(want) - 2, (name, np.flatnonzero(~same)[:8].tolist())
    assert np.abs(got[:, 0:3] - want[:, 0:3]).max() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
def check_rays(got, pts, sample, seed, keys, what):
    tol = F32(bake_ref.BAKE_TOL)
    want, deg = bake_ref.rays(pts, sample, seed, keys)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got[:, 3]), bits(want[:, 3])), what   # time
    assert np.array_equal(bits(got[:, 7]), bits(want[:, 7])), what   # tmax = +inf
    got_deg = (got[:, 4:7] == 0).all(axis=1)
    assert np.array_equal(got_deg, deg), (what, np.flatnonzero(got_deg != deg)[:8].tolist())
    assert np.array_equal(bits(got[deg]), bits(want[deg])), what     # {P, time, 0, 0, 0, +inf} bit for bit, the NaNs of P included
    if (~deg).any():
        err = np.abs(got[~deg][:, [0, 1, 2, 4, 5, 6]] - want[~deg][:, [0, 1, 2, 4, 5, 6]])
        print(f"{what}: max component difference {err.max():.3e} (BAKE_TOL {tol:.3e})")
        assert err.max() <= tol, (what, float(err.max()))


@pytest.mark.parametrize("name", bake_ref.CONTRACT_SCENES)
def test_bake_rays_follow_the_rule(gpu, name):
    pts = bake_ref.contract_points(gpu, name)
    deg = bake_ref.point_degenerate(pts)
    assert deg[-4:].tolist() == [True, True, False, True] and (~deg).sum() >= 100  # N = (1e-20, 0, 0): see tests/test_bake_ref.py
    d_pts = on_gpu(pts)
    for sample, seed in bake_ref.DRAWS:
        for keys in (None, bake_ref.keys_for(len(pts))):
            got = gpu.bake_rays(d_pts, sample, seed, None if keys is None else on_gpu(keys)).cpu().numpy()
            check_rays(got, pts, sample, seed, keys, (name, sample, seed, keys is not None))


def test_bake_rays_at_the_wave_and_workgroup_edges_and_the_edges_of_the_degenerate_rule(gpu):
    base = np.concatenate([bake_ref.contract_points(gpu, "cornell_mesh"), bake_ref.edge_records()])
    sample, seed = bake_ref.DRAWS[1]
    for n in (1, 63, 64, 65, 257):
        pts = np.ascontiguousarray(np.resize(base[::-1], (n, 8)))  # the hand-made records first, so that n = 1 is one of them too
        keys = bake_ref.keys_for(n)
        sentinel = on_gpu(np.full((n + 2, 8), 7.0, F32))
        import ctypes as C
        import torch
        d_pts, d_keys = on_gpu(pts), on_gpu(keys)  # named: a temporary's memory goes back to the allocator, and to the next tensor
        rc = gpu.device_lib().hrt_bake_rays(C.c_void_p(d_pts.data_ptr()), C.c_void_p(d_keys.data_ptr()), n, sample, seed,
                                            C.c_void_p(sentinel.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        out = sentinel.cpu().numpy()
        assert (out[n:] == 7.0).all(), f"n = {n}: records written past the batch"
        check_rays(out[:n], pts, sample, seed, keys, f"n = {n}")
    edge = bake_ref.edge_records()
    got = gpu.bake_rays(on_gpu(edge), 3, 9).cpu().numpy()
    check_rays(got, edge, 3, 9, None, "edge records")
    assert ((got[:, 4:7] == 0).all(axis=1)).tolist() == [True] * 6 + [False, True]


# ---------------------------------------------------------------------------------------------------------------- 2. CONTRACT A
def composed(gpu, dev, d_pts, d_keys, first, S, seed, flags=0):
    """Per-sample outputs of hrt_bake_rays + hrt_trace_radiance (n_samples = 1, the same keys), summed in sample order in fp32."""
    import torch
    acc = torch.zeros((d_pts.shape[0], 3), dtype=torch.float32, device="cuda")
    for s in range(first, first + S):
        acc += dev.trace_radiance(gpu.bake_rays(d_pts, s, seed, d_keys), spp=1, first_sample=s, seed=seed, keys=d_keys, flags=flags)
    return acc.cpu().numpy()


@pytest.mark.parametrize("name", bake_ref.CONTRACT_SCENES)
def test_fused_bake_is_the_composition_of_bake_rays_and_radiance_queries(gpu, name):
    import torch
    S, seed = 5, 3
    desc, dev, cam = scene(gpu, name)
    pts = bake_ref.contract_points(gpu, name)
    deg = bake_ref.point_degenerate(pts)
    d_pts = on_gpu(pts)
    for keys in (None, bake_ref.keys_for(len(pts))):
        what = (name, keys is not None)
        d_keys = None if keys is None else on_gpu(keys)
        sums = composed(gpu, dev, d_pts, d_keys, 0, S, seed)
        assert np.isfinite(sums).all() and sums.any(), what
        assert (bits(sums[deg]) == 0).all(), what
        got = dev.bake(d_pts, S, seed=seed, keys=d_keys).cpu().numpy()
        assert got.shape == (len(pts), 3) and np.array_equal(bits(got), bits(sums / F32(S))), f"{what}: mean of samples [0, {S})"
        assert (bits(got[deg]) == 0).all(), f"{what}: a degenerate point must bake to 0"
        later = dev.bake(d_pts, S, first_sample=3, seed=seed, keys=d_keys, out=torch.full((len(pts), 3), 9.0, device="cuda")).cpu().numpy()
        assert np.array_equal(bits(later), bits(composed(gpu, dev, d_pts, d_keys, 3, S, seed) / F32(S))), f"{what}: mean of samples [3, {3 + S})"
        for splits in ((3, 1, 1), (1, 4)):
            acc = torch.zeros((len(pts), 3), device="cuda")
            acc[torch.from_numpy(deg).to("cuda")] = 7.0  # the sums of a degenerate point are left as they are
            first = 0
            for k in splits:
                assert dev.bake(d_pts, k, first_sample=first, seed=seed, keys=d_keys, out=acc, accumulate=True) is acc
                first += k
            acc = acc.cpu().numpy()
            assert np.array_equal(bits(acc[~deg]), bits(sums[~deg])), f"{what}: accumulated over {splits}"
            assert (acc[deg] == 7.0).all(), f"{what}: accumulated over {splits}: the sums of a degenerate point changed"
        exact = dev.bake(d_pts, S, seed=seed, keys=d_keys, flags=EXACT).cpu().numpy()
        assert np.array_equal(bits(exact), bits(composed(gpu, dev, d_pts, d_keys, 0, S, seed, flags=EXACT) / F32(S))), f"{what}: proof builds"
        assert np.array_equal(bits(dev.bake(d_pts, S, seed=seed, keys=d_keys, flags=NO_LDS).cpu().numpy()), bits(got)), f"{what}: NO_LDS_TREE"


def test_the_contract_scenes_select_both_builds(gpu):
    import ctypes as C
    lights = {}
    for name in bake_ref.CONTRACT_SCENES:
        desc, dev, cam = scene(gpu, name)
        lights[name] = C.cast(desc, C.POINTER(C.c_uint32 * 18)).contents[16] != 0  # hrt_scene_desc::n_lights
    assert any(lights.values()) and not all(lights.values()), lights


# ---------------------------------------------------------------------------------------------------------------------- 3. keys
def test_keys_alone_decide_the_random_numbers_of_a_point(gpu):
    desc, dev, cam = scene(gpu, "cornell_mesh")
    pts = bake_ref.contract_points(gpu, "cornell_mesh")
    n = len(pts)
    plain = dev.bake(on_gpu(pts), 3, seed=11).cpu().numpy()
    perm = np.random.default_rng(5).permutation(n).astype(U32)
    moved = dev.bake(on_gpu(pts[perm]), 3, seed=11, keys=on_gpu(perm)).cpu().numpy()
    assert np.array_equal(bits(moved), bits(plain[perm]))
    lit = int(np.argmax(plain.sum(axis=1)))
    twice = dev.bake(on_gpu(pts[[lit, lit]]), 3, seed=11, keys=on_gpu(np.array([lit, lit + 1000], U32))).cpu().numpy()
    assert np.array_equal(bits(twice[0]), bits(plain[lit])) and not np.array_equal(bits(twice[0]), bits(twice[1]))


# --------------------------------------------------------------------------------------------------------- 4. beyond one grid
def test_lanes_take_further_points_by_grid_stride(gpu):
    import torch
    desc, dev, cam = scene(gpu, "random_spheres")
    pts = bake_ref.contract_points(gpu, "random_spheres")
    m = len(pts)
    assert m == 213
    # The launch is the workgroups that can be resident at once: the bake kernels hold 96 VGPRs, so 5 waves on each of a compute
    # unit's 4 SIMDs, 1280 lanes per compute unit (DESIGN.md section 5 "Baking").
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 5 * 4 * 64
    n = max(400_000, resident + m)
    print(f"resident lanes {resident}, points {n}")
    assert n > resident
    want = dev.bake(on_gpu(pts), 1, seed=4).cpu().numpy()
    idx = torch.arange(n, device="cuda") % m
    many = on_gpu(pts)[idx].contiguous()
    got = dev.bake(many, 1, seed=4, keys=idx.to(torch.int32))
    assert torch.equal(got.view(torch.int32), on_gpu(want)[idx].view(torch.int32))
    assert want.any()


# ---------------------------------------------------------------------------------------------------- 5. analytic irradiance
@pytest.mark.parametrize("seed,key,numpy_off", [(7, 0, 0.49), (2 ** 63 + 5, 12345, 0.46)])
def test_irradiance_under_a_square_emitter_is_the_form_factor(gpu, seed, key, numpy_off):
    """A 2 x 2 emissive quad in the plane z = 0 whose lit side faces +z, a dark sky and nothing else; the point (0, 0, 1) looks down
    at its centre.  A path that hits the emitter returns Le and ends (albedo 0), one that misses returns 0, so 6 x bake / Le is the
    fraction of the cosine-weighted directions that hit: the form factor of the square seen from the point.  For a rectangle with one
    corner under the point, sides X, Y at distance 1, F = (1 / 2 pi) (X / sqrt(1 + X^2) atan(Y / sqrt(1 + X^2)) + Y / sqrt(1 + Y^2)
    atan(X / sqrt(1 + Y^2))); X = Y = 1 and four such corners give (2 / pi) (1 / sqrt 2) atan(1 / sqrt 2) x 2 = 0.554126.  The
    hits are Bernoulli(F): over 4096 samples the standard error is sqrt(F (1 - F) / 4096) = 0.00777."""
    n = 4096
    F = 2 * (2 / np.pi) * (1 / np.sqrt(2)) * np.arctan(1 / np.sqrt(2))
    assert abs(F - 0.554126) < 1e-6
    se = np.sqrt(F * (1 - F) / n)
    s = gpu.HostScene()
    s.set_sky(True)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0,
               gpu.Material.make(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=6.0))
    dev = gpu.DeviceScene(s.flatten())
    P, N = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    rec = dev.trace_rays(qr.make_rays([P], [N]), "shade")
    assert bits(rec)[0, gpu.HIT_KIND] == gpu.KIND_SQUARE and abs(rec[0, gpu.HIT_T] - 1.0) < 1e-5, "the ray from the point along N must hit the emitter"
    Le = rec[0, gpu.SHADE_EMISSION]
    assert (Le > 0).all()
    pt = bake_ref.records([P], [N], bias=0.0)
    keys = np.array([key], U32)
    # the NumPy rule's own hit fraction first, so that a failing device is not blamed on the inputs
    d = np.stack([bake_ref.rays(pt, k, seed, keys)[0][0, 4:7] for k in range(n)]).astype(np.float64)
    at = np.array(P)[None, 0:2] + (-P[2] / d[:, 2])[:, None] * d[:, 0:2]
    frac = ((np.abs(at) <= 1).all(axis=1) & (d[:, 2] < 0)).mean()
    off = abs(frac - F) / se
    print(f"(seed, key) = ({seed}, {key}): NumPy hit fraction {frac:.6f}, {off:.2f} standard errors from F = {F:.6f}")
    assert off <= 5 and abs(off - numpy_off) < 0.01
    got = dev.bake(pt, n, seed=seed, keys=keys)
    ratio = 6.0 * got[0].astype(np.float64) / Le.astype(np.float64)
    print(f"device: 6 x bake / Le = {ratio.tolist()}, {(np.abs(ratio - F) / se).max():.2f} standard errors from F")
    assert (np.abs(ratio - F) <= 5 * se).all(), (ratio.tolist(), F, se)
    back = dev.bake(bake_ref.records([P], [(0.0, 0.0, 1.0)], bias=0.0), n, seed=seed, keys=keys)
    assert (bits(back) == 0).all(), "with the normal reversed no direction reaches the emitter"


# ---------------------------------------------------------------------------------------------------- 6. lightmap end to end
def test_lightmap_of_the_floor_of_the_cornell_box(gpu):
    desc, dev, cam = scene(gpu, "cornell_mesh")
    quads = gpu.scene_quads(desc)
    up = [q for q in quads if bake_ref.quad_points(q.v0, q.v1, q.v3, 1, 1)[0, 5] > 0.99]
    assert len(up) == 1, "the floor is the one quad of the box whose lit side faces up"
    floor = up[0]
    pts = gpu.quad_points(floor, 8, 8)
    assert pts.shape == (64, 8) and np.array_equal(bits(pts), bits(bake_ref.quad_points(floor.v0, floor.v1, floor.v3, 8, 8)))
    assert not bake_ref.point_degenerate(pts).any()
    lightmap = dev.bake(pts, 4, seed=2)
    by_hand = dev.bake(on_gpu(pts), 4, seed=2).cpu().numpy()
    assert lightmap.shape == (64, 3) and np.array_equal(bits(lightmap), bits(by_hand))
    assert np.isfinite(lightmap).all() and (lightmap >= 0).all() and lightmap.any() and np.unique(lightmap, axis=0).shape[0] > 1  # not constant


# ---------------------------------------------------------------------------------------------------------------- 7. concurrency
def test_bake_on_a_second_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    w, h, spp, seed = 480, 270, 8, 3
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", w, h)
    pts = on_gpu(hit_points(gpu, dev, cam, w, h))
    tiles = gpu.tiles_total(w, h)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    want = dev.bake(pts, 2, seed=seed)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    got = torch.empty_like(want)
    torch.cuda.synchronize()
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        dev.bake(pts, 2, seed=seed, out=got)
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert want.any()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the bake beside a render"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside a bake"


# ------------------------------------------------------------------------------------------------------------------- 8. Python
def test_torch_and_numpy_paths_agree(gpu):
    import torch
    spp, seed = 3, 8
    desc, dev, cam = scene(gpu, "random_spheres")
    pts = bake_ref.contract_points(gpu, "random_spheres")
    keys = bake_ref.keys_for(len(pts))
    n = len(pts)
    st = gpu.Stats()
    want = dev.bake(pts, spp, seed=seed, keys=keys, stats=st)
    assert isinstance(want, np.ndarray) and want.shape == (n, 3) and want.dtype == F32 and want.any()
    assert st.samples == n * spp and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
    assert np.array_equal(bits(dev.bake(pts, spp, seed=seed, keys=keys.view(np.int32))), bits(want))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # baked and consumed on the side stream, no synchronisation in between
        d_pts, d_keys = on_gpu(pts), on_gpu(keys)
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        got = dev.bake(d_pts, spp, seed=seed, keys=d_keys, out=out)
        doubled_h = (got * 2).cpu().numpy()
        acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        dev.bake(d_pts, spp, seed=seed, keys=d_keys, out=acc, accumulate=True)
        acc_h = acc.cpu().numpy()
    assert got is out
    assert np.array_equal(bits(doubled_h / F32(2)), bits(want))
    assert np.array_equal(bits(acc_h / F32(spp)), bits(want))
    torch.cuda.current_stream().wait_stream(side)
    sums = np.zeros((n, 3), F32)  # NumPy out: running sums through the host
    assert dev.bake(pts, 2, seed=seed, keys=keys, out=sums, accumulate=True) is sums
    dev.bake(pts, 1, first_sample=2, seed=seed, keys=keys, out=sums, accumulate=True)
    assert np.array_equal(bits(sums), bits(acc_h))
    assert dev.bake(np.zeros((0, 8), F32), spp).shape == (0, 3) and dev.bake(on_gpu(np.zeros((0, 8), F32)), spp).shape == (0, 3)
    with pytest.raises(ValueError):
        dev.bake(d_pts, spp, out=torch.empty((n, 4), device="cuda"))
    for flag, name in ((WAVE, "HRT_FLAG_WAVE_KERNEL"), (GAMMA, "HRT_FLAG_GAMMA"), (256, "HRT_RAYS_NORMALIZE")):
        with pytest.raises(gpu.HrtError, match=name):
            dev.bake(d_pts, spp, flags=flag)
