"""Radiance queries on caller rays (include/hrt.h hrt_trace_radiance) and the render's camera rays (hrt_camera_rays), bit for bit:
camera rays against the oracle's camera and RNG stream, the contract (summed per-sample radiance of the camera rays == hrt_render
without gamma, under every kernel form, and within the parity tolerance of the oracle), accumulation and uneven splits, keys, the
shipped kernel against the proof builds on hard, edge and baking rays, the gradient sky of rays that leave the scene, degenerate
rays, normalisation, batches of 8 M rays, queries beside a render of the same scene, and the Python binding on torch and NumPy."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import test_gpu_parity as parity
import test_gpu_rays as qr
from scene_util import placed_camera

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
EXACT, BRUTE, NO_LDS = 64, 128, 2
WAVE, STREAM, DUAL = 4, 8, 32
bits = qr.bits


def radiance(dev, rays, **kw):
    return dev.trace_radiance(rays, **kw)


def cam_rays_np(gpu, cam, w, h, sample, seed):
    return gpu.camera_rays(cam, w, h, sample, seed).cpu().numpy()


def baking_rays(gpu, dev, cam, w, h, seed):
    """Cosine-hemisphere-like directions from the SHADE hit points of the pixel-centre rays, offset 1e-4 along the normal."""
    rays = qr.pixel_centre_rays(cam, w, h)
    rec = dev.trace_rays(rays, "shade")
    hit = bits(rec)[:, 1] != 0
    p = rays[hit, 0:3].astype(np.float64) + rec[hit, 0:1].astype(np.float64) * rays[hit, 4:7].astype(np.float64)
    n = rec[hit, 4:7].astype(np.float64)
    n = np.where((n * rays[hit, 4:7]).sum(1, keepdims=True) > 0, -n, n)  # face the incoming ray
    rng = np.random.default_rng(seed)
    d = qr.unit(n + qr.unit(rng.normal(size=n.shape)))
    return qr.make_rays(p + 1e-4 * n, d, rays[hit, 3])


# --------------------------------------------------------------------------------------------------------------- 1. camera rays
@pytest.mark.parametrize("placement", [None, ((3.0, -2.0, 5.0), 2.0), ((-1e3, 40.0, 7.0), 0.01)])
def test_camera_rays_equal_the_oracle_camera_and_rng_stream(gpu, placement):
    for w, h in ((37, 23), (1, 1), (65, 3), (8, 17)):
        cam = gpu.default_camera(w / h) if placement is None else placed_camera(gpu, w / h, *placement)
        for sample, seed in ((0, 1), (7, 2 ** 63 + 12345), (2 ** 32 - 1, 2 ** 64 - 1), (2 ** 32 - 2, 0xDEADBEEF00000000)):
            got = cam_rays_np(gpu, cam, w, h, sample, seed)
            draws = np.stack([oracle_lib.path_stream(seed, p, sample, 3) for p in range(w * h)])
            y, x = np.divmod(np.arange(w * h), w)
            uv = np.stack([(x.astype(F32) + draws[:, 0]) / F32(w), (y.astype(F32) + draws[:, 1]) / F32(h)], axis=1).astype(F32)
            cr = oracle_lib.camera_rays(cam, uv)
            want = qr.make_rays(cr[:, 0:3], cr[:, 3:6], draws[:, 2])
            assert np.array_equal(bits(got), bits(want)), (placement, w, h, sample, seed)


# ---------------------------------------------------------------------------------------------------------------- 2. contract
def summed_radiance(gpu, dev, cam, w, h, S, seed, flags=0):
    import torch
    acc = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    for s in range(S):
        acc += dev.trace_radiance(gpu.camera_rays(cam, w, h, s, seed), spp=1, first_sample=s, seed=seed, flags=flags)
    return (acc.cpu().numpy() / F32(S)).reshape(h, w, 3)  # IEEE division (torch may multiply by the reciprocal of a scalar)


@pytest.mark.parametrize("name", qr.SCENES)
def test_summed_radiance_of_camera_rays_is_the_render(gpu, name):
    w, h, seed = 19, 11, 3
    S = 4 + qr.SCENES.index(name) % 5
    _, desc, dev, cam = qr.build(gpu, name, w, h)
    got = summed_radiance(gpu, dev, cam, w, h, S, seed)
    forms = 0
    for form in (WAVE, DUAL, STREAM):
        try:
            img, _ = dev.render(cam, w, h, S, seed, form)
        except gpu.HrtError as e:  # the streaming kernel refuses scenes whose tables exceed its LDS; that is its rule, not ours
            assert form == STREAM and "48 KiB" in str(e), str(e)
            continue
        forms += 1
        assert np.array_equal(bits(got), bits(img)), f"{name} S={S}: summed radiance differs from hrt_render form {form}"
    assert forms >= 2
    img_exact, _ = dev.render(cam, w, h, S, seed, WAVE | EXACT)
    assert np.array_equal(bits(summed_radiance(gpu, dev, cam, w, h, S, seed, flags=EXACT)), bits(img_exact)), f"{name}: proof builds"
    ref = oracle_lib.OracleScene(desc).render(cam, w, h, S, seed=seed, threads=0)
    parity.assert_pixels_agree(got, ref, f"{name} summed radiance vs the oracle")


# ---------------------------------------------------------------------------------------------------- 3. accumulation, splits
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres", "backrooms_pool"])
def test_accumulated_splits_equal_one_call_and_the_mean(gpu, name):
    w, h, seed, S = 23, 13, 5, 7
    _, desc, dev, cam = qr.build(gpu, name, w, h)
    rays = np.concatenate([cam_rays_np(gpu, cam, w, h, 0, seed), baking_rays(gpu, dev, cam, w, h, 1)])
    n = len(rays)
    whole = radiance(dev, rays, spp=S, seed=seed, accumulate=True)
    mean = radiance(dev, rays, spp=S, seed=seed)
    assert np.array_equal(bits(mean), bits(whole / F32(S))), f"{name}: mean != sum / S"
    for splits in ((3, 1, 3), (1, 1, 1, 1, 1, 1, 1), (6, 1), (1, 6)):
        acc = np.zeros((n, 3), F32)
        first = 0
        for k in splits:
            radiance(dev, rays, spp=k, first_sample=first, seed=seed, out=acc, accumulate=True)
            first += k
        assert np.array_equal(bits(acc), bits(whole)), f"{name}: split {splits} differs from one call"
    # accumulate onto non-zero sums: the samples are added in order to what is there
    base = np.random.default_rng(2).uniform(0, 3, (n, 3)).astype(F32)
    acc = base.copy()
    radiance(dev, rays, spp=1, first_sample=0, seed=seed, out=acc, accumulate=True)
    assert np.array_equal(bits(acc), bits(base + radiance(dev, rays, spp=1, first_sample=0, seed=seed)))


# ------------------------------------------------------------------------------------------------------------------- 4. keys
def test_keys(gpu):
    w, h, seed = 23, 13, 9
    _, desc, dev, cam = qr.build(gpu, "random_spheres", w, h)
    rays = np.concatenate([cam_rays_np(gpu, cam, w, h, 0, seed), baking_rays(gpu, dev, cam, w, h, 2)])
    n = len(rays)
    plain = radiance(dev, rays, spp=2, seed=seed)
    assert np.array_equal(bits(plain), bits(radiance(dev, rays, spp=2, seed=seed, keys=np.arange(n, dtype=U32))))
    perm = np.random.default_rng(3).permutation(n)
    assert np.array_equal(bits(radiance(dev, rays[perm], spp=2, seed=seed, keys=perm.astype(U32))), bits(plain[perm]))
    # one ray, many keys: different, independent samples (a ray whose paths scatter diffusely: other keys give it other values)
    other = radiance(dev, rays, spp=2, seed=seed, keys=np.arange(n, 2 * n, dtype=U32))
    moved = np.flatnonzero((bits(other) != bits(plain)).any(axis=1))
    assert moved.size > n // 4, "keys do not change the samples"
    j = int(moved[moved.size // 2])
    one = np.repeat(rays[j][None], 256, axis=0)
    out = radiance(dev, one, spp=1, seed=seed, keys=np.arange(1000, 1256, dtype=U32))
    assert np.unique(bits(out), axis=0).shape[0] > 32, "keys do not give different samples"
    assert np.array_equal(bits(out[5]), bits(radiance(dev, rays[j][None], spp=1, seed=seed, keys=np.array([1005], U32))[0]))
    # key and batch position do not matter: the same (ray, key, sample) anywhere in batches of any size
    pick = [0, 17, n - 1]
    want = radiance(dev, rays[pick], spp=3, first_sample=11, seed=seed, keys=np.array(pick, U32))
    rng = np.random.default_rng(4)
    for size in (3, 64, 65, 1000, 70000):
        batch = rays[rng.integers(0, n, size)]
        keys = rng.integers(0, 2 ** 32, size, dtype=np.uint64).astype(U32)
        pos = rng.choice(size, 3, replace=False)
        batch[pos] = rays[pick]
        keys[pos] = pick
        got = radiance(dev, batch, spp=3, first_sample=11, seed=seed, keys=keys)
        assert np.array_equal(bits(got[pos]), bits(want)), size


# ---------------------------------------------------------------------------------------------------------- 5. proof builds
def assert_builds_agree(dev, rays, what, in_plane):
    base = bits(radiance(dev, rays, spp=2, seed=4))
    for flags in (EXACT, EXACT | BRUTE, NO_LDS, EXACT | NO_LDS):
        neq = (bits(radiance(dev, rays, spp=2, seed=4, flags=flags)) != base).any(axis=1)
        if flags & BRUTE:  # the two limits of the walk (DESIGN section 5 "Ray queries"), as in the query tests
            neq &= ~in_plane
        bad = np.flatnonzero(neq)
        assert bad.size == 0, f"{what} flags {flags}: {bad.size} of {len(rays)} differ, first rays {rays[bad[:2]].tolist()}"


@pytest.mark.parametrize("name", qr.SCENES)
def test_shipped_kernel_equals_the_proof_builds_on_hard_and_baking_rays(gpu, name):
    w, h = 37, 23
    _, desc, dev, cam = qr.build(gpu, name, w, h)
    hard, on_surface = qr.hard_rays(dev, cam, w, h, seed=len(name))
    bake = baking_rays(gpu, dev, cam, w, h, seed=len(name))
    rays = np.concatenate([hard, bake])
    in_plane = (rays[:, 4:7] == 0).any(axis=1) | np.concatenate([on_surface, np.zeros(len(bake), bool)])
    assert_builds_agree(dev, rays, name, in_plane)


def test_shipped_kernel_equals_the_proof_builds_on_edge_rays(gpu):
    host, quads, tet = qr.edge_scene(gpu)
    dev = gpu.DeviceScene(host.flatten())
    rays = qr.edge_rays(quads, tet, seed=1)
    assert_builds_agree(dev, rays, "edge scene", (rays[:, 4:7] == 0).any(axis=1))


# ---------------------------------------------------------------------------------------------------------------- 6. misses
def sky_scene(gpu, dark):
    s = gpu.HostScene()
    s.set_sky(dark)
    s.add_sphere((0.0, 0.0, 0.0), 1.0, gpu.Material.make(albedo=(0.5, 0.5, 0.5)))
    return s


def gradient_sky(d, spp):
    """sky(d, 6) / 6 (hrt_kernels.hip sky, Scene.h:149-161) summed over spp samples and divided, in fp32 as the device does it."""
    a = (0.5 * (d[:, 1].astype(np.float64) + 1.0)).astype(F32)
    k = (1.0 - a.astype(np.float64)).astype(F32)
    c = k[:, None] * F32(1) + (a[:, None] * np.array([0.5, 0.7, 1.0], F32)) * F32(7)
    rad = F32(0) + F32(1) * c
    s = np.zeros_like(rad)
    for _ in range(spp):
        s = s + rad / F32(6)
    return s / F32(spp)


def test_rays_that_leave_the_scene_see_the_sky(gpu):
    rng = np.random.default_rng(5)
    d = qr.unit(rng.normal(size=(4000, 3)))
    d[:, 2] = np.abs(d[:, 2]) + 1e-3  # away from the sphere
    o = np.tile([0.0, 0.0, 5.0], (len(d), 1))
    for scale in (1.0, 0.25, 3.0):  # non-unit directions read the sky with their own d.y
        rays = qr.make_rays(o, d * scale, rng.uniform(0, 1, len(d)))
        light = gpu.DeviceScene(sky_scene(gpu, False).flatten())
        for spp in (1, 3):
            got = radiance(light, rays, spp=spp, seed=2)
            assert np.array_equal(bits(got), bits(gradient_sky(rays[:, 4:7], spp))), (scale, spp)
        dark = gpu.DeviceScene(sky_scene(gpu, True).flatten())
        assert (bits(radiance(dark, rays, spp=2, seed=2)) == 0).all()


# ------------------------------------------------------------------------------------------------------------ 7. input handling
def test_degenerate_rays_normalisation_and_empty_batches(gpu):
    import torch
    w, h, seed = 23, 13, 6
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", w, h)
    good = cam_rays_np(gpu, cam, w, h, 0, seed)
    nan, inf = F32(np.nan), F32(np.inf)
    bad_rows = []
    for col in range(7):
        for v in (nan, inf, -inf):
            r = good[col].copy(); r[col] = v; bad_rows.append(r)
    for z in ((0, 0, 0), (-0.0, 0, -0.0)):
        r = good[5].copy(); r[4:7] = z; bad_rows.append(r)
    bad = np.array(bad_rows, F32)
    mixed = np.concatenate([good, bad])
    order = np.random.default_rng(1).permutation(len(mixed))
    mixed = mixed[order]
    is_bad = order >= len(good)
    keys = np.where(is_bad, 0, order).astype(U32)  # the good rays keep their own keys
    ref = radiance(dev, good, spp=2, seed=seed)
    for flags in (0, EXACT):
        got = radiance(dev, mixed, spp=2, seed=seed, keys=keys, flags=flags)
        assert (bits(got[is_bad]) == 0).all(), flags
        if flags == 0:
            assert np.array_equal(bits(got[~is_bad]), bits(ref[order[~is_bad]])), "good rays changed beside degenerate ones"
        base = np.random.default_rng(2).uniform(1, 2, (len(mixed), 3)).astype(F32)
        acc = base.copy()
        radiance(dev, mixed, spp=2, seed=seed, keys=keys, flags=flags, out=acc, accumulate=True)
        assert np.array_equal(bits(acc[is_bad]), bits(base[is_bad])), "a degenerate ray changed its sums"
    tiny = good[:4].copy(); tiny[:, 4:7] = F32(1e-30)  # degenerate only under normalisation
    assert (bits(radiance(dev, tiny, spp=1, seed=seed, normalize=True)) == 0).all()
    # HRT_RAYS_NORMALIZE == directions normalised by the device beforehand
    rng = np.random.default_rng(7)
    raw = np.concatenate([good, baking_rays(gpu, dev, cam, w, h, 3)])
    raw[:, 4:7] *= rng.choice([1e-3, 0.37, 3.0, 1e3], size=(len(raw), 1)).astype(F32) * rng.uniform(0.5, 2, (len(raw), 3)).astype(F32)
    pre = raw.copy()
    pre[:, 4:7] = gpu.debug_kat(gpu.KAT_NORMALIZE, raw[:, 4:7])
    assert np.array_equal(bits(radiance(dev, raw, spp=2, seed=seed, normalize=True)), bits(radiance(dev, pre, spp=2, seed=seed)))
    # n == 0: OK, nothing launched, the output untouched
    out = torch.full((16, 3), 7.0, device="cuda")
    r = torch.from_numpy(good[:4].copy()).cuda()
    lib = gpu.device_lib()
    for fl in (0, 512):
        assert lib.hrt_trace_radiance(dev._h, C.c_void_p(r.data_ptr()), None, 0, 0, 1, 1, fl, C.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert radiance(dev, np.zeros((0, 8), F32)).shape == (0, 3)


# ------------------------------------------------------------------------------------------------------ 8. scale, concurrency
def test_eight_million_rays_equal_the_same_rays_in_chunks(gpu):
    import torch
    w, h, seed = 1920, 1080, 2
    _, desc, dev, cam = qr.build(gpu, "backrooms_pool", w, h)
    rays = torch.cat([gpu.camera_rays(cam, w, h, s, seed) for s in range(4)])
    n = rays.shape[0]
    assert n == 4 * w * h
    full = dev.trace_radiance(rays, spp=1, seed=seed)
    keys = torch.arange(n, dtype=torch.int32, device="cuda")
    cuts = [0, 1, 1000003, 4 * w * h // 2 + 17, n]
    parts = [dev.trace_radiance(rays[a:b].contiguous(), spp=1, seed=seed, keys=keys[a:b].contiguous()) for a, b in zip(cuts, cuts[1:])]
    torch.cuda.synchronize()
    assert torch.equal(full.view(torch.int32), torch.cat(parts).view(torch.int32))
    assert bool(full.isfinite().all())


def test_radiance_on_a_second_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    w, h, spp, seed = 480, 270, 8, 3
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", w, h)
    rays = torch.cat([gpu.camera_rays(cam, w, h, 0, seed), torch.from_numpy(baking_rays(gpu, dev, cam, 64, 36, 1)).cuda()])
    tiles = gpu.tiles_total(w, h)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    want = dev.trace_radiance(rays, spp=2, seed=seed)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    torch.cuda.synchronize()
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        got = dev.trace_radiance(rays, spp=2, seed=seed)
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "radiance beside a render"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside radiance queries"


# ----------------------------------------------------------------------------------------------------------------- 9. Python
def test_torch_and_numpy_paths_agree_on_the_current_stream(gpu):
    import torch
    w, h, seed = 64, 36, 8
    _, desc, dev, cam = qr.build(gpu, "random_spheres", w, h)
    want = radiance(dev, cam_rays_np(gpu, cam, w, h, 2, seed), spp=3, first_sample=2, seed=seed)
    assert isinstance(want, np.ndarray) and want.shape == (w * h, 3) and want.dtype == F32
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # made, traced and consumed on the side stream, no synchronisation in between
        rays = gpu.camera_rays(cam, w, h, 2, seed)
        got = dev.trace_radiance(rays, spp=3, first_sample=2, seed=seed)
        doubled = got * 2
        acc = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
        dev.trace_radiance(rays, spp=3, first_sample=2, seed=seed, out=acc, accumulate=True)
        doubled_h, acc_h = doubled.cpu().numpy(), acc.cpu().numpy()  # copies ordered on the side stream behind the queries
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and got.shape == (w * h, 3)
    assert np.array_equal(bits(doubled_h / F32(2)), bits(want))
    assert np.array_equal(bits(acc_h / F32(3)), bits(want))
    torch.cuda.current_stream().wait_stream(side)
    keys = torch.arange(w * h, dtype=torch.int32, device="cuda")
    assert torch.equal(dev.trace_radiance(rays, spp=3, first_sample=2, seed=seed, keys=keys).view(torch.int32), got.view(torch.int32))
    with pytest.raises(ValueError):
        dev.trace_radiance(rays.double())
    with pytest.raises(ValueError):
        dev.trace_radiance(rays, keys=keys[:-1])
