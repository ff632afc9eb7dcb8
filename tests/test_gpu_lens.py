"""Lens cameras on the GPU (include/hrt.h "Lens cameras"): the pinhole's records are hrt_camera_rays' bit for bit; every projection's
rays are the NumPy rule's (tests/lens_ref.py) within RAY_TOL, degenerate where it says; the fused frame is the composition of
hrt_lens_rays and hrt_trace_radiance bit for bit (CONTRACT A) and, for the pinhole, hrt_render under every kernel form (CONTRACT B);
depth of field blurs what is out of focus by the radius geometry gives and leaves what is in focus alone; the lens features are
hrt_render_features' for the pinhole and the SHADE records' sums otherwise; a lens frame may run beside a render of the same scene;
and the Python binding on torch and NumPy."""
import numpy as np
import pytest

import lens_ref
import test_gpu_rays as qr
from scene_util import placed_camera

pytestmark = pytest.mark.gpu

F32 = np.float32
EXACT, BRUTE, NO_LDS, GAMMA = 64, 128, 2, 1
WAVE, STREAM, DUAL = 4, 8, 32
bits = qr.bits
CONTRACT_SCENES = ["cornell_mesh", "random_spheres", "backrooms_pool"]
W, H = 19, 11  # the contracts' frame

_built = {}


def scene(gpu, name):
    """(desc, device scene, default camera) of a named scene at the contracts' frame, built once."""
    if name not in _built:
        _, desc, dev, cam = qr.build(gpu, name, W, H)
        _built[name] = (desc, dev, cam)
    return _built[name]


def lenses(gpu, cam):
    """The pinhole and the lenses of lens_ref.CASES behind `cam`, by name."""
    out = {"pinhole": gpu.Lens(cam)}
    for name, (proj, ap, fo, ex) in lens_ref.CASES.items():
        out[name] = gpu.Lens(cam, proj, aperture=ap, focus=fo, extent=ex)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. the pinhole
@pytest.mark.parametrize("placement", [None, ((3.0, -2.0, 5.0), 2.0)])
def test_pinhole_lens_rays_are_the_camera_rays(gpu, placement):
    for w, h in ((37, 23), (1, 1), (65, 3)):
        cam = gpu.default_camera(w / h) if placement is None else placed_camera(gpu, w / h, *placement)
        for sample in (0, 2 ** 32 - 1):
            for seed in (1, 2 ** 64 - 1):
                got = gpu.lens_rays(gpu.Lens(cam, focus=float("nan")), w, h, sample, seed).cpu().numpy()
                want = gpu.camera_rays(cam, w, h, sample, seed).cpu().numpy()
                assert got.shape == (w * h, 8) and np.array_equal(bits(got), bits(want)), (placement, w, h, sample, seed)


# ------------------------------------------------------------------------------------------------------- 2. every projection
@pytest.mark.parametrize("name", list(lens_ref.CASES))
def test_lens_rays_follow_the_rule(gpu, name):
    tol = F32(lens_ref.RAY_TOL)
    for w, h in lens_ref.FRAMES:
        ref, lens = lens_ref.make(gpu, name, w, h)
        E = np.array(list(ref.cam.eye), F32)
        for sample, seed in lens_ref.DRAWS:
            got = gpu.lens_rays(lens, w, h, sample, seed).cpu().numpy()
            want, deg = lens_ref.rays(ref, w, h, sample, seed)
            what = (name, w, h, sample, seed)
            assert np.array_equal(bits(got[:, 3]), bits(want[:, 3])), what   # time
            assert np.array_equal(bits(got[:, 7]), bits(want[:, 7])), what   # tmax = +inf
            got_deg = (got[:, 4:7] == 0).all(axis=1)
            near = np.zeros(w * h, bool)
            if ref.projection == "fisheye":  # a sample the reference places within RAY_TOL of the rim may fall on either side
                near = np.abs(lens_ref.fisheye_radius(ref, w, h, sample, seed) - F32(1)) <= tol
                assert near.mean() <= 0.01, what
                assert deg.any() and not deg.all(), what
            assert np.array_equal(got_deg[~near], deg[~near]), what
            d = got_deg
            assert np.array_equal(bits(got[d, 0:3]), bits(np.tile(E, (int(d.sum()), 1)))), what  # {E, time, 0, 0, 0, +inf}
            assert (bits(got[d, 4:7]) == 0).all(), what
            both = ~got_deg & ~deg
            if ref.projection == "ortho":  # no transcendental step: bit for bit
                assert np.array_equal(bits(got), bits(want)), what
            else:
                err = np.abs(got[both][:, [0, 1, 2, 4, 5, 6]] - want[both][:, [0, 1, 2, 4, 5, 6]])
                print(f"{what}: max component difference {err.max():.3e} (RAY_TOL {tol:.3e})")
                assert err.max() <= tol, (what, float(err.max()))


# ---------------------------------------------------------------------------------------------------------------- 3. CONTRACT A
def composed(gpu, dev, lens, first, S, seed, flags=0):
    """Per-sample frames of hrt_lens_rays + hrt_trace_radiance (n_samples = 1, no keys), summed in sample order in fp32."""
    import torch
    acc = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    for s in range(first, first + S):
        acc += dev.trace_radiance(gpu.lens_rays(lens, W, H, s, seed), spp=1, first_sample=s, seed=seed, flags=flags)
    return acc.cpu().numpy().reshape(H, W, 3)


@pytest.mark.parametrize("name", CONTRACT_SCENES)
def test_fused_frame_is_the_composition_of_lens_rays_and_radiance_queries(gpu, name):
    import torch
    S, seed = 5, 3
    desc, dev, cam = scene(gpu, name)
    for lname, lens in lenses(gpu, cam).items():
        what = (name, lname)
        sums = composed(gpu, dev, lens, 0, S, seed)
        assert np.isfinite(sums).all() and sums.any(), what
        got = dev.render_lens(lens, W, H, S, seed)
        assert got.shape == (H, W, 3) and np.array_equal(bits(got), bits(sums / F32(S))), f"{what}: mean of samples [0, {S})"
        later = dev.render_lens(lens, W, H, S, seed, first_sample=3, out=torch.empty((H, W, 3), device="cuda")).cpu().numpy()
        assert np.array_equal(bits(later), bits(composed(gpu, dev, lens, 3, S, seed) / F32(S))), f"{what}: mean of samples [3, {3 + S})"
        for splits in ((3, 1, 1), (1, 4)):
            acc = torch.zeros((H, W, 3), device="cuda")
            first = 0
            for k in splits:
                dev.render_lens(lens, W, H, k, seed, first_sample=first, out=acc, accumulate=True)
                first += k
            assert np.array_equal(bits(acc.cpu().numpy()), bits(sums)), f"{what}: accumulated over {splits}"
        exact = dev.render_lens(lens, W, H, S, seed, flags=EXACT)
        assert np.array_equal(bits(exact), bits(composed(gpu, dev, lens, 0, S, seed, flags=EXACT) / F32(S))), f"{what}: proof builds"
        assert np.array_equal(bits(dev.render_lens(lens, W, H, S, seed, flags=NO_LDS)), bits(got)), f"{what}: NO_LDS_TREE"


def test_the_contract_frames_have_a_fisheye_rim_that_crosses_pixels(gpu):
    cam = gpu.default_camera(W / H)
    for name in ("fisheye180", "fisheye220"):
        proj, ap, fo, ex = lens_ref.CASES[name]
        ref = lens_ref.Lens(cam, proj, ap, fo, ex)
        outside = np.stack([lens_ref.fisheye_radius(ref, W, H, s, 3) > 1 for s in range(5)])
        mixed = outside.any(axis=0) & ~outside.all(axis=0)
        assert mixed.sum() >= 4 and outside.all(axis=0).any() and (~outside).all(axis=0).any()


# ---------------------------------------------------------------------------------------------------------------- 4. CONTRACT B
@pytest.mark.parametrize("name", CONTRACT_SCENES)
def test_pinhole_frame_is_the_render_under_every_kernel_form(gpu, name):
    S, seed = 5, 3
    desc, dev, cam = scene(gpu, name)
    lens = gpu.Lens(cam)
    for gamma in (0, GAMMA):
        got = dev.render_lens(lens, W, H, S, seed, flags=gamma)
        forms = 0
        for form in (WAVE, DUAL, STREAM):
            try:
                img, _ = dev.render(cam, W, H, S, seed, form | gamma)
            except gpu.HrtError as e:  # the streaming kernel refuses scenes whose tables exceed its LDS; that is its rule, not ours
                assert form == STREAM and "48 KiB" in str(e), str(e)
                continue
            forms += 1
            assert np.array_equal(bits(got), bits(img)), f"{name} gamma {gamma}: the lens frame differs from hrt_render form {form}"
        assert forms >= 2


# ------------------------------------------------------------------------------------------------------------ 5. depth of field
def test_depth_of_field_blurs_by_the_radius_geometry_gives(gpu):
    """An emissive square of side 1 (emission 6: a sample that hits it is exactly 6 / 6 = 1, its albedo 0 ends the path) facing the
    default camera at depth D = 4 under a dark sky, 64 x 64 at 32 spp, lens radius 0.2."""
    w = h = 64
    spp, seed, R, D = 32, 2, 0.2, 4.0
    cam = gpu.default_camera(1.0)
    s = gpu.HostScene()
    s.set_sky(True)
    z = float(cam.eye[2]) - D
    s.add_quad((-0.5, -0.5, z), (1, 0, 0), (0, 1, 0), 1.0, 1.0, gpu.Material.make(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=6.0))
    dev = gpu.DeviceScene(s.flatten())
    pin = dev.render_lens(gpu.Lens(cam), w, h, spp, seed)
    img, _ = dev.render(cam, w, h, spp, seed)
    assert np.array_equal(bits(pin), bits(img))
    pin = pin[:, :, 0]
    assert (pin == 1).sum() > 200 and (pin == 0).sum() > 2000
    edge = (pin != 0) & (pin != 1)
    excluded = np.zeros_like(edge)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            excluded[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= edge[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    assert excluded.mean() <= 0.10, excluded.mean()
    focused = dev.render_lens(gpu.Lens(cam, aperture=R, focus=D), w, h, spp, seed)
    assert np.array_equal(bits(focused[~excluded]), bits(np.repeat(pin[:, :, None], 3, axis=2)[~excluded])), "in focus, the frame changed away from the outline"
    # focused at F = 2: the circle of confusion at the square has radius b = R |D - F| / F world units
    Fd = 2.0
    px_per_unit = h / (2 * D * np.tan(np.radians(22.5)))
    b_px = R * abs(D - Fd) / Fd * px_per_unit
    assert 3.8 < b_px < 4.0
    half = 0.5 * px_per_unit
    yy, xx = np.mgrid[0:h, 0:w] + 0.5
    ax, ay = np.abs(xx - w / 2), np.abs(yy - h / 2)
    inside = (ax <= half) & (ay <= half)
    dist = np.where(inside, np.minimum(half - ax, half - ay), np.hypot(np.maximum(ax - half, 0), np.maximum(ay - half, 0)))  # to the outline
    blurred = dev.render_lens(gpu.Lens(cam, aperture=R, focus=Fd), w, h, spp, seed)[:, :, 0]
    far = dist > b_px + 1
    assert far[inside].any() and far[~inside].any()
    assert np.array_equal(bits(blurred[far]), bits(pin[far])), "out of focus, the frame changed beyond the blur radius"
    ring = (dist >= b_px / 2) & ~far
    assert (blurred[ring & ~inside] > 0).any(), "no light outside the square"
    assert (blurred[ring & inside] < 1).any(), "no darkening inside the square"


# ------------------------------------------------------------------------------------------------------------------ 6. features
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
def test_lens_features(gpu, name):
    seed = 5
    desc, dev, cam = scene(gpu, name)
    for first, n in ((0, 0), (2, 4)):
        want = dev.render_features(cam, W, H, first, n, seed)
        got = dev.render_lens_features(gpu.Lens(cam), W, H, first, n, seed)
        assert got.shape == (H, W, gpu.FEATURE_FLOATS) and np.array_equal(bits(got), bits(want)), f"{name}: pinhole features, n_samples {n}"
    first, n = 1, 4
    for lname in ("thin", "equirect", "fisheye180"):
        lens = lenses(gpu, cam)[lname]
        sums = np.zeros((W * H, gpu.FEATURE_FLOATS), F32)
        for s in range(first, first + n):
            rec = dev.trace_rays(gpu.lens_rays(lens, W, H, s, seed).cpu().numpy(), "shade")
            hit = bits(rec)[:, gpu.HIT_KIND] != 0
            add = np.zeros_like(sums)
            add[:, 0:3], add[:, 3:6], add[:, 6:9] = rec[:, gpu.SHADE_ALBEDO], rec[:, gpu.SHADE_NORMAL], rec[:, gpu.SHADE_EMISSION]
            add[:, 9], add[:, 10] = rec[:, gpu.HIT_T], 1.0
            sums[hit] = sums[hit] + add[hit]
        want = (sums / F32(n)).reshape(H, W, -1)
        got = dev.render_lens_features(lens, W, H, first, n, seed)
        assert want[:, :, 10].any(), (name, lname)
        assert np.array_equal(bits(got), bits(want)), f"{name} {lname}: features differ from the SHADE records' sums"
    # pixel centres (n_samples == 0): one ray per pixel, so a coverage of 0 or 1, and the sums of one sample undivided
    got = dev.render_lens_features(lenses(gpu, cam)["thin"], W, H, 0, 0, seed)
    assert np.isfinite(got).all() and np.isin(got[:, :, 10], (0.0, 1.0)).all() and got[:, :, 10].any()


# ---------------------------------------------------------------------------------------------------------------- 7. concurrency
def test_lens_frame_on_a_second_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    w, h, spp, seed = 480, 270, 8, 3
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", w, h)
    lens = gpu.Lens(cam, aperture=0.1, focus=4.0)
    tiles = gpu.tiles_total(w, h)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    want = dev.render_lens(lens, w, h, 2, seed, out=torch.empty((h, w, 3), device="cuda"))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    got = torch.empty_like(want)
    torch.cuda.synchronize()
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        dev.render_lens(lens, w, h, 2, seed, out=got)
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the lens frame beside a render"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside a lens frame"


# ------------------------------------------------------------------------------------------------------------------- 8. Python
def test_torch_and_numpy_paths_agree(gpu):
    import torch
    w, h, spp, seed = 64, 36, 3, 8
    _, desc, dev, cam = qr.build(gpu, "random_spheres", w, h)
    lens = gpu.Lens(cam, "equirect")
    st = gpu.Stats()
    want = dev.render_lens(lens, w, h, spp, seed, stats=st)
    assert isinstance(want, np.ndarray) and want.shape == (h, w, 3) and want.dtype == F32
    assert st.samples == w * h * spp and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # rendered and consumed on the side stream, no synchronisation in between
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        got = dev.render_lens(lens, w, h, spp, seed, out=out)
        doubled_h = (got * 2).cpu().numpy()
        acc = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        dev.render_lens(lens, w, h, spp, seed, out=acc, accumulate=True)
        acc_h = acc.cpu().numpy()
    assert got is out
    assert np.array_equal(bits(doubled_h / F32(2)), bits(want))
    assert np.array_equal(bits(acc_h / F32(spp)), bits(want))
    torch.cuda.current_stream().wait_stream(side)
    sums = np.zeros((h, w, 3), F32)  # NumPy out: running sums through the host
    assert dev.render_lens(lens, w, h, 2, seed, out=sums, accumulate=True) is sums
    dev.render_lens(lens, w, h, 1, seed, first_sample=2, out=sums, accumulate=True)
    assert np.array_equal(bits(sums), bits(acc_h))
    with pytest.raises(ValueError):
        dev.render_lens(lens, w, h, spp, seed, out=torch.empty((h, w, 4), device="cuda"))
    with pytest.raises(gpu.HrtError, match="HRT_FLAG_WAVE_KERNEL"):
        dev.render_lens(lens, w, h, spp, seed, flags=WAVE)
