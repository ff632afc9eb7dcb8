"""Feature buffers (include/hrt.h hrt_render_features) against the CPU oracle's oracle_features, all 12 channels bit for bit: every
scene, several sample counts, sample indices near 2^32, seeds with high bits, odd and 256-multiple pixel counts, spot checks at
1080p and 4K, launches on several streams; and hrt_render_denoised against its parts."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from scene_util import describe_difference
from test_gpu_views import camera_from_inverse_modelview, trackball_inverse

pytestmark = pytest.mark.gpu

F32 = np.float32
SCENES = ["cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool", "single_sphere", "single_square", "mesh",
          "rt_in_a_weekend", "debug_refraction", "flamingo", "raccoon", "flamingo_pond", "flamingo_lake"]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def build(gpu, name, w, h):
    host = gpu.HostScene().setup(name, w / h, 1)
    desc = host.flatten()
    return host, desc, gpu.DeviceScene(desc), gpu.default_camera(w / h)


def check(got, ref, what):
    assert same_bits(got, ref), f"{what}: {describe_difference(got.reshape(-1, 1, 12), ref.reshape(-1, 1, 12))}"


@pytest.mark.parametrize("name", SCENES)
def test_every_channel_equals_the_oracle_on_every_scene(gpu, name):
    w, h, seed = 23, 13, 5
    _, desc, dev, cam = build(gpu, name, w, h)
    o = oracle_lib.OracleScene(desc)
    for n in (0, 1, 3, 8):
        check(dev.render_features(cam, w, h, 2, n, seed), o.features(cam, w, h, 2, n, seed), f"{name} n={n}")


@pytest.mark.parametrize("n", [1, 3, 8])
def test_sample_indices_near_two_to_the_32_and_seeds_with_high_bits(gpu, n):
    w, h = 19, 11
    _, desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    o = oracle_lib.OracleScene(desc)
    for first, seed in ((2 ** 32 - 1 - n, 1), (0, (0xDEADBEEF << 32) | 7), (2 ** 31 + 5, 0xFFFFFFFF00000000), (2 ** 32 - 1 - n, 2 ** 64 - 1)):
        check(dev.render_features(cam, w, h, first, n, seed), o.features(cam, w, h, first, n, seed), f"first {first} seed {seed:#x}")
    # the high seed bits change the samples
    a = dev.render_features(cam, w, h, 0, 1, 7)
    b = dev.render_features(cam, w, h, 0, 1, (1 << 32) | 7)
    assert not same_bits(a, b)


@pytest.mark.parametrize("w,h", [(1, 1), (15, 17), (255, 1), (256, 1), (257, 1), (1, 257), (16, 16), (17, 15)])
def test_odd_sizes_and_pixel_counts_around_256(gpu, w, h):
    _, desc, dev, cam = build(gpu, "random_spheres", w, h)
    o = oracle_lib.OracleScene(desc)
    for n in (0, 3):
        check(dev.render_features(cam, w, h, 1, n, 3), o.features(cam, w, h, 1, n, 3), f"{w}x{h} n={n}")


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_spot_checks_at_1080p_and_4k(gpu, w, h):
    _, desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    o = oracle_lib.OracleScene(desc)
    npix = w * h
    rng = np.random.default_rng(w)
    pick = np.unique(np.concatenate([[0, w - 1, npix - w, npix - 1, npix // 2], rng.integers(0, npix, 400)])).astype(np.uint32)
    for n in (0, 2):
        got = dev.render_features(cam, w, h, 4, n, 9).reshape(-1, 12)[pick]
        check(got, o.features(cam, w, h, 4, n, 9, pick), f"{w}x{h} n={n}")


# ---------------------------------------------------------------------------------------------------------------- streams
SW, SH, SN = 960, 540, 4


def _cams(gpu):
    host = gpu.HostScene().setup("cornell_mesh", SW / SH, 1)
    desc = host.flatten()
    return host, desc, gpu.default_camera(SW / SH), camera_from_inverse_modelview(gpu, trackball_inverse(20, 10), SW / SH)


def _alone(gpu, desc, cam, seed):
    return gpu.DeviceScene(desc).render_features(cam, SW, SH, 0, SN, seed)


def _launch(dev, cam, seed, buf, stream):
    dev._check(dev._lib.hrt_render_features(dev._h, C.byref(cam), SW, SH, 0, SN, seed,
                                            C.c_void_p(buf.data_ptr()), C.c_void_p(stream.cuda_stream)))


def test_feature_launches_with_two_cameras_on_two_streams(gpu):
    import torch
    host, desc, cam_a, cam_b = _cams(gpu)
    want_a, want_b = _alone(gpu, desc, cam_a, 11), _alone(gpu, desc, cam_b, 12)
    dev = gpu.DeviceScene(desc)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.zeros((SH, SW, 12), dtype=torch.float32, device="cuda")
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    _launch(dev, cam_a, 11, a, s1)
    _launch(dev, cam_b, 12, b, s2)
    torch.cuda.synchronize()
    assert same_bits(a.cpu().numpy(), want_a), "camera A on s1"
    assert same_bits(b.cpu().numpy(), want_b), "camera B on s2"


def test_feature_launches_a_b_a_on_one_stream(gpu):
    import torch
    host, desc, cam_a, cam_b = _cams(gpu)
    runs = ((cam_a, 11), (cam_b, 12), (cam_a, 13))
    want = [_alone(gpu, desc, c, s) for c, s in runs]
    dev = gpu.DeviceScene(desc)
    s1 = torch.cuda.Stream()
    bufs = [torch.zeros((SH, SW, 12), dtype=torch.float32, device="cuda") for _ in runs]
    torch.cuda.synchronize()
    for buf, (cam, seed) in zip(bufs, runs):
        _launch(dev, cam, seed, buf, s1)
    torch.cuda.synchronize()
    for k, (buf, ref) in enumerate(zip(bufs, want)):
        assert same_bits(buf.cpu().numpy(), ref), f"launch {k} ({'ABA'[k]})"


def test_a_feature_launch_beside_a_trace_launch_with_another_camera(gpu):
    import torch
    host, desc, cam_a, cam_b = _cams(gpu)
    want_f = _alone(gpu, desc, cam_b, 12)
    ref_dev = gpu.DeviceScene(desc)
    tiles = gpu.tiles_total(SW, SH)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    ref_dev.render_tiles(cam_a, SW, SH, 8, 11, 0, 0, 1, want_t.data_ptr(), 0)
    torch.cuda.synchronize()
    dev = gpu.DeviceScene(desc)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    f = torch.zeros((SH, SW, 12), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.render_tiles(cam_a, SW, SH, 8, 11, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    _launch(dev, cam_b, 12, f, s2)
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert same_bits(f.cpu().numpy(), want_f), "features of camera B beside a trace launch of camera A"
    assert same_bits(t.cpu().numpy(), want_t.cpu().numpy()), "trace launch of camera A beside features of camera B"


# ---------------------------------------------------------------------------------------------------------------- the whole call
@pytest.mark.parametrize("w,h", [(1, 1), (37, 23), (17, 1)])
def test_render_denoised_equals_its_parts_on_odd_sizes(gpu, w, h):
    import torch
    _, desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    spp, seed = 4, 3
    p = gpu.DenoiseParams(iterations=3)
    img, _ = dev.render(cam, w, h, spp, seed)
    for fspp in (spp, 0):
        for flags in (0, gpu.FLAG_GAMMA):
            whole = dev.render_denoised(cam, w, h, spp, fspp, seed, flags, p)
            f = torch.from_numpy(dev.render_features(cam, w, h, 0, fspp, seed)).cuda()
            c = torch.from_numpy(img).cuda()
            scratch = torch.empty(gpu.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
            out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
            gpu.denoise(c.data_ptr(), f.data_ptr(), w, h, p, flags, scratch.data_ptr(), out.data_ptr(), 0)
            torch.cuda.synchronize()
            parts = out.cpu().numpy()
            assert same_bits(whole, parts), f"{w}x{h} feature_spp {fspp} flags {flags}"
