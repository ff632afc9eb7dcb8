"""Batched views on the GPU (include/hrt.h hrt_render_views, hrt_render_views_device): frame v of one launch over N cameras is
bit for bit `DeviceScene.render` of camera v with seed v and the same flags.  Every comparison is np.array_equal on the float32
BITS (so a NaN would compare like any other value), frames are tiny, and the cases walk the boundaries of the item -> (view, tile)
mapping rather than pixels.

Base shape: 3 views of 21 x 13 pixels = 3 x 2 tiles per view with partial tiles on the right and at the bottom; 6 tiles per view is
a multiple of neither 16 nor 4, so the streaming kernel's grouped units straddle views.  The 18 items are fewer than the 256
workgroups, so the grid is 18 and launch_trace's arithmetic gives, for the streaming form (per_tile = 64 x min(spp, 1024) paths,
units of at most 8192 paths and 16 tiles; a band split only with one tile per unit, while items < 64 x grid and a band keeps
>= 4096 paths per fold):
    spp    1: 16 tiles per unit (views 0, 1 and 2 in the first unit)      spp    3: 16 tiles per unit
    spp   64:  2 tiles per unit                                           spp  128: 1 tile per unit, 2 row bands per tile
    spp  256:  4 row bands per tile                                       spp 1025: 4 row bands, folds of 512 samples: three folds,
                                                                                    the last of one sample (past HRT_SP_SCHUNK = 1024)
"""
import numpy as np
import pytest

from scene_util import describe_difference, many_spheres, many_squares, placed_camera

pytestmark = pytest.mark.gpu

W, H = 21, 13
SEEDS = (11, 2 ** 40 + 5, 3)  # three distinct seeds, one with high bits (seed_hi)
GAMMA, WAVE, STREAM = 1, 4, 8
FORMS = {"default": 0, "wave": WAVE, "stream": STREAM}


def orbited(gpu, cam, degrees, back=0.0):
    """cam turned by `degrees` about the world's up axis, then moved `back` along its own line of sight."""
    a = np.radians(degrees)
    c, s = np.cos(a), np.sin(a)
    out = gpu.Camera()
    for name in ("eye", "right", "up", "forward"):
        x, y, z = getattr(cam, name)
        getattr(out, name)[:] = (np.float32(c * x + s * z), y, np.float32(-s * x + c * z))
    for k in range(3):
        out.eye[k] = np.float32(out.eye[k] - back * out.forward[k])
    out.fovy_deg, out.aspect, out.znear, out.zfar = cam.fovy_deg, cam.aspect, cam.znear, cam.zfar
    return out


def three_cameras(gpu, aspect=W / H):
    cam = placed_camera(gpu, aspect)
    return [cam, orbited(gpu, cam, 25.0), orbited(gpu, cam, -40.0, back=1.5)]


SCENES = {
    "cornell_mesh": lambda gpu: gpu.HostScene().setup("cornell_mesh", W / H, 1),      # a mesh and lights: the streaming default
    "spheres_unlit": lambda gpu: many_spheres(gpu, 5, 0),                               # no mesh, no light: lane-per-pixel default below 8 spp
    "crowd_unlit": lambda gpu: many_spheres(gpu, 12, 0),                                # 8..128 spheres, no light: the unlit sphere-filter build
    "random_spheres": lambda gpu: gpu.HostScene().setup("random_spheres", W / H, 1),  # lights and the sphere-filter builds
    "moving": lambda gpu: many_squares(gpu, 20, 2),                                     # moving squares (a ray's time matters), two meshes, a light
}


@pytest.fixture(scope="module")
def scenes(gpu):
    made = {}

    def get(name):
        if name not in made:
            host = SCENES[name](gpu)
            made[name] = gpu.DeviceScene(host.flatten())
        return made[name]
    yield get
    for dev in made.values():
        dev.close()


@pytest.fixture(scope="module")
def single(scenes):
    """render() of one camera, computed once per (scene, camera, size, spp, seed, flags) and shared."""
    done = {}

    def get(name, cam, w, h, spp, seed, flags):
        key = (name, bytes(cam), w, h, spp, seed, flags)
        if key not in done:
            done[key] = scenes(name).render(cam, w, h, spp, seed, flags)[0]
            done[key].setflags(write=False)
        return done[key]
    return get


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_views(scenes, single, name, cams, seeds, w, h, spp, flags):
    frames = scenes(name).render_views(cams, w, h, spp, seeds=seeds, flags=flags)
    assert frames.shape == (len(cams), h, w, 3) and frames.dtype == np.float32
    for v, (cam, seed) in enumerate(zip(cams, seeds)):
        want = single(name, cam, w, h, spp, seed, flags)
        assert bits_equal(frames[v], want), f"{name} view {v} of {len(cams)}, {w}x{h}@{spp}, flags {flags}: " + describe_difference(frames[v], want)
    return frames


@pytest.mark.parametrize("spp", [1, 3, 64, 128, 256, 1025])
def test_every_unit_and_band_regime_of_the_streaming_form(gpu, scenes, single, spp):
    check_views(scenes, single, "cornell_mesh", three_cameras(gpu), SEEDS, W, H, spp, 0)  # (the regimes: module docstring)


@pytest.mark.parametrize("gamma", [0, GAMMA], ids=["linear", "gamma"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(SCENES))
def test_every_scene_kind_in_every_form(gpu, scenes, single, name, form, gamma):
    check_views(scenes, single, name, three_cameras(gpu), SEEDS, W, H, 3, FORMS[form] | gamma)


@pytest.mark.parametrize("name", ["spheres_unlit", "crowd_unlit", "random_spheres", "moving"])
def test_two_tiles_per_unit_and_band_splits_on_the_other_scenes(gpu, scenes, single, name):
    # 64 spp: the sphere-only scene moves to the streaming form (few tiles, >= 8 spp); 128: one tile per unit in two bands
    for spp in (64, 128):
        check_views(scenes, single, name, three_cameras(gpu), SEEDS, W, H, spp, 0)


@pytest.mark.parametrize("gamma", [0, GAMMA], ids=["linear", "gamma"])
@pytest.mark.parametrize("spp", [8, 64, 128])
def test_the_unlit_sphere_filter_build_by_default(gpu, scenes, single, spp, gamma):
    # 12 spheres and no light: at >= 8 spp the 18 tiles are "small and deep", so the default is the streaming form, which for 8..128
    # spheres is the build with the pair filter and without the lights code (hrt_wgstream_kernel_sph_views); the filter's margin is
    # per lane there.  8 spp: 16 tiles per unit, 64: 2, 128: two row bands.  (Forced with HRT_FLAG_STREAM_KERNEL at 3 spp in
    # test_every_scene_kind_in_every_form.)
    check_views(scenes, single, "crowd_unlit", three_cameras(gpu), SEEDS, W, H, spp, gamma)


def test_one_view_is_render(gpu, scenes, single):
    for form in FORMS.values():
        check_views(scenes, single, "cornell_mesh", three_cameras(gpu)[1:2], SEEDS[1:2], W, H, 3, form)


@pytest.mark.parametrize("spp", [2, 64])
def test_forty_views_of_one_tile_each(gpu, scenes, single, spp):
    # one tile per view: at 2 spp every streaming unit of 16 tiles holds 16 views; at 64 spp a unit holds two
    cam = placed_camera(gpu, 1.0)
    cams = [orbited(gpu, cam, 9.0 * v) for v in range(40)]
    for form in FORMS.values():
        check_views(scenes, single, "cornell_mesh", cams, list(range(100, 140)), 8, 8, spp, form)


def test_five_views_of_one_pixel(gpu, scenes, single):
    cam = placed_camera(gpu, 1.0)
    cams = [orbited(gpu, cam, 3.0 * v) for v in range(5)]
    for form in FORMS.values():
        check_views(scenes, single, "cornell_mesh", cams, [7, 7, 8, 9, 9], 1, 1, 4, form)


@pytest.mark.parametrize("spp", [3, 128])  # 128: the streaming form splits the two tiles into row bands
@pytest.mark.parametrize("w,h", [(1, 9), (9, 1)])
def test_one_column_and_one_row(gpu, scenes, single, w, h, spp):
    for form in FORMS.values():
        check_views(scenes, single, "cornell_mesh", [placed_camera(gpu, w / h)], [5], w, h, spp, form)


def test_the_seed_belongs_to_the_view(gpu, scenes, single):
    cam = three_cameras(gpu)[1]
    for form in FORMS.values():
        f = check_views(scenes, single, "cornell_mesh", [cam, cam, cam], [21, 22, 21], W, H, 3, form)
        assert not bits_equal(f[0], f[1]), "two seeds gave the same frame"
        assert bits_equal(f[0], f[2]), "the same camera and seed gave two frames"


@pytest.mark.parametrize("name", ["random_spheres", "moving"])
def test_eyes_at_different_distances_have_their_own_margins(gpu, scenes, single, name):
    # the filters' margin scale (err_abs) grows with |eye|: 2e-6 x (bound + |eye| + 1) differs by orders of magnitude here
    cam = placed_camera(gpu, W / H)
    cams = [orbited(gpu, cam, 10.0, back=900.0), cam, orbited(gpu, cam, -15.0, back=40.0)]
    for form in FORMS.values():
        check_views(scenes, single, name, cams, SEEDS, W, H, 3, form)


def test_launches_of_one_scene_do_not_disturb_each_other(gpu, scenes, single):
    dev, name = scenes("cornell_mesh"), "cornell_mesh"
    cams = three_cameras(gpu)
    a = dict(cams=cams, seeds=SEEDS, w=W, h=H, spp=3)
    b = dict(cams=[orbited(gpu, cams[0], 70.0), cams[2]], seeds=(9, 10), w=9, h=17, spp=64)
    alone = {k: dev.render_views(v["cams"], v["w"], v["h"], v["spp"], seeds=v["seeds"]) for k, v in (("a", a), ("b", b))}
    one = single(name, cams[1], 30, 10, 5, 77, 0)
    got_a = dev.render_views(a["cams"], a["w"], a["h"], a["spp"], seeds=a["seeds"])
    got_one = dev.render(cams[1], 30, 10, 5, 77)[0]
    got_b = dev.render_views(b["cams"], b["w"], b["h"], b["spp"], seeds=b["seeds"])
    got_a2 = dev.render_views(a["cams"], a["w"], a["h"], a["spp"], seeds=a["seeds"])
    assert bits_equal(got_a, alone["a"]) and bits_equal(got_a2, alone["a"]) and bits_equal(got_b, alone["b"]) and bits_equal(got_one, one)
    for v in range(2):
        assert bits_equal(got_b[v], single(name, b["cams"][v], 9, 17, 64, b["seeds"][v], 0))


def test_torch_output_stays_on_the_device(gpu, scenes, single):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    dev, cams = scenes("cornell_mesh"), three_cameras(gpu)
    want = dev.render_views(cams, W, H, 3, seeds=SEEDS, flags=GAMMA)
    out = torch.empty((3, H, W, 3), dtype=torch.float32, device="cuda")
    got = dev.render_views(cams, W, H, 3, seeds=SEEDS, flags=GAMMA, out=out)
    assert got is out
    dev.check_last_launch()  # HRT_OK after the device form (raises otherwise)
    assert bits_equal(out.cpu().numpy(), want)
    # two launches back to back on the stream, the second with other views: the staged view blocks of the first are not overwritten
    out2 = torch.empty((2, H, W, 3), dtype=torch.float32, device="cuda")
    dev.render_views(cams, W, H, 3, seeds=SEEDS, flags=GAMMA, out=out)
    dev.render_views(cams[::-1][:2], W, H, 3, seeds=SEEDS[::-1][:2], flags=GAMMA, out=out2)
    dev.check_last_launch()
    assert bits_equal(out.cpu().numpy(), want) and bits_equal(out2.cpu().numpy(), want[::-1][:2])
    for bad in (torch.empty((3, H, W, 4), dtype=torch.float32, device="cuda")[..., :3],       # not contiguous
                torch.empty((3, W, H, 3), dtype=torch.float32, device="cuda"),                # wrong shape
                torch.empty((2, H, W, 3), dtype=torch.float32, device="cuda"),                # wrong view count
                torch.empty((3, H, W, 3), dtype=torch.float64, device="cuda"),                # wrong dtype
                torch.empty((3, H, W, 3), dtype=torch.float32)):                              # not on the device
        with pytest.raises(ValueError, match="out must be"):
            dev.render_views(cams, W, H, 3, seeds=SEEDS, out=bad)
