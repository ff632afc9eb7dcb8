"""Parity of the HIP path (through the C ABI, libhrt.so) against the CPU oracle and the committed
golden pixels.  Run on the GPU box with `-m gpu`.

STATED TOLERANCE (fp32, fixed seed, linear pre-gamma pixels; DESIGN.md "Parity") -- set to what is OBSERVED on MI355X
(tools/observe_parity.py, 14 scenes x 3 sizes: worst |gpu - oracle| 7.2e-7 absolute, 2.7e-7 relative; AOVs identical):
  * the kernel evaluates every geometric / branch-deciding expression in the reference's fp32 operation order (its fp64
    islands included), so with the same per-path random numbers a path takes the same decisions and reaches the same
    hit points, bit for bit: first-hit AOVs (t, kind, object / triangle id, shading normal, albedo, emission) must be
    IDENTICAL on every pixel;
  * radiance is summed in throughput form instead of the recursion's inside-out order (1-2 ulp), so EVERY pixel must
    satisfy |gpu - oracle| <= 1e-6 * max(1, |oracle|) on all three channels.  There is no allowance for a fraction of
    diverged pixels: fp64 libm calls (acos / atan2 / asin / pow) are different implementations on the two sides and a
    tie that flips a branch would make one path diverge -- none has shown; if one ever does it gets a NAMED entry in
    LIBM_TIES below (scene, size, seed, pixel), not a looser bound;
  * integer work (RNG stream, hit kind / object / triangle ids, tile mapping) is bit-exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from scene_util import describe_difference, many_squares, same_nonfinite

pytestmark = pytest.mark.gpu

SCENES = {"cornell_box": (64, 64, 4), "cornell_mesh": (64, 36, 4), "random_spheres": (64, 36, 4), "mesh_in_box": (64, 36, 4),
          "backrooms_pool": (64, 36, 4)}


LIBM_TIES = {}  # (scene, w, h, spp, seed) -> [(y, x), ...]: pixels excused because a libm tie flipped a branch.  Empty: none observed.


def assert_pixels_agree(img, ref, what, rel=1e-6, excused=()):
    """Every pixel within rel * max(1, |ref|) on all channels (minus explicitly excused ones).  A value that is non-finite on
    exactly one side, or non-finite on both sides in different ways (NaN against inf, +inf against -inf), is a bad pixel:
    a plain |img - ref| > tol is False for a NaN and would let it through."""
    a, r = img.astype(np.float64), ref.astype(np.float64)
    both = np.isfinite(a) & np.isfinite(r)
    diff = np.abs(np.where(both, a, 0.0) - np.where(both, r, 0.0))
    bad = np.where(both, diff > rel * np.maximum(1.0, np.abs(np.where(both, r, 0.0))), ~same_nonfinite(a, r)).any(axis=2)
    for y, x in excused:
        bad[y, x] = False
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} pixels beyond {rel:g} "
                           f"({int((~both & ~same_nonfinite(a, r)).any(axis=2).sum())} of them non-finite on one side only or differently), "
                           f"worst finite |diff| {diff.max():.3g}, first at (y, x) {np.argwhere(bad)[:5].tolist()}")


def aov(gpu, dev, cam, w, h, which):
    lib = gpu.device_lib()
    lib.hrt_render_aov.argtypes = [C.c_void_p, C.POINTER(gpu.Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    out = np.empty((h, w, 3), np.float32)
    rc = lib.hrt_render_aov(dev._h, C.byref(cam), w, h, which, out.ctypes.data)
    assert rc == 0, lib.hrt_last_error()
    return out


def build(gpu, name, aspect, seed=1):
    host = gpu.HostScene().setup(name, aspect, seed)
    desc = host.flatten()
    return desc, gpu.DeviceScene(desc), gpu.default_camera(aspect)


def test_native_library_is_the_one_running(gpu):
    """libhrt.so is loaded in-tree and the trace kernel exists on this device (no fallback path)."""
    lib = gpu.device_lib()
    assert lib.hrt_device_count() >= 1
    st = gpu.Stats()
    assert lib.hrt_kernel_info(C.byref(st)) == 0 and st.vgprs > 0
    maps = open("/proc/self/maps").read()
    assert "hai719-raytracing_amd/libhrt.so" in maps


def test_rng_stream_bit_exact(gpu, oracle):
    lib = gpu.device_lib()
    lib.hrt_debug_path_stream.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    for seed, pixel, sample in [(1, 0, 0), (1, 2073599, 255), (0xDEADBEEFCAFE, 12345, 7), (2**64 - 1, 2**31 - 1, 1023)]:
        out = np.empty(512, np.float32)
        assert lib.hrt_debug_path_stream(seed, pixel, sample, 512, out.ctypes.data) == 0
        assert np.array_equal(out, oracle.path_stream(seed, pixel, sample, 512))


@pytest.mark.parametrize("name", list(SCENES))
def test_first_hit_aovs_match_oracle_and_golden(gpu, oracle, name):
    """Deterministic AOVs: the closest-hit object / triangle under every pixel centre is identical;
    t, shading normal (normal maps), albedo (textures, face colours) and emission agree to fp32 rounding."""
    w, h = 160, 90
    desc, dev, cam = build(gpu, name, w / h)
    ref = oracle.OracleScene(desc).aov(cam, w, h)
    hit = aov(gpu, dev, cam, w, h, 0)
    assert np.array_equal(hit, ref["hit"]), f"{name}: first hit (t, kind, id) differs on {int((hit != ref['hit']).any(axis=2).sum())} pixels"
    for k, key in ((1, "normal"), (2, "albedo"), (3, "emission")):
        got = aov(gpu, dev, cam, w, h, k)
        assert np.array_equal(got, ref[key]), f"{name} {key}: {int((got != ref[key]).any(axis=2).sum())} pixels differ"
    # committed golden AOVs (generated by the oracle in the build container)
    g = np.load(os.path.join(GOLDEN, "oracle_images.npz"))
    gw, gh, _, _ = (int(x) for x in g[name + "_shape"])
    desc2, dev2, cam2 = build(gpu, name, gw / gh)
    assert np.array_equal(aov(gpu, dev2, cam2, gw, gh, 0), g[name + "_aov_hit"])
    for k, key in ((1, "normal"), (2, "albedo"), (3, "emission")):
        assert np.array_equal(aov(gpu, dev2, cam2, gw, gh, k), g[f"{name}_aov_{key}"])


@pytest.mark.parametrize("name", list(SCENES))
def test_render_matches_oracle_and_golden(gpu, oracle, name):
    w, h, spp = SCENES[name]
    desc, dev, cam = build(gpu, name, w / h)
    img, st = dev.render(cam, w, h, spp, seed=1)
    assert np.isfinite(img).all()
    ref = oracle.OracleScene(desc).render(cam, w, h, spp, seed=1, threads=0)
    assert_pixels_agree(img, ref, name, excused=LIBM_TIES.get((name, w, h, spp, 1), ()))
    assert abs(img.mean() - ref.mean()) <= 1e-6 * max(1.0, abs(ref.mean()))
    g = np.load(os.path.join(GOLDEN, "oracle_images.npz"))
    assert_pixels_agree(img, g[name + "_render"], name + " (committed golden pixels)")
    # a different seed changes the image; the same seed reproduces it bit for bit
    again, _ = dev.render(cam, w, h, spp, seed=1)
    other, _ = dev.render(cam, w, h, spp, seed=2)
    assert np.array_equal(img, again) and not np.array_equal(img, other)


def test_lds_resident_and_global_nodelets_give_identical_pixels(gpu):
    desc, dev, cam = build(gpu, "mesh_in_box", 16 / 9)
    a, _ = dev.render(cam, 128, 72, 2, seed=3)
    b, _ = dev.render(cam, 128, 72, 2, seed=3, flags=gpu.FLAG_NO_LDS_TREE)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("name,w,h,spp", [("cornell_mesh", 200, 120, 5), ("backrooms_pool", 120, 67, 3), ("mesh_in_box", 61, 35, 300),
                                          ("random_spheres", 96, 54, 2), ("cornell_box", 8, 8, 64), ("cornell_mesh", 16, 8, 1100),
                                          ("flamingo", 100, 60, 40), ("cornell_mesh", 1920, 1080, 4), ("backrooms_pool", 1920, 1080, 2)])
def test_all_kernel_forms_give_identical_pixels(gpu, name, w, h, spp):
    """The workgroup-streaming kernel (default where bounces diverge), the one-pixel-per-lane kernel and the
    two-streams-per-lane kernel with its resumable KD walk schedule the same per-path arithmetic differently:
    every pixel must be bit-identical.  Sizes cover ragged tiles, an odd number of tiles, work units of 1, 2
    and 16 tiles, more samples than one ordered fold holds (1100 > 1024), several meshes per ray, two lights."""
    desc, dev, cam = build(gpu, name, w / h)
    a, _ = dev.render(cam, w, h, spp, seed=11)
    b, _ = dev.render(cam, w, h, spp, seed=11, flags=gpu.FLAG_WAVE_KERNEL)
    c, _ = dev.render(cam, w, h, spp, seed=11, flags=gpu.FLAG_STREAM_KERNEL)
    d, _ = dev.render(cam, w, h, spp, seed=11, flags=gpu.FLAG_DUAL_KERNEL)
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)


@pytest.mark.parametrize("name,w,h,spp", [("cornell_mesh", 320, 180, 6), ("backrooms_pool", 200, 112, 3), ("random_spheres", 160, 90, 5)])
def test_the_streaming_scheduler_is_deterministic_over_many_launches(gpu, name, w, h, spp):
    """The streaming kernel's waves hand cycles over through LDS counters (no barrier inside a fold): which wave runs which
    chunk, and which one prepares a stream's next cycle, differs from launch to launch.  Sixty launches of frames that take
    a few hundred scheduler cycles each must give the bits of the lane-per-pixel kernel every time, and never trip the
    scheduler's bounds (hrt_render would return HRT_ERR_DEVICE)."""
    desc, dev, cam = build(gpu, name, w / h)
    want, _ = dev.render(cam, w, h, spp, seed=21, flags=gpu.FLAG_WAVE_KERNEL)
    for k in range(60):
        got, _ = dev.render(cam, w, h, spp, seed=21, flags=gpu.FLAG_STREAM_KERNEL)
        assert np.array_equal(got, want), f"{name}: launch {k} differs: {describe_difference(got, want)}"


@pytest.mark.parametrize("name,w,h,spp", [("random_spheres", 480, 270, 6), ("rt_in_a_weekend", 240, 135, 4), ("flamingo", 160, 90, 2)])
def test_shadow_ray_culling_never_changes_a_pixel(gpu, name, w, h, spp):
    """Shadow rays only test the sphere groups that reach the capsule between the shading point and the light
    (a conservative filter); with HRT_FLAG_NO_SHADOW_CULL they test every sphere, as Scene::computeShadow does.
    ~0.8 M paths x up to 6 bounces x 10 shadow rays: one missed blocker would shift the draws of that path."""
    desc, dev, cam = build(gpu, name, w / h)
    a, _ = dev.render(cam, w, h, spp, seed=5)
    b, _ = dev.render(cam, w, h, spp, seed=5, flags=gpu.FLAG_NO_SHADOW_CULL)
    assert a.max() > 0 and np.array_equal(a, b)


def test_gamma_flag_matches_reference_formula(gpu):
    desc, dev, cam = build(gpu, "cornell_box", 1.0)
    lin, _ = dev.render(cam, 32, 32, 2, seed=1)
    gam, _ = dev.render(cam, 32, 32, 2, seed=1, flags=gpu.FLAG_GAMMA)
    assert np.allclose(gam, np.power(lin.astype(np.float64), 1 / 2.2), rtol=2e-5, atol=1e-6)  # Functions.cpp:56-60


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (9, 17), (61, 35)])
def test_ragged_images(gpu, oracle, w, h):
    """Sizes that are not multiples of the 8x8 tile, down to a single pixel."""
    desc, dev, cam = build(gpu, "cornell_mesh", w / h)
    img, _ = dev.render(cam, w, h, 3, seed=9)
    ref = oracle.OracleScene(desc).render(cam, w, h, 3, seed=9, threads=0)
    assert img.shape == (h, w, 3)
    assert_pixels_agree(img, ref, f"cornell_mesh {w}x{h}")


def test_synthetic_scenes_edge_cases(gpu, oracle):
    """Empty scene (sky only), mesh-only scene, emissive textured quad, glass quad, transparent blockers
    in front of a point light, moving sphere (motion blur)."""
    M = gpu.Material.make
    rng = np.random.default_rng(4)
    w, h, spp = 48, 32, 4

    def check(host):
        desc = host.flatten()
        dev = gpu.DeviceScene(desc)
        cam = gpu.default_camera(w / h)
        img, _ = dev.render(cam, w, h, spp, seed=11)
        ref = oracle.OracleScene(desc).render(cam, w, h, spp, seed=11, threads=0)
        assert np.isfinite(img).all()
        assert_pixels_agree(img, ref, "synthetic scene")
        return img

    s = gpu.HostScene()          # nothing at all: gradient sky x (remaining bounces + 1), Scene.h:152-153
    s.set_sky(False)
    sky = check(s)
    assert sky.min() > 0.25  # ((1-a) + a*(0.5,0.7,1)*7) / 6
    s = gpu.HostScene()          # dark sky
    assert check(s).max() == 0.0

    s = gpu.HostScene()          # a lit, textured, partly transparent world
    s.set_sky(False)
    tex = s.add_texture(rng.integers(0, 256, (16, 24, 3), dtype=np.uint8))
    nm = s.add_normal_map(rng.integers(96, 160, (8, 8, 3), dtype=np.uint8))
    s.add_light((0.5, 3.0, 2.0), 1.0)
    s.add_quad((-3, -1, -4), (1, 0, 0), (0, 0, 1), 6, 6, M(albedo=(1, 1, 1), texture_type=gpu.TEX_IMAGE, image=tex, normal_map=nm, tex_scale=(3, 2)))
    s.add_quad((-1.5, -1, -1), (1, 0, 0), (0, 1, 0), 1.0, 1.5, M(albedo=(0.3, 0.9, 0.9), type=gpu.MAT_GLASS, transparency=0.6, index_medium=1.3))
    s.add_quad((0.8, 0.5, -1.5), (1, 0, 0), (0, 1, 0), 0.7, 0.7, M(emissive=True, light_color=(1, 0.8, 0.6), light_intensity=4.0,
                                                                   texture_type=gpu.TEX_CHECKER, checker1=(1, 0, 0), checker2=(0, 0, 1), tex_scale=(4, 4)))
    s.add_sphere((0.2, -0.3, -1.0), 0.6, M(albedo=(0.9, 0.4, 0.2), transparency=0.5, motion=(0.0, 0.5, 0.0)))
    s.add_sphere((-1.2, 0.2, -2.0), 0.5, M(albedo=(0.8, 0.8, 0.8), type=gpu.MAT_MIRROR))
    v = np.array([[1, -1, -2], [2, -1, -2], [1.5, 0.2, -2.2], [1.5, -1, -1.2]], np.float32)
    t = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.uint32)
    s.add_mesh(v, t, M(albedo=(0.2, 0.8, 0.3)), face_colors=rng.uniform(0, 1, (4, 3)).astype(np.float32))
    check(s)

    s = gpu.HostScene()          # mesh only, no quads / spheres
    s.set_sky(False)
    s.add_mesh(v + np.array([-1.5, 0.5, 0], np.float32), t, M(albedo=(0.7, 0.7, 0.2)))
    check(s)

    s = gpu.HostScene()          # two meshes (T chunks walk per lane), one of them only a zero-area triangle: it has a gate box
    s.set_sky(False)             # (a flat rectangle the camera rays cross) but no tree at all
    s.add_mesh(v + np.array([-1.5, 0.5, 0], np.float32), t, M(albedo=(0.7, 0.7, 0.2)))
    s.add_mesh(np.array([[-2, -2, -1.5], [2, 2, -1.5], [0, 0, -1.5]], np.float32), np.array([[0, 1, 2]], np.uint32), M(albedo=(1, 0, 0)))
    check(s)
    assert s.kd_stats(1)["leaves"] == s.kd_stats(1)["empty_leaves"]


@pytest.mark.parametrize("n_quads,n_meshes", [(33, 0), (64, 2), (70, 5), (3, 32)])
def test_many_squares_and_meshes(gpu, oracle, n_quads, n_meshes):
    """The square filter keeps a 32-bit candidate mask up to 32 squares, a 64-bit one up to 64 and tests every
    square exactly beyond that; mesh bookkeeping is a 32-bit mask (the most hrt_scene_create accepts).  A random
    cloud of small tilted squares and tetrahedra, some glass, some moving, lit: every kernel form against the oracle."""
    s = many_squares(gpu, n_quads, n_meshes)
    desc = s.flatten()
    dev = gpu.DeviceScene(desc)
    w, h, spp = 72, 40, 3
    cam = gpu.default_camera(w / h)
    img, _ = dev.render(cam, w, h, spp, seed=2)
    ref = oracle.OracleScene(desc).render(cam, w, h, spp, seed=2, threads=0)
    assert np.isfinite(img).all() and img.max() > 0
    assert_pixels_agree(img, ref, f"many_squares {n_quads}/{n_meshes}")
    for flag in (gpu.FLAG_WAVE_KERNEL, gpu.FLAG_STREAM_KERNEL, gpu.FLAG_DUAL_KERNEL):
        other, _ = dev.render(cam, w, h, spp, seed=2, flags=flag)
        assert np.array_equal(img, other)


def test_more_than_32_meshes_is_refused_at_scene_creation(gpu):
    s = gpu.HostScene()
    tet = np.array([[0, 0, 0], [0.6, 0, 0], [0.3, 0.6, 0.1], [0.3, 0.2, 0.6]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)
    for i in range(33):
        s.add_mesh(tet + np.float32(i), tri, gpu.Material.make())
    with pytest.raises(gpu.HrtError, match="32"):
        gpu.DeviceScene(s.flatten())


def test_bad_arguments_are_rejected(gpu):
    desc, dev, cam = build(gpu, "cornell_box", 1.0)
    lib = gpu.device_lib()
    out = np.empty((8, 8, 3), np.float32)
    assert lib.hrt_render(dev._h, C.byref(cam), 0, 8, 1, 1, 0, out.ctypes.data, None) == -1
    assert lib.hrt_render(dev._h, C.byref(cam), 8, 8, 0, 1, 0, out.ctypes.data, None) == -1
    assert lib.hrt_render(dev._h, C.byref(cam), 8, 8, 1, 1, 0, None, None) == -1
    assert lib.hrt_render(None, C.byref(cam), 8, 8, 1, 1, 0, out.ctypes.data, None) == -1
    assert b"" != lib.hrt_last_error()


def test_a_cyclic_kd_tree_is_refused(gpu):
    """A flattened tree whose child links loop back would keep a walk descending forever; hrt_scene_create only accepts a tree."""
    from test_host_layer import MeshDesc, SceneDesc
    host = gpu.HostScene().setup("cornell_mesh", 1.0, 1)
    desc = host.flatten()
    d = C.cast(desc, C.POINTER(SceneDesc)).contents
    m = C.cast(d.meshes, C.POINTER(MeshDesc))[0]
    units = np.ctypeslib.as_array(C.cast(m.kd_units, C.POINTER(C.c_uint32)), shape=(m.n_kd_units, 4))
    root = m.kd_root
    assert not root & 0x80000000
    left = int(units[root, 2])
    assert not left & 0x80000000, "the root's left child is an inner node in this scene"
    saved = int(units[left, 2])
    lib = gpu.device_lib()
    lib.hrt_scene_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    try:
        units[left, 2] = root  # the left child's left child is the root again
        h = C.c_void_p()
        assert lib.hrt_scene_create(desc, C.byref(h)) != 0 and b"KD-tree" in lib.hrt_last_error()
    finally:
        units[left, 2] = saved
    h = C.c_void_p()
    assert lib.hrt_scene_create(desc, C.byref(h)) == 0
    lib.hrt_scene_destroy.argtypes = [C.c_void_p]
    lib.hrt_scene_destroy(h)


def test_tile_partition_is_invisible_in_the_pixels(gpu):
    """world = 1, 2, 3 renders of the same frame through hrt_render_tiles + hrt_assemble_frame are
    bit-identical: per-pixel RNG streams make the partition unobservable (the multi-GPU property)."""
    import torch
    w, h, spp = 200, 120, 3
    desc, dev, cam = build(gpu, "cornell_mesh", w / h)
    full, _ = dev.render(cam, w, h, spp, seed=21)
    for world in (2, 3):
        per = gpu.tiles_owned(w, h, 0, world)
        gathered = torch.zeros((world, per, 64, 3), dtype=torch.float32, device="cuda")
        for r in range(world):
            dev.render_tiles(cam, w, h, spp, 21, 0, r, world, gathered[r].data_ptr(), 0)
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gpu.assemble_frame(gathered.data_ptr(), per, w, h, world, frame.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(frame.cpu().numpy(), full)
        # and the host statement of the mapping (used by the CPU gloo test) is the same mapping
        assert np.array_equal(gpu.assemble_frame_host(gathered.cpu().numpy(), w, h, world), full)


def test_row_band_work_items_of_a_deep_multi_rank_share(gpu):
    """A rank's share of a multi-rank frame at many samples per pixel is few, heavy tiles: the streaming kernel's tile queue
    then hands out ROW BANDS of a tile (8 x 4 or 8 x 2 pixels) so that the launch does not end on one workgroup's last whole
    tile.  Same tiles, bit for bit, as the lane-per-pixel kernel -- for every rank of 8, with ragged right and bottom tiles,
    with more samples than one fold holds, and continued progressively."""
    import torch
    w, h, spp, world = 203, 101, 700, 8
    desc, dev, cam = build(gpu, "cornell_mesh", w / h)
    for r in (0, 3, 7):
        per = gpu.tiles_owned(w, h, r, world)
        a = torch.zeros((per, 64, 3), dtype=torch.float32, device="cuda")
        b = torch.zeros_like(a)
        dev.render_tiles(cam, w, h, spp, 9, gpu.FLAG_STREAM_KERNEL, r, world, a.data_ptr(), 0)
        dev.render_tiles(cam, w, h, spp, 9, gpu.FLAG_WAVE_KERNEL, r, world, b.data_ptr(), 0)
        torch.cuda.synchronize()
        assert float(a.max()) > 0 and torch.equal(a, b), f"rank {r}: band items vs lane-per-pixel kernel"
        c = torch.zeros_like(a)  # the same samples in two progressive launches (running sums; the mean is taken by the caller)
        dev.render_accumulate(cam, w, h, 0, 300, 9, gpu.FLAG_STREAM_KERNEL, r, world, c.data_ptr(), 0)
        dev.render_accumulate(cam, w, h, 300, 400, 9, gpu.FLAG_STREAM_KERNEL, r, world, c.data_ptr(), 0)
        d = torch.zeros_like(a)
        dev.render_accumulate(cam, w, h, 0, 700, 9, gpu.FLAG_WAVE_KERNEL, r, world, d.data_ptr(), 0)
        torch.cuda.synchronize()
        assert torch.equal(c, d), f"rank {r}: progressive sums"


def test_full_size_properties_cornell_mesh_1080p(gpu, oracle):
    """BASELINE config 2 at full resolution (low spp to keep the test short): size-independent properties.
    determinism, spp-additivity of the estimator, and agreement of the frame mean with the oracle's
    low-resolution frame mean (same camera, same scene: the pixel average estimates the same integral)."""
    w, h = 1920, 1080
    desc, dev, cam = build(gpu, "cornell_mesh", w / h)
    a, st = dev.render(cam, w, h, 8, seed=1)
    b, _ = dev.render(cam, w, h, 8, seed=1)
    assert np.array_equal(a, b) and np.isfinite(a).all()
    assert st.samples == w * h * 8
    c, _ = dev.render(cam, w, h, 8, seed=77)
    ref = oracle.OracleScene(desc).render(cam, 240, 135, 128, seed=5, threads=0)
    assert abs(a.mean() - ref.mean()) / ref.mean() < 0.05
    assert abs(c.mean() - a.mean()) / a.mean() < 0.03
    # coarse image agreement: 8x8 block means of the GPU frame vs the oracle frame
    blk = a.reshape(135, 8, 240, 8, 3).mean(axis=(1, 3))
    err = np.abs(blk - ref).mean() / ref.mean()
    assert err < 0.35  # Monte-Carlo noise of two independent estimates, not bias (the means agree above)


DEMO_SCENES = ["single_sphere", "single_square", "mesh", "rt_in_a_weekend", "debug_refraction", "flamingo", "raccoon",
               "flamingo_pond", "flamingo_lake"]


@pytest.mark.parametrize("name", DEMO_SCENES)
def test_demo_scenes_match_the_oracle(gpu, oracle, name):
    """the reference's demo scenes outside BASELINE's configs, same bar as the config scenes
    (first-hit ids identical, pixels within the stated tolerance).  They add what the configs lack: two and
    three lights (N2/N3), sphere textures, an emissive moving sphere, per-vertex mesh colours, a glass mesh,
    a normal-mapped glass quad, two meshes under one light."""
    w, h, spp = 96, 54, 3
    desc, dev, cam = build(gpu, name, w / h)
    ref = oracle.OracleScene(desc)
    hit = aov(gpu, dev, cam, w, h, 0)
    rhit = ref.aov(cam, w, h)["hit"]
    assert np.array_equal(hit, rhit), f"{name}: first hit differs on {int((hit != rhit).any(axis=2).sum())} pixels"
    img, _ = dev.render(cam, w, h, spp, seed=4)
    want = ref.render(cam, w, h, spp, seed=4, threads=0)
    assert np.isfinite(img).all() and img.max() > 0
    assert_pixels_agree(img, want, name)
    one, _ = dev.render(cam, w, h, spp, seed=4, flags=gpu.FLAG_WAVE_KERNEL)
    assert np.array_equal(img, one)


def test_skybox_image_lookup(gpu, oracle):
    """Scene::skyboxTexture with an image (Scene.h:154-160): equirectangular lookup by direction, scaled by the
    bounces left.  No config scene has one (the reference's sky.ppm is a missing blob), so a synthetic 64x32
    skybox over a mirror ball, a glass ball and a tilted square checks the lookup on primary and scattered rays."""
    M = gpu.Material.make
    rng = np.random.default_rng(8)
    s = gpu.HostScene()
    sky = rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)
    sky[:, :, 2] = np.linspace(0, 255, 64).astype(np.uint8)[None, :]
    s.set_skybox(sky)
    s.add_sphere((-0.9, 0.0, -1.0), 0.8, M(albedo=(0.9, 0.9, 0.9), type=gpu.MAT_MIRROR))
    s.add_sphere((0.9, 0.1, -0.5), 0.6, M(albedo=(1, 1, 1), type=gpu.MAT_GLASS, transparency=0.9, index_medium=1.5))
    s.add_quad((-2, -1.2, -3), (1, 0, 0.1), (0, 0.2, 1), 4, 4, M(albedo=(0.7, 0.6, 0.5)))
    desc = s.flatten()
    dev = gpu.DeviceScene(desc)
    w, h, spp = 96, 54, 4
    cam = gpu.default_camera(w / h)
    img, _ = dev.render(cam, w, h, spp, seed=6)
    ref = oracle.OracleScene(desc).render(cam, w, h, spp, seed=6, threads=0)
    assert img.max() > 0.5  # a primary miss sees texel/255 * 6 bounces left, and rayTrace divides by 6
    assert_pixels_agree(img, ref, "skybox")
    for flag in (gpu.FLAG_WAVE_KERNEL, gpu.FLAG_STREAM_KERNEL):
        other, _ = dev.render(cam, w, h, spp, seed=6, flags=flag)
        assert np.array_equal(img, other)
    s.set_skybox(None)  # removed again: dark_sky (default true) decides -> black where nothing is hit
    dev2 = gpu.DeviceScene(s.flatten())
    assert dev2.render(cam, w, h, 1, seed=6)[0][0, 0].max() == 0.0


def test_a_leaf_larger_than_the_walk_bound_is_tested_to_its_end(gpu, oracle):
    """the walk's guard used to count triangle tests (8192), so a leaf holding more -- unsplittable coplanar
    duplicates, or a big leaf_max -- silently lost its tail.  The guard now counts cells only.  One leaf of 9 001
    triangles: 9 000 copies of a far triangle and, LAST in the list, a near one that every camera ray must hit."""
    far = np.array([[-3, -3, -4], [3, -3, -4], [0, 3, -4]], np.float32)
    near = np.array([[-3, -3, -1], [3, -3, -1], [0, 3, -1]], np.float32)
    pos = np.concatenate([far, near])
    tri = np.array([[0, 1, 2]] * 9000 + [[3, 4, 5]], np.uint32)
    colors = np.array([[1, 0, 0]] * 9000 + [[0, 1, 0]], np.float32)
    s = gpu.HostScene()
    s.set_sky(False)
    s.set_kd_params(leaf_max=20000)
    s.add_mesh(pos, tri, gpu.Material.make(albedo=(1, 1, 1)), face_colors=colors)
    desc = s.flatten()
    assert s.kd_stats(0)["leaves"] - s.kd_stats(0)["empty_leaves"] == 1
    dev = gpu.DeviceScene(desc)
    w, h = 32, 24
    cam = gpu.default_camera(w / h)
    hit = aov(gpu, dev, cam, w, h, 0)
    ref = oracle.OracleScene(desc).aov(cam, w, h)["hit"]
    assert np.array_equal(hit, ref) and (hit[h // 2, w // 2, 1:] == [3, 9000]).all()   # the LAST triangle of the leaf wins
    for flag in (0, gpu.FLAG_WAVE_KERNEL, gpu.FLAG_DUAL_KERNEL, gpu.FLAG_STREAM_KERNEL):
        img, _ = dev.render(cam, w, h, 2, seed=1, flags=flag)
        assert_pixels_agree(img, oracle.OracleScene(desc).render(cam, w, h, 2, seed=1, threads=0), "big leaf")


def test_a_leaf_at_the_limit_the_abi_admits_renders(gpu, oracle):
    """VERDICT r2 item 4.  hrt_scene_create admits leaves of up to 65 534 triangles; a walk tests 2 per trip and 6 trips per T
    visit, so ONE such leaf is ~5 000 scheduler cycles of one path without a unit being opened or reduced -- the old stall
    bound (65 536 serial sections since a unit was last opened or reduced, both streams' counted) was within reach of a legal
    scene.  The bound now counts only cycles that run nothing.  One leaf of 60 001 triangles, the near one LAST."""
    far = np.array([[-3, -3, -4], [3, -3, -4], [0, 3, -4]], np.float32)
    near = np.array([[-3, -3, -1], [3, -3, -1], [0, 3, -1]], np.float32)
    n = 60000
    pos = np.concatenate([far, near])
    tri = np.array([[0, 1, 2]] * n + [[3, 4, 5]], np.uint32)
    colors = np.array([[1, 0, 0]] * n + [[0, 1, 0]], np.float32)
    s = gpu.HostScene()
    s.set_sky(False)
    s.set_kd_params(leaf_max=65000)
    s.add_mesh(pos, tri, gpu.Material.make(albedo=(1, 1, 1)), face_colors=colors)
    desc = s.flatten()
    assert s.kd_stats(0)["leaves"] - s.kd_stats(0)["empty_leaves"] == 1
    dev = gpu.DeviceScene(desc)
    w, h = 16, 12
    cam = gpu.default_camera(w / h)
    hit = aov(gpu, dev, cam, w, h, 0)
    ref = oracle.OracleScene(desc).aov(cam, w, h)["hit"]
    assert np.array_equal(hit, ref) and (hit[h // 2, w // 2, 1:] == [3, n]).all()   # the LAST triangle of the leaf wins
    want = oracle.OracleScene(desc).render(cam, w, h, 2, seed=1, threads=0)
    for flag in (gpu.FLAG_STREAM_KERNEL, gpu.FLAG_WAVE_KERNEL):
        img, _ = dev.render(cam, w, h, 2, seed=1, flags=flag)
        assert_pixels_agree(img, want, "leaf of 60 001 triangles")


def test_a_rope_that_names_no_nodelet_of_its_kind_is_refused(gpu):
    """the re-layout of hrt_scene_create followed ropes with a range check only.  A rope must name a nodelet the
    root reaches through child links, as what it is: an inner unit named as a LEAF would be read as four units from a
    two-unit slot (past the array for the last one)."""
    from test_host_layer import MeshDesc, SceneDesc
    host = gpu.HostScene().setup("cornell_mesh", 1.0, 1)
    desc = host.flatten()
    d = C.cast(desc, C.POINTER(SceneDesc)).contents
    m = C.cast(d.meshes, C.POINTER(MeshDesc))[0]
    units = np.ctypeslib.as_array(C.cast(m.kd_units, C.POINTER(C.c_uint32)), shape=(m.n_kd_units, 4))
    root = int(m.kd_root)
    assert not root & 0x80000000
    node = root
    while not node & 0x80000000:   # the leftmost leaf
        node = int(units[node, 2])
    leaf = node & 0x7FFFFFFF
    lib = gpu.device_lib()
    lib.hrt_scene_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.hrt_scene_destroy.argtypes = [C.c_void_p]
    saved = int(units[leaf + 2, 1])
    try:
        for bad in (root | 0x80000000,            # an inner nodelet named as a leaf
                    (leaf + 1)):                    # the middle of a leaf named as an inner nodelet
            units[leaf + 2, 1] = bad
            h = C.c_void_p()
            assert lib.hrt_scene_create(desc, C.byref(h)) != 0 and b"KD-tree" in lib.hrt_last_error(), hex(bad)
    finally:
        units[leaf + 2, 1] = saved
    h = C.c_void_p()
    assert lib.hrt_scene_create(desc, C.byref(h)) == 0
    lib.hrt_scene_destroy(h)


def test_image_sides_beyond_the_tile_packing_are_refused(gpu):
    """DESIGN 1 limits: tile origins travel as 16 + 16 bits, so a side of 65 536 or more is HRT_ERR_INVALID (before anything
    is allocated), on every entry point that takes a size."""
    desc, dev, cam = build(gpu, "cornell_box", 1.0)
    lib = gpu.device_lib()
    out = np.empty((1, 1, 3), np.float32)
    for w, h in ((65536, 1), (1, 65536), (70000, 2)):
        assert lib.hrt_render(dev._h, C.byref(cam), w, h, 1, 1, 0, out.ctypes.data, None) == -1 and b"65536" in lib.hrt_last_error()
        with pytest.raises(gpu.HrtError, match="65536"):
            dev.render_tiles(cam, w, h, 1, 1, 0, 0, 1, 8, 0)   # (the buffer pointer is never touched)
    img, _ = dev.render(cam, 8, 8, 1, seed=1)   # still usable
    assert np.isfinite(img).all()


def test_two_launches_of_one_scene_on_two_streams_are_serialised(gpu):
    """DESIGN 1 limits: one hrt_scene carries one launch at a time (tile queue head, path pool, camera block).  A launch on
    ANOTHER stream must wait for the previous one (hipStreamWaitEvent on its end event): two launches issued back to back
    on two streams give the bits of the same two launches run one after the other."""
    import torch
    w, h, spp = 320, 180, 6
    desc, dev, cam = build(gpu, "cornell_mesh", w / h)
    tiles = gpu.tiles_total(w, h)
    want = []
    for seed in (11, 12):
        buf = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
        dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, buf.data_ptr(), 0)
        torch.cuda.synchronize()
        want.append(buf.cpu().numpy())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for trial in range(3):
        a = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
        b = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dev.render_tiles(cam, w, h, spp, 11, 0, 0, 1, a.data_ptr(), s1.cuda_stream)
        dev.render_tiles(cam, w, h, spp, 12, 0, 0, 1, b.data_ptr(), s2.cuda_stream)   # no host wait in between
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), want[0]) and np.array_equal(b.cpu().numpy(), want[1]), trial
    assert gpu.device_lib().hrt_check_last_launch(dev._h) == 0


FOUR_K = (3840, 2160)


@pytest.mark.parametrize("name,exact", [("mesh_in_box", True), ("backrooms_pool", False)])
def test_frames_of_3840_x_2160_agree_between_the_kernel_forms(gpu, name, exact):
    """VERDICT r2 item 3.  BASELINE's cfg 4 and cfg 5 are 3840 x 2160 frames: 129 600 tiles on the queue, four times the
    per-pixel key range and work-unit count of anything else tested.  At 2 spp the streaming kernel's frame must be the
    lane-per-pixel kernel's bit for bit (and, on one scene, the proof build's: no filter, no pruning, IEEE divisions)."""
    w, h = FOUR_K
    desc, dev, cam = build(gpu, name, w / h)
    a, _ = dev.render(cam, w, h, 2, seed=4, flags=gpu.FLAG_STREAM_KERNEL)
    assert np.isfinite(a).all() and a.max() > 0 and (a.reshape(-1, 3).max(axis=1) > 0).mean() > 0.01   # (2 spp: few paths reach the small light)
    b, _ = dev.render(cam, w, h, 2, seed=4, flags=gpu.FLAG_WAVE_KERNEL)
    assert np.array_equal(a, b), f"{name} 4K: streaming vs lane-per-pixel: {describe_difference(a, b)}"
    if exact:
        c, _ = dev.render(cam, w, h, 2, seed=4, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY)
        assert np.array_equal(a, c), f"{name} 4K: shipped vs exact-only: {describe_difference(a, c)}"


def test_rank_5_of_8_at_3840_x_2160_renders_its_tiles_of_the_full_frame(gpu):
    """One rank's share of the 8-GPU step of cfg 4 (tiles 5, 13, 21, ... of 129 600; here @ 16 spp) through hrt_render_tiles
    must be exactly those tiles of the frame one GPU renders alone -- the row-band work items a rank-of-8 launch uses at high
    spp included (64 spp on a quarter-size frame)."""
    import torch
    for (w, h), spp in ((FOUR_K, 16), ((960, 540), 2048)):
        desc, dev, cam = build(gpu, "mesh_in_box", w / h)
        full, _ = dev.render(cam, w, h, spp, seed=8)
        rank, world = 5, 8
        own = gpu.tiles_owned(w, h, rank, world)
        buf = torch.zeros((own, 64, 3), dtype=torch.float32, device="cuda")
        dev.render_tiles(cam, w, h, spp, 8, 0, rank, world, buf.data_ptr(), 0)
        torch.cuda.synchronize()
        assert gpu.device_lib().hrt_check_last_launch(dev._h) == 0
        got = buf.cpu().numpy().reshape(own, 8, 8, 3)
        tiles_x = (w + 7) // 8
        padded = np.zeros((((h + 7) // 8) * 8, tiles_x * 8, 3), np.float32)
        padded[:h, :w] = full
        want = padded.reshape((h + 7) // 8, 8, tiles_x, 8, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 8, 8, 3)[rank::world]
        assert want.shape == got.shape and np.array_equal(got, want), f"{w}x{h}@{spp}: {describe_difference(got.reshape(-1, 8, 3), want.reshape(-1, 8, 3))}"


@pytest.mark.parametrize("name", ["cornell_box", "cornell_mesh", "random_spheres"])
def test_converged_means_agree_statistically(gpu, name):
    """SURVEY 8(c) fixture 5.  tests/golden/oracle_converged.npz holds the oracle's mean of 16 x 64 spp (seeds 1000..1015)
    and the standard error of that mean per pixel and channel.  A GPU render of 1024 spp with an UNRELATED seed estimates the
    same image: with z = (gpu - mean) / (sqrt(2) sem) (both estimates carry about the same error) the z-scores must look
    like unit normals -- |mean z| small (no bias), rms near 1, and no heavy tail beyond what fireflies of an emissive-light
    scene explain.  This checks the estimator (stream keying by pixel and sample, sample accumulation, the / 6 and / spp)
    independently of any seed-for-seed comparison."""
    g = np.load(os.path.join(GOLDEN, "oracle_converged.npz"))
    w, h, batches, spp = (int(x) for x in g[name + "_shape"])
    desc, dev, cam = build(gpu, name, w / h)
    img, _ = dev.render(cam, w, h, batches * spp, seed=987654321)
    mean, sem = g[name + "_mean"].astype(np.float64), g[name + "_sem"].astype(np.float64)
    ok = sem > 1e-7                      # pixels with no variance at all (black background) must simply be equal-ish
    z = (img.astype(np.float64) - mean)[ok] / (np.sqrt(2.0) * sem[ok])
    assert ok.mean() > 0.5
    assert abs(np.median(z)) < 0.1 and abs(z.mean()) < 0.25, f"{name}: biased (median z {np.median(z):.3f}, mean z {z.mean():.3f})"
    assert 0.7 < np.sqrt(np.median(z * z) / 0.4549) < 1.4, f"{name}: spread of z off (robust rms {np.sqrt(np.median(z * z) / 0.4549):.2f})"   # median of chi2_1 = 0.4549
    assert (np.abs(z) > 6).mean() < 0.01
    assert np.abs(img[~ok] - mean[~ok]).max() < 1e-3 if (~ok).any() else True
    rel = abs(img.mean() - mean.mean()) / mean.mean()
    assert rel < 0.01, f"{name}: frame means differ by {100 * rel:.2f} %"
