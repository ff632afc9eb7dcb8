"""The build a trace launch runs is the one the choice function names (include/hrt.h hrt_debug_last_kernel against
hrt_debug_pick_kernel), through every public route to a launch, and whichever build runs gives the bits of the lane-per-pixel
kernel.  One test: scenes whose traits span the build axes (lights, meshes, a sphere count inside and outside the pair filter's
range), frames of 24 x 16 pixels = 3 x 2 tiles (more than a wave's worth of tiles, few enough that 8 samples per pixel take the
small-and-deep route), and at the end every trace kernel the sources define must have run."""
import ctypes as C
import os

import numpy as np
import pytest

from scene_util import many_spheres
from test_gpu_adaptive import assert_tiles_match
from test_kernel_choice import DUAL, EXACT, STREAM, WAVE, defined_kernels

pytestmark = pytest.mark.gpu

W, H, SEED = 24, 16, 5
TILES = 6
FORMS = (0, WAVE, STREAM, DUAL, EXACT, EXACT | WAVE, EXACT | STREAM)
VIEW_SEEDS = (11, 2 ** 40 + 5, 3)


def with_mesh(gpu, host):
    tet = np.array([[0, 0, 0], [1.2, 0, 0], [0.6, 1.2, 0.2], [0.6, 0.4, 1.2]], np.float32) + np.float32([-0.5, -0.5, 0.5])
    host.add_mesh(tet, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32), gpu.Material.make(albedo=(0.9, 0.4, 0.2)))
    return host


SCENES = {
    "unlit, 5 spheres": lambda gpu: many_spheres(gpu, 5, 0),
    "lit, 5 spheres": lambda gpu: many_spheres(gpu, 5, 1),
    "unlit, 12 spheres": lambda gpu: many_spheres(gpu, 12, 0),   # 8..128: the sphere-filter builds
    "lit, 12 spheres": lambda gpu: many_spheres(gpu, 12, 2),
    "unlit, 129 spheres": lambda gpu: many_spheres(gpu, 129, 0),  # past the range again
    "cornell_mesh": lambda gpu: gpu.HostScene().setup("cornell_mesh", W / H, 1),  # a mesh, lit by emissive squares: no point light
    "lit, a mesh": lambda gpu: with_mesh(gpu, many_spheres(gpu, 5, 1)),
}


class DescHead(C.Structure):  # hrt_scene_desc, as far as the counts
    _fields_ = [(n, t) for name in ("materials", "spheres", "quads", "meshes", "lights") for n, t in (("n_" + name, C.c_uint32), (name, C.c_void_p))]


def traits(desc):
    """(n_meshes, n_lights, n_spheres, tab_rows) of a flattened scene.  tab_rows as scene_create lays the tables out: 7 rows per
    square, 8 per material, 2 per sphere, 6 per mesh, 4 per sphere pair -- and the meshes' exception rows, which are not counted
    here; they are at most 1536, and every scene of this test keeps below the 3072 rows the choice turns on either way (a render
    with HRT_FLAG_STREAM_KERNEL, refused past them, is part of the test)."""
    d = C.cast(desc, C.POINTER(DescHead)).contents
    rows = 7 * d.n_quads + 8 * d.n_materials + 2 * d.n_spheres + 6 * d.n_meshes + 4 * ((d.n_spheres + 1) // 2)
    assert rows + (1536 if d.n_meshes else 0) <= 3072
    return d.n_meshes, d.n_lights, d.n_spheres, rows


def shifted(gpu, cam, dx):
    out = gpu.Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(cam))
    out.eye[0] = np.float32(cam.eye[0] + dx)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_every_route_launches_the_build_the_choice_names_and_every_build_is_reached(gpu):
    launched = set()
    for name, make in SCENES.items():
        host = make(gpu)
        desc = host.flatten()
        dev, cam, t = gpu.DeviceScene(desc), gpu.default_camera(W / H), traits(desc)
        assert dev.last_kernel() == ""
        cache = {}

        def wave(spp, cam=cam, seed=SEED):  # the reference: the lane-per-pixel kernel's frame
            key = (spp, bytes(cam), seed)
            if key not in cache:
                cache[key] = dev.render(cam, W, H, spp, seed, WAVE)[0]
            return cache[key]

        def ran(what, **launch):  # called straight after the launch
            want = gpu.pick_kernel(*t, kernel=os.environ.get("HRT_KERNEL", ""), **launch)
            got = dev.last_kernel()
            print(f"{name}: {what} {launch}: {got}")
            assert got == want, (name, what, launch)
            launched.add(got)

        for spp, flags in [(2, f) for f in FORMS] + [(8, 0), (8, EXACT)]:
            frame = dev.render(cam, W, H, spp, SEED, flags)[0]
            ran("render", tiles=TILES, spp=spp, flags=flags)
            assert np.array_equal(bits(frame), bits(wave(spp))), (name, "render", spp, flags)
        for flags in FORMS:  # 1 + 1 samples for every tile, then 2 more over a list of the tiles that have any noise
            frame, counts = dev.render_adaptive(cam, W, H, 2, 4, 0.0, seed=SEED, flags=flags)
            listed = int((counts == 4).sum())
            assert listed > 0 and set(np.unique(counts)) <= {2, 4}, (name, counts)
            ran("render_adaptive", tiles=listed, spp=2, flags=flags, has_list=True)
            assert_tiles_match(frame, counts, {c: wave(c) for c in (2, 4)}, W, H)
        cams = [cam, shifted(gpu, cam, 0.7), shifted(gpu, cam, -1.1)]
        for flags in (0, WAVE, STREAM):
            frames = dev.render_views(cams, W, H, 2, VIEW_SEEDS, flags)
            ran("render_views", tiles=3 * TILES, spp=2, flags=flags, n_views=3)
            for v in range(3):
                assert np.array_equal(bits(frames[v]), bits(wave(2, cams[v], VIEW_SEEDS[v]))), (name, "render_views", flags, v)
        dev.close()
    missing = defined_kernels() - launched
    print("builds never launched:", sorted(missing))
    assert not missing and len(launched) == 30
