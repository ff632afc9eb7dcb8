"""Frames on scenes built for the divisors of the streaming kernel's exact division by known divisors (csrc/hrt_div.h).

The shipped streaming builds divide by a square's side lengths, by a vector's length and by the image size with a reciprocal and
two FMAs; their proof builds (HRT_FLAG_EXACT_ONLY) and the lane-per-pixel kernel keep `/`.  The three forms must give the same
frame bit for bit.  Sizes: 64 x 36 @ 8 (whole tiles) and 199 x 113 @ 3 (ragged edges, odd sample count)."""
import numpy as np
import pytest

from scene_util import describe_difference, many_squares

pytestmark = pytest.mark.gpu

F32 = np.float32
ONES2, ONES4 = float(np.nextafter(F32(2), F32(0))), float(np.nextafter(F32(4), F32(0)))  # all-ones significands


def room(gpu, k=1.0, side=4.0, depth=14.0, floor=None, back=None, extras=True):
    """A closed room around the default camera scaled by k (eye (0, 0, 6.1 k), looking down -z): five walls, a lamp under the
    ceiling, and -- extras -- a glass, a moving and a mirror square standing in it."""
    M = gpu.Material.make
    s = gpu.HostScene()
    s.set_sky(False)                   # the room is open behind the camera: paths that leave meet the bright sky
    h = side / 2
    wall = M(albedo=(0.7, 0.6, 0.5))
    s.add_quad((-h * k, -h * k, -6 * k), (1, 0, 0), (0, 0, 1), side * k, depth * k, floor or wall)                 # floor
    s.add_quad((-h * k, h * k, (depth - 6) * k), (1, 0, 0), (0, 0, -1), side * k, depth * k, wall)                 # ceiling
    s.add_quad((-h * k, -h * k, -6 * k), (1, 0, 0), (0, 1, 0), side * k, side * k, back or M(albedo=(0.3, 0.7, 0.4)))  # back, square to the view axis
    s.add_quad((-h * k, -h * k, (depth - 6) * k), (0, 0, -1), (0, 1, 0), depth * k, side * k, M(albedo=(0.8, 0.3, 0.3)))  # left
    s.add_quad((h * k, -h * k, -6 * k), (0, 0, 1), (0, 1, 0), depth * k, side * k, M(albedo=(0.3, 0.3, 0.8)))      # right
    s.add_quad((-0.5 * h * k, 0.99 * h * k, -3 * k), (1, 0, 0), (0, 0, 1), h * k, h * k,
               M(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=6.0))                     # lamp, facing down
    if extras:
        s.add_quad((-0.8 * h * k, -0.9 * h * k, -1 * k), (1, 0.2, 0.3), (0, 1, 0.1), 0.6 * h * k, 0.9 * h * k,
                   M(albedo=(0.9, 0.9, 1.0), type=gpu.MAT_GLASS, transparency=0.7, index_medium=1.4))
        s.add_quad((0.1 * h * k, -0.9 * h * k, 0.5 * k), (1, 0, -0.4), (0.1, 1, 0), 0.5 * h * k, 0.7 * h * k,
                   M(albedo=(0.9, 0.8, 0.2), motion=(0.0, 0.25 * k, 0.05 * k)))
        s.add_quad((-0.2 * h * k, -0.2 * h * k, -4 * k), (1, 0.1, 0.5), (0, 1, 0), 0.5 * h * k, 0.5 * h * k, M(albedo=(0.9, 0.9, 0.9), type=gpu.MAT_MIRROR))
    return s


def camera(gpu, aspect, k=1.0, eye_y=0.0):
    cam = gpu.default_camera(aspect)
    cam.eye[:] = (0.0, eye_y * k, 6.1 * k)
    return cam


def case(gpu, name, aspect):
    M = gpu.Material.make
    if name == "all_ones_sides":       # every wall's |R| and |U| is nextafter(4, 0) or nextafter(2, 0) x ...: the significands the theorem leaves out
        r = F32(ONES4)
        assert np.sqrt(r * r) == r
        return room(gpu, side=ONES4, depth=ONES4 * 4), camera(gpu, aspect)
    if name == "sides_1e-3":
        return room(gpu, k=2.5e-4), camera(gpu, aspect, k=2.5e-4)          # 4 k = 1e-3
    if name == "sides_1e3":
        return room(gpu, k=250.0), camera(gpu, aspect, k=250.0)            # 4 k = 1e3
    if name == "normal_map_grazing":   # the eye a hair above a normal-mapped floor: rays meet it at grazing incidence
        s = room(gpu, floor=M(albedo=(0.7, 0.7, 0.7), normal_map=0), extras=False)
        assert s.add_normal_map(np.random.default_rng(5).integers(0, 256, (16, 16, 3)).astype(np.uint8)) == 0
        return s, camera(gpu, aspect, eye_y=-1.98)
    if name == "mirror_back_wall":     # a mirror square to the view axis: reflected directions with exact zero and equal components
        return room(gpu, back=M(albedo=(0.95, 0.95, 0.95), type=gpu.MAT_MIRROR), extras=False), camera(gpu, aspect)
    _, nq, nm = name.split(":")        # clouds of tilted squares (glass, mirror, moving) on both sides of the filter's 32 / 64 limits; meshes
    return many_squares(gpu, int(nq), int(nm)), gpu.default_camera(aspect)


CASES = ["all_ones_sides", "sides_1e-3", "sides_1e3", "normal_map_grazing", "mirror_back_wall", "many_squares:33:0", "many_squares:65:0",
         "many_squares:9:1", "many_squares:9:3"]


@pytest.mark.parametrize("w,h,spp", [(64, 36, 8), (199, 113, 3)])
@pytest.mark.parametrize("name", CASES)
def test_the_three_forms_give_the_same_frame(gpu, name, w, h, spp):
    host, cam = case(gpu, name, w / h)
    dev = gpu.DeviceScene(host.flatten())
    a, _ = dev.render(cam, w, h, spp, seed=9, flags=gpu.FLAG_STREAM_KERNEL)
    assert dev.last_kernel().startswith("hrt_wgstream_kernel") and "exact" not in dev.last_kernel()
    b, _ = dev.render(cam, w, h, spp, seed=9, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY)
    assert "exact" in dev.last_kernel()
    c, _ = dev.render(cam, w, h, spp, seed=9, flags=gpu.FLAG_WAVE_KERNEL)
    assert dev.last_kernel().startswith("hrt_trace_kernel")
    assert np.isfinite(a).all() and (a.max(axis=2) > 0).mean() > 0.9 and len(np.unique(a)) > 1000   # a frame: lit nearly everywhere, not flat
    assert np.array_equal(a, b), f"{name}: streaming vs its proof build: {describe_difference(a, b)}"
    assert np.array_equal(a, c), f"{name}: streaming vs lane-per-pixel: {describe_difference(a, c)}"
    dev.close()
