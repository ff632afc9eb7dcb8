"""The squares' filter at frame scale, on the loop shapes of csrc/hrt_kernels.hip quad_filter: the shipped builds against the
proof builds (HRT_FLAG_EXACT_ONLY: every square through the exact test, no filter), bit for bit, 64 x 64 @ 8 spp.

The filter rows lie in four sections (squares in an axis plane by normal axis x, y, z, then all others), each walked in pairs
from two register sets with the odd last square peeled, and the candidates are bits of a 32-bit mask up to 32 squares and of a
64-bit one up to 64.  Scenes, built through HostScene:
  * 0, 1, 2 and 3 squares in each of the four sections, alone and beside other counts: the empty section, the peeled trip
    alone, one pair, a pair and the tail;
  * 31, 32, 33 and 64 squares: the last bit of either mask and the switch between them -- the square added last (the highest
    index) is the wall behind everything, which most paths reach;
  * one square of each section made of glass.
Every scene goes through the streaming, the lane-per-pixel and the two-stream form, forced by their flags (what HRT_KERNEL =
stream | single | dual asks for at hrt_init, here per launch in one process).  The two-stream form has no proof build: it is
held against the lane-per-pixel one.  A tetrahedron is in every scene because the two-stream form runs only where a mesh is."""
import numpy as np
import pytest

from scene_util import describe_difference

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 8
AXES = np.eye(3)


def build(gpu, counts, glass_section=None):
    """counts = squares per section (x, y, z, general), added interleaved so that the indices of a section are spread; the
    last one added is the back wall (normal +z, section 2) when counts[2] > 0."""
    M = gpu.Material.make
    rng = np.random.default_rng([*counts, 0 if glass_section is None else 1 + glass_section])
    s = gpu.HostScene()
    s.set_sky(False)
    s.add_light((0.0, 4.0, 3.0), 1.0)
    left = list(counts)
    wall = left[2] > 0
    if wall:
        left[2] -= 1
    order = []
    while any(left):
        for k in range(4):
            if left[k]:
                left[k] -= 1
                order.append(k)
    glass_done = glass_section is None
    for k in order:
        c = rng.uniform((-2.5, -1.5, -6), (2.5, 1.5, -2))
        if k < 3:  # in an axis plane: the edges along the two other axes, either sign, so both normal signs occur
            i, j = (k + 1) % 3, (k + 2) % 3
            if rng.integers(0, 2):
                i, j = j, i
            r, u = AXES[i] * rng.choice([-1.0, 1.0]), AXES[j] * rng.choice([-1.0, 1.0])
        else:
            r = rng.normal(size=3)
            u = np.cross(r, rng.normal(size=3))
        glass = not glass_done and k == glass_section
        glass_done |= glass
        mat = M(albedo=tuple(rng.uniform(0.3, 1, 3)), type=gpu.MAT_GLASS if glass else gpu.MAT_DIFFUSE, transparency=0.5 if glass else 0.0,
                index_medium=1.4)
        s.add_quad(tuple(c), tuple(r), tuple(u), float(rng.uniform(0.8, 2.0)), float(rng.uniform(0.8, 2.0)), mat)
    if wall:
        glass = not glass_done and glass_section == 2
        s.add_quad((-5, -4, -7), (1, 0, 0), (0, 1, 0), 10.0, 8.0,
                   M(albedo=(0.8, 0.7, 0.6), type=gpu.MAT_GLASS if glass else gpu.MAT_DIFFUSE, transparency=0.5 if glass else 0.0, index_medium=1.4))
    tet = np.array([[0, 0, 0], [0.6, 0, 0], [0.3, 0.6, 0.1], [0.3, 0.2, 0.6]], np.float32) + np.array([0.4, -0.8, -3.0], np.float32)
    s.add_mesh(tet, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32), M(albedo=(0.9, 0.4, 0.3)))
    return s


CASES = ([((c, c, c, c), None) for c in range(4)]
         + [((0, 1, 2, 3), None), ((3, 2, 1, 0), None), ((1, 0, 3, 2), None), ((2, 3, 0, 1), None)]
         + [((8, 8, 8, 7), None), ((8, 8, 8, 8), None), ((9, 8, 8, 8), None), ((16, 16, 16, 16), None), ((0, 0, 32, 0), None), ((0, 0, 1, 63), None)]
         + [((2, 2, 2, 2), k) for k in range(4)])


@pytest.mark.parametrize("counts,glass", CASES, ids=[f"{'-'.join(map(str, c))}{'' if g is None else f'-glass{g}'}" for c, g in CASES])
def test_shipped_forms_equal_the_proof_builds(gpu, counts, glass):
    host = build(gpu, counts, glass)
    dev = gpu.DeviceScene(host.flatten())
    cam = gpu.default_camera(W / H)
    proof_stream, _ = dev.render(cam, W, H, SPP, seed=3, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY)
    proof_lane, _ = dev.render(cam, W, H, SPP, seed=3, flags=gpu.FLAG_WAVE_KERNEL | gpu.FLAG_EXACT_ONLY)
    assert np.isfinite(proof_stream).all() and proof_stream.max() > 0
    assert np.array_equal(proof_stream, proof_lane), f"the two proof builds differ: {describe_difference(proof_stream, proof_lane)}"
    for form, label in ((gpu.FLAG_STREAM_KERNEL, "streaming"), (gpu.FLAG_WAVE_KERNEL, "lane-per-pixel"), (gpu.FLAG_DUAL_KERNEL, "two-stream")):
        got, _ = dev.render(cam, W, H, SPP, seed=3, flags=form)
        assert np.array_equal(got, proof_stream), f"{counts} ({label}): filtered vs exact-only: {describe_difference(got, proof_stream)}"
    dev.close()
