"""The streaming kernel's hit records travel with their queue position (csrc/hrt_stream.hip, sp_hr_at): a path that goes from a
new-path chunk or a hit visit to a hit queue leaves its 64-byte state at the position it takes in that queue, not in its slot; the
entry's flag tells the next visit where to look; a T visit that finishes a walk leaves the state in the slot; the records of a
queue's deferred tail are copied to the front of the next cycle's array.

None of that may be visible: every frame of the streaming form (FLAG_STREAM_KERNEL) must have the bits of the lane-per-pixel form
(FLAG_WAVE_KERNEL) of the same launch, which keeps a path in registers from its first ray to its last.  Equality, no tolerance.
The shapes are the smallest at which the addressing can go wrong:
  * cornell_box 64 x 64 @ 8          no mesh, so hit -> hit only; spheres from the front and squares from the back of buffer A
  * cornell_mesh 64 x 64 @ 8         T visits hand paths back "in slot" beside positional entries of the same chunk
  * cornell_mesh 72 x 40 @ 4         45 tiles at 4 spp: units of 4 096 paths, so that deferral switches off while units drain
  * random_spheres 64 x 36 @ 8       the builds whose in-place miss ends a path from the state the lane still holds
  * mesh_in_box 70 x 50 @ 3          ragged right and bottom tiles, an odd sample count
  * cornell_mesh 64 x 64 @ 300       more than one fold per unit, thousands of cycles of carried tails
  * rank 1 of 3, two views in one launch, the proof build (FLAG_EXACT_ONLY)
(tests/test_gpu_parity.py holds the lane-per-pixel form of these scenes against the CPU oracle.)"""
import ctypes as C

import numpy as np
import pytest

from scene_util import describe_difference

pytestmark = pytest.mark.gpu


def build(gpu, name, aspect):
    desc = gpu.HostScene().setup(name, aspect, 1).flatten()
    return gpu.DeviceScene(desc), gpu.default_camera(aspect)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(got, want, what):
    assert np.isfinite(want).all() and want.max() > 0, what
    assert np.array_equal(bits(got), bits(want)), f"{what}: streaming vs lane-per-pixel: {describe_difference(got, want)}"


@pytest.mark.parametrize("name,w,h,spp", [("cornell_box", 64, 64, 8), ("cornell_mesh", 64, 64, 8), ("cornell_mesh", 72, 40, 4),
                                          ("random_spheres", 64, 36, 8), ("mesh_in_box", 70, 50, 3), ("cornell_mesh", 64, 64, 300)])
def test_streaming_frames_have_the_bits_of_the_lane_per_pixel_form(gpu, name, w, h, spp):
    dev, cam = build(gpu, name, w / h)
    got, st = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_STREAM_KERNEL)
    assert "wgstream" in dev.last_kernel() and st.samples == w * h * spp
    want, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_WAVE_KERNEL)
    assert "trace_kernel" in dev.last_kernel()
    assert_same_bits(got, want, f"{name} {w}x{h}@{spp}")
    again, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_STREAM_KERNEL)  # the hit-record array now holds the last launch's records
    assert_same_bits(again, want, f"{name} {w}x{h}@{spp}, second launch")


def test_the_proof_build_has_the_same_bits(gpu):
    w, h, spp = 64, 64, 8
    dev, cam = build(gpu, "cornell_mesh", w / h)
    got, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY)
    assert "wgstream" in dev.last_kernel() and "exact" in dev.last_kernel()
    want, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_WAVE_KERNEL | gpu.FLAG_EXACT_ONLY)
    assert_same_bits(got, want, "cornell_mesh 64x64@8, exact only")
    shipped, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_WAVE_KERNEL)
    assert_same_bits(got, shipped, "cornell_mesh 64x64@8, exact only vs shipped")


def test_rank_1_of_3_renders_its_tiles_of_the_whole_frame(gpu):
    import torch
    w, h, spp, rank, world = 64, 64, 8, 1, 3
    dev, cam = build(gpu, "cornell_mesh", w / h)
    full, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_WAVE_KERNEL)
    own = gpu.tiles_owned(w, h, rank, world)
    buf = torch.zeros((own, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, 13, gpu.FLAG_STREAM_KERNEL, rank, world, buf.data_ptr(), 0)
    torch.cuda.synchronize()
    assert gpu.device_lib().hrt_check_last_launch(dev._h) == 0 and "wgstream" in dev.last_kernel()
    got = buf.cpu().numpy().reshape(own, 8, 8, 3)
    want = full.reshape(h // 8, 8, w // 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 8, 8, 3)[rank::world]
    assert want.shape == got.shape
    assert_same_bits(got.reshape(-1, 8, 3), want.reshape(-1, 8, 3), "rank 1 of 3")


def test_two_views_in_one_launch_are_two_single_renders(gpu):
    w, h, spp = 32, 32, 8
    dev, cam = build(gpu, "cornell_mesh", w / h)
    other = gpu.Camera()
    C.memmove(C.byref(other), C.byref(cam), C.sizeof(cam))
    other.eye[0] = np.float32(cam.eye[0] + 0.7)
    cams, seeds = [cam, other], [13, 2 ** 40 + 5]
    frames = dev.render_views(cams, w, h, spp, seeds, gpu.FLAG_STREAM_KERNEL)
    assert "wgstream" in dev.last_kernel() and "views" in dev.last_kernel()
    for v in range(2):
        want, _ = dev.render(cams[v], w, h, spp, seeds[v], gpu.FLAG_WAVE_KERNEL)
        assert_same_bits(frames[v], want, f"view {v}")
    assert not np.array_equal(frames[0], frames[1])
