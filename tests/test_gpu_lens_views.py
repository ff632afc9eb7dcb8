"""Batched lens views on the GPU (include/hrt.h "Batched lens views"): frame v of a batch is hrt_render_lens_device of view v BIT FOR
BIT -- for batches that mix every projection, at a frame size whose waves straddle views, with one view per lane, across the
grid-stride hand-over from one view to another, under every permitted flag set, from a later first sample and accumulated over
splits; a pinhole batch is hrt_render_views; the batched features are the single-lens features; a batch may run beside a render of
the same scene; and the Python binding on torch and NumPy.  No tolerance anywhere: the contract is bit-exact against code that exists."""
import itertools

import numpy as np
import pytest

import lens_ref
import test_gpu_rays as qr
from scene_util import placed_camera

pytestmark = pytest.mark.gpu

F32 = np.float32
EXACT, BRUTE, NO_LDS, GAMMA, WAVE = 64, 128, 2, 1, 4
bits = qr.bits
CONTRACT_SCENES = ["cornell_mesh", "random_spheres", "backrooms_pool"]
W, H = 19, 11  # 209 pixels: no multiple of 64, so waves straddle views

_built = {}


def scene(gpu, name):
    if name not in _built:
        _built[name] = qr.build(gpu, name, W, H)[2]
    return _built[name]


def turned(gpu, aspect, k):
    """The default camera of `aspect` moved INSIDE the rooms of cornell_mesh and backrooms_pool, a little elsewhere for every k.
    Those two scenes are closed rooms under a dark sky that the default camera looks into from outside: at 19 x 11 x 5 samples a
    panorama or a fisheye from there has the lit room in a handful of pixels and is black as often as not, which would make
    "the frames are non-zero" a matter of the seed.  From inside every direction ends on a wall: a tenth to a quarter of the pixels
    of any view are lit (counted with the CPU oracle for pinholes of 45 and 150 degrees, forwards and backwards)."""
    cam = gpu.default_camera(aspect)
    cam.eye[0] = -0.3 + 0.1 * (k % 7)
    cam.eye[1] = 0.05 * (k % 3)
    cam.eye[2] = 1.5 - 0.03 * (k % 11)
    return cam


def mixed(gpu, n, aspect):
    """n lenses: the pinhole and every case of lens_ref.CASES, cycled view by view, each behind its own camera; seeds all distinct."""
    kinds = [("perspective", 0.0, 1.0, 0.0)] + list(lens_ref.CASES.values())
    lenses = []
    for k, (proj, ap, fo, ex) in zip(range(n), itertools.cycle(kinds)):
        lenses.append(gpu.Lens(turned(gpu, aspect, k), proj, aperture=ap, focus=fo, extent=ex))
    seeds = [3 + 7 * k + (2 ** 40 if k % 2 else 0) for k in range(n)]
    return lenses, seeds


def contract_batch(gpu):
    """Eight views: the pinhole, the five cases, a thin lens behind a placed camera, a second pinhole elsewhere."""
    lenses, seeds = mixed(gpu, 6, W / H)
    lenses.append(gpu.Lens(placed_camera(gpu, W / H, (0.4, -0.3, -4.7)), aperture=0.15, focus=3.0))
    lenses.append(gpu.Lens(turned(gpu, W / H, 9)))
    seeds += [2 ** 64 - 1, 5]
    assert len(lenses) >= 7 and len(set(seeds)) == len(seeds)
    return lenses, seeds


def per_view(dev, lenses, seeds, w, h, spp, flags=0, first=0):
    """hrt_render_lens_device of every view, one call each."""
    import torch
    out = torch.empty((len(lenses), h, w, 3), dtype=torch.float32, device="cuda")
    for v, (lens, seed) in enumerate(zip(lenses, seeds)):
        dev.render_lens(lens, w, h, spp, seed, flags=flags, first_sample=first, out=out[v])
    return out.cpu().numpy()


def batched(dev, lenses, seeds, w, h, spp, flags=0, first=0):
    import torch
    out = torch.empty((len(lenses), h, w, 3), dtype=torch.float32, device="cuda")
    got = dev.render_lens_views(lenses, w, h, spp, seeds, flags=flags, first_sample=first, out=out)
    assert got is out
    return out.cpu().numpy()


def differing(got, want):
    bad = (bits(got) != bits(want)).any(axis=(1, 2, 3))
    return f"views that differ: {np.flatnonzero(bad).tolist()}"


# ---------------------------------------------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("name", CONTRACT_SCENES)
def test_every_frame_of_a_mixed_batch_is_the_single_lens_frame(gpu, name):
    import torch
    S = 5
    dev = scene(gpu, name)
    lenses, seeds = contract_batch(gpu)
    n = len(lenses)
    want = per_view(dev, lenses, seeds, W, H, S)
    assert np.isfinite(want).all() and all(want[v].any() for v in range(n)), name
    for a, b in itertools.combinations(range(n), 2):
        assert not np.array_equal(bits(want[a]), bits(want[b])), (name, a, b)
    got = batched(dev, lenses, seeds, W, H, S)
    assert got.shape == (n, H, W, 3) and np.array_equal(bits(got), bits(want)), f"{name}: {differing(got, want)}"
    for flags in (EXACT, NO_LDS, GAMMA):
        got = batched(dev, lenses, seeds, W, H, S, flags=flags)
        ref = per_view(dev, lenses, seeds, W, H, S, flags=flags)
        assert np.array_equal(bits(got), bits(ref)), f"{name} flags {flags}: {differing(got, ref)}"
    got = batched(dev, lenses, seeds, W, H, S, first=3)
    ref = per_view(dev, lenses, seeds, W, H, S, first=3)
    assert np.array_equal(bits(got), bits(ref)) and not np.array_equal(bits(ref), bits(want)), f"{name} first_sample 3: {differing(got, ref)}"
    acc = torch.zeros((n, H, W, 3), device="cuda")
    for v, (lens, seed) in enumerate(zip(lenses, seeds)):
        dev.render_lens(lens, W, H, S, seed, out=acc[v], accumulate=True)
    sums = acc.cpu().numpy()  # the per-view sums of samples [0, S)
    for splits in ((3, 1, 1), (1, 4)):
        acc = torch.zeros((n, H, W, 3), device="cuda")
        first = 0
        for k in splits:
            dev.render_lens_views(lenses, W, H, k, seeds, first_sample=first, out=acc, accumulate=True)
            first += k
        got = acc.cpu().numpy()
        assert np.array_equal(bits(got), bits(sums)), f"{name} accumulated over {splits}: {differing(got, sums)}"


# ---------------------------------------------------------------------------------------------------------- 2. one view per lane
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
@pytest.mark.parametrize("w,h,n", [(1, 1, 130), (3, 1, 70)])
def test_one_view_per_lane(gpu, name, w, h, n):
    """Frames of one and of three pixels: neighbouring lanes of one wave hold different views with different projections, the
    smallest shape at which a wave-uniform choice of the lens goes wrong; 130 and 210 items are more than one wave and no multiple."""
    dev = scene(gpu, name)
    lenses, seeds = mixed(gpu, n, w / h)
    S = 4
    want = per_view(dev, lenses, seeds, w, h, S)
    assert np.isfinite(want).all() and want.any()
    got = batched(dev, lenses, seeds, w, h, S)
    assert np.array_equal(bits(got), bits(want)), f"{name} {w}x{h} x {n}: {differing(got, want)}"
    got = batched(dev, lenses, seeds, w, h, S, flags=EXACT)
    ref = per_view(dev, lenses, seeds, w, h, S, flags=EXACT)
    assert np.array_equal(bits(got), bits(ref)), f"{name} {w}x{h} x {n} proof builds: {differing(got, ref)}"


# -------------------------------------------------------------------------------------------------------- 3. grid-stride hand-over
def test_lanes_hand_over_to_another_view_by_grid_stride(gpu):
    """96 views of 64 x 64 at 1 spp: 393 216 items.  The grid of a query launch is the workgroups that can be resident at once: on
    this part 256 CUs x 4 SIMDs x 5 waves per SIMD (the launch bounds of the default builds, HRT_RADIANCE_MIN_WAVES) / 4 waves per
    256-lane workgroup = 5 workgroups per CU, 256 x 5 x 256 = 327 680 lanes.  The batch has more items than that, so some lanes
    take a second item -- 80 views further on -- while their neighbours in the wave are still on their first."""
    w = h = 64
    n = 96
    assert n * w * h > 256 * 5 * 256
    dev = scene(gpu, "random_spheres")
    lenses, seeds = mixed(gpu, n, 1.0)
    want = per_view(dev, lenses, seeds, w, h, 1)
    assert np.isfinite(want).all() and all(want[v].any() for v in range(n))
    got = batched(dev, lenses, seeds, w, h, 1)
    assert np.array_equal(bits(got), bits(want)), differing(got, want)


# ------------------------------------------------------------------------------------------------- 4. pinholes: hrt_render_views
@pytest.mark.parametrize("name", CONTRACT_SCENES)
def test_a_pinhole_batch_is_render_views(gpu, name):
    S = 5
    dev = scene(gpu, name)
    cams = [turned(gpu, W / H, k) for k in range(7)]
    seeds = [11 + k for k in range(7)]
    for gamma in (0, GAMMA):
        want = dev.render_views(cams, W, H, S, seeds=seeds, flags=WAVE | gamma)
        got = dev.render_lens_views([gpu.Lens(c) for c in cams], W, H, S, seeds, flags=gamma)
        assert isinstance(got, np.ndarray) and got.shape == (7, H, W, 3)
        assert np.array_equal(bits(got), bits(want)), f"{name} gamma {gamma}: {differing(got, want)}"


# ---------------------------------------------------------------------------------------------------------------- 5. features
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
@pytest.mark.parametrize("w,h,n", [(W, H, 8), (1, 1, 130)])
def test_features_of_a_batch_are_the_single_lens_features(gpu, name, w, h, n):
    dev = scene(gpu, name)
    if n == 8:
        lenses, seeds = contract_batch(gpu)
    else:
        lenses, seeds = mixed(gpu, n, w / h)
    for first, ns in ((0, 0), (2, 3)):
        want = np.stack([dev.render_lens_features(lens, w, h, first, ns, seed) for lens, seed in zip(lenses, seeds)])
        got = dev.render_lens_views_features(lenses, w, h, first, ns, seeds)
        assert got.shape == (n, h, w, gpu.FEATURE_FLOATS) and want[..., 10].any()
        assert np.array_equal(bits(got), bits(want)), f"{name} {w}x{h} x {n}, n_samples {ns}: {differing(got, want)}"


# ------------------------------------------------------------------------------------------------------------------ 6. overlap
def test_a_batch_on_a_second_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    w, h, spp, seed = 480, 270, 8, 3
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", w, h)
    lenses, seeds = mixed(gpu, 12, 1.0)
    tiles = gpu.tiles_total(w, h)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    want = dev.render_lens_views(lenses, 48, 48, 2, seeds, out=torch.empty((12, 48, 48, 3), device="cuda"))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    got = torch.empty_like(want)
    torch.cuda.synchronize()
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        dev.render_lens_views(lenses, 48, 48, 2, seeds, out=got)
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the batch beside a render"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside a batch"


def test_batches_of_one_scene_on_two_streams_keep_their_own_tables(gpu):
    """Two batches with different lenses, back to back on different streams: the second call's table must not reach the first
    call's kernel."""
    import torch
    dev = scene(gpu, "random_spheres")
    a, seeds_a = mixed(gpu, 9, 1.0)
    b, seeds_b = mixed(gpu, 33, 1.0)
    b, seeds_b = b[::-1], seeds_b[::-1]
    want_a, want_b = per_view(dev, a, seeds_a, 40, 40, 3), per_view(dev, b, seeds_b, 8, 8, 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got_a, got_b = torch.empty((9, 40, 40, 3), device="cuda"), torch.empty((33, 8, 8, 3), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        dev.render_lens_views(a, 40, 40, 3, seeds_a, out=got_a)
    with torch.cuda.stream(s2):
        dev.render_lens_views(b, 8, 8, 2, seeds_b, out=got_b)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got_a.cpu().numpy()), bits(want_a)) and np.array_equal(bits(got_b.cpu().numpy()), bits(want_b))


def test_a_larger_batch_on_a_second_stream_grows_the_table_under_the_previous_batch(gpu):
    """One view on s1, then at once five on s2: the scene's table of views must grow while the first batch's kernel may still be
    reading the old one.  Then two views on s1 again: the grown table reused across streams.  Every frame is render_lens' bit for bit."""
    import torch
    w, h, spp = 16, 16, 2
    dev = qr.build(gpu, "cornell_mesh", w, h)[2]  # a scene of its own: its table starts empty (a mesh, and the lamp)
    lenses, seeds = mixed(gpu, 8, 1.0)  # pinhole | thin, ortho, equirect, two fisheyes | pinhole, thin
    want = per_view(dev, lenses, seeds, w, h, spp)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = torch.empty((8, h, w, 3), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        dev.render_lens_views(lenses[:1], w, h, spp, seeds[:1], out=got[:1])
    with torch.cuda.stream(s2):
        dev.render_lens_views(lenses[1:6], w, h, spp, seeds[1:6], out=got[1:6])
    torch.cuda.synchronize()
    assert np.array_equal(bits(got[:6].cpu().numpy()), bits(want[:6])), differing(got[:6].cpu().numpy(), want[:6])
    with torch.cuda.stream(s1):
        dev.render_lens_views(lenses[6:], w, h, spp, seeds[6:], out=got[6:])
    torch.cuda.synchronize()
    assert np.array_equal(bits(got[6:].cpu().numpy()), bits(want[6:])), differing(got[6:].cpu().numpy(), want[6:])


# ----------------------------------------------------------------------------------------------------------------- 7. bindings
def test_torch_and_numpy_paths_agree(gpu):
    import torch
    w, h, spp = 24, 10, 3
    dev = scene(gpu, "random_spheres")
    lenses, seeds = mixed(gpu, 5, w / h)
    n = len(lenses)
    st = gpu.Stats()
    want = dev.render_lens_views(lenses, w, h, spp, seeds, stats=st)
    assert isinstance(want, np.ndarray) and want.shape == (n, h, w, 3) and want.dtype == F32
    assert st.samples == n * w * h * spp and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
    assert np.array_equal(bits(want), bits(per_view(dev, lenses, seeds, w, h, spp)))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # rendered and consumed on the side stream, no synchronisation in between
        out = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
        got = dev.render_lens_views(lenses, w, h, spp, seeds, out=out)
        doubled_h = (got * 2).cpu().numpy()
        acc = torch.zeros((n, h, w, 3), dtype=torch.float32, device="cuda")
        dev.render_lens_views(lenses, w, h, spp, seeds, out=acc, accumulate=True)
        acc_h = acc.cpu().numpy()
    assert got is out
    assert np.array_equal(bits(doubled_h / F32(2)), bits(want))
    assert np.array_equal(bits(acc_h / F32(spp)), bits(want))
    torch.cuda.current_stream().wait_stream(side)
    sums = np.zeros((n, h, w, 3), F32)  # NumPy out: running sums through the host
    assert dev.render_lens_views(lenses, w, h, 2, seeds, out=sums, accumulate=True) is sums
    dev.render_lens_views(lenses, w, h, 1, seeds, first_sample=2, out=sums, accumulate=True)
    assert np.array_equal(bits(sums), bits(acc_h))
    default_seeds = dev.render_lens_views(lenses[:2], w, h, spp)  # seeds default to 1, as render_lens
    assert np.array_equal(bits(default_seeds), bits(per_view(dev, lenses[:2], [1, 1], w, h, spp)))
    empty = dev.render_lens_views([], w, h, spp, stats=st)
    assert empty.shape == (0, h, w, 3) and st.samples == 0
    with pytest.raises(ValueError):
        dev.render_lens_views(lenses, w, h, spp, seeds, out=torch.empty((n, h, w, 4), device="cuda"))
    with pytest.raises(ValueError):
        dev.render_lens_views(lenses, w, h, spp, seeds[:-1])
    with pytest.raises(gpu.HrtError, match="HRT_FLAG_WAVE_KERNEL"):
        dev.render_lens_views(lenses, w, h, spp, seeds, flags=WAVE)
    with pytest.raises(gpu.HrtError, match=r"views\[1\]\.lens"):
        dev.render_lens_views([lenses[0], gpu.Lens(gpu.default_camera(w / h), "ortho")], w, h, spp)
