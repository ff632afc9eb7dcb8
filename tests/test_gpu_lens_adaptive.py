"""Adaptive lens frames on the GPU (include/hrt.h hrt_render_lens_adaptive*): per-tile sample counts under any projection.

CONTRACT A: every tile of an adaptive lens frame is bit-identical to the same tile of a plain hrt_render_lens at the count that
tile was given, for every projection, with and without gamma, and the counts are what the rule of hrt_render_adaptive gives from
the tile errors of uniform lens renders (recomputed in NumPy, tests/adaptive_ref.py).  CONTRACT B: a pinhole lens gives the frame
and counts of hrt_render_adaptive under every kernel form.  Then the edges of the rounds, the flags, and the device form on a
stream of its own beside a render of the same scene.  Uniform renders are made once per (scene, lens, count, flags) and shared."""
import numpy as np
import pytest

from adaptive_ref import errors_from, expected_counts, samples, sequence, tiles_differing
import lens_ref

pytestmark = pytest.mark.gpu

W, H, SEED = 120, 67, 11  # 15 x 9 tiles; the last column and row are partly outside the image
MN, MX = 4, 32
GAMMA, NO_LDS, WAVE, STREAM, EXACT, BRUTE = 1, 2, 4, 8, 64, 128
# (scene, lens): the thin lens is focused on the mesh (the eye is at z = 6.1, the mesh stands about z = -0.6)
CASES = {"thin": ("cornell_mesh", ("perspective", 0.2, 6.7, 0.0)), "equirect": ("random_spheres", ("equirect", 0.0, 1.0, 0.0)),
         "fisheye": ("backrooms_pool", ("fisheye", 0.0, 1.0, 180.0)), "ortho": ("cornell_box", ("ortho", 0.0, 1.0, 3.0))}

_scenes, _uniform = {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scene(gpu, name, w=W, h=H):
    """(device scene, default camera) of a named scene for a w x h frame, built once."""
    if (name, w, h) not in _scenes:
        desc = gpu.HostScene().setup(name, w / h, 1).flatten()
        _scenes[name, w, h] = (desc, gpu.DeviceScene(desc), gpu.default_camera(w / h))
    return _scenes[name, w, h][1:]


def case(gpu, which, w=W, h=H):
    name, (proj, ap, fo, ex) = CASES[which]
    dev, cam = scene(gpu, name, w, h)
    return dev, cam, gpu.Lens(cam, proj, aperture=ap, focus=fo, extent=ex)


def uniform(gpu, which, counts, flags=0, w=W, h=H):
    """{count: hrt_render_lens at that count} for the lens of `which` (`which` may also be (key, dev, lens))."""
    key, dev, lens = which if isinstance(which, tuple) else (which, *case(gpu, which, w, h)[::2])
    out = {}
    for c in np.unique(np.asarray(counts)):
        k = (key, w, h, int(c), flags)
        if k not in _uniform:
            _uniform[k] = dev.render_lens(lens, w, h, int(c), SEED, flags=flags)
        out[int(c)] = _uniform[k]
    return out


def errors_at(gpu, which, mn=MN, mx=MX, w=W, h=H):
    return errors_from(uniform(gpu, which, sequence(mn, mx), 0, w, h), mn, mx)


def threshold_of(err, mn=MN):
    """The median of the positive tile errors at min_spp: tiles of error 0 (outside a fisheye's circle) do not pull it down."""
    e = err[mn]
    return float(np.median(e[e > 0]))


def assert_tiles_match(frame, counts, refs, w=W, h=H):
    assert frame.shape == (h, w, 3)
    bad = tiles_differing(frame, counts, refs)
    assert not bad, f"{len(bad)} tiles differ from hrt_render_lens at their count, first (tile y, tile x, count): {bad[:5]}"


# ---------------------------------------------------------------------------------------------------------------- CONTRACT A
@pytest.mark.parametrize("which", list(CASES))
def test_every_tile_is_the_lens_render_at_its_count(gpu, which):
    dev, cam, lens = case(gpu, which)
    err = errors_at(gpu, which)
    thr = threshold_of(err)
    for gamma in (0, GAMMA):
        st = gpu.Stats()
        frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=gamma, stats=st)
        assert counts.shape == ((H + 7) // 8, (W + 7) // 8) and counts.dtype == np.uint32
        print(f"{which} gamma {gamma}: threshold {thr:.6g}, counts {dict(zip(*np.unique(counts, return_counts=True)))}")
        assert counts.min() == MN and counts.max() > MN, f"threshold {thr} gave no spread of counts {np.unique(counts)}"
        assert set(np.unique(counts).tolist()) <= set(sequence(MN, MX)[1:])
        assert_tiles_match(frame, counts, uniform(gpu, which, counts, gamma))
        assert st.samples == samples(counts, W, H)
        assert st.kernel_ms > 0 and st.total_ms >= st.kernel_ms


def test_fisheye_tiles_outside_the_image_circle_stop_at_the_minimum_and_are_black(gpu):
    """At 120 x 67 the 180 degree circle is inscribed in the frame's height: the corner tiles lie wholly outside it, every sample
    of theirs is degenerate, their error is 0 and their pixels are 0."""
    dev, cam, lens = case(gpu, "fisheye")
    thr = threshold_of(errors_at(gpu, "fisheye"))
    frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED)
    # a tile is wholly outside when the corner of its pixel area nearest the centre is: |q| of any film position in it exceeds 1
    aspect = np.float64(cam.aspect)
    ty, tx = counts.shape
    outside = np.zeros(counts.shape, bool)
    for y in range(ty):
        for x in range(tx):
            x0, x1 = x * 8, min(x * 8 + 8, W)
            y0, y1 = y * 8, min(y * 8 + 8, H)
            u = np.clip(0.5, x0 / W, x1 / W)  # the film position of the tile nearest the centre
            v = np.clip(0.5, y0 / H, y1 / H)
            outside[y, x] = np.hypot((2 * u - 1) * aspect, 1 - 2 * v) > 1 + 1e-4
    assert outside[0, 0] and outside[0, -1] and outside[-1, 0] and outside[-1, -1] and 8 <= outside.sum() < counts.size // 2, outside.sum()
    assert (counts[outside] == MN).all(), counts[outside]
    pp = np.repeat(np.repeat(outside, 8, axis=0), 8, axis=1)[:H, :W]
    assert (bits(frame[pp]) == 0).all(), "pixels of tiles outside the image circle"
    assert frame[~pp].any()


# -------------------------------------------------------------------------------------------------------------------- policy
@pytest.mark.parametrize("which", list(CASES))
def test_counts_follow_the_policy(gpu, which):
    """Every count is what the stated rule gives from the tile errors of uniform lens renders; tiles whose error lies within a
    relative 1e-5 of the threshold at a judged count are left out, at most 5 of the 135."""
    dev, cam, lens = case(gpu, which)
    err = errors_at(gpu, which)
    thr = threshold_of(err)
    near = np.zeros(err[MN].shape, dtype=bool)
    for n, e in err.items():
        near |= np.abs(e - np.float32(thr)) <= 1e-5 * thr
    print(f"{which}: threshold {thr:.6g}, {int(near.sum())} tiles within 1e-5 of it")
    assert near.sum() <= 5, int(near.sum())
    frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED)
    exp = expected_counts(err, MN, MX, thr)
    assert len(np.unique(exp)) > 1
    assert np.array_equal(counts[~near], exp[~near]), np.argwhere((counts != exp) & ~near)[:5]


# ---------------------------------------------------------------------------------------------------------------- CONTRACT B
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
def test_a_pinhole_lens_is_the_adaptive_render_under_every_kernel_form(gpu, name):
    dev, cam = scene(gpu, name)
    lens = gpu.Lens(cam)
    err = errors_at(gpu, ("pinhole " + name, dev, lens))
    thr = threshold_of(err)
    for gamma in (0, GAMMA):
        frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=gamma)
        assert len(np.unique(counts)) > 1
        for form in (0, WAVE, STREAM):
            want, want_counts = dev.render_adaptive(cam, W, H, MN, MX, thr, seed=SEED, flags=gamma | form)
            assert np.array_equal(counts, want_counts), f"{name} gamma {gamma} form {form}: other counts"
            assert np.array_equal(bits(frame), bits(want)), f"{name} gamma {gamma} form {form}: other pixels"


# --------------------------------------------------------------------------------------------------------------------- edges
def test_extreme_thresholds_equal_bounds_and_a_clipped_last_round(gpu):
    dev, cam, lens = case(gpu, "thin")
    for gamma in (0, GAMMA):
        frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, 0.0, seed=SEED, flags=gamma)
        assert (counts == MX).all()
        assert np.array_equal(bits(frame), bits(uniform(gpu, "thin", [MX], gamma)[MX]))
        frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, float("inf"), seed=SEED, flags=gamma)
        assert (counts == MN).all()
        assert np.array_equal(bits(frame), bits(uniform(gpu, "thin", [MN], gamma)[MN]))
        frame, counts = dev.render_lens_adaptive(lens, W, H, 6, 6, 0.0, seed=SEED, flags=gamma)
        assert (counts == 6).all()
        assert np.array_equal(bits(frame), bits(uniform(gpu, "thin", [6], gamma)[6]))
        # max = 22 is no power-of-two multiple of 4: 4, 8, 16, then a last round of 6
        frame, counts = dev.render_lens_adaptive(lens, W, H, MN, 22, 0.0, seed=SEED, flags=gamma)
        assert (counts == 22).all()
        assert np.array_equal(bits(frame), bits(uniform(gpu, "thin", [22], gamma)[22]))
    err = errors_at(gpu, "thin", MN, 22)
    thr = threshold_of(err)
    frame, counts = dev.render_lens_adaptive(lens, W, H, MN, 22, thr, seed=SEED)
    assert counts.max() == 22 and counts.min() == MN and set(np.unique(counts).tolist()) <= {4, 8, 16, 22}
    assert_tiles_match(frame, counts, uniform(gpu, "thin", counts))


@pytest.mark.parametrize("w,h", [(8, 8), (9, 1)])
def test_tiny_frames(gpu, w, h):
    """8 x 8: one tile, and the list stays NULL through round 1.  9 x 1: two tiles, 9 of their 128 lanes in the image."""
    for which in ("thin", "equirect"):
        dev, cam, lens = case(gpu, which, w, h)
        err = errors_at(gpu, which, MN, MX, w, h)
        for thr in (0.0, float(err[MN].max()), float("inf")):  # every tile to max; the noisiest tile alone goes on; none does
            frame, counts = dev.render_lens_adaptive(lens, w, h, MN, MX, thr, seed=SEED)
            assert counts.shape == ((h + 7) // 8, (w + 7) // 8)
            assert np.array_equal(counts, expected_counts(err, MN, MX, thr)), (which, thr, counts)
            assert_tiles_match(frame, counts, uniform(gpu, which, counts, 0, w, h), w, h)
            st = gpu.Stats()
            dev.render_lens_adaptive(lens, w, h, MN, MX, thr, seed=SEED, stats=st)
            assert st.samples == samples(counts, w, h)


# --------------------------------------------------------------------------------------------------------------------- flags
def test_the_proof_builds_and_the_tree_from_global_memory_give_the_same_frame_and_counts(gpu):
    dev, cam, lens = case(gpu, "thin")
    thr = threshold_of(errors_at(gpu, "thin"))
    base, base_counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED)
    assert len(np.unique(base_counts)) > 1
    for f in (EXACT, EXACT | BRUTE, NO_LDS):
        frame, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=f)
        assert np.array_equal(counts, base_counts), f"flags {f}: other counts"
        assert np.array_equal(bits(frame), bits(base)), f"flags {f}: other pixels"
    with pytest.raises(gpu.HrtError, match="HRT_FLAG_WAVE_KERNEL"):
        dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=WAVE)


# --------------------------------------------------------------------------------------------------------------- device form
def test_device_form_on_its_own_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    dev, cam, lens = case(gpu, "thin")
    thr = threshold_of(errors_at(gpu, "thin"))
    spp = 8
    want, want_counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=GAMMA)
    tiles = gpu.tiles_total(W, H)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, W, H, spp, SEED, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.render_tiles(cam, W, H, spp, SEED, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        got, counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=GAMMA, out=out)
        got_h, counts_h = got.cpu().numpy(), counts.cpu().numpy()  # consumed on the same stream
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert got is out and counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == want_counts.shape
    assert np.array_equal(counts_h.astype(np.uint32), want_counts), "the counts of the device form"
    assert np.array_equal(bits(got_h), bits(want)), "the frame of the device form"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside an adaptive lens frame"
    again, again_counts = dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, flags=GAMMA, out=torch.empty_like(out))  # default stream, after s2
    assert np.array_equal(bits(again.cpu().numpy()), bits(want)) and np.array_equal(again_counts.cpu().numpy().astype(np.uint32), want_counts)


# ------------------------------------------------------------------------------------------------- the scene's shared scratch
def test_camera_and_lens_rounds_share_one_scenes_scratch(gpu):
    """hrt_render_adaptive and hrt_render_lens_adaptive carve one grow-only pair of buffers of the scene (the compact sums; two
    lists, keep flags, count map and counter) by the tile count of their own call.  Alternating the two on ONE scene over frames
    that shrink and grow, each (frame, counts) has the bits of the same call on a fresh scene of the same description: at
    threshold 0 (every round runs), +inf (round 1 ends it) and the median tile error of that frame (lists of mixed length).
    Then the binding's refusals that need a tensor on the GPU, text for text (tests/test_python_refusals.py)."""
    import json
    import torch
    import test_python_refusals as refusals
    mn, mx = 4, 16
    desc = gpu.HostScene().setup("cornell_mesh", 40 / 24, 1).flatten()
    big, small = gpu.default_camera(40 / 24), gpu.default_camera(24 / 16)
    fish = gpu.Lens(small, "fisheye", extent=180.0)
    thin = gpu.Lens(big, "perspective", aperture=0.05, focus=6.7)
    calls = [("render_adaptive", big, 40, 24), ("render_lens_adaptive", fish, 24, 16), ("render_adaptive", small, 24, 16),
             ("render_lens_adaptive", thin, 40, 24)]
    ref = gpu.DeviceScene(desc)
    medians = []
    for fn, view, w, h in calls:
        plain = ref.render if fn == "render_adaptive" else ref.render_lens
        frames = {c: plain(view, w, h, c, SEED) for c in sequence(mn, mx)}
        frames = {c: f[0] if isinstance(f, tuple) else f for c, f in frames.items()}  # render also returns its Stats
        medians.append(threshold_of(errors_from(frames, mn, mx), mn))
    ref.close()
    shared = gpu.DeviceScene(desc)
    for which in ("zero", "inf", "median"):
        for (fn, view, w, h), median in zip(calls, medians):
            thr = {"zero": 0.0, "inf": float("inf"), "median": median}[which]
            frame, counts = getattr(shared, fn)(view, w, h, mn, mx, thr, seed=SEED)
            fresh = gpu.DeviceScene(desc)
            want, want_counts = getattr(fresh, fn)(view, w, h, mn, mx, thr, seed=SEED)
            fresh.close()
            print(f"{fn} {w}x{h} threshold {thr:.6g}: counts {dict(zip(*np.unique(counts, return_counts=True)))}")
            assert counts.shape == ((h + 7) // 8, (w + 7) // 8)
            assert np.array_equal(counts, want_counts), f"{fn} {w}x{h} threshold {thr}: other counts than on a fresh scene"
            assert np.array_equal(bits(frame), bits(want)), f"{fn} {w}x{h} threshold {thr}: other pixels than on a fresh scene"
            if which == "zero":
                assert (counts == mx).all()
            elif which == "inf":
                assert (counts == mn).all()
            else:
                assert len(np.unique(counts)) > 1, f"{fn} {w}x{h}: threshold {thr} gave no spread of counts"
    shared.close()
    golden = json.load(open(refusals.GOLDEN))
    cases = refusals.gpu_cases(gpu, torch)
    assert {"gpu_rad_keys", "gpu_rad_out", "gpu_bake_rays_keys", "gpu_la_stats"} <= set(cases)
    for name, call in cases.items():
        assert refusals.refusal(call) == golden[name], name
