"""Adaptive lit frames on the GPU (include/hrt.h "Adaptive lit frames"): per-tile sample counts for a lens frame whose paths end in
a probe volume.

CONTRACT A: every tile of an adaptive lit frame is bit-identical to the same tile of hrt_render_lit at the count that tile was
given -- for a thin lens with one segment, an equirectangular lens with tail_after = 1 and a fisheye with tail_after = 2 and the
facing, visible look-up --, with and without gamma, and the counts are what the rule of hrt_render_adaptive gives from the tile
errors of uniform hrt_render_lit frames (recomputed in NumPy, tests/adaptive_ref.py) on EVERY tile: the threshold is put into the
widest gap between two neighbouring judged errors, so no tile has to be excused.  Then the fisheye's corners, the extreme thresholds,
tiny frames, the round scratch shared with the two other adaptive calls, the device form on a stream of its own, the refusals that
need a volume, resources and the command-line tool.  Uniform frames are made once per (case, count, flags) and shared."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import probe_ref
import test_gpu_live_resources as tlr
import test_gpu_probe_lit as tl
from adaptive_ref import errors_from, expected_counts, samples, sequence, tiles_differing
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, SEED = 120, 67, 11  # 15 x 9 tiles; the last column and row are partly outside the image
MN, MX = 4, 32
GAMMA, WAVE = 1, 4
HRT_ERR_INVALID = -1
NAN, INF = float("nan"), float("inf")
FACING, VISIBLE = tl.FACING, tl.VISIBLE
# (scene, lens, the lit arguments): the thin lens is focused on the mesh (the eye is at z = 6.1, the mesh stands about z = -0.6)
CASES = {"thin": ("cornell_mesh", ("perspective", 0.2, 6.7, 0.0), dict(tail_after=None)),
         "equirect": ("random_spheres", ("equirect", 0.0, 1.0, 0.0), dict(tail_after=1)),
         "fisheye": ("backrooms_pool", ("fisheye", 0.0, 1.0, 180.0), dict(tail_after=2, eval_flags=FACING | VISIBLE))}

_scenes, _volumes, _uniform = {}, {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scene(gpu, name, w=W, h=H):
    """(device scene, default camera) of a named scene for a w x h frame, built once."""
    if (name, w, h) not in _scenes:
        desc = gpu.HostScene().setup(name, w / h, 1).flatten()
        _scenes[name, w, h] = (gpu.DeviceScene(desc), gpu.default_camera(w / h))
    return _scenes[name, w, h]


def volume(gpu, name):
    """A volume of random coefficients and depth moments over the scene's probe box, made once."""
    if name not in _volumes:
        _volumes[name] = tl.random_volume(gpu, probe_ref.BOXES[name][:2], 5)[0]
    return _volumes[name]


def case(gpu, which, w=W, h=H):
    name, (proj, ap, fo, ex), lit = CASES[which]
    dev, cam = scene(gpu, name, w, h)
    return dev, cam, gpu.Lens(cam, proj, aperture=ap, focus=fo, extent=ex), volume(gpu, name), lit


def uniform(gpu, which, counts, flags=0, w=W, h=H):
    """{count: hrt_render_lit at that count} for the case `which`: the parent's code, the reference of everything here."""
    dev, cam, lens, vol, lit = case(gpu, which, w, h)
    out = {}
    for c in np.unique(np.asarray(counts)):
        k = (which, w, h, int(c), flags)
        if k not in _uniform:
            _uniform[k] = dev.render_lit(lens, vol, w, h, int(c), SEED, flags=flags, **lit)
        out[int(c)] = _uniform[k]
    return out


def errors_at(gpu, which, mn=MN, mx=MX, w=W, h=H):
    return errors_from(uniform(gpu, which, sequence(mn, mx), 0, w, h), mn, mx)


def threshold_of(err, mn=MN):
    """The threshold no tile has to be excused from: of the sorted distinct positive judged errors of all counts, the neighbouring
    pair (a, b) inside the interquartile range of the (positive) errors at min_spp with the largest ratio, and sqrt(a b) between them.  The
    judge's arithmetic is allowed a relative 1e-5 by the existing policy test; the pair must be ten times that apart -- asserted,
    not skipped."""
    every = np.unique(np.concatenate([e.ravel() for e in err.values()]).astype(np.float64))
    every = every[every > 0]
    at_min = err[mn].astype(np.float64)
    q25, q75 = np.percentile(at_min[at_min > 0], [25, 75])  # of the positive ones, as step 1: tiles of error 0 (outside a fisheye's circle) judge nothing
    lo, hi = every[:-1], every[1:]
    inside = (lo >= q25) & (hi <= q75)
    assert inside.any(), f"no two neighbouring judged errors inside the interquartile range {q25:.6g} .. {q75:.6g} of the errors at {mn} samples"
    k = np.flatnonzero(inside)[np.argmax(hi[inside] / lo[inside])]
    a, b = lo[k], hi[k]
    print(f"threshold between {a:.9g} and {b:.9g} (ratio {b / a:.6f}) in the interquartile range {q25:.6g} .. {q75:.6g}")
    assert b / a >= 1 + 1e-4, (a, b)
    thr = float(np.sqrt(a * b))
    assert a < F32(thr) < b
    return thr


def assert_tiles_match(frame, counts, refs, w=W, h=H):
    assert frame.shape == (h, w, 3)
    bad = tiles_differing(frame, counts, refs)
    assert not bad, f"{len(bad)} tiles differ from hrt_render_lit at their count, first (tile y, tile x, count): {bad[:5]}"


# ---------------------------------------------------------------------------------------------------------------- CONTRACT A
@pytest.mark.parametrize("which", list(CASES))
def test_every_tile_is_the_lit_frame_at_its_count(gpu, which):
    dev, cam, lens, vol, lit = case(gpu, which)
    thr = threshold_of(errors_at(gpu, which))
    for gamma in (0, GAMMA):
        st = gpu.Stats()
        frame, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, seed=SEED, flags=gamma, stats=st, **lit)
        assert counts.shape == ((H + 7) // 8, (W + 7) // 8) and counts.dtype == np.uint32
        print(f"{which} gamma {gamma}: threshold {thr:.6g}, counts {dict(zip(*np.unique(counts, return_counts=True)))}")
        assert counts.min() == MN and counts.max() > MN, f"threshold {thr} gave no spread of counts {np.unique(counts)}"
        assert set(np.unique(counts).tolist()) <= set(sequence(MN, MX)[1:])
        assert_tiles_match(frame, counts, uniform(gpu, which, counts, gamma))
        assert st.samples == samples(counts, W, H)
        assert st.kernel_ms > 0 and st.total_ms >= st.kernel_ms


# -------------------------------------------------------------------------------------------------------------------- policy
@pytest.mark.parametrize("which", list(CASES))
def test_counts_follow_the_policy_on_every_tile(gpu, which):
    dev, cam, lens, vol, lit = case(gpu, which)
    err = errors_at(gpu, which)
    thr = threshold_of(err)
    frame, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, seed=SEED, **lit)
    exp = expected_counts(err, MN, MX, thr)
    assert len(np.unique(exp)) > 1
    assert np.array_equal(counts, exp), np.argwhere(counts != exp)[:5]


def test_fisheye_tiles_outside_the_image_circle_stop_at_the_minimum_and_are_exact_zeros(gpu):
    """At 120 x 67 the 180 degree circle is inscribed in the frame's height: the corner tiles lie wholly outside it, every sample
    of theirs is degenerate, their error is 0 and their pixels are 0."""
    dev, cam, lens, vol, lit = case(gpu, "fisheye")
    thr = threshold_of(errors_at(gpu, "fisheye"))
    frame, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, seed=SEED, **lit)
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


# --------------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("which", list(CASES))
def test_extreme_thresholds(gpu, which):
    dev, cam, lens, vol, lit = case(gpu, which)
    err = errors_at(gpu, which)
    above = float(np.nextafter(F32(max(e.max() for e in err.values())), F32(np.inf)))
    for gamma in (0, GAMMA):
        for thr in (above, INF):
            frame, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, seed=SEED, flags=gamma, **lit)
            assert (counts == MN).all()
            assert np.array_equal(bits(frame), bits(uniform(gpu, which, [MN], gamma)[MN])), "a threshold above every error: render_lit at 4, whole frame"
        frame, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, 0.0, seed=SEED, flags=gamma, **lit)
        positive = np.all([e > 0 for e in err.values()], axis=0)
        assert positive.any() and (counts[positive] == MX).all(),"threshold 0: every tile whose judged errors are all positive goes to 32"
        assert_tiles_match(frame, counts, uniform(gpu, which, counts, gamma))


@pytest.mark.parametrize("w,h", [(8, 8), (9, 1)])
def test_tiny_frames(gpu, w, h):
    """8 x 8: one tile, and the list stays NULL through round 1.  9 x 1: two tiles, 9 of their 128 lanes in the image."""
    for which in ("thin", "equirect"):
        dev, cam, lens, vol, lit = case(gpu, which, w, h)
        err = errors_at(gpu, which, MN, MX, w, h)
        for thr in (0.0, float(err[MN].max()), INF):  # every tile to max; the noisiest tile alone goes on; none does
            frame, counts = dev.render_lit_adaptive(lens, vol, w, h, MN, MX, thr, seed=SEED, **lit)
            assert counts.shape == ((h + 7) // 8, (w + 7) // 8)
            assert np.array_equal(counts, expected_counts(err, MN, MX, thr)), (which, thr, counts)
            assert_tiles_match(frame, counts, uniform(gpu, which, counts, 0, w, h), w, h)
            st = gpu.Stats()
            dev.render_lit_adaptive(lens, vol, w, h, MN, MX, thr, seed=SEED, stats=st, **lit)
            assert st.samples == samples(counts, w, h)


# ------------------------------------------------------------------------------------------------- the scene's shared scratch
def test_the_three_adaptive_calls_share_one_scenes_scratch(gpu):
    """hrt_render_adaptive, hrt_render_lens_adaptive and hrt_render_lit_adaptive carve one grow-only set of buffers of the scene by
    the tile count of their own call.  Called alternately on ONE scene over frames that shrink and grow, each gives the bits of the
    same call on a fresh scene of the same description, pass after pass."""
    mn, mx = 4, 16
    desc = gpu.HostScene().setup("cornell_mesh", 40 / 24, 1).flatten()
    big, small = gpu.default_camera(40 / 24), gpu.default_camera(24 / 16)
    vol = volume(gpu, "cornell_mesh")
    fish = gpu.Lens(small, "fisheye", extent=180.0)
    thin = gpu.Lens(big, "perspective", aperture=0.05, focus=6.7)
    calls = [("render_adaptive", (big, 40, 24), {}), ("render_lit_adaptive", (fish, vol, 24, 16), dict(tail_after=1)),
             ("render_lens_adaptive", (thin, 40, 24), {}), ("render_lit_adaptive", (thin, vol, 40, 24), dict(eval_flags=VISIBLE)),
             ("render_adaptive", (small, 24, 16), {}), ("render_lens_adaptive", (fish, 24, 16), {})]
    want = []
    for fn, args, kw in calls:
        fresh = gpu.DeviceScene(desc)
        frames = {c: (fresh.render(*args, c, SEED)[0] if fn == "render_adaptive" else
                      fresh.render_lens(*args, c, SEED) if fn == "render_lens_adaptive" else fresh.render_lit(*args, c, SEED, **kw)) for c in sequence(mn, mx)}
        e = errors_from(frames, mn, mx)[mn]
        thr = float(np.median(e[e > 0]))
        frame, counts = getattr(fresh, fn)(*args, mn, mx, thr, seed=SEED, **kw)
        assert len(np.unique(counts)) > 1, f"{fn}: threshold {thr} gave no spread of counts"
        want.append((thr, frame, counts))
        fresh.close()
    shared = gpu.DeviceScene(desc)
    for round_ in range(2):
        for (fn, args, kw), (thr, frame, counts) in zip(calls, want):
            got, got_counts = getattr(shared, fn)(*args, mn, mx, thr, seed=SEED, **kw)
            assert np.array_equal(got_counts, counts), f"pass {round_}, {fn}: other counts than on a fresh scene"
            assert np.array_equal(bits(got), bits(frame)), f"pass {round_}, {fn}: other pixels than on a fresh scene"
    shared.close()


# --------------------------------------------------------------------------------------------------------------- device form
def test_device_form_on_its_own_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    dev, cam, lens, vol, lit = case(gpu, "thin")
    thr = threshold_of(errors_at(gpu, "thin"))
    spp = 8
    want, want_counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, seed=SEED, flags=GAMMA, **lit)
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
        got, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, seed=SEED, flags=GAMMA, out=out, **lit)
        got_h, counts_h = got.cpu().numpy(), counts.cpu().numpy()  # consumed on the same stream
    torch.cuda.synchronize()
    dev.check_last_launch()
    assert got is out and counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == want_counts.shape
    assert np.array_equal(counts_h.astype(np.uint32), want_counts), "the counts of the device form"
    assert np.array_equal(bits(got_h), bits(want)), "the frame of the device form"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside an adaptive lit frame"
    with pytest.raises(ValueError, match="render_lit_adaptive: stats are the blocking form's"):
        dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, out=out, stats=gpu.Stats())
    with pytest.raises(gpu.HrtError, match="HRT_FLAG_WAVE_KERNEL"):
        dev.render_lit_adaptive(lens, vol, W, H, MN, MX, thr, flags=WAVE)


# ------------------------------------------------------------------------------------------- refusals that need a volume
def test_the_refusals_that_need_a_volume_come_in_the_order_of_lit_rays(gpu):
    lib = gpu.device_lib()
    OUT = 0x2000
    L = gpu.Lens(gpu.default_camera(W / H))
    P = gpu.Adaptive(MN, MX, 0.1)

    def call(entry, v, ef=0, bias=0.0, tail=0):
        rc = getattr(lib, entry)(None, v._h, C.byref(L), W, H, C.byref(P), 1, 0, ef, bias, tail, C.c_void_p(OUT), None, None)
        return rc, lib.hrt_last_error().decode()

    for entry in ("hrt_render_lit_adaptive_device", "hrt_render_lit_adaptive"):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as v:
            for tail in (0, 2):
                assert call(entry, v, ef=1 | VISIBLE, bias=NAN, tail=tail)[1].startswith(entry + ": eval_flags: HRT_PROBE_EVAL_RADIANCE"), "by name, first"
                assert call(entry, v, ef=VISIBLE, bias=NAN, tail=tail) == (HRT_ERR_INVALID, entry + ": the volume has no coefficients yet (hrt_probe_volume_update)")
            v.update(np.zeros((2, 9, 3), F32))
            for tail in (0, 2):
                assert call(entry, v, ef=VISIBLE | FACING, bias=NAN, tail=tail) == \
                    (HRT_ERR_INVALID, entry + ": eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet (hrt_probe_volume_update_depth)")
                for bad in (NAN, INF, -INF):
                    assert call(entry, v, ef=FACING, bias=bad, tail=tail)[1].startswith(entry + ": bias must be finite"), bad
                assert call(entry, v, ef=FACING, tail=tail) == (HRT_ERR_INVALID, entry + ": scene is NULL")
            v.update_depth(np.zeros((2, 64, 3), F32))
            assert call(entry, v, ef=VISIBLE) == (HRT_ERR_INVALID, entry + ": scene is NULL")
            assert call(entry, v, ef=VISIBLE, tail=7)[1].startswith(entry + ": tail_after must be in 1 .. HRT_MAXBOUNCES"), "tail_after before the volume"
        closed = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1)
        closed.close()
        assert call(entry, closed) == (HRT_ERR_INVALID, entry + ": volume is NULL"), "a closed volume has no handle"
    dev, cam, lens, vol, lit = case(gpu, "thin")
    with pytest.raises(gpu.HrtError, match="hrt_render_lit_adaptive: eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet"):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as v:
            dev.render_lit_adaptive(lens, v.update(np.zeros((2, 9, 3), F32)), W, H, MN, MX, 0.1, eval_flags=VISIBLE)


# ------------------------------------------------------------------------------------------------------------ resources
def test_repeated_calls_leave_no_device_buffers_behind(gpu):
    import torch
    torch.cuda.synchronize()
    see = tlr.Peak(gpu)
    before = see()
    desc = gpu.HostScene().setup("cornell_mesh", 40 / 24, 1).flatten()
    dev, cam = gpu.DeviceScene(desc), gpu.default_camera(40 / 24)
    vol = tl.zero_volume(gpu, probe_ref.BOXES["cornell_mesh"][:2])
    L = gpu.Lens(cam, "perspective", aperture=0.05, focus=6.7)
    out = torch.zeros((24, 40, 3), dtype=torch.float32, device="cuda")

    def round_():
        for tail in (None, 2):
            dev.render_lit_adaptive(L, vol, 40, 24, 4, 16, 0.05, tail_after=tail)
            dev.render_lit_adaptive(L, vol, 40, 24, 4, 16, 0.05, out=out, tail_after=tail)
        torch.cuda.synchronize()
        return see()

    held = round_()  # the sums, the round scratch and the frame are the scene's own grow-only buffers: freed with the scene
    for _ in range(3):
        assert round_() == held, "repeated calls leave hrt_debug_live_resources where the first left it"
    peak = see.peak
    round_()
    assert see.peak == peak, "a further round peaks where the earlier ones did"
    vol.close()
    dev.close()
    assert gpu.live_resources() == before


# ------------------------------------------------------------------------------------------------------------------ the CLI
def test_the_cli_writes_the_frame_the_library_computes_and_prints_its_mean_spp(gpu, tmp_path):
    lo, hi, counts, w, h = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (2, 2, 1), 40, 24
    desc = gpu.HostScene().setup("cornell_box", w / h, 1).flatten()
    dev, cam = gpu.DeviceScene(desc), gpu.default_camera(w / h)
    lens = gpu.Lens(cam, "perspective", aperture=0.2, focus=6.7)
    base = [os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", str(w), "--h", str(h),
            "--probe-grid", "2,2,1", "--probe-box", "-1.0,-1.0,-1.0,1.0,1.0,1.0", "--probe-lit", "--spp", str(MX), "--spp-min", str(MN),
            "--lens", "perspective", "--aperture", "0.2", "--focus", "6.7", "--probe-tail", "1", "--out", str(tmp_path / "out.ppm")]
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        vol.update(dev.probes(gpu.probe_grid(lo, hi, *counts), MX, seed=1))  # without --probe-bounces the grid is path-traced, at --spp
        frames = {c: dev.render_lit(lens, vol, w, h, c, 1, tail_after=1) for c in sequence(MN, MX)}
        e = errors_from(frames, MN, MX)[MN]
        thr = float(F32(np.median(e[e > 0])))
        frame, tile_spp = dev.render_lit_adaptive(lens, vol, w, h, MN, MX, thr, seed=1, flags=GAMMA, tail_after=1)
    r = subprocess.run(base + ["--adaptive", f"{thr:.9g}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    mine = tmp_path / "mine.ppm"
    gpu.write_ppm(str(mine), frame)
    assert (tmp_path / "out.ppm").read_bytes() == mine.read_bytes()
    m = re.search(r"mean ([0-9.eE+-]+) spp", r.stdout)
    assert m, r.stdout
    mean = float(m.group(1))
    assert MN < mean < MX and abs(mean - samples(tile_spp, w, h) / (w * h)) <= 1e-3 * mean, (mean, r.stdout)
    r = subprocess.run(base + ["--adaptive", f"{thr:.9g}", "--views", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--views renders plain frames on one GPU: it cannot be combined with --adaptive" in r.stderr, r.stderr
    dev.close()
