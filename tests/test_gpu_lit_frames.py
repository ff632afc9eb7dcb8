"""Lit frames on the GPU (include/hrt.h "Lit frames"), every comparison bit for bit: (A) the fused frame is the fold of hrt_lens_rays
and hrt_trace_lit[_paths] over its samples, for every lens, tail, look-up and bias; (B) running sums, gamma and a sentinel border;
(C) a pinhole lit frame is hrt_camera_rays' composition, also in the proof builds; (D) where no path reaches the tail the lit frame
is hrt_render_lens'; (E) frame v of a batch is the single frame of view v; (F) the blocking forms are the device forms and fill
their stats; (G) the refusals that need a volume, as hrt_trace_lit refuses them; (H) the command-line tool writes the bytes the old
per-sample loop wrote; (I) repeated calls leave no device buffer behind.  Frames are 19 x 11 = 209 pixels: the last wave is
partial, and in a batch waves straddle views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lit_paths_ref as lp
import test_gpu_lens as tlens
import test_gpu_lit_paths as tp
import test_gpu_live_resources as tlr
import test_gpu_probe_lit as tl
import test_gpu_rays as qr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W, H = 19, 11
NPIX = W * H
EXACT, GAMMA, ACCUMULATE = 64, 1, 512
HRT_ERR_INVALID = -1
NAN, INF = float("nan"), float("inf")
FACING, VISIBLE = tl.FACING, tl.VISIBLE
SCENES = sorted(tl.TAIL_SCENES)  # cornell_mesh, random_spheres
TAILS = (None, 1, 2, 6)
FIRST, S, SEED = 3, 5, 11
bits = qr.bits

_cases, _rays = {}, {}


def case(gpu, name):
    """(device scene, camera, volume of random coefficients and depth, the lenses by name) of a scene, built once."""
    if name not in _cases:
        _, desc, dev, cam = qr.build(gpu, name, W, H)
        vol, _, _ = tl.random_volume(gpu, tl.TAIL_SCENES[name], 5)
        lenses = {k: v for k, v in tlens.lenses(gpu, cam).items() if k in ("pinhole", "thin", "ortho", "equirect")}
        lenses["fisheye200"] = gpu.Lens(cam, "fisheye", extent=200.0)
        _cases[name] = (dev, cam, vol, lenses)
    return _cases[name]


def lens_rays(gpu, name, lname, s, seed=SEED):
    """hrt_lens_rays(lens, W, H, s, seed) of a case's lens on the device, made once and left unchanged."""
    key = (name, lname, s, seed)
    if key not in _rays:
        _rays[key] = gpu.lens_rays(case(gpu, name)[3][lname], W, H, s, seed)
    return _rays[key]


def folded(gpu, name, lname, vol, first, n, seed=SEED, flags=0, **lit):
    """The running sums of the composition: per sample hrt_lens_rays, then hrt_trace_lit[_paths] of one sample, accumulated."""
    import torch
    dev = case(gpu, name)[0]
    acc = torch.zeros((NPIX, 3), dtype=torch.float32, device="cuda")
    for s in range(first, first + n):
        dev.trace_lit(lens_rays(gpu, name, lname, s, seed), vol, 1, first_sample=s, seed=seed, out=acc, accumulate=True, flags=flags, **lit)
    return acc.cpu().numpy().reshape(H, W, 3)


def frame(dev, lens, vol, spp, seed=SEED, **kw):
    """render_lit through the device form into a torch tensor, back as NumPy."""
    import torch
    return dev.render_lit(lens, vol, W, H, spp, seed, out=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"), **kw).cpu().numpy()


# ------------------------------------------------------------------------------------ A. the fused frame is the fold of the query
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("name", SCENES)
def test_the_fused_frame_is_the_fold_of_lens_rays_and_lit_rays(gpu, name, tail):
    dev, cam, vol, lenses = case(gpu, name)
    for lname, lens in lenses.items():
        for ef in tl.EVAL_FLAGS:
            for bias in (0.0, 1e-3):
                what = (name, tail, lname, ef, bias)
                want = folded(gpu, name, lname, vol, FIRST, S, eval_flags=ef, bias=bias, tail_after=tail) / F32(S)
                got = frame(dev, lens, vol, S, first_sample=FIRST, eval_flags=ef, bias=bias, tail_after=tail)
                assert np.isfinite(want).all() and want.any(), what
                assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).any(axis=2).sum()))


def test_the_fisheye_has_pixels_outside_its_circle_and_they_are_zero(gpu):
    for name in SCENES:
        dev, cam, vol, lenses = case(gpu, name)
        outside = np.ones(NPIX, bool)
        for s in range(FIRST, FIRST + S):
            outside &= (lens_rays(gpu, name, "fisheye200", s).cpu().numpy()[:, 4:7] == 0).all(axis=1)
        # the circle is inscribed in the frame's height: it covers pi * H / (4 * W) = 0.455 of the frame, the rest lies outside
        assert 8 <= outside.sum() <= int(NPIX * (1 - np.pi * H / (4 * W))), "the pixels with all five samples outside the circle"
        for tail in TAILS:
            got = frame(dev, lenses["fisheye200"], vol, S, first_sample=FIRST, tail_after=tail).reshape(NPIX, 3)
            assert (bits(got[outside]) == 0).all() and got[~outside].any(), (name, tail)


@pytest.mark.parametrize("name", SCENES)
def test_the_frames_see_specular_first_hits_and_misses_so_the_tails_differ(gpu, name):
    dev, cam, vol, lenses = case(gpu, name)
    seen = np.zeros(3, int)  # pixels over the five lenses whose first hit is diffuse, mirror or glass, none
    followed = 0
    for lname, lens in lenses.items():
        ru = bits(dev.trace_rays(lens_rays(gpu, name, lname, FIRST).cpu().numpy(), "shade"))
        hit, diffuse, specular = tp.first_hits(gpu, ru)
        seen += (int(diffuse.sum()), int(specular.sum()), int((~hit).sum()))
        one = frame(dev, lens, vol, 1, first_sample=FIRST).reshape(NPIX, 3)
        k1 = frame(dev, lens, vol, 1, first_sample=FIRST, tail_after=1).reshape(NPIX, 3)
        same = (bits(one) == bits(k1)).all(axis=1)
        assert same[diffuse | ~hit].all(), (name, lname, "tail_after = 1 is the one-segment frame where the first hit is diffuse or a miss")
        followed += int((~same[specular]).sum())
    print(f"{name}: first hits over the five lenses: diffuse {seen[0]}, mirror or glass {seen[1]}, none {seen[2]}; tail_after = 1 differs on {followed}")
    assert seen[0] >= 20 and seen[1] >= 2 and seen[2] >= 2, (name, seen.tolist())
    assert followed >= 1, "tail_after = 1 follows mirror and glass, so the two frames differ somewhere"


# ------------------------------------------------------------------------------------------------- B. running sums and gamma
@pytest.mark.parametrize("tail", (None, 2))
def test_running_sums_gamma_and_a_sentinel_border(gpu, tail):
    import torch
    name, lname = "cornell_mesh", "thin"
    dev, cam, vol, lenses = case(gpu, name)
    lens = lenses[lname]
    sums = folded(gpu, name, lname, vol, 0, 5, tail_after=tail)
    big = torch.full((NPIX + 128, 3), -7.0, dtype=torch.float32, device="cuda")  # 64 pixels of sentinel on either side
    acc = big[64:64 + NPIX].view(H, W, 3)
    acc.zero_()
    dev.render_lit(lens, vol, W, H, 2, SEED, first_sample=0, out=acc, accumulate=True, tail_after=tail)
    dev.render_lit(lens, vol, W, H, 3, SEED, first_sample=2, out=acc, accumulate=True, tail_after=tail)
    assert np.array_equal(bits(acc.cpu().numpy()), bits(sums)), "2 + 3 samples accumulated are the 5 sums"
    once = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    dev.render_lit(lens, vol, W, H, 5, SEED, out=once, accumulate=True, tail_after=tail)
    assert np.array_equal(bits(once.cpu().numpy()), bits(sums)), "one accumulate call of 5"
    border = big.cpu().numpy()
    assert (border[:64] == -7.0).all() and (border[64 + NPIX:] == -7.0).all(), "nothing is written outside the frame"
    # gamma: the render's expression on the means -- hrt_finalize_tiles with one sample divides by 1.f, which is exact
    means = sums / F32(5)
    assert np.array_equal(bits(frame(dev, lens, vol, 5, tail_after=tail)), bits(means))
    padded = torch.zeros((4 * 64, 3), dtype=torch.float32, device="cuda")
    padded[:NPIX] = torch.from_numpy(means.reshape(NPIX, 3)).cuda()
    gpu.finalize_tiles(padded.data_ptr(), 4, 1, gpu.FLAG_GAMMA, padded.data_ptr())
    want = padded[:NPIX].cpu().numpy().reshape(H, W, 3)
    got = frame(dev, lens, vol, 5, flags=GAMMA, tail_after=tail)
    assert not np.array_equal(bits(want), bits(means)) and np.array_equal(bits(got), bits(want), ), "gamma after the division"
    with pytest.raises(gpu.HrtError, match="HRT_FLAG_GAMMA cannot be combined with HRT_RADIANCE_ACCUMULATE"):
        dev.render_lit(lens, vol, W, H, 1, SEED, flags=GAMMA, out=once, accumulate=True, tail_after=tail)


# ------------------------------------------------------------------------------------------ C. a pinhole lit frame is the camera's
@pytest.mark.parametrize("name", SCENES)
def test_a_pinhole_lit_frame_is_camera_rays_and_lit_rays_sample_by_sample(gpu, name):
    import torch
    dev, cam, vol, lenses = case(gpu, name)
    for tail in (None, 1, 2):
        for flags in (0, EXACT):
            acc = torch.zeros((NPIX, 3), dtype=torch.float32, device="cuda")
            for s in range(4):
                dev.trace_lit(gpu.camera_rays(cam, W, H, s, SEED), vol, 1, first_sample=s, seed=SEED, out=acc, accumulate=True, flags=flags,
                              eval_flags=FACING, tail_after=tail)
                got = frame(dev, gpu.Lens(cam, focus=NAN), vol, s + 1, flags=flags, eval_flags=FACING, tail_after=tail, accumulate=True)
                assert np.array_equal(bits(got.reshape(NPIX, 3)), bits(acc.cpu().numpy())), (name, tail, flags, s)


# --------------------------------------------------------------------------- D. where nothing can be gathered, the frame is the render
@pytest.mark.parametrize("name", SCENES)
def test_pixels_whose_paths_reach_no_tail_are_the_lens_frames(gpu, name):
    import torch
    dev, cam, _, lenses = case(gpu, name)
    zero = tl.zero_volume(gpu, tl.TAIL_SCENES[name])
    n_reached = n_differ = 0
    for lname in ("equirect", "thin"):
        for K in (2, 6):
            for s in (0, 4):
                T = dev.path_tails(lens_rays(gpu, name, lname, s, 9).cpu().numpy(), K, s, seed=9)
                reached = lp.split(T)[3]  # lens rays are never degenerate here: both lenses trace every pixel
                lit = frame(dev, lenses[lname], zero, 1, seed=9, first_sample=s, tail_after=K).reshape(NPIX, 3)
                ren = dev.render_lens(lenses[lname], W, H, 1, 9, first_sample=s, out=torch.zeros((H, W, 3), device="cuda")).cpu().numpy().reshape(NPIX, 3)
                assert np.array_equal(bits(lit[~reached]), bits(ren[~reached])), (name, lname, K, s)
                if K == 6:  # six diffuse hits in a row: any mirror, glass or miss on the way leaves the path without a tail
                    assert (~reached).sum() >= 1, (name, lname, s, int((~reached).sum()))
                else:
                    n_reached += int(reached.sum())
                    n_differ += int((bits(lit[reached]) != bits(ren[reached])).any(axis=1).sum())
    print(f"{name}: tail_after = 2 reached on {n_reached} pixel samples, {n_differ} of them differ from the render")
    assert n_reached >= 1 and n_differ >= 1, "where the tail is reached a zero volume ends the path: it is not the render's"
    zero.close()


# ------------------------------------------------------------------------------------------------------------------ E. batches
@pytest.mark.parametrize("tail", (None, 2))
@pytest.mark.parametrize("name", SCENES)
def test_frame_v_of_a_batch_is_the_single_frame_of_view_v(gpu, name, tail):
    import torch
    dev, cam, vol, lenses = case(gpu, name)
    views, seeds = [lenses["pinhole"], lenses["equirect"], lenses["thin"]], [7, 2 ** 40 + 3, 1]
    kw = dict(eval_flags=VISIBLE, bias=1e-3, tail_after=tail)
    for flags in (0, GAMMA):
        got = dev.render_lit_views(views, vol, W, H, 3, seeds, flags=flags, first_sample=2, out=torch.zeros((3, H, W, 3), device="cuda"), **kw).cpu().numpy()
        for v in range(3):
            want = frame(dev, views[v], vol, 3, seed=seeds[v], flags=flags, first_sample=2, **kw)
            assert want.any() and np.array_equal(bits(got[v]), bits(want)), (name, tail, flags, v)
    acc = torch.zeros((3, H, W, 3), dtype=torch.float32, device="cuda")
    dev.render_lit_views(views, vol, W, H, 1, seeds, out=acc, accumulate=True, **kw)
    dev.render_lit_views(views, vol, W, H, 2, seeds, first_sample=1, out=acc, accumulate=True, **kw)
    for v in range(3):
        want = frame(dev, views[v], vol, 3, seed=seeds[v], accumulate=True, **kw)
        assert np.array_equal(bits(acc[v].cpu().numpy()), bits(want)), (name, tail, "accumulate", v)
    empty = dev.render_lit_views([], vol, W, H, 3, **kw)
    assert empty.shape == (0, H, W, 3) and empty.dtype == F32


# --------------------------------------------------------------------------------------------------------- F. the blocking forms
def test_the_blocking_forms_are_the_device_forms_and_fill_their_stats(gpu):
    dev, cam, vol, lenses = case(gpu, "cornell_mesh")
    for tail in (None, 1):
        st = gpu.Stats()
        got = dev.render_lit(lenses["thin"], vol, W, H, 3, SEED, flags=GAMMA, stats=st, eval_flags=FACING, tail_after=tail)
        assert got.shape == (H, W, 3) and st.samples == NPIX * 3 and st.kernel_ms > 0
        assert np.array_equal(bits(got), bits(frame(dev, lenses["thin"], vol, 3, flags=GAMMA, eval_flags=FACING, tail_after=tail)))
        views, seeds = [lenses["ortho"], lenses["fisheye200"]], [4, 5]
        st = gpu.Stats()
        got = dev.render_lit_views(views, vol, W, H, 2, seeds, stats=st, tail_after=tail)
        assert got.shape == (2, H, W, 3) and st.samples == 2 * NPIX * 2 and st.kernel_ms > 0
        for v in range(2):
            assert np.array_equal(bits(got[v]), bits(frame(dev, views[v], vol, 2, seed=seeds[v], tail_after=tail))), (tail, v)
        later = dev.render_lit(lenses["thin"], vol, W, H, 2, SEED, first_sample=3, tail_after=tail)  # NumPy through the device form
        assert np.array_equal(bits(later), bits(frame(dev, lenses["thin"], vol, 2, first_sample=3, tail_after=tail)))
    with pytest.raises(gpu.HrtError, match="hrt_render_lit: flags: HRT_RADIANCE_ACCUMULATE needs the running sums on the device"):
        gpu.DeviceScene._frames_blocking(dev, "hrt_render_lit", (vol._h, C.byref(lenses["thin"]), W, H, 1, 1, ACCUMULATE, 0, 0.0, 0), (H, W, 3), None)


# ------------------------------------------------------------------------------------------- G. refusals that need a volume
def test_the_refusals_that_need_a_volume_are_those_of_a_lit_ray(gpu):
    lib = gpu.device_lib()
    dev, cam, vol, lenses = case(gpu, "cornell_mesh")
    OUT = 0x2000
    L = lenses["pinhole"]
    views = (gpu.LensView * 1)()
    C.memmove(C.byref(views[0].lens), C.byref(L), C.sizeof(gpu.Lens))

    def call(entry, v, scene_h=None, ef=0, bias=0.0, tail=0):
        if entry == "hrt_render_lit_device":
            rc = lib.hrt_render_lit_device(scene_h, v._h, C.byref(L), W, H, 0, 1, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        elif entry == "hrt_render_lit":
            rc = lib.hrt_render_lit(scene_h, v._h, C.byref(L), W, H, 1, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        elif entry == "hrt_render_lit_views_device":
            rc = lib.hrt_render_lit_views_device(scene_h, v._h, views, 1, W, H, 0, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        else:
            rc = lib.hrt_render_lit_views(scene_h, v._h, views, 1, W, H, 1, 0, ef, bias, tail, C.c_void_p(OUT), None)
        return rc, lib.hrt_last_error().decode()

    def trace_lit(v, ef=0, bias=0.0):
        rc = lib.hrt_trace_lit(None, v._h, C.c_void_p(0x1000), None, 5, 0, 1, 1, 0, ef, bias, C.c_void_p(OUT), None)
        return rc, lib.hrt_last_error().decode().replace("hrt_trace_lit", "{}")

    for entry in ("hrt_render_lit_device", "hrt_render_lit", "hrt_render_lit_views_device", "hrt_render_lit_views"):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as v:
            for tail in (0, 2):
                for state in ("empty", "loaded", "depth"):
                    if tail == 0 and state == "loaded":
                        v.update(np.zeros((2, 9, 3), F32))
                    if tail == 0 and state == "depth":
                        v.update_depth(np.zeros((2, 64, 3), F32))
                    if tail == 2 and state != "depth":
                        continue
                    for ef, bias in ((1 | VISIBLE, NAN), (8, NAN), (VISIBLE | FACING, NAN), (VISIBLE, 0.0), (0, NAN), (0, INF), (0, 0.0)):
                        rc, msg = trace_lit(v, ef, bias)
                        assert call(entry, v, ef=ef, bias=bias, tail=tail) == (rc, msg.format(entry)), (entry, tail, state, ef, bias)
                        passes = state != "empty" and bias == 0.0 and (ef == 0 or (ef == VISIBLE and state == "depth"))
                        assert rc == HRT_ERR_INVALID and (msg == "{}: scene is NULL") == passes, (entry, tail, state, ef, bias, msg)
        closed = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1)
        closed.close()
        assert call(entry, closed) == (HRT_ERR_INVALID, entry + ": volume is NULL"), "a closed volume has no handle"
    # a volume of another scene is any volume: a volume belongs to a device, not to a scene, and is refused only across devices
    other = qr.build(gpu, "random_spheres", W, H)[2]
    assert frame(other, L, vol, 1).any()
    other.close()
    with pytest.raises(gpu.HrtError, match="hrt_render_lit_device: eval_flags: HRT_LIT_VISIBLE: the volume has no depth moments yet"):
        with gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1) as v:
            frame(dev, L, v.update(np.zeros((2, 9, 3), F32)), 1, eval_flags=VISIBLE)
    closed = gpu.ProbeVolume((0, 0, 0), (1, 1, 1), 2, 1, 1)
    closed.close()
    for fn in (lambda: frame(dev, L, closed, 1), lambda: dev.trace_lit(lens_rays(gpu, "cornell_mesh", "pinhole", FIRST), closed)):
        with pytest.raises(gpu.HrtError, match="volume is NULL"):
            fn()


# ------------------------------------------------------------------------------------------------------------------ H. the CLI
def cli(tmp_path, extra, spp, out="out.ppm"):
    path = tmp_path / out
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--assets", os.path.join(ROOT, "assets"), "--scene", "cornell_box", "--w", str(W), "--h", str(H),
                        "--probe-grid", "2,2,1", "--probe-box", "-1.0,-1.0,-1.0,1.0,1.0,1.0", "--probe-lit", "--spp", str(spp), "--out", str(path)] + extra,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return path


@pytest.mark.parametrize("tail", (None, 1))
def test_the_cli_writes_the_bytes_the_per_sample_loop_wrote(gpu, tmp_path, tail):
    import torch
    lo, hi, spp, counts = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 4, (2, 2, 1)
    got = cli(tmp_path, [] if tail is None else ["--probe-tail", str(tail)], spp).read_bytes()
    _, desc, dev, cam = qr.build(gpu, "cornell_box", W, H)
    with gpu.ProbeVolume(lo, hi, *counts) as vol:
        vol.update(dev.probes(gpu.probe_grid(lo, hi, *counts), spp, seed=1))  # without --probe-bounces the grid is path-traced
        acc = torch.zeros((4 * 64, 3), dtype=torch.float32, device="cuda")  # the sums padded to whole tiles, as the loop held them
        for s in range(spp):
            dev.trace_lit(gpu.camera_rays(cam, W, H, s, 1), vol, 1, first_sample=s, seed=1, out=acc[:NPIX], accumulate=True, tail_after=tail)
    assert np.isfinite(acc.cpu().numpy()).all() and acc.any()
    gpu.finalize_tiles(acc.data_ptr(), 4, spp, gpu.FLAG_GAMMA, acc.data_ptr())
    mine = tmp_path / "mine.ppm"
    gpu.write_ppm(str(mine), acc[:NPIX].cpu().numpy().reshape(H, W, 3))
    assert got == mine.read_bytes()
    dev.close()


def test_the_cli_writes_lens_frames_and_views(gpu, tmp_path):
    pinhole = cli(tmp_path, [], 2).read_bytes()
    pano = cli(tmp_path, ["--lens", "equirect"], 2, "pano.ppm").read_bytes()
    assert pano.startswith(b"P3\n19 11\n255\n") and pano != pinhole
    cli(tmp_path, ["--views", "2", "--orbit", "30", "--probe-tail", "1"], 2, "turn.ppm")
    a, b = (tmp_path / "turn_000.ppm").read_bytes(), (tmp_path / "turn_001.ppm").read_bytes()
    assert a.startswith(b"P3\n19 11\n255\n") and b.startswith(b"P3\n19 11\n255\n") and a != b and not (tmp_path / "turn.ppm").exists()
    assert a == cli(tmp_path, ["--probe-tail", "1"], 2, "first.ppm").read_bytes(), "view 0 is the single frame: the same camera and seed"


# ------------------------------------------------------------------------------------------------------------ I. resources
def test_repeated_calls_leave_no_device_buffers_behind(gpu):
    import torch
    torch.cuda.synchronize()
    see = tlr.Peak(gpu)
    before = see()
    _, desc, dev, cam = qr.build(gpu, "cornell_mesh", W, H)
    vol = tl.zero_volume(gpu, tl.TAIL_SCENES["cornell_mesh"])
    L = gpu.Lens(cam, "equirect")
    out = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda")

    def round_():
        for tail in (None, 2):
            dev.render_lit(L, vol, W, H, 2, tail_after=tail)
            dev.render_lit(L, vol, W, H, 2, out=out[0], tail_after=tail)
            dev.render_lit_views([L, gpu.Lens(cam)], vol, W, H, 2, tail_after=tail)
            dev.render_lit_views([L, gpu.Lens(cam)], vol, W, H, 2, out=out, tail_after=tail)
        torch.cuda.synchronize()
        return see()

    held = round_()  # the scene's table of views is its own grow-only scratch: allocated by the first batch, freed with the scene
    for _ in range(3):
        assert round_() == held
    peak = see.peak
    round_()
    assert see.peak == peak, "a further round peaks where the earlier ones did"
    vol.close()
    dev.close()
    assert gpu.live_resources() == before
