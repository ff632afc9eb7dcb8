"""Adaptive sampling (include/hrt.h hrt_render_adaptive*): per-tile sample counts set by a noise estimate.

The contract every test here leans on: each tile of an adaptive frame is bit-identical to the same tile of a plain hrt_render at
the count that tile was given.  The policy (which count a tile gets) is recomputed in numpy from uniform renders, with the
estimate stated in include/hrt.h."""
import os

import numpy as np
import pytest

from adaptive_ref import errors_from, expected_counts, samples, sequence, tile_err, tiles_differing

pytestmark = pytest.mark.gpu

W, H, SEED = 120, 67, 11  # 15 x 9 tiles; the last column and row are partly outside the image


def build(gpu, name, w=W, h=H):
    host = gpu.HostScene().setup(name, w / h, 1)
    desc = host.flatten()
    return desc, gpu.DeviceScene(desc), gpu.default_camera(w / h)


def uniform(dev, cam, counts, flags=0, w=W, h=H):
    return {int(c): dev.render(cam, w, h, int(c), seed=SEED, flags=flags)[0] for c in np.unique(np.asarray(counts))}


def errors_at(dev, cam, min_spp, max_spp, w=W, h=H):
    """tile_err of every judged count n (the error computed in the round that brought the tile to n)."""
    return errors_from(uniform(dev, cam, sequence(min_spp, max_spp), 0, w, h), min_spp, max_spp)


def assert_tiles_match(frame, counts, refs, w=W, h=H):
    """Every tile has the bits of the same tile of the uniform render at its count."""
    assert frame.shape == (h, w, 3)
    bad = tiles_differing(frame, counts, refs)
    assert not bad, f"{len(bad)} tiles differ from hrt_render at their count, first (tile y, tile x, count): {bad[:5]}"


@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres", "cornell_box", "backrooms_pool"])
def test_every_tile_is_the_uniform_render_at_its_count(gpu, name):
    desc, dev, cam = build(gpu, name)
    mn, mx = 4, 32
    err = errors_at(dev, cam, mn, mx)
    thr = float(np.median(err[mn]))
    for gamma in (0, gpu.FLAG_GAMMA):
        st = gpu.Stats()
        frame, counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED, flags=gamma, stats=st)
        assert counts.shape == ((H + 7) // 8, (W + 7) // 8)
        assert counts.min() == mn and counts.max() > mn, f"threshold {thr} gave no spread of counts {np.unique(counts)}"
        assert_tiles_match(frame, counts, uniform(dev, cam, counts, gamma))
        assert st.samples == samples(counts, W, H)
        assert st.kernel_ms > 0


@pytest.mark.parametrize("name,mn,mx", [("cornell_mesh", 4, 32), ("random_spheres", 4, 24), ("backrooms_pool", 2, 16)])
def test_counts_follow_the_policy(gpu, name, mn, mx):
    """Every count is what the stated rule gives from the tile errors of uniform renders (tiles within 1e-5 of the threshold
    at a judged count are left out)."""
    desc, dev, cam = build(gpu, name)
    err = errors_at(dev, cam, mn, mx)
    thr = float(np.median(err[mn]))  # both sides populated
    frame, counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED)
    seq = sequence(mn, mx)
    assert set(np.unique(counts).tolist()) <= set(seq[1:])
    near = np.zeros(counts.shape, dtype=bool)
    for n, e in err.items():
        near |= np.abs(e - thr) <= 1e-5 * thr
    prev = {n: p for p, n in zip(seq[1:], seq[2:])}
    checked_stop = checked_go = 0
    for (y, x), c in np.ndenumerate(counts):
        if near[y, x]:
            continue
        c = int(c)
        if c < mx:
            assert err[c][y, x] < thr, f"tile {(y, x)} stopped at {c} with error {err[c][y, x]} >= {thr}"
            checked_stop += 1
        if c > mn:
            assert err[prev[c]][y, x] >= thr, f"tile {(y, x)} went on past {prev[c]} with error {err[prev[c]][y, x]} < {thr}"
            checked_go += 1
    assert checked_stop > 0 and checked_go > 0
    exp = expected_counts(err, mn, mx, thr)
    assert np.array_equal(counts[~near], exp[~near])


def test_extreme_thresholds_and_equal_bounds(gpu):
    desc, dev, cam = build(gpu, "cornell_mesh")
    mn, mx = 4, 16
    for gamma in (0, gpu.FLAG_GAMMA):
        frame, counts = dev.render_adaptive(cam, W, H, mn, mx, 0.0, seed=SEED, flags=gamma)
        assert (counts == mx).all()
        assert np.array_equal(frame, dev.render(cam, W, H, mx, seed=SEED, flags=gamma)[0])
        frame, counts = dev.render_adaptive(cam, W, H, mn, mx, float("inf"), seed=SEED, flags=gamma)
        assert (counts == mn).all()
        assert np.array_equal(frame, dev.render(cam, W, H, mn, seed=SEED, flags=gamma)[0])
        frame, counts = dev.render_adaptive(cam, W, H, 6, 6, 0.0, seed=SEED, flags=gamma)
        assert (counts == 6).all()
        assert np.array_equal(frame, dev.render(cam, W, H, 6, seed=SEED, flags=gamma)[0])


def test_every_kernel_form_gives_the_same_frame_and_counts(gpu):
    desc, dev, cam = build(gpu, "cornell_mesh")
    mn, mx = 4, 32
    err = errors_at(dev, cam, mn, mx)
    thr = float(np.median(err[mn]))
    base, base_counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA)
    assert len(np.unique(base_counts)) > 1
    for f in (gpu.FLAG_WAVE_KERNEL, gpu.FLAG_DUAL_KERNEL, gpu.FLAG_STREAM_KERNEL, gpu.FLAG_EXACT_ONLY,
              gpu.FLAG_EXACT_ONLY | gpu.FLAG_WAVE_KERNEL, gpu.FLAG_EXACT_ONLY | gpu.FLAG_STREAM_KERNEL):
        frame, counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA | f)
        assert np.array_equal(counts, base_counts), f"flags {f}: other counts"
        assert np.array_equal(frame, base), f"flags {f}: other pixels"


@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
def test_rank_partition_gives_the_whole_frame_call(gpu, name):
    """hrt_render_adaptive_tiles over world 3 (rank r: tiles r, r + 3, ...) + hrt_assemble_frame == hrt_render_adaptive."""
    import torch
    desc, dev, cam = build(gpu, name)
    mn, mx, world = 4, 32, 3
    err = errors_at(dev, cam, mn, mx)
    thr = float(np.median(err[mn]))
    ref, ref_counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA)
    per = gpu.tiles_owned(W, H, 0, world)
    gathered = torch.zeros((world, per, 64, 3), dtype=torch.float32, device="cuda")
    spp = torch.zeros((world, per), dtype=torch.int32, device="cuda")
    for r in range(world):
        dev.render_adaptive_tiles(cam, W, H, mn, mx, thr, SEED, gpu.FLAG_GAMMA, r, world, gathered[r].data_ptr(), spp[r].data_ptr(), 0)
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gpu.assemble_frame(gathered.data_ptr(), per, W, H, world, frame.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy(), ref)
    spp = spp.cpu().numpy()
    counts = np.array([spp[t % world, t // world] for t in range(gpu.tiles_total(W, H))]).reshape(ref_counts.shape)
    assert np.array_equal(counts.astype(np.uint32), ref_counts)


def test_a_list_of_one_tile_runs_to_max_bit_exact(gpu):
    """Threshold just below the error the most persistent tile keeps through every round: late rounds launch over a list of
    (about) one tile, and at 128 samples per round the streaming kernel splits that tile into row bands."""
    desc, dev, cam = build(gpu, "cornell_mesh")
    mn, mx = 8, 256
    err = errors_at(dev, cam, mn, mx)
    judged = sequence(mn, mx)[1:-1]  # the counts at which a tile must still be judged active to reach mx
    persist = np.minimum.reduce([err[n] for n in judged])
    best = np.unravel_index(int(np.argmax(persist)), persist.shape)
    thr = float(np.nextafter(np.float32(persist[best]), np.float32(0)))
    frame, counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA)
    assert counts[best] == mx
    assert int((counts == mx).sum()) <= 2, np.unique(counts, return_counts=True)
    assert np.array_equal(counts, expected_counts(err, mn, mx, thr))
    assert_tiles_match(frame, counts, uniform(dev, cam, counts, gpu.FLAG_GAMMA))
    for f in (gpu.FLAG_STREAM_KERNEL, gpu.FLAG_WAVE_KERNEL, gpu.FLAG_DUAL_KERNEL):
        other, other_counts = dev.render_adaptive(cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA | f)
        assert np.array_equal(other_counts, counts) and np.array_equal(other, frame), f"flags {f}"


def test_raytracer_adaptive_writes_the_file_the_library_renders(gpu, tmp_path):
    import subprocess
    from conftest import PKG, ROOT
    w, h, seed = 96, 54, 5
    desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    a, b = (dev.render(cam, w, h, n, seed=seed)[0] for n in (4, 8))
    thr = repr(float(np.float32(np.median(tile_err(a, b, w, h)))))  # a float32 value, printed so that strtof reads it back exactly
    out = tmp_path / "rendu.ppm"
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--scene", "cornell_mesh", "--w", str(w), "--h", str(h), "--spp", "32",
                        "--spp-min", "8", "--adaptive", thr, "--seed", str(seed), "--assets", os.path.join(ROOT, "assets"),
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mean" in r.stdout and "spp" in r.stdout
    img, counts = dev.render_adaptive(cam, w, h, 8, 32, float(thr), seed=seed, flags=gpu.FLAG_GAMMA)
    assert len(np.unique(counts)) > 1
    assert out.read_bytes() == gpu.ppm_text_reference(img)
    ref = tmp_path / "lib.ppm"
    gpu.write_ppm(str(ref), img)
    assert out.read_bytes() == ref.read_bytes()
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--adaptive", "0.1", "--gpus", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--adaptive" in r.stderr


def test_a_round_whose_kernel_gives_up_ends_the_call(gpu):
    """libhrt_var_bound.so (Makefile) is the library whose streaming kernel gives up after 3 serial sections: the adaptive entry
    points check every trace launch and must return HRT_ERR_DEVICE, not a frame, and leave the process usable."""
    import subprocess, sys, textwrap
    code = textwrap.dedent('''
        import ctypes as C, importlib, sys
        import numpy as np
        sys.path.insert(0, %r)
        hrt = importlib.import_module("hai719-raytracing_amd")
        import torch
        hrt.init(0)
        w, h = 64, 48
        host = hrt.HostScene().setup("cornell_mesh", w / h, 1); desc = host.flatten(); cam = hrt.default_camera(w / h)
        dev = hrt.DeviceScene(desc)
        lib = hrt.device_lib()
        p = hrt.Adaptive(16, 32, 0.0)  # round 0: one launch of 8 samples, as in tests/test_gpu_output.py
        out = np.empty((h, w, 3), np.float32)
        rc1 = lib.hrt_render_adaptive(dev._h, C.byref(cam), w, h, C.byref(p), 1, hrt.FLAG_STREAM_KERNEL, out.ctypes.data, None, None)
        msg = lib.hrt_last_error().decode()
        tiles = torch.zeros((hrt.tiles_total(w, h), 64, 3), dtype=torch.float32, device="cuda")
        spp = torch.zeros(hrt.tiles_total(w, h), dtype=torch.int32, device="cuda")
        rc2 = lib.hrt_render_adaptive_tiles(dev._h, C.byref(cam), w, h, C.byref(p), 1, hrt.FLAG_STREAM_KERNEL, 0, 1,
                                            C.c_void_p(tiles.data_ptr()), C.c_void_p(spp.data_ptr()), None)
        img, counts = dev.render_adaptive(cam, w, h, 2, 4, 0.0, 1, flags=hrt.FLAG_WAVE_KERNEL)   # still alive
        print("RC", rc1, rc2, float(img.max()) > 0, int(counts.min()), "|", msg)
    ''') % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    env = dict(os.environ, HRT_LIBNAME="libhrt_var_bound.so")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("RC")][0]
    assert line.startswith("RC -2 -2 True 4 |") and "gave up" in line, line
