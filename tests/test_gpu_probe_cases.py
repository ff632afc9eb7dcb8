"""The probe family (probes, probe_depth, probes_lit with and without a tail, ProbeVolume.relight, and bakes) on what the rest of its
GPU tests hold constant -- tests/probe_cases.py has the inputs, tests/test_probe_cases.py what the CPU can say about them:

1. probes at NON-ZERO TIMES, each its own, on the moving scenes, two lights, the skybox image, the dark sky and the two small
   meshes of radiance_oracle.EXTRA, and on random_spheres;
2. a FAR probe whose chosen keys send its rays into the scene, so that the far-origin mesh rule decides something;
3. the fused kernels against the CPU ORACLE directly, and not only against the device's own pieces;
4. the build with blocks of 256 samples, in which a lane has several samples of an item.

A. COMPOSITION, bit for bit: every fused kernel is the fixed-order fold (tests/probe_ref.py, tests/probe_depth_ref.py) of the
   per-sample outputs of hrt_probe_rays + hrt_trace_radiance / hrt_trace_rays / hrt_trace_lit for the same records, times included;
   by grid stride every row keeps its own probe's time; relight(time=) is the loop written by hand; bakes at random times follow
   the oracle.
B. THE ORACLE: probes within a tolerance derived from the per-sample bar (probe_cases.coefficient_tolerance), the depth sums on
   bits (first hits are bit-identical).
C. THE BLOCK SIZE: libhrt_var_probe256.so in a process of its own (tests/probe_block_run.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bake_ref
import probe_block_run as block_run
import probe_cases as pc
import probe_ref
import radiance_oracle as ro
import test_gpu_lit_paths as lp
import test_gpu_probe_depth as tpd
import test_gpu_probe_lit as tl
import test_gpu_probes as tp
import test_gpu_radiance_oracle as orc
import test_gpu_rays as qr
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
EXACT = 64
SEED, S = pc.SEED, pc.S
COUNTS = (1, S)
FIRSTS = (0, 2 ** 32 - S)
EF, BIAS = tl.FACING | tl.VISIBLE, 1e-3
TAILS = (None, 1, 3)
bits = qr.bits
on_gpu = tp.on_gpu


def device(gpu, name):
    """(the CPU scene tests/probe_cases.py made the probes on, a DeviceScene of the same description), built once."""
    return orc.device(gpu, name)


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])] if len(bad) else None,
                                                        want[tuple(bad[0])] if len(bad) else None)


def matrix(exact):
    """(with keys, first sample, counts): the whole matrix for the shipped kernels, one case under HRT_FLAG_EXACT_ONLY."""
    if exact:
        return [(True, 0, (S,))]
    return [(k, first, COUNTS) for k in (False, True) for first in FIRSTS]


# ============================================================================================================ A. composition
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_fused_probes_are_the_fold_of_radiance_queries_at_the_probes_own_times(gpu, name, exact):
    _, dev = device(gpu, name)
    p, flags = pc.probes(gpu, name), EXACT if exact else 0
    pdeg = probe_ref.probe_degenerate(p)
    d_p = on_gpu(p)
    for with_keys, first, counts in matrix(exact):
        keys = pc.keys(name, with_keys)
        d_keys = None if keys is None else on_gpu(keys)
        Y, v, deg = tp.series(gpu, dev, d_p, d_keys, first, S, SEED, flags)
        assert np.isfinite(v).all() and v.any() and np.array_equal(deg, np.tile(pdeg, (S, 1)))
        for n in counts:
            got = dev.probes(d_p, n, first_sample=first, seed=SEED, keys=d_keys, flags=flags).cpu().numpy()
            same_bits(got, probe_ref.fold(Y[:n], v[:n], deg[:n]) / F32(n), (name, exact, with_keys, first, n))
            assert (bits(got[pdeg]) == 0).all() and (n < S or got[:5].any(axis=(1, 2)).all())  # the probe behind a hit may see nothing


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_fused_depth_is_the_fold_of_closest_hits_at_the_probes_own_times(gpu, name, exact):
    _, dev = device(gpu, name)
    p, flags, r_max = pc.probes(gpu, name), EXACT if exact else 0, pc.R_MAX[name]
    pdeg = probe_ref.probe_degenerate(p)
    d_p = on_gpu(p)
    for with_keys, first, counts in matrix(exact):
        keys = pc.keys(name, with_keys)
        d_keys = None if keys is None else on_gpu(keys)
        d, r, deg, hit = tpd.series(gpu, dev, d_p, d_keys, first, S, SEED, r_max, flags)
        assert np.array_equal(deg, np.tile(pdeg, (S, 1))) and (r[~deg] < F32(r_max)).any() and (r[~deg] == F32(r_max)).any()
        for n in counts:
            got = dev.probe_depth(d_p, n, first_sample=first, seed=SEED, keys=d_keys, r_max=r_max, flags=flags).cpu().numpy()
            same_bits(got, tpd.fold_all(d[:n], r[:n], deg[:n]), (name, exact, with_keys, first, n))
            assert (bits(got[pdeg]) == 0).all() and got[~pdeg].any(axis=(1, 2)).all()


def lit_pieces(gpu, dev, vol, d_p, d_keys, first, flags, K):
    if K is None:
        return tl.lit_series(gpu, dev, vol, d_p, d_keys, first, S, SEED, flags, EF, BIAS)
    return lp.lit_path_series(gpu, dev, vol, d_p, d_keys, first, S, SEED, flags, EF, BIAS, K)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_fused_lit_probes_are_the_fold_of_lit_rays_at_the_probes_own_times(gpu, name, exact):
    _, dev = device(gpu, name)
    p, flags = pc.probes(gpu, name), EXACT if exact else 0
    pdeg = probe_ref.probe_degenerate(p)
    d_p = on_gpu(p)
    vol, _, _ = tl.random_volume(gpu, pc.volume_box(gpu, name), 17)
    with vol:
        for with_keys, first, counts in matrix(exact):
            keys = pc.keys(name, with_keys)
            d_keys = None if keys is None else on_gpu(keys)
            seen = []
            for K in TAILS:
                Y, v, deg = lit_pieces(gpu, dev, vol, d_p, d_keys, first, flags, K)
                assert np.isfinite(v).all() and v.any() and np.array_equal(deg, np.tile(pdeg, (S, 1)))
                for n in counts:
                    got = dev.probes_lit(d_p, vol, n, first_sample=first, seed=SEED, keys=d_keys, eval_flags=EF, bias=BIAS, flags=flags,
                                         tail_after=K).cpu().numpy()
                    same_bits(got, probe_ref.fold(Y[:n], v[:n], deg[:n]) / F32(n), (name, exact, K, with_keys, first, n))
                    assert (bits(got[pdeg]) == 0).all()
                seen.append(got)
            assert not np.array_equal(seen[0], seen[2]), "a tail after three diffuse hits is another sum than one segment"


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_a_far_probe_whose_rays_meet_the_scene_is_the_fold_of_its_pieces(gpu, name, exact):
    """n_samples = 1, 64 keys: every sample decides the far-origin rule for itself (radiance_body, a per_sample source)."""
    sc, dev = device(gpu, name)
    p, keys, aimed = pc.far_set(gpu, name)
    flags, r_max = EXACT if exact else 0, pc.far_r_max(gpu, name)
    d_p, d_keys = on_gpu(p), on_gpu(keys)
    Y, v, deg = tp.series(gpu, dev, d_p, d_keys, 0, 1, SEED, flags)
    assert not deg.any() and np.isfinite(v).all()
    same_bits(dev.probes(d_p, 1, seed=SEED, keys=d_keys, flags=flags).cpu().numpy(), probe_ref.fold(Y, v, deg) / F32(1), (name, exact, "probes"))
    d, r, deg, hit = tpd.series(gpu, dev, d_p, d_keys, 0, 1, SEED, r_max, flags)
    print(f"{name}: {int(hit[0][aimed].sum())} of {pc.AIMED} aimed rays hit, {int(hit[0][~aimed].sum())} of {pc.STRAY} stray ones")
    assert hit[0][aimed].sum() >= 40 and not hit[0][~aimed].any(), "the device's rays hit and miss as the rule's do"
    same_bits(dev.probe_depth(d_p, 1, seed=SEED, keys=d_keys, r_max=r_max, flags=flags).cpu().numpy(), tpd.fold_all(d, r, deg), (name, exact, "depth"))
    vol, _, _ = tl.random_volume(gpu, pc.volume_box(gpu, name), 17)
    with vol:
        for K in TAILS:
            Y, v, deg = (tl.lit_series(gpu, dev, vol, d_p, d_keys, 0, 1, SEED, flags, EF, BIAS) if K is None else
                         lp.lit_path_series(gpu, dev, vol, d_p, d_keys, 0, 1, SEED, flags, EF, BIAS, K))
            got = dev.probes_lit(d_p, vol, 1, seed=SEED, keys=d_keys, eval_flags=EF, bias=BIAS, flags=flags, tail_after=K).cpu().numpy()
            same_bits(got, probe_ref.fold(Y, v, deg) / F32(1), (name, exact, "lit", K))


def test_by_grid_stride_every_row_keeps_its_own_probes_time(gpu):
    """More (probe, block) items than waves can be resident, cycling through the eight probes with keys = index % 8: a wave takes
    items of different probes one after the other, and a time carried over from the item before shows in a moving scene."""
    import torch
    name = "many_squares"
    _, dev = device(gpu, name)
    p = pc.probes(gpu, name)
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 7
    idx = torch.arange(n, device="cuda") % 8
    d_p = on_gpu(p)
    many, many_keys = d_p[idx].contiguous(), idx.to(torch.int32)
    assert len(set(p[pc.LIVE, 3].tolist())) == 6
    vol, _, _ = tl.random_volume(gpu, pc.volume_box(gpu, name), 17)
    with vol:
        calls = {"probes": lambda q, k: dev.probes(q, S, seed=SEED, keys=k),
                 "probe_depth": lambda q, k: dev.probe_depth(q, S, seed=SEED, keys=k, r_max=pc.R_MAX[name]),
                 "probes_lit": lambda q, k: dev.probes_lit(q, vol, S, seed=SEED, keys=k, eval_flags=EF, bias=BIAS),
                 "probes_lit, tail 2": lambda q, k: dev.probes_lit(q, vol, S, seed=SEED, keys=k, eval_flags=EF, bias=BIAS, tail_after=2)}
        for who, call in calls.items():
            want = call(d_p, None)
            got = call(many, many_keys)
            assert want[:6].any() and got.shape[0] == n and torch.equal(got.view(torch.int32), want[idx].view(torch.int32)), who


def test_relight_at_a_time_is_the_loop_written_by_hand(gpu):
    import torch
    name = "many_spheres"
    _, dev = device(gpu, name)
    box, counts, spp, rounds, keep, r_max = pc.volume_box(gpu, name), (2, 2, 2), S, 2, 0.5, 3.0
    rng = np.random.default_rng(9)
    lo, hi = np.asarray(box[0], F32), np.asarray(box[1], F32)
    pts = np.zeros((64, 8), F32)
    pts[:, 0:3] = lo + rng.random((64, 3)).astype(F32) * (hi - lo)
    pts[:, 3], pts[:, 4:7], pts[:, 7] = 0.5, tl.unit(rng.standard_normal((64, 3))), 1e-3

    def look(vol):
        return vol.eval(pts, facing=True), vol.eval_visible(pts, facing=True)

    with gpu.ProbeVolume(*box, *counts) as vol:
        assert vol.relight(dev, spp, rounds, keep=keep, seed=SEED, eval_flags=EF, bias=BIAS, depth_rmax=r_max, time=0.5) is vol
        got = look(vol)
    with gpu.ProbeVolume(*box, *counts) as vol:
        grid = gpu.probe_grid(*box, *counts, time=0.5)
        assert (grid[:, 3] == F32(0.5)).all()
        d_grid = on_gpu(grid)
        vol.update_depth(dev.probe_depth(d_grid, spp, seed=SEED, r_max=r_max))
        vol.update(torch.zeros((8, 9, 3), dtype=torch.float32, device="cuda"))
        for r in range(rounds):
            vol.blend(dev.probes_lit(d_grid, vol, spp, first_sample=r * spp, seed=SEED, eval_flags=EF, bias=BIAS), keep)
        by_hand = look(vol)
    with gpu.ProbeVolume(*box, *counts) as vol:
        still = look(vol.relight(dev, spp, rounds, keep=keep, seed=SEED, eval_flags=EF, bias=BIAS, depth_rmax=r_max, time=0.0))
    for g, w, s, who in zip(got, by_hand, still, ("eval", "eval_visible")):
        same_bits(g, w, who)
        assert g.any() and not np.array_equal(g, s), f"{who}: the time of the probes does not matter"


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("name", ["random_spheres", "many_spheres"])
def test_bakes_at_random_times_follow_the_oracle_on_the_devices_own_rays(gpu, name, with_keys):
    """test_gpu_radiance_oracle.test_bakes_follow_the_oracle_on_the_devices_own_rays with every live point at a time of its own, at
    the same bar."""
    import torch
    sc, dev = orc.device(gpu, name, orc.LW, orc.LH)
    pts = bake_ref.frame_points(sc.desc, sc.cam)
    deg = bake_ref.point_degenerate(pts)
    pts[~deg, 3] = np.random.default_rng(21).random(int((~deg).sum())).astype(F32)
    assert (~deg).sum() > 25 and len(set(pts[~deg, 3].tolist())) == (~deg).sum() and np.array_equal(bake_ref.point_degenerate(pts), deg)
    keys = bake_ref.keys_for(len(pts)) if with_keys else None
    d_pts = torch.from_numpy(pts).cuda()
    d_keys = None if keys is None else torch.from_numpy(keys.view(np.int32)).cuda()
    recs = [gpu.bake_rays(d_pts, s, SEED, d_keys).cpu().numpy() for s in range(orc.S)]
    assert all(((r[:, 4:7] == 0).all(axis=1) == deg).all() and np.array_equal(bits(r[:, 3]), bits(pts[:, 3])) for r in recs)
    sums, ties = orc.oracle_of_records(sc, recs, keys, 0, SEED)
    got = dev.bake(pts, orc.S, seed=SEED, keys=keys)
    orc.agree(got, sums / F32(orc.S), f"{name} bake at random times, mean ({ties} tie rays)")
    assert (bits(got[deg]) == 0).all() and got[~deg].any()
    still = pts.copy()
    still[:, 3] = 0
    moved = (bits(got) != bits(dev.bake(still, orc.S, seed=SEED, keys=keys))).any(axis=1)
    print(f"{name}: the time changes the bake of {int(moved.sum())} of {int((~deg).sum())} live points")
    assert moved.any() or name != "random_spheres", "the times of the points do not matter"  # many_spheres: 31 points x 3 samples see few movers
    base = np.random.default_rng(3).uniform(0, 2, (len(pts), 3)).astype(F32)
    recs = [gpu.bake_rays(d_pts, s, SEED, d_keys).cpu().numpy() for s in range(2, 2 + orc.S)]
    sums, ties = orc.oracle_of_records(sc, recs, keys, 2, SEED, start=base)
    acc = torch.from_numpy(base).cuda()
    dev.bake(d_pts, orc.S, first_sample=2, seed=SEED, keys=d_keys, out=acc, accumulate=True)
    acc = acc.cpu().numpy()
    orc.agree(acc, sums, f"{name} bake at random times, accumulated ({ties} tie rays)")
    assert np.array_equal(bits(acc[deg]), bits(base[deg]))


# ============================================================================================================== B. the oracle
def device_records(gpu, d_p, d_keys, count):
    """The device's own ray records of samples 0 .. count - 1 (so that sinf and cosf do not enter): (count, n, 8)."""
    return np.stack([gpu.probe_rays(d_p, s, SEED, d_keys).cpu().numpy() for s in range(count)])


def check_against_the_oracle(got, Y, v, deg, what):
    """|got - fold(Y, v_oracle) / S| <= probe_cases.coefficient_tolerance on EVERY coefficient; returns the worst ratio."""
    want = probe_ref.fold(Y, v, deg) / F32(len(v))
    tol = pc.coefficient_tolerance(Y, v, deg)
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ratio = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    print(f"{what}: worst error over tolerance {ratio:.3f} (largest error {err.max():.3e}, chain of {pc.chain(len(v))} operations)")
    assert (err <= tol).all(), (what, ratio, np.argwhere(err > tol)[:4].tolist())
    return ratio


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_fused_probes_follow_the_oracle(gpu, name, with_keys):
    """The bound, per coefficient k and channel c: (1e-6 + D 2^-24) sum_j |Y_jk| max(1, |v_jc|) / S with D = 11 at S = 65 -- one
    multiply, one addition in the lane, six halvings, two block additions, one division.  Measured on MI355X: the worst ratio of
    error to bound over the six scenes and both key modes is 0.032, on many_spheres; on most coefficients
    the two folds agree on bits."""
    sc, dev = device(gpu, name)
    p, keys = pc.probes(gpu, name), pc.keys(name, with_keys)
    d_p, d_keys = on_gpu(p), None if keys is None else on_gpu(keys)
    recs = device_records(gpu, d_p, d_keys, S)
    tp.check_rays(recs[S - 1], p, S - 1, SEED, keys, (name, with_keys, "rays"))
    v, tie = pc.oracle_values(sc, recs, keys, 0)
    deg = (recs[:, :, 4:7] == 0).all(axis=2)
    Y = np.stack([probe_ref.basis(r[:, 4:7]) for r in recs])
    got = dev.probes(d_p, S, seed=SEED, keys=d_keys).cpu().numpy()
    check_against_the_oracle(got, Y, v, deg, f"{name}, keys {with_keys} ({int(tie.sum())} tie rays)")
    assert (bits(got[6:8]) == 0).all() and v[:, :6].any()


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_fused_depth_is_the_fold_of_the_oracles_first_hits_bit_for_bit(gpu, name, with_keys):
    sc, dev = device(gpu, name)
    p, keys, r_max = pc.probes(gpu, name), pc.keys(name, with_keys), pc.R_MAX[name]
    d_p, d_keys = on_gpu(p), None if keys is None else on_gpu(keys)
    recs = device_records(gpu, d_p, d_keys, S)
    kind, t, _, tie = pc.first_segments(sc, recs, keys, 0)
    assert tie.sum() <= ro.tie_cap(tie.size), (name, int(tie.sum()))
    r = pc.depths(kind, t, r_max)
    deg = (recs[:, :, 4:7] == 0).all(axis=2)
    got = dev.probe_depth(d_p, S, seed=SEED, keys=d_keys, r_max=r_max).cpu().numpy()
    print(f"{name}, keys {with_keys}: {(kind[~deg] != 0).mean():.3f} of the oracle's first segments hit, {int(tie.sum())} ties")
    same_bits(got, tpd.fold_all(recs[:, :, 4:7], r, deg), (name, with_keys))
    assert (r[~deg] < F32(r_max)).any() and (r[~deg] == F32(r_max)).any() and (bits(got[6:8]) == 0).all()


@pytest.mark.parametrize("name", pc.SCENES)
def test_a_far_probe_follows_the_oracle_key_by_key(gpu, name):
    """The fold of one sample is the product Y x v: the per-sample bar itself, through the same expression on both sides."""
    sc, dev = device(gpu, name)
    p, keys, aimed = pc.far_set(gpu, name)
    d_p, d_keys = on_gpu(p), on_gpu(keys)
    recs = device_records(gpu, d_p, d_keys, 1)
    v, tie = pc.oracle_values(sc, recs, keys, 0)
    Y = probe_ref.basis(recs[0][:, 4:7])
    got = dev.probes(d_p, 1, seed=SEED, keys=d_keys).cpu().numpy()
    want = (Y[:, :, None] * v[0][:, None, :]).astype(F32) / F32(1)
    tol = 1e-6 * np.abs(Y.astype(np.float64))[:, :, None] * np.maximum(1.0, np.abs(v[0].astype(np.float64)))[:, None, :] \
        + 2.0 ** -23 * np.abs(want.astype(np.float64))  # the bar of the sample times |Y|, and the rounding of the product on either side
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name} far set: worst error over tolerance {float((err / np.maximum(tol, 1e-300)).max()):.3f}, {int(tie.sum())} tie rays; "
          f"values differ between aimed and stray keys: {not np.array_equal(v[0][aimed][:16], v[0][~aimed])}")
    assert np.isfinite(got).all() and (err <= tol).all(), (name, np.argwhere(err > tol)[:4].tolist())
    kind, t, _, stie = pc.first_segments(sc, recs, keys, 0)
    assert (kind[0][aimed] != 0).sum() >= 40 and not kind[0][~aimed].any() and stie.sum() <= ro.tie_cap(64)
    r_max = pc.far_r_max(gpu, name)
    depth = dev.probe_depth(d_p, 1, seed=SEED, keys=d_keys, r_max=r_max).cpu().numpy()
    want = tpd.fold_all(recs[:, :, 4:7], pc.depths(kind, t, r_max), np.zeros((1, 64), bool))
    same_bits(depth[aimed], want[aimed], (name, "depth of the aimed keys"))
    same_bits(depth[~aimed], want[~aimed], (name, "depth of the stray keys: r_max"))


# =========================================================================================================== C. the block size
BLOCK_LIB = "libhrt_var_probe256.so"


@pytest.fixture(scope="module")
def block_build(gpu, tmp_path_factory):
    """tests/probe_block_run.py from a process of its own that loads the build with blocks of 256 samples."""
    path = str(tmp_path_factory.mktemp("probe_block") / "block256.npz")
    env = dict(os.environ, HRT_LIBNAME=BLOCK_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "probe_block_run.py"), path], capture_output=True, text=True, env=env, timeout=300)
    loaded = [line for line in r.stdout.splitlines() if line.startswith("library ")]
    assert r.returncode == 0 and len(loaded) == 1 and os.path.basename(loaded[0].split()[1]) == BLOCK_LIB, r.stdout + r.stderr
    return dict(np.load(path))


@pytest.mark.parametrize("kind", list(block_run.KINDS))
@pytest.mark.parametrize("name", block_run.SCENES)
def test_blocks_of_256_samples_give_the_fold_at_that_block_size(block_build, name, kind):
    """With 256 samples to a block a lane adds up to four samples of an item in ascending order before the halving; 513 samples are
    two full blocks and a block of one.  The per-sample pieces do not depend on the block size; probe_ref.fold(block=256) states the
    sum.  At 513 samples that sum differs from the header's block of 64, so a build that kept the header's block would fail."""
    assert probe_ref.BLOCK == 64, "the shipped block is the other one of the pair"
    b = block_build
    Y, deg, v = b[f"{name}__Y"], b[f"{name}__deg"], b[f"{name}__v_{kind}"]
    assert Y.shape == (block_run.SMAX, 8, 9) and v.shape == (block_run.SMAX, 8, 3) and np.isfinite(v).all() and v[:, :6].any()
    for n in block_run.COUNTS:
        got = b[f"{name}__{kind}__{n}"]
        same_bits(got, probe_ref.fold(Y[:n], v[:n], deg[:n], block=256) / F32(n), (name, kind, n))
        assert (bits(got[6:8]) == 0).all()
    n = block_run.SMAX
    assert not np.array_equal(bits(b[f"{name}__{kind}__{n}"]), bits(probe_ref.fold(Y, v, deg, block=64) / F32(n))), "blocks of 64 give another sum"
    if kind == "probes":
        a, c = block_run.RUNNING
        want = (b[f"{name}__base"] + probe_ref.fold(Y[:a], v[:a], deg[:a], block=256)) + probe_ref.fold(Y[a:a + c], v[a:a + c], deg[a:a + c], block=256)
        same_bits(b[f"{name}__running"], want, (name, "running sums"))
