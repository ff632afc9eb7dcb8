"""hrt_trace_radiance, the lens frames and the bakes against the independent CPU oracle (oracle_radiance) on rays that do NOT leave a
pinhole camera: baking rays, origins inside glass, closed meshes and behind walls, origins 1e4 and 1e6 away, axis-parallel and
in-plane rays, non-unit directions raw and normalised, motion-blur times, keys other than the index, samples at the top of the
sample range, seeds with high bits, accumulation onto non-zero sums, one and two lights, the skybox image, the gradient and the
dark sky, and degenerate rows among good ones.

The bar is the project's stated one (tests/test_gpu_parity.assert_pixels_agree): |gpu - oracle| <= 1e-6 max(1,
|oracle|) on EVERY value, a value that is non-finite on one side only fails.  THE TIE RULE (tests/radiance_oracle.py): off the tie
rays the device is held to the oracle's MESH_REF_TREE value, on them to its MESH_ROPE_TREE value; no ray is left out.  The rays are
made on the CPU from the oracle's first hits, so tests/test_oracle_radiance.py counts the ties of these very batches.  Every test
prints its worst relative difference."""
import numpy as np
import pytest

import bake_ref
import lens_ref
import radiance_oracle as ro
import test_gpu_parity as parity
import test_gpu_rays as qr
from test_oracle_radiance import mixed_batch

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
bits = qr.bits
SEED = ro.SEED
S = 3
LW, LH = 19, 11  # the frame of the lens and bake contracts

_devices = {}


def device(gpu, name, w=ro.W, h=ro.H):
    """(shared CPU scene, DeviceScene of the same description), built once."""
    if (name, w, h) not in _devices:
        sc = ro.scene(gpu, name, w, h)
        _devices[name, w, h] = (sc, gpu.DeviceScene(sc.desc))
    return _devices[name, w, h]


def agree(got, want, what):
    print(f"{what}: worst relative difference {ro.worst(got, want):.3g} over {got.shape[0]} rays")
    parity.assert_pixels_agree(got.reshape(1, -1, 3), want.reshape(1, -1, 3), what)


# ------------------------------------------------------------------------------------------------------------------- families
@pytest.mark.parametrize("family", ro.FAMILIES)
@pytest.mark.parametrize("name", qr.SCENES + ro.EXTRA)
def test_family_follows_the_oracle(gpu, name, family):
    """[flamingo_pond-far] is the case that found a defect: from 1e6 away one ulp of t is 0.0625, triangles that are not neighbours
    tie exactly, and the device's far-origin loop over the leaf-ordered soup kept another triangle (525, 8683) than the reference's
    tree and every mesh mode of the oracle (515, 8555) on 2 of 405 rays, up to 2.08e-3 off, in the shipped and the proof builds
    alike.  The loop now gives an exact tie to the lower triangle id, the order in which the reference's leaves test."""
    sc, dev = device(gpu, name)
    rays = ro.rays(gpu, name, family)
    want, tie = ro.family_expected(gpu, name, family, S)
    got = dev.trace_radiance(rays, spp=S, seed=SEED)
    agree(got, want, f"{name} {family} ({int(tie.sum())} tie rays)")
    if family == "nonunit":  # once more with HRT_RAYS_NORMALIZE, against the oracle on the normalised rays
        want, tie = ro.family_expected(gpu, name, family, S, normalize=True)
        agree(dev.trace_radiance(rays, spp=S, seed=SEED, normalize=True), want, f"{name} {family} normalised ({int(tie.sum())} tie rays)")


# ---------------------------------------------------------------------------------------------------------------------- times
@pytest.mark.parametrize("name", ["many_squares", "many_spheres", "edge_scene"])
def test_the_time_of_the_ray_places_the_moving_objects_along_the_whole_path(gpu, name):
    sc, dev = device(gpu, name)
    rays = np.concatenate([ro.rays(gpu, name, "baking")[:301], ro.rays(gpu, name, "interior")[:200]])
    seen = []
    for time in (F32(0), F32(0.5), np.nextafter(F32(1), F32(0))):
        rays[:, 3] = time
        want, tie = ro.expected(sc, rays, n_samples=S, seed=SEED)
        agree(dev.trace_radiance(rays, spp=S, seed=SEED), want, f"{name} time {time!r}")
        seen.append(want)
    moved = (bits(seen[0]) != bits(seen[1])).any(axis=1) | (bits(seen[1]) != bits(seen[2])).any(axis=1)
    print(f"{name}: {int(moved.sum())} of {len(rays)} rays change with the time")
    assert moved.sum() >= 5, "the times do not move anything these rays see"


# ----------------------------------------------------------------------------------------------------------- keys and samples
@pytest.mark.parametrize("name", qr.SCENES)
def test_keys_high_samples_and_seeds_and_accumulation_follow_the_oracle(gpu, name):
    sc, dev = device(gpu, name)
    rays = np.concatenate([ro.rays(gpu, name, "baking")[:250], ro.rays(gpu, name, "interior")[:151]])
    n = len(rays)
    rng = np.random.default_rng(5)
    keys = ro.random_keys(n, rng)
    rays[n - 1] = rays[n - 2]  # the same ray under the same key, twice: the same value
    keys[n - 1] = keys[n - 2]
    first = 2 ** 32 - S
    want, _ = ro.expected(sc, rays, keys=keys, first_sample=first, n_samples=S, seed=2 ** 64 - 1)
    got = dev.trace_radiance(rays, spp=S, first_sample=first, seed=2 ** 64 - 1, keys=keys)
    agree(got, want, f"{name} random keys, samples from 2^32 - {S}, seed 2^64 - 1")
    assert np.array_equal(bits(got[n - 1]), bits(got[n - 2]))
    base = rng.uniform(0, 3, (n, 3)).astype(F32)
    want, _ = ro.expected(sc, rays, keys=keys, first_sample=5, n_samples=S, seed=0xDEADBEEF00000000, accumulate=base)
    acc = base.copy()
    dev.trace_radiance(rays, spp=S, first_sample=5, seed=0xDEADBEEF00000000, keys=keys, out=acc, accumulate=True)
    agree(acc, want, f"{name} accumulated onto non-zero sums, seed 0xDEADBEEF00000000")


# ---------------------------------------------------------------------------------------------------------------- mixed batch
@pytest.mark.parametrize("name", ["cornell_mesh", "many_spheres"])
def test_degenerate_rows_among_good_ones(gpu, name):
    sc, dev = device(gpu, name)
    good = np.concatenate([ro.rays(gpu, name, "baking")[:300], ro.rays(gpu, name, "far")[:130], ro.rays(gpu, name, "nonunit")[:130]])
    mixed, is_bad, keys, _ = mixed_batch(good)
    assert len(mixed) > 2 * 256 and len(mixed) % 64 and is_bad.sum() == 23
    want, _ = ro.expected(sc, mixed, keys=keys, n_samples=S, seed=SEED)
    got = dev.trace_radiance(mixed, spp=S, seed=SEED, keys=keys)
    assert (bits(got[is_bad]) == 0).all() and (bits(want[is_bad]) == 0).all()
    agree(got, want, f"{name} mixed batch")
    base = np.random.default_rng(2).uniform(1, 2, (len(mixed), 3)).astype(F32)
    acc = base.copy()
    dev.trace_radiance(mixed, spp=S, seed=SEED, keys=keys, out=acc, accumulate=True)
    assert np.array_equal(bits(acc[is_bad]), bits(base[is_bad])), "a degenerate ray changed its sums"
    agree(acc, ro.expected(sc, mixed, keys=keys, n_samples=S, seed=SEED, accumulate=base)[0], f"{name} mixed batch, accumulated")


# ---------------------------------------------------------------------------------------------------------------- lens frames
def oracle_of_records(sc, per_sample_records, keys, first, seed, start=None):
    """The ordered fp32 sum, from `start` or +0, of the oracle's values of the device's own ray records of samples first, first + 1,
    ...: under the tie rule sample by sample.  Returns (sums, number of tie rays)."""
    acc = np.zeros((len(per_sample_records[0]), 3), F32) if start is None else start.copy()
    ties = 0
    for k, rec in enumerate(per_sample_records):
        want, tie = ro.expected(sc, rec, keys=keys, first_sample=first + k, n_samples=1, seed=seed, accumulate=acc)
        acc, ties = want, ties + int(tie.sum())
    return acc, ties


def make_lens(gpu, cam, case):
    proj, ap, fo, ex = lens_ref.CASES[case]
    return gpu.Lens(cam, proj, aperture=ap, focus=fo, extent=ex)


@pytest.mark.parametrize("case", list(lens_ref.CASES))
@pytest.mark.parametrize("name", bake_ref.CONTRACT_SCENES)
def test_lens_frames_follow_the_oracle_on_the_devices_own_rays(gpu, name, case):
    sc, dev = device(gpu, name, LW, LH)
    proj, lens = lens_ref.CASES[case][0], make_lens(gpu, sc.cam, case)
    recs = [gpu.lens_rays(lens, LW, LH, s, SEED).cpu().numpy() for s in range(S)]
    dead = np.stack([(r[:, 4:7] == 0).all(axis=1) for r in recs])
    if proj == "fisheye":  # samples outside the image circle are not traced: they add nothing on both sides
        assert dead.any() and not dead.all()
    else:
        assert not dead.any()
    sums, ties = oracle_of_records(sc, recs, None, 0, SEED)
    got = dev.render_lens(lens, LW, LH, S, SEED)
    agree(got.reshape(-1, 3), sums / F32(S), f"{name} {case} ({ties} tie rays)")
    assert (bits(got.reshape(-1, 3)[dead.all(axis=0)]) == 0).all()


def test_batched_lens_views_with_their_own_seeds_follow_the_oracle(gpu):
    sc, dev = device(gpu, "cornell_mesh", LW, LH)
    seeds = [SEED, 0xDEADBEEF00000000]
    lenses = [make_lens(gpu, sc.cam, case) for case in ("thin", "equirect")]
    frames = dev.render_lens_views(lenses, LW, LH, S, seeds=seeds)
    for v, (lens, seed) in enumerate(zip(lenses, seeds)):
        recs = [gpu.lens_rays(lens, LW, LH, s, seed).cpu().numpy() for s in range(S)]
        sums, ties = oracle_of_records(sc, recs, None, 0, seed)
        agree(frames[v].reshape(-1, 3), sums / F32(S), f"view {v} ({ties} tie rays)")
    assert (bits(frames[0]) != bits(dev.render_lens(lenses[0], LW, LH, S, seeds[1]))).any(), "the views' seeds do not matter"


# ---------------------------------------------------------------------------------------------------------------------- bakes
@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("name", bake_ref.CONTRACT_SCENES)
def test_bakes_follow_the_oracle_on_the_devices_own_rays(gpu, name, with_keys):
    import torch
    sc, dev = device(gpu, name, LW, LH)
    pts = bake_ref.contract_points(gpu, name)
    deg = bake_ref.point_degenerate(pts)
    keys = bake_ref.keys_for(len(pts)) if with_keys else None
    d_pts = torch.from_numpy(pts).cuda()
    d_keys = None if keys is None else torch.from_numpy(keys.view(np.int32)).cuda()
    recs = [gpu.bake_rays(d_pts, s, SEED, d_keys).cpu().numpy() for s in range(S)]
    assert all(((r[:, 4:7] == 0).all(axis=1) == deg).all() for r in recs)
    sums, ties = oracle_of_records(sc, recs, keys, 0, SEED)
    got = dev.bake(pts, S, seed=SEED, keys=keys)
    agree(got, sums / F32(S), f"{name} bake, mean ({ties} tie rays)")
    assert (bits(got[deg]) == 0).all() and got[~deg].any()
    # accumulate form: samples [2, 2 + S) onto non-zero sums
    base = np.random.default_rng(3).uniform(0, 2, (len(pts), 3)).astype(F32)
    recs = [gpu.bake_rays(d_pts, s, SEED, d_keys).cpu().numpy() for s in range(2, 2 + S)]
    sums, ties = oracle_of_records(sc, recs, keys, 2, SEED, start=base)
    acc = torch.from_numpy(base).cuda()
    dev.bake(d_pts, S, first_sample=2, seed=SEED, keys=d_keys, out=acc, accumulate=True)
    acc = acc.cpu().numpy()
    agree(acc, sums, f"{name} bake, accumulated ({ties} tie rays)")
    assert np.array_equal(bits(acc[deg]), bits(base[deg]))
