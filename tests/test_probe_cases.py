"""The inputs of tests/test_gpu_probe_cases.py (tests/probe_cases.py), on the CPU: the probes are finite where they should be and
pairwise distinct in time; with the oracle their times change what they see; the far probe lies beyond the far-origin threshold
and its chosen keys do what they were chosen for -- the aimed rays hit (a mesh among them where the scene has one), the stray rays
miss; the tie rays of every batch the GPU test traces stay within radiance_oracle.tie_cap; r_max lies between the depths that occur;
and the point generators carry their time."""
import numpy as np
import pytest

import bake_ref
import oracle_lib
import probe_cases as pc
import probe_ref
import radiance_oracle as ro

F32, U32 = np.float32, np.uint32
MESH_SCENES = ("many_squares", "edge_scene")


@pytest.mark.parametrize("name", pc.SCENES)
def test_probes_are_live_and_pairwise_distinct_in_time(hrt, oracle, name):
    p = pc.probes(hrt, name)
    assert p.shape == (8, 4) and p.dtype == F32 and np.array_equal(p.view(U32), pc.probes(hrt, name).view(U32))
    live = p[pc.LIVE]
    assert np.isfinite(live).all() and len(set(live[:, 3].tolist())) == 6
    assert {0.0, 0.5, float(np.nextafter(F32(1), F32(0)))} <= set(live[:, 3].tolist()) and ((0 <= live[:, 3]) & (live[:, 3] < 1)).all()
    assert (np.diff(p[:, 3]) != 0).all(), "a probe's time differs from its neighbours' in the batch"
    assert np.array_equal(probe_ref.probe_degenerate(p), np.arange(8) >= 6) and np.isnan(p[6, 0]) and np.isinf(p[7, 3])
    lo, hi = pc.volume_box(hrt, name)
    assert ((np.asarray(lo) < live[:, 0:3]) & (live[:, 0:3] < np.asarray(hi))).all()
    assert pc.keys(name, False) is None and {0, 0xFFFFFFFF} < set(pc.keys(name, True).tolist())


def test_the_bound_is_the_packed_scenes(hrt, oracle):
    """tests/golden/pack_hashes.json records the bound csrc/hrt_pack.h computes for pack_check's cases; one of them is a scene
    the host layer sets up by name."""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "pack_hashes.json")) as f:
        recorded = json.load(f)["hash"]
    for name in ("cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool"):  # spheres, squares, meshes, motion
        host = hrt.HostScene().setup(name, 16 / 9, 1)  # as tests/pack/pack_cases.h sets them up
        assert np.array([pc.bound(hrt, host.flatten())], F32).view(U32)[0] == int(recorded[name]["bound"], 16), name


@pytest.mark.parametrize("name", pc.SCENES)
def test_the_times_change_what_the_probes_see(hrt, oracle, name):
    """SH band 0 over S samples on the NumPy rule's rays, at the probes' own times and with every time set to 0."""
    sc = ro.scene(hrt, name)
    p = pc.probes(hrt, name)[pc.LIVE]
    still = p.copy()
    still[:, 3] = 0
    band0 = []
    for q in (p, still):
        v = np.stack([sc.oracle().radiance(rec, first_sample=s, n_samples=1, seed=pc.SEED, threads=ro.THREADS)
                      for s, rec in enumerate(pc.rule_records(q, None, 0))])
        band0.append((probe_ref.C0 * v).astype(np.float64).sum(axis=0) / pc.S)
    moved = (band0[0] != band0[1]).any(axis=1)
    print(f"{name}: the time changes band 0 of {int(moved.sum())} of the 6 live probes {np.flatnonzero(moved).tolist()}")
    assert not moved[p[:, 3] == 0].any()
    if name in pc.STATIC:  # nothing moves in the skybox scene
        assert not moved.any()
    else:
        assert moved.sum() >= 3, "the times do not move anything these probes see"


@pytest.mark.parametrize("name", pc.SCENES)
def test_the_far_keys_hit_and_miss_as_chosen(hrt, oracle, name):
    sc = ro.scene(hrt, name)
    rec, keys, aimed = pc.far_set(hrt, name)
    pos, dist, b, far = pc.far_position(hrt, name)
    centre, radius, meshes = pc.box(hrt, sc.desc)
    assert dist > far == 16.0 * (b + 1.0) and (rec[:, 0:3] == pos).all() and (rec[:, 3] == pc.FAR_TIME).all()
    assert len(set(keys.tolist())) == 64 and aimed.sum() == pc.AIMED and (~aimed).sum() == pc.STRAY
    # the device's direction is within PROBE_TOL per component of the rule's: at this distance that moves a ray by far less than
    # the margins the keys were chosen with (half the radius inside, twice the radius outside)
    reach = dist + np.linalg.norm(centre) + 2 * radius
    assert probe_ref.PROBE_TOL * reach < 0.1 * (radius / 2), (name, reach, radius)
    rays = pc.rule_records(rec, keys, 0, 1)
    off, t = pc.line_distance(rays[0, :, 0:3].astype(np.float64), rays[0, :, 4:7].astype(np.float64), centre)
    assert (off[aimed] < radius / 2).all() and (t[aimed] > 0).all() and ((off[~aimed] > 2 * radius) | (t[~aimed] <= 0)).all()
    kind, t, _, tie = pc.first_segments(sc, rays, keys, 0)
    kind, tie = kind[0], tie[0]
    r = pc.depths(kind, t, pc.far_r_max(hrt, name))[0][aimed]
    assert (r < F32(pc.far_r_max(hrt, name))).any() and (r == F32(pc.far_r_max(hrt, name))).any(), "r_max lies between the depths that occur"
    hits, mesh_hits = int((kind[aimed] != 0).sum()), int((kind[aimed] == hrt.KIND_MESH).sum())
    print(f"{name}: far probe {dist:.1f} from the origin (bound {b:.3f}, far beyond {far:.1f}); {hits} of {pc.AIMED} aimed keys hit, "
          f"{mesh_hits} of them a mesh; {int((kind[~aimed] != 0).sum())} of {pc.STRAY} stray keys hit; {int(tie.sum())} first-segment ties")
    assert hits >= 40 and (kind[~aimed] == 0).all()
    assert (mesh_hits >= 1) == (name in MESH_SCENES), (name, mesh_hits, len(meshes))
    _, _, vtie = ro.oracle_pair(sc, rays[0], keys=keys, first_sample=0, n_samples=1, seed=pc.SEED)
    print(f"{name}: far set: {int(vtie.sum())} tie rays of 64 (cap {ro.tie_cap(64)})")
    assert vtie.sum() <= ro.tie_cap(64) and tie.sum() <= ro.tie_cap(64)


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("name", pc.SCENES)
def test_tie_rays_stay_within_the_cap_and_r_max_lies_between_the_depths(hrt, oracle, name, with_keys):
    """On the NumPy rule's rays, which the device's own are within PROBE_TOL of."""
    sc = ro.scene(hrt, name)
    p, keys = pc.probes(hrt, name), pc.keys(name, with_keys)
    recs = pc.rule_records(p, keys, 0)
    total = 0
    for s, rec in enumerate(recs):
        _, _, tie = ro.oracle_pair(sc, rec, keys=keys, first_sample=s, n_samples=1, seed=pc.SEED)
        assert tie.sum() <= ro.tie_cap(len(rec)), (name, s, int(tie.sum()))
        total += int(tie.sum())
    kind, t, _, stie = pc.first_segments(sc, recs, keys, 0)
    r = pc.depths(kind, t, pc.R_MAX[name])[:, pc.LIVE]
    print(f"{name}, keys {with_keys}: {total} tie rays and {int(stie.sum())} first-segment ties of {recs.shape[0] * recs.shape[1]} samples "
          f"(cap {ro.tie_cap(recs.shape[0] * recs.shape[1])}); {(r < F32(pc.R_MAX[name])).mean():.3f} of the depths are below r_max {pc.R_MAX[name]}")
    assert total <= ro.tie_cap(recs.shape[0] * recs.shape[1]) and stie.sum() <= ro.tie_cap(recs.shape[0] * recs.shape[1])
    assert 0.1 < (r < F32(pc.R_MAX[name])).mean() < 0.9, "r_max lies between the depths that occur"


def test_the_chain_and_the_tolerance():
    assert pc.chain(65, 64) == 1 + 1 + 6 + 2 + 1 and pc.chain(1, 64) == 10 and pc.chain(513, 256) == 1 + 4 + 6 + 3 + 1
    rng = np.random.default_rng(1)
    Y, v = rng.standard_normal((65, 2, 9)).astype(F32), (100 * rng.standard_normal((65, 2, 3))).astype(F32)
    deg = np.zeros((65, 2), bool)
    deg[:, 1] = True
    tol = pc.coefficient_tolerance(Y, v, deg)
    assert tol.shape == (2, 9, 3) and (tol[0] > 0).all() and not tol[1].any()
    # a perturbation of every sample at the bar stays within it; ten times the bar does not
    nudge = (1e-6 * np.maximum(1, np.abs(v))).astype(F32)
    a, b, c = (probe_ref.fold(Y, w, deg) / F32(65) for w in (v, v + nudge, v + F32(20) * nudge))
    assert (np.abs(b.astype(np.float64) - a) <= tol).all() and (np.abs(c.astype(np.float64) - a) > tol).any()


def test_the_point_generators_carry_their_time(hrt):
    quad = hrt.Quad.make((0, 0, 0), (2, 0, 0), (0, 0, -3))
    q = hrt.quad_points(quad, 4, 3, time=0.75)
    assert q.shape == (12, 8) and (q[:, 3] == F32(0.75)).all()
    assert np.array_equal(q.view(U32), bake_ref.quad_points(quad.v0[:], quad.v1[:], quad.v3[:], 4, 3, time=0.75).view(U32))
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], U32)
    m = hrt.mesh_points(pos, tri, time=0.75)
    assert m.shape == (4, 8) and (m[:, 3] == F32(0.75)).all() and np.array_equal(m.view(U32), bake_ref.mesh_points(pos, tri, time=0.75).view(U32))
    g = hrt.probe_grid((-1, -1, -1), (1, 1, 1), 2, 2, 2, time=0.5)
    assert (g[:, 3] == F32(0.5)).all() and np.array_equal(g.view(U32), probe_ref.grid((-1, -1, -1), (1, 1, 1), 2, 2, 2, time=0.5).view(U32))
    assert (hrt.quad_points(quad, 4, 3)[:, 3] == 0).all() and (hrt.probe_grid((-1, -1, -1), (1, 1, 1), 2, 2, 2)[:, 3] == 0).all()
