"""The oracle's radiance of a caller's ray (oracle/oracle.cpp oracle_radiance, oracle_lib.OracleScene.radiance), on the CPU alone.

THE PIN: fed the camera rays of each sample it reproduces oracle_render bit for bit on every scene, so the entry adds no second
integrator beside the pinned one.  THE WRAPPER's restatement of include/hrt.h "radiance queries": keys, accumulated splits,
degenerate rays, tmax.  THE TIE CONDITION: how many rays of each batch tests/test_gpu_radiance_oracle.py traces are settled
differently by the oracle's own two mesh modes (radiance_oracle.py states the rule)."""
import numpy as np
import pytest

import oracle_lib
import radiance_oracle as ro
import test_gpu_rays as qr

F32 = np.float32
U32 = np.uint32
bits = qr.bits
PIN_SCENES = qr.SCENES + ["many_squares", "many_spheres"]
PW, PH = 19, 11
SEED = ro.SEED  # high bits set


def camera_sample_rays(cam, w, h, sample, seed):
    """The render's camera rays of one sample as ray records: draws 0..2 of stream (seed, pixel, sample) are u, v, time."""
    draws = np.stack([oracle_lib.path_stream(seed, p, sample, 3) for p in range(w * h)])
    y, x = np.divmod(np.arange(w * h), w)
    uv = np.stack([(x.astype(F32) + draws[:, 0]) / F32(w), (y.astype(F32) + draws[:, 1]) / F32(h)], axis=1).astype(F32)
    cr = oracle_lib.camera_rays(cam, uv)
    return qr.make_rays(cr[:, 0:3], cr[:, 3:6], draws[:, 2])


# -------------------------------------------------------------------------------------------------------------------- the pin
@pytest.mark.parametrize("name", PIN_SCENES)
def test_radiance_of_the_camera_rays_is_the_render_bit_for_bit(hrt, name):
    S = 3 + PIN_SCENES.index(name) % 3
    sc = ro.scene(hrt, name, PW, PH)
    cam, o = sc.cam, sc.oracle()
    acc = np.zeros((PW * PH, 3), F32)
    for s in range(S):
        acc = acc + o.radiance(camera_sample_rays(cam, PW, PH, s, SEED), first_sample=s, n_samples=1, seed=SEED, threads=ro.THREADS)
    want = o.render(cam, PW, PH, S, seed=SEED, threads=ro.THREADS)
    assert np.array_equal(bits(acc / F32(S)), bits(want.reshape(-1, 3))), f"{name} S={S}"
    assert np.isfinite(want).all() and want.any()


def test_samples_at_the_top_of_the_sample_range_follow_the_splits_rule(hrt):
    """first_sample = 2^32 - S: no render starts there, so the samples are held to the splits rule alone, and shown to be other
    samples than [0, S)."""
    S = 7
    sc = ro.scene(hrt, "cornell_mesh")
    o = sc.oracle()
    rays = camera_sample_rays(hrt.default_camera(PW / PH), PW, PH, 0, SEED)
    first = 2 ** 32 - S
    whole = o.radiance(rays, first_sample=first, n_samples=S, seed=SEED, accumulate=np.zeros((len(rays), 3), F32), threads=ro.THREADS)
    assert np.array_equal(bits(o.radiance(rays, first_sample=first, n_samples=S, seed=SEED, threads=ro.THREADS)), bits(whole / F32(S)))
    acc = np.zeros((len(rays), 3), F32)
    for k in (3, 1, 3):
        acc = o.radiance(rays, first_sample=first, n_samples=k, seed=SEED, accumulate=acc, threads=ro.THREADS)
        first += k
    assert first == 2 ** 32 and np.array_equal(bits(acc), bits(whole))
    low = o.radiance(rays, first_sample=0, n_samples=S, seed=SEED, accumulate=np.zeros((len(rays), 3), F32), threads=ro.THREADS)
    assert (bits(low) != bits(whole)).any(), "the sample index does not reach the random numbers"


# ---------------------------------------------------------------------------------------------------------------- the wrapper
@pytest.fixture(scope="module")
def batch(hrt):
    sc = ro.scene(hrt, "random_spheres")
    rays = np.concatenate([ro.rays(hrt, "random_spheres", "baking")[:150], ro.rays(hrt, "random_spheres", "interior")[:150]])
    return sc.oracle(), rays, sc.oracle().radiance(rays, n_samples=2, seed=SEED, threads=ro.THREADS)


def test_a_permuted_batch_with_its_keys_gives_the_permuted_values(batch):
    o, rays, plain = batch
    n = len(rays)
    assert np.array_equal(bits(o.radiance(rays, keys=np.arange(n, dtype=U32), n_samples=2, seed=SEED)), bits(plain))
    perm = np.random.default_rng(3).permutation(n)
    got = o.radiance(rays[perm], keys=perm.astype(U32), n_samples=2, seed=SEED, threads=ro.THREADS)
    assert np.array_equal(bits(got), bits(plain[perm]))
    other = o.radiance(rays, keys=np.arange(n, 2 * n, dtype=U32), n_samples=2, seed=SEED, threads=ro.THREADS)
    assert (bits(other) != bits(plain)).any(axis=1).sum() > n // 4, "keys do not change the samples"


def test_accumulated_splits_equal_one_call(batch):
    o, rays, _ = batch
    n, S = len(rays), 7
    zero = np.zeros((n, 3), F32)
    whole = o.radiance(rays, n_samples=S, seed=SEED, accumulate=zero, threads=ro.THREADS)
    assert not zero.any(), "accumulate was modified"
    assert np.array_equal(bits(o.radiance(rays, n_samples=S, seed=SEED, threads=ro.THREADS)), bits(whole / F32(S)))
    acc, first = zero, 0
    for k in (3, 1, 3):
        acc = o.radiance(rays, first_sample=first, n_samples=k, seed=SEED, accumulate=acc, threads=ro.THREADS)
        first += k
    assert np.array_equal(bits(acc), bits(whole))
    base = np.random.default_rng(2).uniform(0, 3, (n, 3)).astype(F32)  # onto non-zero sums: added in order to what is there
    one = o.radiance(rays, n_samples=1, seed=SEED)
    assert np.array_equal(bits(o.radiance(rays, n_samples=1, seed=SEED, accumulate=base)), bits(base + one))


def degenerate_rows(good):
    """The degenerate rows of test_gpu_radiance.test_degenerate_rays_normalisation_and_empty_batches."""
    nan, inf = F32(np.nan), F32(np.inf)
    rows = []
    for col in range(7):
        for v in (nan, inf, -inf):
            r = good[col].copy(); r[col] = v; rows.append(r)
    for z in ((0, 0, 0), (-0.0, 0, -0.0)):
        r = good[5].copy(); r[4:7] = z; rows.append(r)
    return np.array(rows, F32)


def mixed_batch(good, seed=1):
    """`good` with degenerate_rows scattered among it: (batch, is_bad, keys that leave every good ray its own key)."""
    mixed = np.concatenate([good, degenerate_rows(good)])
    order = np.random.default_rng(seed).permutation(len(mixed))
    is_bad = order >= len(good)
    return mixed[order], is_bad, np.where(is_bad, 0, order).astype(U32), order


def test_degenerate_rays_give_zero_or_leave_their_sums_alone(batch):
    o, good, plain = batch
    mixed, is_bad, keys, order = mixed_batch(good)
    assert is_bad.sum() == 23
    got = o.radiance(mixed, keys=keys, n_samples=2, seed=SEED, threads=ro.THREADS)
    assert (bits(got[is_bad]) == 0).all()
    assert np.array_equal(bits(got[~is_bad]), bits(plain[order[~is_bad]])), "good rays changed beside degenerate ones"
    base = np.random.default_rng(2).uniform(1, 2, (len(mixed), 3)).astype(F32)
    acc = o.radiance(mixed, keys=keys, n_samples=2, seed=SEED, accumulate=base, threads=ro.THREADS)
    assert np.array_equal(bits(acc[is_bad]), bits(base[is_bad])), "a degenerate ray changed its sums"
    assert (bits(acc[~is_bad]) != bits(base[~is_bad])).any()
    # a direction whose length under- or overflows is degenerate only under normalisation
    odd = good[:6].copy()
    odd[:3, 4:7] = F32(1e-30)
    odd[3:, 4:7] = F32(3e38)
    assert (bits(o.radiance(odd, n_samples=1, seed=SEED, normalize=True)) == 0).all()
    assert np.array_equal(bits(o.radiance(odd, n_samples=1, seed=SEED, normalize=True, accumulate=base[:6])), bits(base[:6]))
    # normalize == the directions normalised beforehand
    raw = good.copy()
    raw[:, 4:7] *= np.random.default_rng(7).choice([1e-3, 0.37, 3.0, 1e3], size=(len(raw), 1)).astype(F32)
    pre = raw.copy()
    pre[:, 4:7] = oracle_lib.kat_normalize(raw[:, 4:7])
    assert np.array_equal(bits(o.radiance(raw, n_samples=2, seed=SEED, normalize=True, threads=ro.THREADS)),
                          bits(o.radiance(pre, n_samples=2, seed=SEED, threads=ro.THREADS)))
    assert o.radiance(np.zeros((0, 8), F32)).shape == (0, 3)


def test_tmax_is_never_read(batch):
    o, rays, plain = batch
    for tmax in (0.0, np.nan, 1e-4, np.inf):
        r = rays.copy()
        r[:, 7] = tmax
        assert np.array_equal(bits(o.radiance(r, n_samples=2, seed=SEED, threads=ro.THREADS)), bits(plain)), tmax


def test_the_path_instrument_records_the_path_radiance_runs(hrt):
    """trace_ray_path of (ray, key, sample): the first query is the caller's ray as given, every later one starts at the hit before
    it and carries the ray's time; for a camera ray it is trace_path's record of that pixel and sample."""
    sc = ro.scene(hrt, "random_spheres")
    o = sc.oracle()
    cam = hrt.default_camera(PW / PH)
    rays = camera_sample_rays(cam, PW, PH, 2, SEED)
    for p in (0, 57, PW * PH - 1):
        want = oracle_lib.trace_path(o, cam, PW, PH, p % PW, p // PW, 2, SEED)
        got = o.trace_ray_path(rays[p], p, 2, SEED)
        assert len(got) >= 1 and np.array_equal(bits(got), bits(want)), p
    r = ro.rays(hrt, "random_spheres", "nonunit")[3]
    rows = o.trace_ray_path(r, 0xFFFFFFFF, 2 ** 32 - 1, SEED)
    assert np.array_equal(bits(rows[0, 0:7]), bits(np.concatenate([r[0:3], r[4:7], r[3:4]]))), "the first segment is not the ray as given"
    assert (bits(rows[:, 6]) == bits(r[3:4])).all(), "a segment lost the ray's time"
    for a, b in zip(rows, rows[1:]):
        assert a[7] != 0 and np.abs(a[0:3] + a[9] * a[3:6] - b[0:3]).max() < 1e-3


# ---------------------------------------------------------------------------------------------------------- the tie condition
@pytest.mark.parametrize("name", qr.SCENES + ro.EXTRA)
def test_tie_rays_stay_inside_the_cap(hrt, name):
    """For every (scene, family) the GPU test traces with rays made here: the rays on which MESH_REF_TREE and MESH_ROPE_TREE
    disagree bit-wise number at most max(1, n // 100)."""
    for family in ro.FAMILIES:
        _, tie = ro.family_expected(hrt, name, family)  # asserts the cap
        print(f"{name} {family}: {int(tie.sum())} tie rays of {len(tie)}")
    _, tie = ro.family_expected(hrt, name, "nonunit", normalize=True)
    print(f"{name} nonunit, normalised: {int(tie.sum())} tie rays of {len(tie)}")
