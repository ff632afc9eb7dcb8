"""The NumPy statement of path features (tests/path_features_ref.py, include/hrt.h "Path features") on hand-made paths: what the rule
does with the surfaces a path meets, what the fold does with the records of a pixel, and what a tail record says of the same path.
No GPU, no library."""
import numpy as np

import lit_paths_ref as lp
import path_features_ref as pf

F32, U32 = np.float32, np.uint32
D, G, M = pf.DIFFUSE, 1, 2
bits = lambda a: np.ascontiguousarray(a, F32).view(U32)


def seg(typ, albedo, emission=(0, 0, 0), t=1.0, normal=(0, 0, 1)):
    return (typ, np.asarray(albedo, F32), np.asarray(emission, F32), F32(t), np.asarray(normal, F32))


def test_a_mirror_then_a_diffuse_wall_is_reached_on_segment_two():
    m, a = np.array([0.9, 0.8, 0.7], F32), np.array([0.6, 0.5, 0.4], F32)
    e_m, e_a = np.array([0.25, 0.5, 1.0], F32), np.array([2.0, 3.0, 4.0], F32)
    r = pf.record([seg(M, m, e_m, 1.5, (1, 0, 0)), seg(D, a, e_a, 0.3, (0, -1, 0)), seg(D, (9, 9, 9), (9, 9, 9), 9.0)])
    assert r.dtype == F32 and r.shape == (12,)
    assert np.array_equal(bits(r[pf.ALBEDO]), bits((F32(1) * m) * a)), "thr = (1 * m) * a, in that order"
    assert np.array_equal(r[pf.NORMAL], np.array([0, -1, 0], F32)), "the diffuse surface's normal, not the mirror's"
    assert np.array_equal(bits(r[pf.EMISSION]), bits((np.zeros(3, F32) + np.ones(3, F32) * e_m) + (F32(1) * m) * e_a)), "E before thr is updated"
    assert r[pf.DEPTH] == F32(F32(0) + F32(1.5)) + F32(0.3) and r[pf.COVERAGE] == 1 and r[11] == 0
    # the third surface is never met: the path does not scatter at a diffuse hit
    assert np.array_equal(bits(r), bits(pf.record([seg(M, m, e_m, 1.5, (1, 0, 0)), seg(D, a, e_a, 0.3, (0, -1, 0))])))


def test_a_first_diffuse_hit_and_a_first_miss_are_the_first_hit_values():
    a, e, n = np.array([0.3, 0.7, 0.1], F32), np.array([5, 0, 2], F32), np.array([0.6, 0, -0.8], F32)
    r = pf.record([seg(D, a, e, 7.25, n)])
    want = np.concatenate([a, n, e, [F32(7.25), F32(1), F32(0)]]).astype(F32)
    assert np.array_equal(bits(r), bits(want)), "1 * x, 0 + x and 0 + 1 * x are exact"
    assert not bits(pf.record([None])).any() and not bits(pf.record([None, seg(D, a, e)])).any(), "a first-segment miss: twelve zeros"
    assert not bits(pf.record([])).any()


def test_six_glass_hits_are_unreached_and_keep_the_emission():
    g, e = np.array([0.5, 1.0, 0.25], F32), np.array([1, 2, 3], F32)
    r = pf.record([seg(G, g, e, 2.0)] * 6)
    E, thr = np.zeros(3, F32), np.ones(3, F32)
    for _ in range(6):
        E, thr = E + thr * e, thr * g
    assert np.array_equal(bits(r[pf.EMISSION]), bits(E)) and E.all()
    assert not bits(r[pf.ALBEDO]).any() and not bits(r[pf.NORMAL]).any() and r[pf.DEPTH] == 0 and r[pf.COVERAGE] == 0 and r[11] == 0
    # a miss after two glass hits: unreached as well, with the emission of those two, and no sky
    r2 = pf.record([seg(G, g, e), seg(G, g, e), None])
    assert np.array_equal(bits(r2[pf.EMISSION]), bits((np.zeros(3, F32) + e) + g * e)) and not bits(r2[[0, 1, 2, 3, 4, 5, 9, 10, 11]]).any()
    # seven segments are not a path
    try:
        pf.record([seg(G, g, e)] * 7)
    except AssertionError:
        pass
    else:
        raise AssertionError("more than MAXBOUNCES segments were accepted")


def test_the_fold_sums_in_sample_order_from_plus_zero_and_divides_by_the_count():
    rng = np.random.default_rng(3)
    R = rng.uniform(-4, 4, (5, 7, 12)).astype(F32)
    R[0, 0, 3] = F32(-0.0)
    R[1:, 0, 3] = 0
    want = np.zeros((7, 12), F32)
    for s in range(5):
        want = want + R[s]
    want = want / F32(5)
    got = pf.fold(R)
    assert got.dtype == F32 and np.array_equal(bits(got), bits(want))
    assert bits(got[0, 3]) == 0, "+0 + -0 is +0: the sum starts from +0"
    back = pf.fold(R[::-1])
    assert not np.array_equal(bits(back), bits(got)), "the order of the samples is part of the rule"
    traced = np.ones((5, 7), bool)
    traced[2, 4] = traced[:, 6] = False
    got = pf.fold(R, traced)
    assert np.array_equal(bits(got[:4]), bits(want[:4])) and not bits(got[6]).any(), "a pixel the lens never traces is twelve zeros"
    skip = np.zeros(12, F32)
    for s in (0, 1, 3, 4):
        skip = skip + R[s, 4]
    assert np.array_equal(bits(got[4]), bits(skip / F32(5))), "an untraced sample adds nothing and counts in the divisor"


def test_a_tail_record_gives_albedo_normal_coverage_and_emission_over_six():
    T = np.zeros((3, lp.TAIL_FLOATS), F32)
    T[0, 4:7], T[0, 8:11], T[0, 12:15] = (0, 1, 0), (0.5, 0.25, 0.125), (1, 2, 3)
    T.view(U32)[:, lp.TAIL_WORD] = (0x80000002, 6, 1)
    T[1, 12:15] = (4, 5, 6)
    albedo, normal, coverage, e6 = pf.from_tail(T)
    assert coverage.tolist() == [1.0, 0.0, 0.0] and coverage.dtype == F32
    assert np.array_equal(albedo[0], np.array([0.5, 0.25, 0.125], F32)) and not albedo[1:].any()
    assert np.array_equal(normal[0], np.array([0, 1, 0], F32)) and not normal[1:].any()
    assert np.array_equal(e6, np.array([[1, 2, 3], [4, 5, 6], [0, 0, 0]], F32))
