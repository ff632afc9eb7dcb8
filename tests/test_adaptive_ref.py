"""The numpy statement of the adaptive rule (tests/adaptive_ref.py) on hand-built arrays: no GPU.  The GPU tests trust it to say
which count every tile must get, so its edges are pinned here: partial tiles, non-finite pixels, the count sequences."""
import numpy as np
import pytest

from adaptive_ref import (expected_counts, list_lengths, near_threshold, per_pixel, pixel_err, samples, same_bits, sequence,
                          tile_err, tiles_differing, tiles_shape)

F = np.float32


def flat(h, w, value):
    return np.full((h, w, 3), value, dtype=np.float32)


@pytest.mark.parametrize("mn,mx,want", [(2, 2, [1, 2]), (2, 1024, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]),
                                        (6, 50, [3, 6, 12, 24, 48, 50]), (10, 10, [5, 10]), (16, 256, [8, 16, 32, 64, 128, 256]),
                                        (10, 40, [5, 10, 20, 40]), (2, 4096, [2 ** k for k in range(13)])])
def test_sequence(mn, mx, want):
    assert sequence(mn, mx) == want


def test_pixel_err_is_the_stated_fp32_formula():
    a = np.array([[[0.25, 0.5, 1.0]]], np.float32)
    b = np.array([[[0.5, 0.25, 2.0]]], np.float32)
    num = (F(0.25) + F(0.25)) + F(1.0)
    den = np.sqrt(((F(1e-4) + F(0.5)) + F(0.25)) + F(2.0))
    e = pixel_err(a, b)
    assert e.dtype == np.float32 and e.shape == (1, 1)
    assert e[0, 0] == F(num / den)
    # the sums go left to right: 1 + 2^-24 + 2^-24 rounds to 1 step by step, to 1 + 2^-23 if the two small terms were added first
    tiny = F(2.0 ** -24)
    a = np.zeros((1, 1, 3), np.float32)
    b = np.array([[[1.0, tiny, tiny]]], np.float32)
    assert pixel_err(a, b)[0, 0] == F(F(1.0) / np.sqrt((F(1e-4) + F(1.0)) + tiny + tiny))
    assert (F(1.0) + tiny) + tiny == F(1.0) and F(1.0) + (tiny + tiny) != F(1.0)
    # equal means: no error; the brightness floor 1e-4 keeps black pixels finite
    assert pixel_err(flat(2, 2, 0.0), flat(2, 2, 0.0)).max() == 0
    assert pixel_err(flat(1, 1, 0.0), flat(1, 1, 1e-3))[0, 0] == F(F(3e-3) / np.sqrt(F(F(F(1e-4) + F(1e-3)) + F(1e-3)) + F(1e-3)))


def test_tile_err_takes_the_max_over_each_tile():
    h, w = 16, 24
    a, b = flat(h, w, 0.5), flat(h, w, 0.5)
    b[3, 5] = (0.6, 0.5, 0.5)   # tile (0, 0)
    b[9, 20] = (0.5, 0.9, 0.5)  # tile (1, 2)
    b[10, 21] = (0.5, 0.7, 0.5)
    err = tile_err(a, b)
    assert err.shape == (2, 3) and err.dtype == np.float32
    e = pixel_err(a, b)
    assert err[0, 0] == e[3, 5] and err[1, 2] == e[9, 20] > e[10, 21]
    assert err[0, 1] == err[0, 2] == err[1, 0] == err[1, 1] == 0


@pytest.mark.parametrize("h,w", [(1, 1), (9, 17), (1, 37), (37, 1), (67, 120)])
def test_partial_tiles_see_only_their_in_image_pixels(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    a = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    b = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    err = tile_err(a, b, w, h)
    ty, tx = tiles_shape(w, h)
    assert err.shape == (ty, tx)
    e = pixel_err(a, b)
    for y in range(ty):
        for x in range(tx):
            assert err[y, x] == e[y * 8:y * 8 + 8, x * 8:x * 8 + 8].max()
    # the last row and column of tiles: only the pixels that exist count
    assert err[-1, -1] == e[(ty - 1) * 8:, (tx - 1) * 8:].max()
    if (h, w) == (1, 1):
        assert err[0, 0] == e[0, 0]


def test_a_mixed_tile_ignores_its_non_finite_pixels():
    a, b = flat(8, 8, 0.5), flat(8, 8, 0.5)
    b[2, 2] = (0.5, 0.75, 0.5)
    for bad in (np.nan, np.inf, -np.inf):
        aa, bb = a.copy(), b.copy()
        aa[0, 0] = bb[0, 0] = (bad, 0.5, 0.5)  # a mean that is NaN, or inf on both sides (inf - inf = NaN)
        aa[7, 7] = (0.5, 0.5, 0.5)
        bb[7, 7] = (np.inf, 0.5, 0.5)          # finite before, inf after: inf / inf = NaN
        e = pixel_err(aa, bb)
        assert e[0, 0] == 0 and e[7, 7] == 0
        assert tile_err(aa, bb)[0, 0] == pixel_err(a, b)[2, 2] > 0


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_tile_of_only_non_finite_pixels_has_error_zero(bad):
    a, b = flat(8, 16, 0.5), flat(8, 16, 0.5)
    b[:, 8:] = 0.75
    a[:, :8] = b[:, :8] = bad  # tile (0, 0): every pixel non-finite
    err = tile_err(a, b)
    assert err[0, 0] == 0 and err[0, 1] > 0
    # so threshold 0 takes it to max_spp, any positive threshold stops it at min_spp
    table = {4: err, 8: err, 16: err}
    assert expected_counts(table, 4, 16, 0.0).tolist() == [[16, 16]]
    assert expected_counts(table, 4, 16, 1e-30).tolist() == [[4, 16]]
    assert expected_counts(table, 4, 16, np.inf).tolist() == [[4, 4]]


def test_a_partial_tile_of_non_finite_pixels_has_error_zero():
    """9 x 17: the tile at the bottom right has one in-image pixel; when it is NaN, nothing else counts."""
    a, b = flat(9, 17, 0.25), flat(9, 17, 0.5)
    a[8, 16] = b[8, 16] = np.nan
    err = tile_err(a, b, 17, 9)
    assert err.shape == (2, 3)
    assert err[1, 2] == 0 and (np.delete(err.ravel(), 5) > 0).all()


def test_expected_counts_on_a_table_worked_by_hand():
    """min 4, max 20: counts 4 -> 8 -> 16 -> 20; threshold 1.  A tile goes on from n while its error at n is >= 1."""
    err = {4: np.array([[0.5, 1.0, 2.0, 3.0, 1.0]], np.float32),
           8: np.array([[9.0, 0.9, 1.0, 3.0, 1.5]], np.float32),
           16: np.array([[9.0, 9.0, 0.999, 1.0, 9.0]], np.float32),
           20: np.array([[9.0, 9.0, 9.0, 9.0, 9.0]], np.float32)}  # judged at max: never goes further
    counts = expected_counts(err, 4, 20, 1.0)
    assert counts.dtype == np.uint32
    assert counts.tolist() == [[4, 8, 16, 20, 20]]
    assert expected_counts(err, 4, 20, 0.0).tolist() == [[20] * 5]
    assert expected_counts(err, 4, 20, np.inf).tolist() == [[4] * 5]
    assert list_lengths(counts, 4, 20) == {8: 4, 16: 3, 20: 2}
    near = near_threshold(err, 1.0)
    assert near.tolist() == [[False, True, True, True, True]]
    # min == max: a uniform render whatever the threshold
    assert expected_counts({6: np.array([[5.0]], np.float32)}, 6, 6, 0.0).tolist() == [[6]]


def test_per_pixel_counts_and_samples():
    counts = np.array([[4, 8, 16]], np.uint32)
    pp = per_pixel(counts, 17, 5)
    assert pp.shape == (5, 17)
    assert (pp[:, :8] == 4).all() and (pp[:, 8:16] == 8).all() and (pp[:, 16] == 16).all()
    assert samples(counts, 17, 5) == 5 * (8 * 4 + 8 * 8 + 1 * 16)


def test_same_bits_and_tiles_differing():
    nan2 = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
    a = flat(9, 17, 1.0)
    a[0, 0, 0] = np.nan
    b = a.copy()
    assert same_bits(a, b)
    b[0, 0, 0] = nan2
    assert not same_bits(a, b)        # another NaN payload
    assert not same_bits(flat(1, 1, 0.0), flat(1, 1, -0.0))
    assert not same_bits(flat(1, 2, 0.0), flat(2, 1, 0.0))
    counts = np.array([[4, 4, 8], [8, 4, 4]], np.uint32)
    refs = {4: a.copy(), 8: a.copy()}
    frame = a.copy()
    assert tiles_differing(frame, counts, refs) == []
    refs[8][8, 16, 2] = 2.0           # tile (1, 2) is at 4: the 8-spp reference does not matter there
    assert tiles_differing(frame, counts, refs) == []
    refs[4][8, 16, 2] = 2.0
    assert tiles_differing(frame, counts, refs) == [(1, 2, 4)]
    frame[0, 0, 0] = nan2
    assert tiles_differing(frame, counts, refs) == [(0, 0, 4), (1, 2, 4)]
