"""Plain numpy statement of the adaptive-sampling rule of include/hrt.h (hrt_render_adaptive*), shared by the adaptive tests.

Everything here is host arithmetic on frames: no GPU, no library.  tests/test_adaptive_ref.py checks it on hand-built arrays;
the GPU tests recompute the counts a frame must get from uniform renders with it."""
import numpy as np

TILE = 8


def tiles_shape(w, h):
    """(tiles_y, tiles_x) of a w x h frame."""
    return (h + TILE - 1) // TILE, (w + TILE - 1) // TILE


def sequence(min_spp, max_spp):
    """The counts a tile passes through: min/2 (round 0), min (round 1), then doubling, clipped at max."""
    seq = [min_spp // 2, min_spp]
    while seq[-1] < max_spp:
        seq.append(min(2 * seq[-1], max_spp))
    return seq


def pixel_err(a, b):
    """include/hrt.h, per pixel in fp32: e = (|B.r - A.r| + |B.g - A.g| + |B.b - A.b|) / sqrtf(1e-4 + |B.r| + |B.g| + |B.b|), the sums
    added left to right; a pixel whose e is NaN (a mean that is inf or NaN) counts as 0.  a, b: (h, w, 3) means at n_old and n_new
    samples (no gamma): exactly S_old / n_old and S_new / n_new."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.abs(b - a)
        num = (d[..., 0] + d[..., 1]) + d[..., 2]
        den = np.sqrt(((np.float32(1e-4) + np.abs(b[..., 0])) + np.abs(b[..., 1])) + np.abs(b[..., 2]))
        e = (num / den).astype(np.float32)
        return np.where(e >= np.float32(0), e, np.float32(0)).astype(np.float32)


def tile_err(a, b, w=None, h=None):
    """The error of every tile: the max of pixel_err over the tile's in-image pixels (lanes outside the image are ignored), as a
    (tiles_y, tiles_x) float32 array.  w, h default to the frames' own size."""
    e = pixel_err(a, b)
    h = e.shape[0] if h is None else h
    w = e.shape[1] if w is None else w
    assert e.shape == (h, w), (e.shape, (h, w))
    ty, tx = tiles_shape(w, h)
    pad = np.zeros((ty * TILE, tx * TILE), dtype=np.float32)  # every e is >= 0: the padding never wins the max
    pad[:h, :w] = e
    return pad.reshape(ty, TILE, tx, TILE).max(axis=(1, 3))


def errors_from(frames, min_spp, max_spp):
    """tile_err of every judged count n (the error computed in the round that brought a tile to n), from uniform frames keyed by
    count: {n: error table}."""
    seq = sequence(min_spp, max_spp)
    return {n: tile_err(frames[p], frames[n]) for p, n in zip(seq, seq[1:])}


def expected_counts(err, min_spp, max_spp, thr):
    """The count every tile gets: it starts at min_spp and moves on to the next count of the sequence while its error at the
    current count is at or above the threshold."""
    seq = sequence(min_spp, max_spp)[1:]
    counts = np.full(err[seq[0]].shape, seq[0], dtype=np.uint32)
    for cur, nxt in zip(seq, seq[1:]):
        go = (counts == cur) & (err[cur] >= np.float32(thr))
        counts[go] = nxt
    return counts


def near_threshold(err, thr, rel=1e-5):
    """Tiles whose error at some judged count lies within `rel` (relative) of the threshold: the tests leave them out of the count
    comparison."""
    near = None
    for e in err.values():
        m = np.abs(e - np.float32(thr)) <= rel * thr
        near = m if near is None else near | m
    return near


def list_lengths(counts, min_spp, max_spp):
    """{samples reached by the round: length of that round's tile list} for the rounds after round 1 (which renders every tile),
    read from the final counts: a round that brings the active tiles to n ran over every tile whose count is at least n."""
    seq = sequence(min_spp, max_spp)
    return {n: int((counts >= n).sum()) for n in seq[2:]}


def per_pixel(counts, w, h):
    """Each pixel's count, (h, w), from the (tiles_y, tiles_x) tile counts."""
    return np.repeat(np.repeat(np.asarray(counts), TILE, axis=0), TILE, axis=1)[:h, :w]


def samples(counts, w, h):
    """hrt_stats.samples of an adaptive frame: the sum over in-image pixels of their tile's count."""
    return int(per_pixel(counts, w, h).astype(np.uint64).sum())


def same_bits(a, b):
    """The same shape and the same bits, NaN payloads and signed zeros included."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def tiles_differing(frame, counts, refs):
    """The tiles of `frame` whose bits differ from the same tile of refs[count] (uniform frames keyed by count): a list of
    (tile_y, tile_x, count)."""
    h, w = frame.shape[:2]
    f = np.ascontiguousarray(frame, dtype=np.float32).view(np.uint32)
    pp = per_pixel(counts, w, h)
    bad = np.zeros((h, w), dtype=bool)
    for c in np.unique(counts):
        m = pp == c
        bad[m] = (f[m] != np.ascontiguousarray(refs[int(c)], dtype=np.float32).view(np.uint32)[m]).any(axis=-1)
    ty, tx = tiles_shape(w, h)
    pad = np.zeros((ty * TILE, tx * TILE), dtype=bool)
    pad[:h, :w] = bad
    return [(int(y), int(x), int(counts[y, x])) for y, x in zip(*np.nonzero(pad.reshape(ty, TILE, tx, TILE).any(axis=(1, 3))))]
