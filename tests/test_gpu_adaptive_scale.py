"""Adaptive sampling at frame scale and at the edges of its parameters (include/hrt.h hrt_render_adaptive*).

tests/test_gpu_adaptive.py checks the contract on one 120x67 frame (135 tiles).  Here: 1080p frames (32 400 tiles: the list
compaction walks its flags in 32 passes of 1024, the trace kernels get lists of thousands of scattered tiles, and on a scene
without meshes or lights the default kernel form changes between rounds), first lists of exactly 1 / 1023 / 1024 / 1025 / 2049
tiles, a 4K frame over 8 ranks, odd and long count sequences (rounds of 2 and of 2048 samples), ragged frames, ranks without
tiles, scratch reuse across calls on one scene, and tiles whose every pixel is non-finite.  Every tile is compared bit for bit
with a uniform hrt_render at its count, every count with the rule recomputed in numpy (tests/adaptive_ref.py)."""
import numpy as np
import pytest

from adaptive_ref import (errors_from, expected_counts, list_lengths, near_threshold, samples, same_bits, sequence, tile_err,
                          tiles_differing, tiles_shape)
from scene_util import overflow_scene

pytestmark = pytest.mark.gpu

SEED = 11
W, H = 1920, 1080  # 240 x 135 = 32 400 tiles
LANE_LIST_MAX = 5120  # launch_trace: a list of at most this many tiles (>= 8 samples) runs the streaming kernel on every scene


class Frames:
    """One scene at one frame size: its DeviceScene, camera and the uniform renders made so far, by (count, flags)."""

    def __init__(self, gpu, name, w, h, desc=None, seed=SEED):
        self.gpu, self.name, self.w, self.h, self.seed = gpu, name, w, h, seed
        if desc is None:
            self.host = gpu.HostScene().setup(name, w / h, 1)
            desc = self.host.flatten()
        self.desc = desc
        self.dev = gpu.DeviceScene(desc)
        self.cam = gpu.default_camera(w / h)
        self._frames = {}

    def at(self, n, flags=0):
        key = (int(n), flags)
        if key not in self._frames:
            self._frames[key] = self.dev.render(self.cam, self.w, self.h, int(n), seed=self.seed, flags=flags)[0]
        return self._frames[key]

    def errors(self, mn, mx):
        return errors_from({n: self.at(n) for n in sequence(mn, mx)}, mn, mx)

    def adaptive(self, mn, mx, thr, flags=0, stats=None):
        return self.dev.render_adaptive(self.cam, self.w, self.h, mn, mx, float(thr), seed=self.seed, flags=flags, stats=stats)

    def assert_tiles(self, frame, counts, flags=0, what=""):
        assert frame.shape == (self.h, self.w, 3) and counts.shape == tiles_shape(self.w, self.h)
        bad = tiles_differing(frame, counts, {int(c): self.at(c, flags) for c in np.unique(counts)})
        assert not bad, f"{self.name} {self.w}x{self.h} {what}: {len(bad)} tiles differ from hrt_render at their count, " \
                        f"first (tile y, tile x, count): {bad[:5]}"


_frames = {}


@pytest.fixture(scope="module", autouse=True)
def _release_frames():
    yield
    _frames.clear()


def frames(gpu, name, w, h, seed=SEED):
    """The shared Frames of (scene, size, seed): the uniform renders are made once per module."""
    key = (name, w, h, seed)
    if key not in _frames:
        _frames[key] = Frames(gpu, name, w, h, seed=seed)
    return _frames[key]


def check_counts(counts, err, mn, mx, thr, both=True):
    """counts == the rule's, leaving out tiles within 1e-5 of the threshold at a judged count; that band must stay under 0.5 %
    of the tiles, and (with `both`) the tiles checked must include one that stopped before max_spp and one that went past min_spp."""
    exp = expected_counts(err, mn, mx, thr)
    near = near_threshold(err, thr)
    assert near.mean() < 0.005, f"threshold {thr}: {int(near.sum())} of {near.size} tiles lie within 1e-5 of it"
    diff = np.argwhere((counts != exp) & ~near)
    assert len(diff) == 0, f"threshold {thr}: {len(diff)} tiles differ from the rule, first " \
                           f"{[(tuple(t), int(counts[tuple(t)]), int(exp[tuple(t)])) for t in diff[:5]]}"
    if both:
        checked = exp[~near]
        assert (checked < mx).any() and (checked > mn).any(), f"threshold {thr}: counts {np.unique(checked)} test only one outcome"
    return exp


def persist(err, mn, mx):
    """Per tile, the smallest error over the counts at which it must be judged active to reach max_spp."""
    return np.minimum.reduce([err[n] for n in sequence(mn, mx)[1:-1]])


def quiet_threshold(err, target):
    """A float32 threshold near `target` that the tile errors keep clear of: the midpoint of the widest gap (relative) between
    neighbouring error values, over all judged counts, among the values closest to `target` in rank.  A quantile itself can land
    in a cluster of nearly equal errors (a tile's largest error often comes from one rare bright sample)."""
    v = np.unique(np.concatenate([e.ravel() for e in err.values()])).astype(np.float64)
    v = v[v > 0]
    i = int(np.clip(np.searchsorted(v, float(target)), 1, len(v) - 1))
    r = max(2, len(v) // 200)
    lo, hi = max(0, i - r), min(len(v) - 1, i + r)
    a, b = v[lo:hi], v[lo + 1:hi + 1]
    j = int(np.argmax((b - a) / b))
    return float(np.float32((a[j] + b[j]) / 2))


def separating(hi, lo):
    """The float32 threshold between two neighbouring tile errors lo < hi: the one that keeps hi and drops lo."""
    hi, lo = np.float32(hi), np.float32(lo)
    thr = np.float32((float(hi) + float(lo)) / 2)
    return float(thr if lo < thr <= hi else hi)


@pytest.mark.parametrize("name,mn,mx", [("cornell_mesh", 16, 256), ("cornell_box", 16, 128)])
def test_1080p_at_the_quartile_thresholds(gpu, name, mn, mx):
    """DESIGN's setup: thresholds at the quartiles of the tile error at min_spp.  On cornell_box (no meshes, no lights) the
    default form is the lane-per-pixel kernel for the long lists of the first rounds, the streaming kernel for the short later
    ones: assert that this switch happens."""
    fr = frames(gpu, name, W, H)
    err = fr.errors(mn, mx)
    thrs = [quiet_threshold(err, q) for q in np.quantile(err[mn], [0.25, 0.5, 0.75])]
    switched = []
    for i, thr in enumerate(thrs):
        st = gpu.Stats()
        frame, counts = fr.adaptive(mn, mx, thr, stats=st)
        check_counts(counts, err, mn, mx, thr)
        fr.assert_tiles(frame, counts, 0, f"threshold {thr}")
        assert st.samples == samples(counts, W, H)
        lens = [n for n in list_lengths(counts, mn, mx).values()]
        switched.append(any(a > LANE_LIST_MAX and 0 < b <= LANE_LIST_MAX for j, a in enumerate(lens) for b in lens[j + 1:]))
        if i == 1:
            gframe, gcounts = fr.adaptive(mn, mx, thr, flags=gpu.FLAG_GAMMA)
            assert np.array_equal(gcounts, counts)
            fr.assert_tiles(gframe, gcounts, gpu.FLAG_GAMMA, f"threshold {thr}, gamma")
    if name == "cornell_box":
        assert any(switched), "no threshold gave a list over 5120 tiles followed by one of at most 5120"


def test_1080p_first_lists_around_the_compaction_chunk(gpu):
    """Thresholds between neighbouring tile errors at min_spp: the list after round 1 is exactly k tiles long, so the compaction
    of the following round walks k flags (over a list) and the one of round 1 carries partial totals across its 32 chunks.  The
    threshold sits within an ulp or two of some tiles here, so every count must be the rule's exactly: the judge computes the
    errors in the fp32 arithmetic include/hrt.h states, bit for bit with tests/adaptive_ref.py."""
    mn, mx = 16, 64
    ks = (1, 1023, 1024, 1025, 2049)
    for seed in range(SEED, SEED + 8):  # the first seed whose k-th and (k+1)-th largest errors differ for every k
        fr = frames(gpu, "cornell_mesh", W, H, seed)
        ranked = np.sort(fr.errors(mn, mn)[mn].ravel())[::-1]
        if all(ranked[k - 1] > ranked[k] for k in ks):
            break
    else:
        pytest.fail("eight seeds, each with tied tile errors at one of the list lengths")
    err = fr.errors(mn, mx)
    for k in ks:
        thr = separating(ranked[k - 1], ranked[k])
        frame, counts = fr.adaptive(mn, mx, thr)
        assert int((counts > mn).sum()) == k, f"seed {seed}: first list of {int((counts > mn).sum())} tiles, want {k}"
        exp = expected_counts(err, mn, mx, thr)
        diff = np.argwhere(counts != exp)
        assert len(diff) == 0, f"seed {seed}, first list {k}: {len(diff)} tiles differ from the rule, first " \
                               f"{[(tuple(t), int(counts[tuple(t)]), int(exp[tuple(t)])) for t in diff[:5]]}"
        fr.assert_tiles(frame, counts, 0, f"seed {seed}, first list of {k}")


def test_1080p_extreme_thresholds(gpu):
    """Threshold 0: every round's list is the whole frame (32 compaction passes, every flag kept); +inf: one round."""
    fr = frames(gpu, "cornell_mesh", W, H)
    mn, mx = 16, 64
    for thr, want in ((0.0, mx), (float("inf"), mn)):
        st = gpu.Stats()
        frame, counts = fr.adaptive(mn, mx, thr, stats=st)
        assert (counts == want).all(), f"threshold {thr}: counts {np.unique(counts)}"
        assert same_bits(frame, fr.at(want)), f"threshold {thr}: not the uniform render at {want}"
        assert st.samples == W * H * want


def test_1080p_every_kernel_form_gives_the_same_frame_and_counts(gpu):
    fr = frames(gpu, "cornell_mesh", W, H)
    mn, mx = 16, 64
    thr = float(np.float32(np.median(fr.errors(mn, mx)[mn])))
    base, base_counts = fr.adaptive(mn, mx, thr, flags=gpu.FLAG_GAMMA)
    assert len(np.unique(base_counts)) == 3
    for f in (gpu.FLAG_WAVE_KERNEL, gpu.FLAG_DUAL_KERNEL, gpu.FLAG_STREAM_KERNEL, gpu.FLAG_EXACT_ONLY,
              gpu.FLAG_EXACT_ONLY | gpu.FLAG_WAVE_KERNEL, gpu.FLAG_EXACT_ONLY | gpu.FLAG_STREAM_KERNEL):
        frame, counts = fr.adaptive(mn, mx, thr, flags=gpu.FLAG_GAMMA | f)
        assert np.array_equal(counts, base_counts), f"flags {f}: other counts"
        assert same_bits(frame, base), f"flags {f}: other pixels"


def test_scratch_reuse_on_one_scene(gpu):
    """Calls of different sizes and kinds, one after the other on one DeviceScene, each equal to the same call on a fresh scene:
    the adaptive scratch (tile lists, flags and counts at offsets set by the call's tile count, compact sums) and the shared
    tile buffer and streaming scratch are resized and reused."""
    import torch
    base = frames(gpu, "cornell_mesh", W, H)
    mn, mx = 16, 64
    thr = float(np.float32(np.median(base.errors(mn, mx)[mn])))
    sw, sh = 120, 67
    small_cam = gpu.default_camera(sw / sh)
    world = 3
    per = gpu.tiles_owned(W, H, 0, world)

    def tiles_call(dev, stream):
        out = torch.full((world, per, 64, 3), -1.0, dtype=torch.float32, device="cuda")
        spp = torch.full((world, per), -1, dtype=torch.int32, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for r in range(world):
                dev.render_adaptive_tiles(base.cam, W, H, mn, mx, thr, SEED, gpu.FLAG_GAMMA, r, world, out[r].data_ptr(),
                                          spp[r].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return out.cpu().numpy(), spp.cpu().numpy()

    calls = [("adaptive 1080p", lambda d, s: d.render_adaptive(base.cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA)),
             ("adaptive 120x67", lambda d, s: d.render_adaptive(small_cam, sw, sh, 4, 32, thr, seed=SEED)),
             ("render 1080p", lambda d, s: (d.render(base.cam, W, H, 16, seed=SEED)[0],)),
             ("adaptive tiles, world 3, side stream", tiles_call),
             ("adaptive 1080p again", lambda d, s: d.render_adaptive(base.cam, W, H, mn, mx, thr, seed=SEED, flags=gpu.FLAG_GAMMA))]
    stream = torch.cuda.Stream()
    dev = gpu.DeviceScene(base.desc)
    try:
        got = [call(dev, stream) for _, call in calls]
    finally:
        dev.close()
    want = {}
    for i, (label, call) in enumerate(calls):
        key = "adaptive 1080p" if label == "adaptive 1080p again" else label
        if key not in want:
            fresh = gpu.DeviceScene(base.desc)
            try:
                want[key] = call(fresh, stream)
            finally:
                fresh.close()
        for a, b in zip(got[i], want[key]):
            if a.dtype == np.float32:
                assert same_bits(a, b), f"{label}: other pixels than on a fresh scene"
            else:
                assert np.array_equal(a, b), f"{label}: other counts than on a fresh scene"
    assert len(np.unique(got[0][1])) > 1 and np.array_equal(got[0][1], got[4][1])


# ------------------------------------------------------------------------------------------------------------ 4K, 8 ranks
def test_4k_over_8_ranks_is_the_whole_frame_call(gpu):
    """3840x2160 = 129 600 tiles, 16 200 per rank: each rank's compaction runs 16 passes, and its rounds of 2, 4 and 8 samples
    pack 16 list items into one streaming work unit."""
    import torch
    w, h, world, mn, mx = 3840, 2160, 8, 4, 16
    fr = Frames(gpu, "backrooms_pool", w, h)
    e = tile_err(fr.dev.render(fr.cam, w, h, 2, seed=SEED)[0], fr.dev.render(fr.cam, w, h, 4, seed=SEED)[0])
    thr = quiet_threshold({mn: e}, np.median(e))
    ref, ref_counts = fr.adaptive(mn, mx, thr, flags=gpu.FLAG_GAMMA)
    assert set(np.unique(ref_counts).tolist()) == {4, 8, 16}
    near = np.abs(e - np.float32(thr)) <= 1e-5 * thr
    assert near.mean() < 0.005
    assert np.array_equal((ref_counts > mn)[~near], (e >= np.float32(thr))[~near])
    per = gpu.tiles_owned(w, h, 0, world)
    assert per == 16200 and per * world == gpu.tiles_total(w, h)
    gathered = torch.zeros((world, per, 64, 3), dtype=torch.float32, device="cuda")
    spp = torch.zeros((world, per), dtype=torch.int32, device="cuda")
    for r in range(world):
        fr.dev.render_adaptive_tiles(fr.cam, w, h, mn, mx, thr, SEED, gpu.FLAG_GAMMA, r, world, gathered[r].data_ptr(),
                                     spp[r].data_ptr(), 0)
    frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    gpu.assemble_frame(gathered.data_ptr(), per, w, h, world, frame.data_ptr(), 0)
    torch.cuda.synchronize()
    assert same_bits(frame.cpu().numpy(), ref)
    counts = spp.cpu().numpy().T.reshape(ref_counts.shape)  # tile t = slot * world + rank
    assert np.array_equal(counts.astype(np.uint32), ref_counts)
    fr.dev.close()


# ------------------------------------------------------------------------------------------------ odd and long sequences
@pytest.mark.parametrize("name,w,h,mn,mx", [("cornell_mesh", 120, 67, 6, 50),       # 3, 6, 12, 24, 48, 50: the last round adds 2
                                            ("cornell_mesh", 120, 67, 10, 40),      # round 0 and round 1 add 5 each
                                            ("random_spheres", 64, 48, 2, 1024)])   # 11 counts, rounds up to 512 samples
def test_odd_and_long_count_sequences(gpu, name, w, h, mn, mx):
    fr = frames(gpu, name, w, h)
    err = fr.errors(mn, mx)
    thr = quiet_threshold(err, np.median(persist(err, mn, mx)))  # about half the tiles run to max_spp
    frame, counts = fr.adaptive(mn, mx, thr, flags=gpu.FLAG_GAMMA)
    assert set(np.unique(counts).tolist()) <= set(sequence(mn, mx)[1:])
    exp = check_counts(counts, err, mn, mx, thr)
    assert (exp == mx).any(), f"no tile reached {mx}: the last round did not run"
    fr.assert_tiles(frame, counts, gpu.FLAG_GAMMA, f"({mn}, {mx}) at {thr}")


def test_equal_odd_bounds_are_a_uniform_render(gpu):
    """(10, 10): two rounds of 5 samples, one judgement that cannot continue."""
    fr = frames(gpu, "cornell_mesh", 120, 67)
    for thr in (0.0, 0.5, float("inf")):
        frame, counts = fr.adaptive(10, 10, thr)
        assert (counts == 10).all()
        assert same_bits(frame, fr.at(10)), f"threshold {thr}"


def test_rounds_of_2048_samples_fold_twice(gpu):
    """(2, 4096) at threshold 0 on 24x16 (6 tiles): the last round adds 2048 samples to a list, which the streaming kernel
    traces as two folds of 1024 and the lane-per-pixel kernel in one walk."""
    fr = frames(gpu, "cornell_mesh", 24, 16)
    want = fr.at(4096)
    for f in (gpu.FLAG_STREAM_KERNEL, gpu.FLAG_WAVE_KERNEL):
        st = gpu.Stats()
        frame, counts = fr.adaptive(2, 4096, 0.0, flags=f, stats=st)
        assert (counts == 4096).all(), f"flags {f}: counts {np.unique(counts)}"
        assert same_bits(frame, want), f"flags {f}: not the uniform render at 4096"
        assert st.samples == 24 * 16 * 4096


@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (37, 1), (9, 17)])
def test_ragged_frames(gpu, w, h):
    fr = frames(gpu, "cornell_mesh", w, h)
    mn, mx = 4, 32
    err = fr.errors(mn, mx)
    for thr in (0.0, float(np.float32(np.median(err[mn]))), float("inf")):
        frame, counts = fr.adaptive(mn, mx, thr)
        assert counts.shape == tiles_shape(w, h)
        if thr == 0.0:
            assert (counts == mx).all()
        elif thr == float("inf"):
            assert (counts == mn).all()
        else:
            exp = expected_counts(err, mn, mx, thr)
            near = near_threshold(err, thr)
            assert np.array_equal(counts[~near], exp[~near])
        fr.assert_tiles(frame, counts, 0, f"threshold {thr}")


@pytest.mark.parametrize("w,h", [(16, 8), (1, 1)])
def test_ranks_without_tiles_return_ok_and_touch_nothing(gpu, w, h):
    """World 3 on frames of 2 and 1 tiles: the ranks that own no tile return HRT_OK and leave their buffers as they were; the
    others assemble to the whole-frame call."""
    import torch
    fr = frames(gpu, "cornell_mesh", w, h)
    world, mn, mx = 3, 2, 16
    thr = 0.5
    ref, ref_counts = fr.adaptive(mn, mx, thr, flags=gpu.FLAG_GAMMA)
    tiles = gpu.tiles_total(w, h)
    assert tiles < world
    gathered = torch.full((world, 1, 64, 3), 7.25, dtype=torch.float32, device="cuda")
    spp = torch.full((world, 1), 123456, dtype=torch.int32, device="cuda")
    for r in range(world):
        fr.dev.render_adaptive_tiles(fr.cam, w, h, mn, mx, thr, SEED, gpu.FLAG_GAMMA, r, world, gathered[r].data_ptr(),
                                     spp[r].data_ptr(), 0)
    frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    gpu.assemble_frame(gathered.data_ptr(), 1, w, h, world, frame.data_ptr(), 0)
    torch.cuda.synchronize()
    assert same_bits(frame.cpu().numpy(), ref)
    g, s = gathered.cpu().numpy(), spp.cpu().numpy()
    assert np.array_equal(s[:tiles, 0].astype(np.uint32), ref_counts.ravel())
    assert (g[tiles:] == np.float32(7.25)).all() and (s[tiles:] == 123456).all()


# ---------------------------------------------------------------------------------------------------- non-finite pixels
NF_W, NF_H, NF_MIN, NF_MAX = 256, 144, 4, 16  # the lamp of the emission-overflow box covers whole tiles at this size


def nonfinite_frames(gpu):
    key = ("overflow_emission_lit", NF_W, NF_H)
    if key not in _frames:
        host = overflow_scene(gpu, "emission", True)
        fr = Frames(gpu, "emission overflow", NF_W, NF_H, host.flatten())
        fr.host = host
        _frames[key] = fr
    return _frames[key]


def nonfinite_tiles(frame):
    """(every in-image pixel non-finite, some pixel non-finite) per tile."""
    h, w = frame.shape[:2]
    ty, tx = tiles_shape(w, h)
    bad = np.ones((ty * 8, tx * 8), dtype=bool)  # outside the image: no pixel, nothing to spoil "every"
    bad[:h, :w] = ~np.isfinite(frame).all(axis=-1)
    some = np.zeros_like(bad)
    some[:h, :w] = bad[:h, :w]
    return bad.reshape(ty, 8, tx, 8).all(axis=(1, 3)), some.reshape(ty, 8, tx, 8).any(axis=(1, 3))


def test_a_tile_of_only_nonfinite_pixels_reaches_max_at_threshold_zero(gpu):
    """include/hrt.h: a pixel whose error is NaN counts as 0, so threshold 0 gives every tile max_spp, even one whose every
    pixel is inf or NaN."""
    fr = nonfinite_frames(gpu)
    full, _ = nonfinite_tiles(fr.at(NF_MIN))
    assert full.any(), "no tile of the frame is entirely non-finite at min_spp: the test would mean nothing"
    for f in (0, gpu.FLAG_STREAM_KERNEL, gpu.FLAG_WAVE_KERNEL):
        frame, counts = fr.adaptive(NF_MIN, NF_MAX, 0.0, flags=f)
        assert (counts == NF_MAX).all(), f"flags {f}: counts {np.unique(counts)}; entirely non-finite tiles at " \
                                         f"{np.unique(counts[full])}"
        assert same_bits(frame, fr.at(NF_MAX)), f"flags {f}: not the uniform render at {NF_MAX}"


def test_nonfinite_pixels_follow_the_rule(gpu):
    fr = nonfinite_frames(gpu)
    err = fr.errors(NF_MIN, NF_MAX)
    full, some = nonfinite_tiles(fr.at(NF_MIN))
    mixed = some & ~full
    assert full.any() and mixed.any(), "the frame needs tiles of only non-finite pixels and tiles of both kinds"
    assert (err[NF_MIN][full] == 0).all() and (err[NF_MIN][mixed] > 0).any()
    frame, counts = fr.adaptive(NF_MIN, NF_MAX, float("inf"))
    assert (counts == NF_MIN).all()
    assert same_bits(frame, fr.at(NF_MIN))
    positive = err[NF_MIN][err[NF_MIN] > 0]
    thr = float(np.float32(np.median(positive)))
    frame, counts = fr.adaptive(NF_MIN, NF_MAX, thr)
    check_counts(counts, err, NF_MIN, NF_MAX, thr)
    assert (counts[full] == NF_MIN).all()
    fr.assert_tiles(frame, counts, 0, f"threshold {thr}")
