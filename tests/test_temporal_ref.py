"""Properties of the numpy statement of temporal accumulation (tests/temporal_ref.py, include/hrt.h hrt_temporal_accumulate) on
synthetic 13 x 9 frames: the first frame, the running mean under a still camera, saturation, alpha_min = 1, non-finite pixels in
either frame, a sideways pan over a plane and a camera turned round."""
from types import SimpleNamespace

import numpy as np

import denoise_ref as dr
import temporal_ref as tr

F32 = np.float32
H, W = 9, 13
OFF = dict(depth_tol=np.inf, normal_tol=np.inf, albedo_tol=np.inf)
LONG = dict(alpha_min=1e-6, max_history=1e6)


def camera(eye=(0, 0, 0), right=(1, 0, 0), up=(0, 1, 0), forward=(0, 0, -1), fovy_deg=90.0, aspect=1.0):
    return SimpleNamespace(eye=list(eye), right=list(right), up=list(up), forward=list(forward), fovy_deg=fovy_deg, aspect=aspect, znear=0.1, zfar=100.0)


def frames(n, seed=0):
    """n colour frames with their half frames over one set of features (a still scene)."""
    rng = np.random.default_rng(seed)
    f = dr.synthetic_features(H, W, seed=seed)
    c = [(rng.uniform(0, 1, (H, W, 3)).astype(F32) + f[..., 6:9] / F32(6)).astype(F32) for _ in range(n)]
    ch = [(v + rng.normal(0, 0.1, (H, W, 3)).astype(F32)).astype(F32) for v in c]
    return c, ch, f


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def run(c, ch, f, cam, n, **params):
    """n frames under one camera: the list of (out, out_half, history)."""
    prev, outs = None, []
    for k in range(n):
        o, oh, hist = tr.temporal_accumulate(c[k], ch[k], f, prev, cam, cam, None, **params)
        prev = dict(color=o, half=oh, feat=f, history=hist)
        outs.append((o, oh, hist))
    return outs


def test_first_frame_passes_through():
    c, ch, f = frames(1)
    o, oh, hist = tr.temporal_accumulate(c[0], ch[0], f)
    assert np.array_equal(bits(o), bits(c[0])) and np.array_equal(bits(oh), bits(ch[0])) and (hist == 1).all()
    o, oh, hist = tr.temporal_accumulate(c[0], None, f)
    assert np.array_equal(bits(o), bits(c[0])) and oh is None and (hist == 1).all()


def test_still_camera_gives_the_running_mean_and_history_counts_the_frames():
    n = 6
    c, ch, f = frames(n, seed=1)
    outs = run(c, ch, f, camera(), n, **LONG, **OFF)
    hit = f[..., 10] > 0
    assert hit.any() and (~hit).any()
    # the same recurrence written out per channel: acc <- remodulate(xacc + (1/k) (x_k - xacc)), xacc = demodulate(acc)
    d = np.where(f[..., 0:3] > 0, f[..., 0:3], F32(1)).astype(F32)
    e6 = (f[..., 6:9] / F32(6)).astype(F32)
    for frames_, which in ((c, 0), (ch, 1)):
        acc = frames_[0].copy()
        for k in range(2, n + 1):
            xacc = ((acc - e6) / d).astype(F32)
            xk = ((frames_[k - 1] - e6) / d).astype(F32)
            alpha = F32(1) / F32(k)
            y = (xacc + (alpha * (xk - xacc).astype(F32)).astype(F32)).astype(F32)
            acc = np.where(hit[..., None], ((d * y).astype(F32) + e6).astype(F32), frames_[k - 1])
            assert np.array_equal(outs[k - 1][which], acc), f"frame {k}"
    for k in range(1, n + 1):
        assert (outs[k - 1][2][hit] == k).all() and (outs[k - 1][2][~hit] == 1).all()
    # and it is a mean: close to the plain average of the frames where the surface is hit
    mean = np.mean(np.stack(c).astype(np.float64), axis=0)
    assert np.abs(outs[-1][0] - mean)[hit].max() < 1e-5


def test_history_saturates_at_max_history():
    c, ch, f = frames(7, seed=2)
    outs = run(c, ch, f, camera(), 7, alpha_min=1e-6, max_history=4.0, **OFF)
    hit = f[..., 10] > 0
    assert [float(o[2][hit].max()) for o in outs] == [1, 2, 3, 4, 4, 4, 4]
    assert all((o[2][hit] == o[2][hit].max()).all() for o in outs)


def test_alpha_min_one_ignores_history():
    c, ch, f = frames(3, seed=3)
    outs = run(c, ch, f, camera(), 3, alpha_min=1.0, max_history=64.0, **OFF)
    # y = xhist + 1 * (x - xhist): x up to two roundings of size 2^-24 max(|x|, |xhist|, |x - xhist|) <= 2^-24 * 20 here (c < 2, d >= 0.1)
    assert np.abs(outs[2][0] - c[2]).max() <= 1e-5 and np.abs(outs[2][1] - ch[2]).max() <= 1e-5
    hit = f[..., 10] > 0
    assert (outs[2][2][hit] == 3).all()


def test_non_finite_pixels_restart_in_the_current_frame_and_are_skipped_in_the_previous_one():
    c, ch, f = frames(2, seed=4)
    cam = camera()
    first = tr.temporal_accumulate(c[0], ch[0], f)
    prev = dict(color=first[0], half=first[1], feat=f, history=first[2])
    hit = f[..., 10] > 0
    base = tr.temporal_accumulate(c[1], ch[1], f, prev, cam, cam, None, **LONG, **OFF)
    assert (base[2][hit] == 2).all()
    # current frame: +inf in the colour, NaN in the half colour
    cur, curh = c[1].copy(), ch[1].copy()
    cur[2, 3, 1] = np.inf
    curh[4, 5, 0] = np.nan
    o, oh, hist = tr.temporal_accumulate(cur, curh, f, prev, cam, cam, None, **LONG, **OFF)
    for y, x in ((2, 3), (4, 5)):
        assert hit[y, x] and hist[y, x] == 1
        assert dr_same(o[y, x], cur[y, x]) and dr_same(oh[y, x], curh[y, x])
    rest = hit.copy(); rest[2, 3] = rest[4, 5] = False
    assert np.array_equal(o[rest], base[0][rest]) and (hist[rest] == 2).all()
    # previous frame, still camera: the one tap with weight is skipped, nothing is left, the pixel restarts
    pc, pch = first[0].copy(), first[1].copy()
    pc[2, 3, 1] = np.inf
    pch[4, 5, 0] = np.nan
    o, oh, hist = tr.temporal_accumulate(c[1], ch[1], f, dict(color=pc, half=pch, feat=f, history=first[2]), cam, cam, None, **LONG, **OFF)
    for y, x in ((2, 3), (4, 5)):
        assert hist[y, x] == 1 and np.array_equal(o[y, x], c[1][y, x]) and np.array_equal(oh[y, x], ch[1][y, x])
    assert np.array_equal(o[rest], base[0][rest]) and (hist[rest] == 2).all()


def dr_same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# A plane facing the camera at distance D = W / 2 with fovy 90 and aspect 1 (kx = ky = 1): a pixel is then one world unit wide, and
# the point seen through the centre of column x is P = (x - (W - 1) / 2, ., -D) -- all exact in fp32.  The rays handed to the
# statement are not unit length (d = P, z = 1), so the depth test is off; the frame does not depend on y, because a pixel is
# W / H units high and the rows do not project exactly.
D = W / 2.0


def plane(seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([xs - (W - 1) / 2.0, ((H - 1) / 2.0 - ys) * (W / H), np.full((H, W), -D)], -1).astype(F32)
    o = np.zeros((H, W, 3), F32)
    f = np.zeros((H, W, 12), F32)
    f[..., 0:3] = -1          # d = 1, e = 0: x = c
    f[..., 5] = 1
    f[..., 9] = 1
    f[..., 10] = 1
    col = lambda: np.repeat(rng.uniform(0.25, 1, (1, W, 3)).astype(F32), H, axis=0)
    return (o, d), f, col


def test_a_pan_by_whole_pixels_takes_the_previous_pixel_k_columns_over_and_restarts_what_left():
    rays, f, col = plane(5)
    prev_c, prev_h, cur, curh = col(), col(), col(), col()
    prev = dict(color=prev_c, half=prev_h, feat=f, history=np.full((H, W), 3, F32))
    for k in (1, 3, -2):
        # the current camera stands at the origin; the previous one stood k pixels to its left, so column x shows what x + k showed
        o, oh, hist = tr.temporal_accumulate(cur, curh, f, prev, camera(), camera(eye=(-float(k), 0, 0)), rays, **LONG, **OFF)
        px, py, zexp, zc = tr.project(rays, f[..., 9], camera(eye=(-float(k), 0, 0)), W, H)
        xs = np.arange(W)
        assert np.abs(px - (xs + k)[None, :]).max() < 1e-5 and (zc == F32(D)).all()
        for x in range(W):
            src = x + k
            blend = lambda a, b: b[:, src] + 0.25 * (a[:, x] - b[:, src])  # history 3 -> 4, alpha 1/4
            if 0 <= src < W:
                # px is src to within 1e-5, so the neighbouring column has at most that weight: values are below 1
                assert np.abs(o[:, x] - blend(cur, prev_c)).max() < 1e-4 and np.abs(oh[:, x] - blend(curh, prev_h)).max() < 1e-4, (k, x)
                assert np.abs(hist[:, x] - 4).max() < 1e-4
            elif src <= -2 or src >= W + 1:
                assert np.array_equal(o[:, x], cur[:, x]) and np.array_equal(oh[:, x], curh[:, x]) and (hist[:, x] == 1).all(), (k, x)
            else:
                # exactly one pixel outside: px is -1 or W to rounding, so the pixel restarts, or the edge column has a weight
                # of some 1e-7 and, being the only tap, is renormalised to 1
                edge = 0 if src < 0 else W - 1
                restarted = np.array_equal(o[:, x], cur[:, x]) and (hist[:, x] == 1).all()
                took_edge = np.abs(o[:, x] - (prev_c[:, edge] + 0.25 * (cur[:, x] - prev_c[:, edge]))).max() < 1e-4
                assert restarted or took_edge, (k, x)


def test_a_pan_by_half_a_pixel_blends_two_columns_and_renormalises_when_one_is_not_usable():
    rays, f, col = plane(6)
    prev_c, prev_h, cur, curh = col(), col(), col(), col()
    history = np.ones((H, W), F32)
    prev_cam = camera(eye=(0.5, 0, 0))   # px = x - 0.5: columns x - 1 and x, half each
    o, _, hist = tr.temporal_accumulate(cur, curh, f, dict(color=prev_c, half=prev_h, feat=f, history=history), camera(), prev_cam, rays, **LONG, **OFF)
    mix = 0.5 * (prev_c[:, :-1] + prev_c[:, 1:])
    assert np.abs(o[:, 1:] - (mix + 0.5 * (cur[:, 1:] - mix))).max() < 1e-5 and (np.abs(hist[:, 1:] - 2) < 1e-5).all()
    assert np.abs(o[:, 0] - (prev_c[:, 0] + 0.5 * (cur[:, 0] - prev_c[:, 0]))).max() < 1e-5   # column -1 is outside: column 0 alone
    for spoil in ("nan", "inf", "history", "coverage", "depth"):
        pc, pf, ph = prev_c.copy(), f.copy(), history.copy()
        if spoil == "nan": pc[:, 4, 2] = np.nan
        if spoil == "inf": pc[:, 4, 0] = np.inf
        if spoil == "history": ph[:, 4] = 0
        if spoil == "coverage": pf[:, 4, 10] = 0
        if spoil == "depth": pf[:, 4, 9] = np.nan
        o2, _, hist2 = tr.temporal_accumulate(cur, curh, f, dict(color=pc, half=prev_h, feat=pf, history=ph), camera(), prev_cam, rays, **LONG, **OFF)
        # columns 4 and 5 are left with one tap each, columns 3 and 5 of the previous frame
        for x, other in ((4, 3), (5, 5)):
            assert np.abs(o2[:, x] - (prev_c[:, other] + 0.5 * (cur[:, x] - prev_c[:, other]))).max() < 1e-5, (spoil, x)
        keep = np.ones(W, bool); keep[[4, 5]] = False
        assert np.array_equal(o2[:, keep], o[:, keep]) and np.isfinite(o2).all() and np.array_equal(hist2, hist), spoil
    # a checkerboard of history 0: the rule never reads colour through it
    ys, xs = np.mgrid[0:H, 0:W]
    board = ((ys + xs) % 2).astype(F32)
    o3, _, hist3 = tr.temporal_accumulate(cur, curh, f, dict(color=prev_c, half=prev_h, feat=f, history=board), camera(), prev_cam, rays, **LONG, **OFF)
    assert np.isfinite(o3).all() and (np.abs(hist3[:, 1:] - 2) < 1e-5).all()   # one of the two columns is usable everywhere
    assert np.array_equal(hist3[:, 0], 1 + board[:, 0])                         # column 0 has that one tap only: none where it is 0


def test_tolerances_reject_taps_and_plus_infinity_switches_a_test_off():
    rays, f, col = plane(7)
    prev_c, prev_h, cur, curh = col(), col(), col(), col()
    pf = f.copy()
    pf[:, 6, 3:6] = (1, 0, 0)     # another normal: |dn|^2 = 2
    pf[:, 8, 0:3] = -0.5          # another albedo: |da|^2 = 0.75
    pf[:, 10, 9] = 1.5            # another depth: |1 - 1.5| > 0.1 * 1
    prev = dict(color=prev_c, half=prev_h, feat=pf, history=np.ones((H, W), F32))
    cam = camera()
    tight = tr.temporal_accumulate(cur, curh, f, prev, cam, cam, None, alpha_min=1e-6, max_history=64.0, depth_tol=0.1, normal_tol=0.5, albedo_tol=0.5)
    assert [x for x in range(W) if (tight[2][:, x] == 1).all()] == [6, 8, 10] and (np.delete(tight[2], [6, 8, 10], axis=1) == 2).all()
    for off, col_ in (("normal_tol", 6), ("albedo_tol", 8), ("depth_tol", 10)):
        kw = dict(depth_tol=0.1, normal_tol=0.5, albedo_tol=0.5)
        kw[off] = np.inf
        hist = tr.temporal_accumulate(cur, curh, f, prev, cam, cam, None, alpha_min=1e-6, max_history=64.0, **kw)[2]
        assert (hist[:, col_] == 2).all() and sorted(x for x in range(W) if (hist[:, x] == 1).all()) == sorted({6, 8, 10} - {col_})


def test_a_camera_turned_round_restarts_everywhere():
    rays, f, col = plane(8)
    prev_c, prev_h, cur, curh = col(), col(), col(), col()
    prev = dict(color=prev_c, half=prev_h, feat=f, history=np.full((H, W), 5, F32))
    back = camera(right=(-1, 0, 0), forward=(0, 0, 1))   # turned by 180 degrees about the up axis: zc = -D
    o, oh, hist = tr.temporal_accumulate(cur, curh, f, prev, camera(), back, rays, **LONG, **OFF)
    assert (tr.project(rays, f[..., 9], back, W, H)[3] < 0).all()
    assert np.array_equal(bits(o), bits(cur)) and np.array_equal(bits(oh), bits(curh)) and (hist == 1).all()
