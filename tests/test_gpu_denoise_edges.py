"""The device filter (include/hrt.h hrt_denoise) against the numpy statement (tests/denoise_ref.py) at its edges: bit for bit in the
exact regime (weights h_j h_k or 0), within the per-pixel expf bound where the weights go through exp, at the sizes, signs,
sigmas and non-finite values where a kernel goes wrong, at the size limit, and on other streams."""
import numpy as np
import pytest

import denoise_ref as dr

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = np.inf
FMAX = np.finfo(F32).max
LIMIT = 0x7FFFFFFF // 16  # the largest pixel count the denoiser's frame-size check admits


def dev_denoise(gpu, c, f, iterations, flags=0, stream=None, **params):
    """hrt_denoise on torch tensors (or numpy arrays, copied up) -> the output tensor; waits unless a stream is given."""
    import torch
    c = torch.from_numpy(np.ascontiguousarray(c, F32)).cuda() if isinstance(c, np.ndarray) else c
    f = torch.from_numpy(np.ascontiguousarray(f, F32)).cuda() if isinstance(f, np.ndarray) else f
    h, w = c.shape[0], c.shape[1]
    scratch = torch.empty(gpu.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    p = gpu.DenoiseParams(iterations=iterations, **params)
    s = stream if stream is not None else torch.cuda.current_stream()
    gpu.denoise(c.data_ptr(), f.data_ptr(), w, h, p, flags, scratch.data_ptr(), out.data_ptr(), s.cuda_stream)
    if stream is None:
        s.synchronize()
        return out.cpu().numpy()
    return out, scratch


def same(got, ref):
    """Bit for bit, except that any NaN equals any NaN (the sign of a NaN from pow differs between host and device)."""
    g, r = np.ascontiguousarray(got, F32), np.ascontiguousarray(ref, F32)
    return (np.isnan(g) == np.isnan(r)).all() and np.array_equal(g.view(np.uint32)[~np.isnan(g)], r.view(np.uint32)[~np.isnan(r)])


def diff_text(got, ref):
    bad = ~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref)))
    idx = np.argwhere(bad.any(axis=-1))[:4].tolist()
    return f"{int(bad.any(axis=-1).sum())} pixels differ, first {idx}: " + "; ".join(f"{got[y, x]} vs {ref[y, x]}" for y, x in idx)


def check_exact(gpu, c, f, iterations, what, **params):
    ref = dr.denoise(c, f, iterations=iterations, **params)
    got = dev_denoise(gpu, c, f, iterations, **params)
    assert same(got, ref), f"{what}: {diff_text(got, ref)}"
    return got, ref


def check_bound(gpu, c, f, iterations, what, **params):
    ref = dr.denoise(c, f, iterations=iterations, **params)
    got = dev_denoise(gpu, c, f, iterations, **params)
    bound = dr.expf_bound(c, f, iterations, **params)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all() and same(got[~fin], ref[~fin]), f"{what}: non-finite values differ"
    err = np.abs(got.astype(np.float64) - ref)
    bad = fin & ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} values beyond the bound, first {np.argwhere(bad)[:4].tolist()}"
    return got, ref


# ------------------------------------------------------------------------------------------------- exact regime: shapes and steps
SIZES = [(1, 1), (1, 2), (2, 1), (15, 17), (16, 16), (17, 15), (31, 33), (255, 257), (1, 300), (300, 1)]


@pytest.mark.parametrize("h,w", SIZES)
def test_exact_regime_bit_for_bit_at_every_step(gpu, h, w):
    c, f = dr.hard_edge_frame(h, w, seed=h * 1000 + w, block=(3, 4))
    for it in range(1, 9):
        check_exact(gpu, c, f, it, f"{h}x{w} iterations {it}", **dr.EXACT)
    for it in (1, 8):  # gamma: device and host pow in double may round apart by one fp32 ulp
        ref = dr.denoise(c, f, iterations=it, gamma=True, **dr.EXACT)
        got = dev_denoise(gpu, c, f, it, flags=gpu.FLAG_GAMMA, **dr.EXACT)
        fin = np.isfinite(ref)
        assert (np.isnan(got) == np.isnan(ref)).all()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert (ulps[fin] <= 1).all(), f"{h}x{w} gamma: {int((ulps[fin] > 1).sum())} values more than 1 ulp apart"


# ------------------------------------------------------------------------------------------------- signs and subnormals
def signed_frame(h=48, w=64):
    c, f = dr.hard_edge_frame(h, w, seed=9, block=(4, 4))
    ys, xs = np.mgrid[0:h, 0:w]
    band = (ys // 8) % 4
    for b, a in ((0, (-0.3, -0.7, 0.3)), (1, (0.0, 0.5, 1e-39)), (2, (1e-39, 2e-39, 1e-38))):
        sel = (band == b) & (f[..., 10] > 0)
        f[sel, 0:3] = np.array(a, F32)
    col = xs % 6
    c[col == 0] = (np.array([1e-40, 3e-41, 1e-45], F32) * (1 + (ys[col == 0] % 3))[:, None]).astype(F32)
    c[col == 1] = -c[col == 1]
    c[col == 2] = F32(-0.0)
    c[(col == 3) & (ys % 2 == 0)] = np.array([1e-39, 2e-3, 5e-39], F32)
    return c, f


@pytest.mark.parametrize("iterations", [1, 3])
def test_negative_zero_and_subnormal_albedo_and_colours(gpu, iterations):
    c, f = signed_frame()
    assert (f[..., 0:3] < 0).any() and ((f[..., 0:3] > 0) & (f[..., 0:3] < np.finfo(F32).tiny)).any()
    assert ((f[..., 6:9] > 0) & (f[..., 0:3] > 0)).any(), "emitters with albedo > 0"
    got, ref = check_exact(gpu, c, f, iterations, "signs and subnormals", **dr.EXACT)
    assert ((ref != 0) & (np.abs(ref) < np.finfo(F32).tiny)).any(), "the frame should keep subnormal results"
    assert (np.signbit(ref) & (ref == 0)).any(), "and -0.0 results"


# ------------------------------------------------------------------------------------------------- sigma edges
FINITE = dict(sigma_color=0.6, sigma_normal=0.3, sigma_albedo=0.2, sigma_depth=0.1)


def noisy_guides(h, w, seed):
    f = dr.synthetic_features(h, w, seed=seed)
    f[..., 3:6] += np.random.default_rng(seed).normal(0, 0.05, (h, w, 3)).astype(F32)
    c = (0.5 + np.random.default_rng(seed + 1).uniform(-0.5, 0.5, (h, w, 3))).astype(F32)
    return c, f


@pytest.mark.parametrize("name", ["sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"])
def test_each_sigma_at_infinity_alone(gpu, name):
    c, f = noisy_guides(37, 45, 3)
    params = dict(FINITE, **{name: INF})
    check_bound(gpu, c, f, 1, f"{name} = inf, 1 iteration", **params)
    if name == "sigma_color":
        check_bound(gpu, c, f, 6, f"{name} = inf, 6 iterations", **params)


def test_all_sigmas_at_infinity_are_the_plain_spline(gpu):
    c, f = noisy_guides(37, 45, 4)
    for it in (1, 4, 8):
        check_exact(gpu, c, f, it, f"all inf, {it} iterations", sigma_color=INF, sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)


@pytest.mark.parametrize("sigma", [1e-30, 1e-20, 1e-41], ids=["square-0", "square-subnormal", "subnormal"])
def test_tiny_guide_sigmas(gpu, sigma):
    c, f = dr.hard_edge_frame(40, 52, seed=5)
    f[..., 3:6] += (np.arange(52, dtype=F32) % 2 * F32(1e-3))[None, :, None]  # normals 1e-3 apart: E = 1e-6 / sigma^2
    for it in (1, 5):
        check_exact(gpu, c, f, it, f"sigma {sigma}", sigma_color=INF, sigma_normal=sigma, sigma_albedo=sigma, sigma_depth=sigma)


def test_a_colour_sigma_whose_square_overflows_in_early_iterations_only(gpu):
    """sigma_color = 1e20: (1e20 2^-i)^2 is +inf for i <= 2 (term off) and finite from i = 3 (terms of about 1e-38)."""
    sc = F32(1e20)
    assert [np.isinf(np.float32(sc * F32(2.0 ** -i)) ** 2) for i in range(5)] == [True, True, True, False, False]
    c, f = dr.hard_edge_frame(60, 70, seed=6)
    check_exact(gpu, c, f, 8, "sigma_color 1e20", sigma_color=1e20, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=1e-30)


def test_zero_and_overflowing_depths(gpu):
    """Depth 0 (misses) beside depths of 1e20 and 3e20: (sz * max z)^2 overflows, so the depth term is switched off for those
    pairs (den = +inf) even where (z_p - z_q)^2 overflows too; every weight is then h_j h_k."""
    h, w = 40, 48
    c, f = dr.hard_edge_frame(h, w, seed=7)
    f[..., 0:9] = f[0, 0, 0:9]
    f[..., 6:9] = 0
    ys, xs = np.mgrid[0:h, 0:w]
    f[..., 9] = np.array([0.0, 1e20, 3e20], F32)[(ys // 5 + xs // 6) % 3]
    for it in (1, 3, 6):
        got, _ = check_exact(gpu, c, f, it, f"huge depths, {it} iterations", sigma_color=INF, sigma_normal=INF, sigma_albedo=INF,
                             sigma_depth=1.0)
        assert np.isfinite(got).all()
    f[..., 9] = 0
    check_exact(gpu, c, f, 4, "all misses", sigma_color=INF, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=0.05)


# ------------------------------------------------------------------------------------------------- non-finite values
def bad_pixel_frame(h=60, w=64):
    """One non-finite value per pixel on a sparse grid: NaN, +inf, -inf in each of colour 0..2 and feature 0..11."""
    c, f = dr.hard_edge_frame(h, w, seed=11, block=(6, 8))
    spots = []
    k = 0
    for val in (np.nan, INF, -INF):
        for where in [("c", j) for j in range(3)] + [("f", j) for j in range(12)]:
            y, x = 3 + 6 * (k // 8), 3 + 8 * (k % 8)
            (c if where[0] == "c" else f)[y, x, where[1]] = val
            spots.append((y, x, where))
            k += 1
    return c, f, spots


@pytest.mark.parametrize("params", [dict(dr.EXACT), dict(sigma_color=INF, sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)],
                         ids=["exact", "spline"])
def test_a_non_finite_value_in_one_channel(gpu, params):
    c, f, spots = bad_pixel_frame()
    clean_c, clean_f = dr.hard_edge_frame(60, 64, seed=11, block=(6, 8))
    for it in (1, 3):
        got, ref = check_exact(gpu, c, f, it, f"one bad channel, {it} iterations", **params)
        for y, x, (kind, j) in spots:
            if kind == "f" and j >= 10:  # coverage and the spare channel are not guides
                continue
            assert same(got[y, x], c[y, x]), f"{kind}{j} non-finite at ({y}, {x}): the pixel should pass through"
        # channels 10 and 11 change nothing: the same frame with only those restored equals the one with them spoiled
        keep = np.array([(kind == "f" and j >= 10) for _, _, (kind, j) in spots])
        c2, f2 = c.copy(), f.copy()
        for (y, x, (kind, j)), k in zip(spots, keep):
            if k:
                f2[y, x, j] = clean_f[y, x, j]
        assert same(dev_denoise(gpu, c2, f2, it, **params), got)


@pytest.mark.parametrize("sc", [0.5, INF], ids=["colour-on", "colour-off"])
def test_a_colour_difference_whose_square_overflows_gets_no_weight(gpu, sc):
    """x = +-3e38 beside ordinary pixels: |x_p - x_q|^2 overflows.  Colour term on: that tap gets weight 0 (against the bound, the
    other weights go through exp).  Colour term off: the term stays 0 (T(inf, inf) = 0, never inf / inf), bit for bit."""
    h, w = 30, 34
    c, f = dr.hard_edge_frame(h, w, seed=12, block=(30, 34))
    f[..., 0:3] = 1
    f[..., 6:9] = 0
    c[::4, ::3] = F32(3e38)
    c[2::4, 1::3] = F32(-3e38)
    params = dict(sigma_color=sc, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=1e-30)
    for it in ((1,) if sc != INF else (1, 3)):
        got, _ = (check_bound if sc != INF else check_exact)(gpu, c, f, it, f"overflowing colour differences, sigma_color {sc}", **params)
        assert np.isfinite(got).all(), "a finite input never gives a non-finite linear output"


def test_an_overflowing_demodulation_makes_the_pixel_invalid(gpu):
    c, f = dr.hard_edge_frame(20, 24, seed=13)
    c[5, 7], f[5, 7, 0:3] = (3e38, 0.5, 0.5), (1e-3, 0.5, 0.5)
    c[12, 3], f[12, 3, 0:3] = (0.5, 0.5, 3e38), (0.5, 0.5, 1e-3)
    got, _ = check_exact(gpu, c, f, 3, "x = 3e41", **dr.EXACT)
    assert same(got[5, 7], c[5, 7]) and same(got[12, 3], c[12, 3])


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_a_remodulation_overflow_falls_back_to_the_input(gpu, channel):
    """a_p = 1e30 beside a_q = 1e-30 in one channel, the albedo term off: y_p averages x_q ~ 1e29 in, d_p y_p overflows."""
    h, w = 12, 14
    c, f = dr.hard_edge_frame(h, w, seed=14, block=(12, 14))
    f[..., 0:3] = 0.5
    f[..., 6:9] = 0
    f[6, 6, channel], f[6, 7, channel] = 1e30, 1e-30
    params = dict(sigma_color=INF, sigma_normal=1e-30, sigma_albedo=INF, sigma_depth=1e-30)
    got, ref = check_exact(gpu, c, f, 1, f"remodulation overflow in channel {channel}", **params)
    assert same(got[6, 6], c[6, 6]) and np.isfinite(got).all()


def test_a_channel_that_overflows_during_the_iterations_is_skipped_as_a_tap(gpu):
    """x.g = FLT_MAX everywhere: some pixels' y.g rounds to +inf in iteration 0 while y.r stays finite.  From iteration 1 those
    pixels are no taps for their neighbours (every channel of x_q must be finite).  Which pixels overflow depends on the last bit of
    exp, so only the number of pixels written through as their input is compared: about a third of the frame, where a kernel that
    took such taps would spread the infinity and write through nearly all of it."""
    h, w = 32, 32
    rng = np.random.default_rng(15)
    f = np.zeros((h, w, 12), F32)
    f[..., 0:3], f[..., 3:6], f[..., 10] = 1, (0, 0, 1), 1
    f[..., 9] = rng.uniform(1, 2, (h, w)).astype(F32)
    c = rng.uniform(0, 1, (h, w, 3)).astype(F32)
    c[..., 1] = FMAX
    params = dict(sigma_color=INF, sigma_normal=1e-30, sigma_albedo=1e-30, sigma_depth=0.5)
    x, _ = dr.demodulate(c, f)
    y = dr.iterate(x, f, 0, **params)
    assert (np.isinf(y[..., 1]) & np.isfinite(y[..., 0])).sum() > 20
    ref = dr.denoise(c, f, iterations=2, **params)
    got = dev_denoise(gpu, c, f, 2, **params)
    assert np.isfinite(got).all()
    through_ref = (ref == c).all(axis=-1)
    through_dev = (got == c).all(axis=-1)
    assert abs(int(through_dev.sum()) - int(through_ref.sum())) <= through_ref.sum() // 4 and through_ref.sum() < 0.6 * h * w, \
        f"pixels written through: {int(through_dev.sum())} on the device, {int(through_ref.sum())} in the statement"


# ------------------------------------------------------------------------------------------------- the expf regime
def test_expf_regime_one_iteration_with_the_colour_term(gpu):
    for h, w, seed in ((64, 80, 1), (17, 300, 2)):
        c, f = noisy_guides(h, w, seed)
        check_bound(gpu, c, f, 1, f"{h}x{w} colour on", **FINITE)
        check_bound(gpu, c, f, 1, f"{h}x{w} colour on, narrow", sigma_color=0.05, sigma_normal=0.1, sigma_albedo=0.05, sigma_depth=0.02)


def test_expf_regime_every_iteration_count_with_the_colour_term_off(gpu):
    c, f = noisy_guides(70, 90, 5)
    for it in range(1, 9):
        check_bound(gpu, c, f, it, f"colour off, {it} iterations", **dict(FINITE, sigma_color=INF))


# ------------------------------------------------------------------------------------------------- scale
def test_1080p_eight_iterations_on_the_full_frame(gpu):
    c, f = dr.hard_edge_frame(1080, 1920, seed=21, block=(7, 9))
    check_exact(gpu, c, f, 8, "1080p", **dr.EXACT)


def device_coord_frame(h, w, seed):
    import torch
    ys = torch.arange(h, dtype=torch.int64, device="cuda")[:, None].expand(h, w)
    xs = torch.arange(w, dtype=torch.int64, device="cuda")[None, :].expand(h, w)
    return dr.coord_frame(ys, xs, seed)


def check_windows(gpu, h, w, iterations, seed, windows):
    c, f = device_coord_frame(h, w, seed)
    import torch
    out, _ = dev_denoise(gpu, c, f, iterations, stream=torch.cuda.current_stream(), **dr.EXACT)
    torch.cuda.synchronize()
    del c, f
    for y0, y1, x0, x1 in windows:
        ref = dr.denoise_window(lambda a, b, p, q: dr.coord_window(a, b, p, q, seed), h, w, y0, y1, x0, x1, iterations, **dr.EXACT)
        got = out[y0:y1, x0:x1].cpu().numpy()
        assert same(got, ref), f"{h}x{w} window rows {y0}:{y1} cols {x0}:{x1}: {diff_text(got, ref)}"
    del out
    torch.cuda.empty_cache()


def test_4k_on_windows(gpu):
    h, w, k = 2160, 3840, 48
    wins = [(y, y + k, x, x + k) for y in (0, h // 2 - k // 2, h - k) for x in (0, w // 2 - k // 2, w - k)]
    check_windows(gpu, h, w, 6, 22, wins)


@pytest.mark.parametrize("h,w", [(LIMIT, 1), (1, LIMIT)], ids=["tallest", "widest"])
def test_the_largest_frames_the_size_check_admits(gpu, h, w):
    n = max(h, w)
    k = 300
    spans = [(0, k), (n // 2 - k // 2, n // 2 + k // 2), (n - k, n)]
    wins = [(a, b, 0, 1) for a, b in spans] if w == 1 else [(0, 1, a, b) for a, b in spans]
    check_windows(gpu, h, w, 8, 23, wins)


# ------------------------------------------------------------------------------------------------- streams
def test_denoise_on_a_side_stream_right_after_the_kernel_that_writes_its_input(gpu):
    import torch
    h, w = 540, 960
    c0, f0 = dr.hard_edge_frame(h, w, seed=31)
    want = dev_denoise(gpu, c0, f0, 5, **dr.EXACT)
    f = torch.from_numpy(f0).cuda()
    src = torch.from_numpy(c0).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = torch.full_like(src, float("nan"))
        busy = torch.ones(1 << 26, device="cuda")
        for _ in range(20):  # keep the stream busy, so the write below is still pending when hrt_denoise is queued
            busy = busy * 1.0000001
        c.copy_(src * (busy[0] * 0 + 1))
        out, scratch = dev_denoise(gpu, c, f, 5, stream=s, **dr.EXACT)
    s.synchronize()
    assert same(out.cpu().numpy(), want)


def test_two_denoise_calls_on_two_streams_in_flight_together(gpu):
    import torch
    h, w = 540, 960
    ca, fa = dr.hard_edge_frame(h, w, seed=32)
    cb, fb = dr.hard_edge_frame(h, w, seed=33)
    pa, pb = dict(dr.EXACT), dict(sigma_color=INF, sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)
    want_a, want_b = dev_denoise(gpu, ca, fa, 8, **pa), dev_denoise(gpu, cb, fb, 7, **pb)
    ta, tfa, tb, tfb = (torch.from_numpy(v).cuda() for v in (ca, fa, cb, fb))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    oa, _ = dev_denoise(gpu, ta, tfa, 8, stream=s1, **pa)
    ob, _ = dev_denoise(gpu, tb, tfb, 7, stream=s2, **pb)
    torch.cuda.synchronize()
    assert same(oa.cpu().numpy(), want_a) and same(ob.cpu().numpy(), want_b)
