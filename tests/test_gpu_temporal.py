"""Temporal accumulation on the GPU (include/hrt.h hrt_temporal_accumulate, hrt_render_temporal) against the numpy statement
(tests/temporal_ref.py): every pixel of colour, half colour and history bit for bit -- the rule has no transcendental in it -- on
rendered frames under orbiting cameras, at the seams of the frame and of the workgroup tiles, under a still camera, through the frame
loop against its parts, and the quality against a converged render."""
import math

import numpy as np
import pytest

import denoise_ref as dr
import temporal_ref as tr
from test_gpu_denoise import build, rmse
from test_gpu_denoise_var import dev_denoise_var, params_dict

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = math.inf
LONG = dict(alpha_min=1e-6, max_history=1e6)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same_bits(got, ref, what):
    for name, g, r in zip(("colour", "half colour", "history"), got, ref):
        if r is None:
            assert g is None
            continue
        bad = bits(g) != bits(r)
        assert not bad.any(), f"{what}: {name} differs on {int(bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=-1).sum())} pixels, " \
                              f"first {np.argwhere(bad)[:4].tolist()}"


def orbit(gpu, cam, deg):
    """cam turned by deg about the world's up axis (y) through the origin."""
    a = math.radians(deg)
    rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    out = gpu.Camera.from_buffer_copy(cam)
    for field in ("eye", "right", "up", "forward"):
        getattr(out, field)[:] = [float(v) for v in rot @ np.array(list(getattr(cam, field)), np.float64)]
    return out


def centre_rays(gpu, cam, w, h):
    """The pixel-centre rays of cam as the kernel draws them: hrt_debug_kat(HRT_KAT_CAMERA)."""
    u, v = tr.pixel_uv(w, h)
    r = gpu.debug_kat(gpu.KAT_CAMERA, np.stack([u, v], -1).reshape(-1, 2), cam=cam)
    return r[:, 0:3].reshape(h, w, 3), r[:, 3:6].reshape(h, w, 3)


def dev_accumulate(gpu, cam, prev_cam, c, ch, f, prev, stream=None, **params):
    """hrt_temporal_accumulate on numpy arrays -> (out, out_half or None, history) as numpy arrays.  The outputs start as NaN."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    h, w = c.shape[0], c.shape[1]
    tc, tch, tf = up(c), up(ch), up(f)
    pc, pch, pf, ph = (up(prev[k]) for k in ("color", "half", "feat", "history")) if prev is not None else (None,) * 4
    if ch is None:
        pch = None  # the previous half frame goes with the current one
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    outh = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda") if ch is not None else None
    hist = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream() if stream is None else stream
    gpu.temporal_accumulate(cam, prev_cam if prev is not None else None, w, h, ptr(tc), ptr(tch), ptr(tf), ptr(pc), ptr(pch), ptr(pf), ptr(ph),
                            gpu.TemporalParams(**params), ptr(out), ptr(outh), ptr(hist), s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy(), (None if outh is None else outh.cpu().numpy()), hist.cpu().numpy()


def state(o, oh, f, hist):
    return dict(color=o, half=oh, feat=f, history=hist)


def check(gpu, cam, prev_cam, c, ch, f, prev, what, rays=None, **params):
    """The device against the statement on one call; returns the device's outputs."""
    h, w = c.shape[0], c.shape[1]
    got = dev_accumulate(gpu, cam, prev_cam, c, ch, f, prev, **params)
    if rays is None and prev is not None and not tr.same_camera(cam, prev_cam):
        rays = centre_rays(gpu, cam, w, h)
    ref = tr.temporal_accumulate(c, ch, f, prev, cam, prev_cam, rays, **{**tr.DEFAULTS, **params})
    assert_same_bits(got, ref, what)
    return got


_frames = {}


def rendered(gpu, name, w, h, deg, seed, fspp, spp=4):
    """(camera, colour, half colour, features) of scene `name` from the default camera orbited by deg; rendered once per session."""
    key = (name, w, h, deg, seed, fspp, spp)
    if key not in _frames:
        if ("scene", name, w, h) not in _frames:
            _frames[("scene", name, w, h)] = build(gpu, name, w, h)
        _, _, dev, cam0 = _frames[("scene", name, w, h)]
        cam = orbit(gpu, cam0, deg) if deg else cam0
        c, _ = dev.render(cam, w, h, spp, seed)
        ch, _ = dev.render(cam, w, h, spp // 2, seed)
        _frames[key] = (cam, c, ch, dev.render_features(cam, w, h, 0, fspp, seed))
    return _frames[key]


# 1. rendered frames under an orbiting camera
TOLERANCES = [dict(), dict(depth_tol=INF), dict(normal_tol=INF), dict(albedo_tol=INF), dict(depth_tol=INF, normal_tol=INF, albedo_tol=INF),
              dict(depth_tol=1e-4, normal_tol=1e-6, albedo_tol=1e-6)]


@pytest.mark.parametrize("deg", [2.0, 40.0])
@pytest.mark.parametrize("name", ["cornell_mesh", "random_spheres"])
def test_rendered_frames_bit_for_bit_under_an_orbiting_camera(gpu, name, deg):
    w, h = 37, 29
    for fspp in (4, 0):
        cam1, c1, ch1, f1 = rendered(gpu, name, w, h, 0.0, 1, fspp)
        cam2, c2, ch2, f2 = rendered(gpu, name, w, h, deg, 2, fspp)
        rays = centre_rays(gpu, cam2, w, h)
        for use_half in (True, False):
            first = check(gpu, cam1, None, c1, ch1 if use_half else None, f1, None, f"{name} frame 1")
            assert np.array_equal(bits(first[0]), bits(c1)) and (first[2] == 1).all()
            prev = state(first[0], first[1], f1, first[2])
            hists = []
            for tol in TOLERANCES:
                got = check(gpu, cam2, cam1, c2, ch2 if use_half else None, f2, prev, f"{name} {deg} deg features {fspp} half {use_half} {tol}",
                            rays=rays, **LONG, **tol)
                hists.append(got[2])
            assert (hists[4] == 2).any(), "with every test off, pixels that project into the frame find history"
            assert ((hists[5] == 1) & (hists[4] == 2)).any(), "the tight tolerances reject taps the loose ones accept"
            assert (hists[4] == 1).any() or deg < 10, "a 40 degree orbit uncovers pixels"
            # a third frame on top of the second: histories above 1 and fractional enter the sums
            prev2 = state(got[0], got[1], f2, got[2])
            cam3, c3, ch3, f3 = rendered(gpu, name, w, h, deg + 1.5, 3, fspp)
            check(gpu, cam3, cam2, c3, ch3 if use_half else None, f3, prev2, f"{name} third frame", **LONG)


# 2. seams: frames of one row or column, the workgroup tile boundary, partial tap sets, non-finite values, sky
def synthetic(h, w, seed):
    """A frame over dr.synthetic_features with depths near the default camera's view of the origin, its half frame, and a previous
    frame of the same kind with fractional histories."""
    rng = np.random.default_rng(seed)
    rows = max(h, 2)   # a frame of one row would be all sky: take the first row of two
    f, pf = dr.synthetic_features(rows, w, seed=seed)[:h].copy(), dr.synthetic_features(rows, w, seed=seed)[:h].copy()
    hit = f[..., 10] > 0
    f[..., 9] = np.where(hit, 6.0 + rng.uniform(0, 0.02, (h, w)), 0).astype(F32)
    pf[..., 9] = np.where(hit, 6.0 + rng.uniform(0, 0.02, (h, w)), 0).astype(F32)
    col = lambda: (rng.uniform(0, 1, (h, w, 3)).astype(F32) + f[..., 6:9] / F32(6)).astype(F32)
    prev = state(col(), col(), pf, rng.uniform(1, 9, (h, w)).astype(F32))
    return col(), col(), f, prev


def pan(gpu, cam, pixels, h):
    """cam moved along its right axis by `pixels` pixels' worth at depth 6."""
    out = gpu.Camera.from_buffer_copy(cam)
    step = 2 * 6.0 * math.tan(math.radians(cam.fovy_deg) / 2) / h * pixels
    out.eye[:] = [cam.eye[k] + step * cam.right[k] for k in range(3)]
    return out


@pytest.mark.parametrize("h,w,pixels", [(1, 1, 0.3), (1, 40, 1.0), (40, 1, 0.4), (9, 65, 1.0), (9, 65, -17.5), (33, 35, 2.25)])
def test_seams_bit_for_bit(gpu, h, w, pixels):
    cam_prev = gpu.default_camera(w / h)
    cam = pan(gpu, cam_prev, pixels, h)
    c, ch, f, prev = synthetic(h, w, seed=h * 100 + w)
    loose = dict(depth_tol=0.05, normal_tol=INF, albedo_tol=INF, **LONG)
    got = check(gpu, cam, cam_prev, c, ch, f, prev, f"{h}x{w} pan {pixels}", **loose)
    if h * w > 1:
        assert (got[2] > 1).any()   # history is found
    check(gpu, cam, cam_prev, c, None, f, prev, f"{h}x{w} pan {pixels} without the half frame", **loose)
    check(gpu, cam, cam_prev, c, ch, f, prev, f"{h}x{w} pan {pixels}, defaults")
    # a checkerboard of history 0: partial tap sets are renormalised
    ys, xs = np.mgrid[0:h, 0:w]
    board = dict(prev, history=np.where((ys + xs) % 2 == 0, prev["history"], 0).astype(F32))
    check(gpu, cam, cam_prev, c, ch, f, board, f"{h}x{w} checkerboard history", **loose)
    # non-finite values in the current colour, the previous colour(s), the previous depth and the previous history
    rng = np.random.default_rng(w)
    def spoil(a, values):
        a = a.copy()
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, max(1, flat.size // 7)), replace=False)
        flat[idx] = rng.choice(np.array(values, F32), size=idx.size)
        return a
    bad = [np.nan, np.inf, -np.inf]
    pf = prev["feat"].copy()
    pf[..., 9] = spoil(pf[..., 9], bad)
    pf[..., 10] = spoil(pf[..., 10], bad + [0.0])
    cases = [(spoil(c, bad), spoil(ch, bad), f, prev),
             (c, ch, f, dict(prev, color=spoil(prev["color"], bad), half=spoil(prev["half"], bad))),
             (c, ch, f, dict(prev, feat=pf)),
             (c, ch, f, dict(prev, history=spoil(prev["history"], bad + [0.5, 0.0]))),
             (c, ch, spoil(f, bad + [0.0]), prev)]
    for k, (cc, cch, ff, pp) in enumerate(cases):
        o, oh, hist = check(gpu, cam, cam_prev, cc, cch, ff, pp, f"{h}x{w} non-finite case {k}", **loose)
        check(gpu, cam_prev, cam_prev, cc, cch, ff, pp, f"{h}x{w} non-finite case {k}, still camera", **loose)
        if k in (1, 2):  # a finite current frame never gives a non-finite output
            assert np.isfinite(o).all() and np.isfinite(oh).all() and np.isfinite(hist).all()
    sky = f[..., 10] == 0
    o, oh, hist = dev_accumulate(gpu, cam, cam_prev, c, ch, f, prev, **loose)
    assert sky.any() or h == 1
    assert (hist[sky] == 1).all() and np.array_equal(bits(o[sky]), bits(c[sky])) and np.array_equal(bits(oh[sky]), bits(ch[sky]))


# 3. a still camera: pixel onto pixel, history counts the frames
def test_still_camera_counts_frames_and_matches_the_statement(gpu):
    w, h, n = 37, 29, 6
    prev = None
    for k in range(1, n + 1):
        cam, c, ch, f = rendered(gpu, "cornell_mesh", w, h, 0.0, k, 0)
        got = check(gpu, cam, gpu.Camera.from_buffer_copy(cam), c, ch, f, prev, f"still camera frame {k}", **LONG)
        hit = (f[..., 10] > 0) & np.isfinite(c).all(axis=-1) & np.isfinite(ch).all(axis=-1)
        assert hit.mean() > 0.5 and (got[2][hit] == k).all() and (got[2][~hit] == 1).all()
        prev = state(got[0], got[1], f, got[2])


# 4. the frame loop against its parts
def device_gamma(gpu, frame):
    """hrt_finalize_tiles' gamma on a frame: one sample, the buffer padded to whole tiles."""
    import torch
    n = frame.size
    tiles = (n + 191) // 192
    buf = torch.ones(tiles * 192, dtype=torch.float32, device="cuda")
    buf[:n] = torch.from_numpy(np.ascontiguousarray(frame, F32).reshape(-1)).cuda()
    s = torch.cuda.current_stream()
    gpu.finalize_tiles(buf.data_ptr(), tiles, 1, gpu.FLAG_GAMMA, buf.data_ptr(), s.cuda_stream)
    s.synchronize()
    return buf[:n].cpu().numpy().reshape(frame.shape)


@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("flags_name", ["linear", "gamma"])
def test_render_temporal_equals_its_parts(gpu, filtered, flags_name):
    w, h, spp, fspp = 37, 29, 4, 4
    _, _, dev, cam0 = build(gpu, "cornell_mesh", w, h)
    flags = gpu.FLAG_GAMMA if flags_name == "gamma" else 0
    tp, dp = gpu.TemporalParams(), (gpu.DenoiseVarParams() if filtered else None)
    hist = gpu.History(dev)

    def by_hand(cam, seed, prev, prev_cam):
        c, _ = dev.render(cam, w, h, spp, seed)
        ch, _ = dev.render(cam, w, h, spp // 2, seed)
        f = dev.render_features(cam, w, h, 0, fspp, seed)
        o, oh, n = dev_accumulate(gpu, cam, prev_cam, c, ch, f, prev)
        if filtered:
            frame, _ = dev_denoise_var(gpu, o, oh, f, flags, variance=False, **params_dict(dp))
        else:
            frame = device_gamma(gpu, o) if flags else o
        return frame, state(o, oh, f, n)

    prev, prev_cam = None, None
    for k in range(3):
        cam = orbit(gpu, cam0, 3.0 * k)
        frame, n = dev.render_temporal(hist, cam, w, h, spp, fspp, 10 + k, flags, tp, dp)
        ref, prev = by_hand(cam, 10 + k, prev, prev_cam)
        prev_cam = cam
        assert np.array_equal(bits(frame), bits(ref)), f"frame {k}"
        assert np.array_equal(bits(n), bits(prev["history"])), f"frame {k} history"
    assert (n > 2).any()
    # reset: the next frame restarts everywhere
    hist.reset()
    frame, n = dev.render_temporal(hist, cam, w, h, spp, fspp, 20, flags, tp, dp)
    ref, prev = by_hand(cam, 20, None, None)
    assert (n == 1).all() and np.array_equal(bits(frame), bits(ref))
    frame, n = dev.render_temporal(hist, cam, w, h, spp, fspp, 21, flags, tp, dp)
    ref, prev = by_hand(cam, 21, prev, cam)
    assert (n == 2).any() and np.array_equal(bits(frame), bits(ref)) and np.array_equal(bits(n), bits(prev["history"]))
    # another frame size restarts too, and the history goes on from there
    w2, h2 = 24, 20
    cam_s = gpu.default_camera(w2 / h2)
    frame, n = dev.render_temporal(hist, cam_s, w2, h2, spp, fspp, 22, 0, tp, None)
    assert (n == 1).all() and np.array_equal(bits(frame), bits(dev.render(cam_s, w2, h2, spp, 22)[0]))
    frame, n = dev.render_temporal(hist, cam_s, w2, h2, spp, fspp, 23, 0, tp, None)
    assert (n == 2).any()
    st = gpu.Stats()
    dev.render_temporal(hist, cam_s, w2, h2, spp, 0, 24, 0, tp, None, st)
    assert st.kernel_ms > 0 and st.samples == w2 * h2 * spp
    with pytest.raises(gpu.HrtError, match="spp must be even"):
        dev.render_temporal(hist, cam_s, w2, h2, 3, 0, 25)
    hist.close()


def test_a_launch_on_another_stream_gives_the_same_bits(gpu):
    import torch
    h, w = 33, 35
    cam_prev = gpu.default_camera(w / h)
    cam = pan(gpu, cam_prev, 1.5, h)
    c, ch, f, prev = synthetic(h, w, seed=9)
    a = dev_accumulate(gpu, cam, cam_prev, c, ch, f, prev)
    b = dev_accumulate(gpu, cam, cam_prev, c, ch, f, prev, stream=torch.cuda.Stream())
    assert_same_bits(b, a, "non-default stream")


# 5. it helps: 8 frames of 4 spp against a 4096-spp render at the last camera
def test_accumulated_frames_are_closer_to_the_converged_render(gpu):
    w, h, n, spp = 64, 48, 8, 4
    _, _, dev, cam0 = build(gpu, "cornell_mesh", w, h)
    tp = gpu.TemporalParams(alpha_min=1e-6, max_history=64.0)
    # still camera
    truth, _ = dev.render(cam0, w, h, 4096, 1000)
    hist = gpu.History(dev)
    for k in range(n):
        acc, lens = dev.render_temporal(hist, cam0, w, h, spp, 0, 1 + k, 0, tp, None)
    last, _ = dev.render(cam0, w, h, spp, n)
    direct, _ = dev.render(cam0, w, h, n * spp, 77)
    r_acc, r_last, r_direct = rmse(acc, truth), rmse(last, truth), rmse(direct, truth)
    print(f"TEMPORAL still camera: last frame {r_last:.5f} accumulated {r_acc:.5f} (ratio {r_acc / r_last:.4f}) direct {n * spp} spp {r_direct:.5f} "
          f"(accumulated / direct {r_acc / r_direct:.4f}), mean history {lens.mean():.2f}")
    assert r_acc < r_last
    assert abs(r_acc / r_direct - 1.0) <= 0.10, "both are means of 32 independent samples per pixel"
    # an orbit of 1 degree per frame
    hist.reset()
    for k in range(n):
        cam = orbit(gpu, cam0, 1.0 * k)
        acc, lens = dev.render_temporal(hist, cam, w, h, spp, spp, 1 + k, 0, gpu.TemporalParams(), None)
    truth, _ = dev.render(cam, w, h, 4096, 1000)
    last, _ = dev.render(cam, w, h, spp, n)
    r_acc, r_last = rmse(acc, truth), rmse(last, truth)
    print(f"TEMPORAL 1 degree orbit: last frame {r_last:.5f} accumulated {r_acc:.5f} (ratio {r_acc / r_last:.4f}), mean history {lens.mean():.2f}")
    assert r_acc < r_last
    hist.close()
