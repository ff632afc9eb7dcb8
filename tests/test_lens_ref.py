"""The NumPy statement of the lens rule (tests/lens_ref.py) on its own, without a GPU: its RNG is the oracle's stream, a thin lens
focuses where it says and fills its disk uniformly, an equirectangular frame covers the sphere evenly, a fisheye frame is degenerate
exactly outside its image circle -- and RAY_TOL, the tolerance of tests/test_gpu_lens.py, is what its derivation says."""
import numpy as np
import pytest

import lens_ref
import oracle_lib

F32 = np.float32


@pytest.mark.parametrize("seed,pixel,sample", [(1, 0, 0), (7, 12345, 3), (2 ** 63 + 12345, 850 * 480 - 1, 2 ** 32 - 1), (2 ** 64 - 1, 2 ** 31 - 2, 2 ** 32 - 1),
                                               (0xDEADBEEF00000000, 1, 2 ** 31), (0, 2 ** 24 + 1, 17)])
def test_the_numpy_rng_is_the_oracle_stream(oracle, seed, pixel, sample):
    want = oracle_lib.path_stream(seed, pixel, sample, 512)
    got = lens_ref.draws(seed, np.full(512, pixel), sample, np.arange(512))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # one call over many pixels is the per-pixel stream
    px = np.array([pixel, 0, 5, 2 ** 31 - 2])
    many = lens_ref.draws(seed, px, sample, 2)
    assert np.array_equal(many, np.array([oracle_lib.path_stream(seed, int(p), sample, 3)[2] for p in px], F32))
    far = lens_ref.draws(seed, np.full(4, pixel), sample, lens_ref.LENS_DRAW + np.arange(4))
    assert ((far >= 0) & (far < 1)).all() and np.unique(far).size == 4


def thin(hrt, w, h, aperture=0.2, focus=4.0):
    cam = hrt.default_camera(w / h)
    return lens_ref.Lens(cam, "perspective", aperture, focus), lens_ref.Lens(cam, "perspective")


def test_thin_lens_rays_meet_their_pinhole_ray_in_the_plane_of_focus(hrt, oracle):
    w = h = 64  # 4096 samples
    for focus in (4.0, 0.5, 37.0):
        lens, pin = thin(hrt, w, h, 0.2, focus)
        r, deg = lens_ref.rays(lens, w, h, 3, 11)
        p, _ = lens_ref.rays(pin, w, h, 3, 11)
        assert not deg.any()
        assert np.array_equal(r[:, 3], p[:, 3]) and (r[:, 7] == np.inf).all()
        Fw = np.array(list(lens.cam.forward), np.float64)
        po, pd = p[:, 0:3].astype(np.float64), p[:, 4:7].astype(np.float64)
        target = po + (focus / (pd @ Fw))[:, None] * pd  # the pinhole ray's point at depth `focus` along forward
        o, d = r[:, 0:3].astype(np.float64), r[:, 4:7].astype(np.float64)
        t = ((target - o) * d).sum(1)
        miss = np.linalg.norm(o + t[:, None] * d - target, axis=1)
        assert miss.max() <= 1e-5 * focus, (focus, miss.max())
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6


def test_thin_lens_origins_fill_the_disk_uniformly(hrt, oracle):
    w = h = 64
    R = 0.2
    lens, _ = thin(hrt, w, h, R, 4.0)
    r, _ = lens_ref.rays(lens, w, h, 0, 5)
    E = np.array(list(lens.cam.eye), np.float64)
    off = r[:, 0:3].astype(np.float64) - E
    assert np.abs(off @ np.array(list(lens.cam.forward), np.float64)).max() < 1e-6  # in the lens plane
    q = (np.linalg.norm(off, axis=1) / R) ** 2
    assert q.max() <= 1 + 1e-5
    # (|O - E| / R)^2 is uniform on [0, 1) for a uniform disk: mean 1/2, sigma 1/sqrt(12 n) = 0.0045 for n = 4096; 5 sigma
    assert abs(q.mean() - 0.5) <= 0.023, q.mean()


def test_equirect_looks_along_forward_and_covers_the_sphere(hrt, oracle):
    w, h = 64, 32
    cam = hrt.default_camera(w / h)
    lens = lens_ref.Lens(cam, "equirect")
    Fw = np.array(list(cam.forward), F32)
    o, d, deg = lens_ref.project(lens, np.array([0.5], F32), np.array([0.5], F32), np.zeros(1, F32), np.zeros(1, F32), np.zeros(1, F32))
    assert not deg.any() and np.array_equal(o[0], np.array(list(cam.eye), F32))
    assert np.abs(d[0] - Fw / np.linalg.norm(Fw)).max() < 1e-6
    u, v, tm, l0, l1 = lens_ref.centres(w, h)
    _, d, deg = lens_ref.project(lens, u, v, tm, l0, l1)
    assert not deg.any()
    wgt = np.cos((0.5 - v.astype(np.float64)) * np.pi)  # the solid angle of a row
    mean = (d.astype(np.float64) * wgt[:, None]).sum(0) / wgt.sum()
    assert np.abs(mean).max() <= 0.05, mean
    # left edge looks backwards, top row up
    _, d, _ = lens_ref.project(lens, np.array([0.0, 0.5], F32), np.array([0.5, 0.0], F32), np.zeros(2, F32), np.zeros(2, F32), np.zeros(2, F32))
    assert np.abs(d[0] + Fw / np.linalg.norm(Fw)).max() < 1e-6
    assert np.abs(d[1] - np.array(list(cam.up), F32)).max() < 1e-6


def test_fisheye_is_degenerate_exactly_outside_its_image_circle(hrt, oracle):
    w, h = 37, 23
    cam = hrt.default_camera(w / h)
    lens = lens_ref.Lens(cam, "fisheye", extent=180.0)
    r, deg = lens_ref.rays(lens, w, h, 0, 1)
    rr = lens_ref.fisheye_radius(lens, w, h, 0, 1)
    assert np.array_equal(deg, rr > 1) and deg.any() and not deg.all()
    E = np.array(list(cam.eye), F32)
    assert (r[deg, 4:7] == 0).all() and (r[deg, 0:3] == E).all() and (r[deg, 7] == np.inf).all()
    u, _, tm, _, _ = lens_ref.film(w, h, 0, 1)
    assert np.array_equal(r[:, 3], tm)
    x = np.arange(w * h) % w
    assert deg[(x == 0) | (x == w - 1)].all()  # the frame is wider than the circle
    # on the rim of 180 degrees a ray is perpendicular to forward; at the centre it is forward
    Fw = np.array(list(cam.forward), np.float64)
    cosang = r[~deg, 4:7].astype(np.float64) @ Fw
    assert np.abs(cosang - np.cos(rr[~deg].astype(np.float64) * np.pi / 2)).max() < 1e-6
    o, d, dg = lens_ref.project(lens, np.array([0.5], F32), np.array([0.5], F32), np.zeros(1, F32), np.zeros(1, F32), np.zeros(1, F32))
    assert not dg.any() and np.abs(d[0] - Fw).max() < 1e-6


def test_ray_tol_is_four_times_the_fp32_to_fp64_gap_of_the_gpu_tests_inputs(hrt, oracle):
    gap = lens_ref.fp_gap(hrt)
    print(f"largest |fp32 - fp64| component difference: {gap:.3e}; RAY_TOL {lens_ref.RAY_TOL:.3e}")
    assert 0 < gap < 1e-5
    assert abs(lens_ref.RAY_TOL / (4 * gap) - 1) < 0.01, (gap, lens_ref.RAY_TOL)
    # the rim: a sample within RAY_TOL of it may fall on either side on the device; such samples must stay rare
    for name in ("fisheye180", "fisheye220"):
        for w, h in lens_ref.FRAMES:
            ref, _ = lens_ref.make(hrt, name, w, h)
            for sample, seed in lens_ref.DRAWS:
                rr = lens_ref.fisheye_radius(ref, w, h, sample, seed)
                assert (np.abs(rr - 1) <= lens_ref.RAY_TOL).mean() <= 0.01
