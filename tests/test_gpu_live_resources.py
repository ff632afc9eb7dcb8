"""Every device buffer, pinned buffer, event and stream of libhrt.so has one owner that frees it (csrc/hrt_api.hip "The owners"),
and hrt_debug_live_resources counts them.  One cycle creates scenes, runs every family of entry points once at the smallest shapes
that still reach every buffer, and closes everything explicitly: the counts are back where they started, a second cycle peaks
where the first did (nothing accumulates), and a call refused after it has allocated leaves nothing behind.  Only the library's own
counter is read: the device's free memory belongs to everyone on the machine.  (About 2 s inside the suite; 12 s as the first test
of a process, where it is the one that loads every kernel family's code.)"""
import ctypes as C
import gc

import numpy as np
import pytest

import kd_meshes as km
import kd_ref

pytestmark = pytest.mark.gpu
W, H, SPP = 24, 17, 2  # 3 x 3 tiles, partial ones on both edges
PW, PH = 41, 25        # 1025 pixels: two blocks of the P3 scan


@pytest.fixture(scope="module")
def descs(gpu):
    """The flattened scenes, built once: emissive squares and a mesh; point lights (the _lights builds)."""
    return {name: gpu.HostScene().setup(name, W / H, 1).flatten() for name in ("cornell_mesh", "random_spheres")}


class Peak:
    def __init__(self, gpu):
        self.gpu, self.peak = gpu, gpu.live_resources()

    def __call__(self):
        now = self.gpu.live_resources()
        self.peak = tuple(max(a, b) for a, b in zip(self.peak, now))
        return now


def rays(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-0.5, 0.5, (n, 3))
    d = rng.normal(size=(n, 3))
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 7] = 1e30
    return r


def refused_encode(gpu, frame, fmt, need):
    """A capacity one byte short: refused with the parent's message after the P3 form has allocated, nothing left behind."""
    import torch
    out = torch.zeros(need, dtype=torch.uint8, device="cuda")
    held = gpu.live_resources()
    with pytest.raises(gpu.HrtError) as e:
        gpu.encode_ppm(frame.data_ptr(), PW, PH, fmt, out.data_ptr(), need - 1, 0)
    assert str(e.value) == f"hrt_encode_ppm failed (-1): hrt_encode_ppm: output buffer too small (need {need})"
    assert gpu.live_resources() == held
    assert gpu.encode_ppm(frame.data_ptr(), PW, PH, fmt, out.data_ptr(), need, 0) == need
    assert gpu.live_resources() == held


def scene_families(gpu, name, desc, see):
    """Every entry point that takes a scene, once; everything it creates is closed before it returns."""
    import torch
    cam = gpu.default_camera(W / H)
    held = gpu.live_resources()
    dev = gpu.DeviceScene(desc)
    made = see()
    assert made[0] > held[0] and made[2] > held[2], (held, made)  # the counter is alive
    dev.render(cam, W, H, SPP)
    made = see()
    lib = gpu.device_lib()
    lib.hrt_render_aov.argtypes = [C.c_void_p, C.POINTER(gpu.Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    aov = np.empty((H, W, 3), np.float32)
    assert lib.hrt_render_aov(dev._h, C.byref(cam), W, H, 1, aov.ctypes.data) == 0, lib.hrt_last_error()
    assert see() == made  # its frame buffer is the call's own
    dev.render_adaptive(cam, W, H, 2, 4, 0.05); see()
    dev.render_denoised(cam, W, H, SPP, 1); see()
    dev.render_denoised_var(cam, W, H, SPP, 1, variance=True); see()
    hist = gpu.History(dev)
    for frame in range(2):
        dev.render_temporal(hist, cam, W, H, SPP, 1, seed=1 + frame, dparams=gpu.DenoiseVarParams()); see()
    dev.render_features(cam, W, H, 0, 1); see()
    r = rays(65, 3)  # one wave and one more ray
    dev.trace_rays(r); see()
    dev.trace_radiance(r, spp=SPP); see()
    pts = r.copy()
    pts[:, 7] = 1e-4
    dev.bake(pts, spp=SPP, keys=np.arange(65, dtype=np.uint32)[::-1].copy()); see()  # the blocking form
    dev.render_views([cam, cam], W, H, SPP, seeds=[1, 2]); see()
    lens = gpu.Lens(cam, "fisheye", extent=180.0)
    dev.render_lens(lens, W, H, SPP); see()
    dev.render_lens_views([lens, gpu.Lens(cam)], W, H, SPP, seeds=[1, 2]); see()
    dev.render_lens_adaptive(lens, W, H, 2, 4, 0.05); see()
    torch.cuda.synchronize()
    hist.close()
    dev.close()
    assert see() == held, name


def cycle(gpu, descs):
    """One whole cycle; returns its peak counts.  Ends where it started."""
    import torch
    gc.collect()  # nothing of an earlier test is freed half way
    before = gpu.live_resources()
    see = Peak(gpu)
    for name, desc in descs.items():
        scene_families(gpu, name, desc, see)
    # the entry points without a scene
    frame = torch.from_numpy(np.random.default_rng(7).uniform(0, 1.2, (PH, PW, 3)).astype(np.float32)).cuda()
    refused_encode(gpu, frame, 6, len(f"P6\n{PW} {PH}\n255\n") + PW * PH * 3)
    refused_encode(gpu, frame, 3, len(gpu.ppm_text_reference(frame.cpu().numpy())))
    see()
    kat_cam = gpu.default_camera(1.0)
    prims = {gpu.KAT_TRIANGLE: 9, gpu.KAT_AABB: 6, gpu.KAT_SPHERE: 7, gpu.KAT_QUAD: 13, gpu.KAT_QUAD_RCP: 13}
    for which in range(11):
        inp = np.random.default_rng(which).uniform(0.1, 0.9, (3, gpu._KAT_IN[which])).astype(np.float32)
        prim = None
        if which in prims:
            prim = np.zeros(prims[which], np.float32)
            prim[:9] = (0, 0, -2, 1, 0, -2, 0, 1, -2)[:min(9, prims[which])]  # three corners; a centre and radius; a box
            if which == gpu.KAT_AABB:
                prim[:] = (-1, -1, -3, 1, 1, -2)
        gpu.debug_kat(which, inp, prim=prim, cam=kat_cam if which == gpu.KAT_CAMERA else None)
        assert see() == before, which
    lib = gpu.device_lib()
    lib.hrt_debug_path_stream.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    draws = np.empty(16, np.float32)
    assert lib.hrt_debug_path_stream(5, 1, 2, 16, draws.ctypes.data) == 0, lib.hrt_last_error()
    pos, tri = km.soup(17, 1)  # enough for a second level: the ping-pong arrays and the partition's counters
    lo, hi, cl, ch = kd_ref.soup_refs(pos, tri)
    rc, nodes, _, _, _ = kd_ref.call_builder(C.cast(lib.hrt_kd_build_gpu, C.c_void_p).value, np.arange(len(lo), dtype=np.uint32), lo, hi, cl, ch, 1, 12)
    assert rc == 0 and len(nodes) > 1
    assert see() == before
    multi = gpu.MultiScene(descs["cornell_mesh"], (0, 0))  # the peer form: two slots on one device
    assert multi.gather == "peer"
    made = see()
    assert made[3] == before[3] + 2 and made[2] > before[2]
    multi.render(gpu.default_camera(W / H), W, H, SPP); see()
    multi.close()
    assert gpu.live_resources() == before
    return see.peak, before


def test_every_family_gives_back_what_it_took_and_a_second_cycle_peaks_where_the_first_did(gpu, descs):
    first, before = cycle(gpu, descs)
    assert all(p > b for p, b in zip(first, before)), (first, before)  # pinned buffers and streams were reached, too
    second, again = cycle(gpu, descs)
    assert again == before and second == first


def test_a_history_destroyed_after_shutdown_frees_its_buffers(gpu, descs):
    """hrt_history_destroy after hrt_shutdown used to leave the history's eight buffers behind.  hrt_shutdown only forgets which
    devices are prepared, and hrt_init prepares device 0 again at once: the scenes other tests hold stay valid."""
    gc.collect()
    before = gpu.live_resources()
    cam = gpu.default_camera(W / H)
    dev = gpu.DeviceScene(descs["cornell_mesh"])
    hist = gpu.History(dev)
    dev.render_temporal(hist, cam, W, H, SPP, 1)
    dev.render_temporal(hist, cam, W, H, SPP, 1, seed=2)
    with_history = gpu.live_resources()
    try:
        gpu.device_lib().hrt_shutdown()
        hist.close()
        freed = gpu.live_resources()
    finally:
        gpu.init(0)
    assert with_history[0] - freed[0] == 8, (with_history, freed)
    dev.close()
    assert gpu.live_resources() == before
