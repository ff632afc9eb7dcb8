"""Mrays/s of the ray queries (hrt_trace_rays) per mode on one GPU, HIP-event timed, for two batches of a 1920x1080 frame:
  coherent    the pixel-centre camera rays, in pixel order
  incoherent  secondary rays built with torch on the device from the SHADE records of the coherent batch: origin p + 1e-5 dir,
              directions drawn about the shading normal (on the side the ray came from)
with the default flags and with HRT_FLAG_NO_LDS_TREE, and hrt_render_features(n_samples=0) on the same frame as the point of comparison
(it runs closest hit + shade per pixel, one launch).  One JSON line per (scene, batch, mode, form); a table at the end.  The default
build reads the tree from global memory, so both forms are the same there; a build with -DHRT_RAYS_STAGE_TREE (tools/variants.sh,
loaded with HRT_LIBNAME) stages the tree prefix in LDS unless HRT_FLAG_NO_LDS_TREE is given: that is the A/B of DESIGN section 5.

  python tools/rays_bench.py [--scenes cornell_mesh backrooms_pool] [--reps 10]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
hrt = importlib.import_module("hai719-raytracing_amd")
import oracle_lib  # noqa: E402

W, H = 1920, 1080


def timed(fn, reps):
    """Median over `reps` launches of HIP-event time (ms), after two warm-up launches."""
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def coherent_rays(cam):
    y, x = np.mgrid[0:H, 0:W]
    uv = np.stack([(x.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(W),
                   (y.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(H)], axis=1)
    cr = oracle_lib.camera_rays(cam, uv)
    r = np.empty((W * H, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = cr[:, 0:3], 0.0, cr[:, 3:6], np.inf
    return torch.from_numpy(r).cuda()


def incoherent_rays(rays, shade, seed=1):
    hit = shade[:, hrt.HIT_KIND].view(torch.int32) != 0
    r, s = rays[hit], shade[hit]
    p = r[:, 0:3] + s[:, 0:1] * r[:, 4:7]
    n = s[:, hrt.SHADE_NORMAL]
    n = torch.where((n * r[:, 4:7]).sum(1, keepdim=True) > 0, -n, n)  # face the incoming ray
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.randn(p.shape, device="cuda", generator=g)
    d = torch.nn.functional.normalize(n + torch.nn.functional.normalize(u, dim=1), dim=1)
    out = torch.empty((p.shape[0], 8), dtype=torch.float32, device="cuda")
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p + 1e-5 * d, 0.0, d, float("inf")
    return out.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_mesh", "backrooms_pool"])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    hrt.init(0)
    rows = []
    for name in a.scenes:
        host = hrt.HostScene().setup(name, W / H, 1)
        desc = host.flatten()
        dev = hrt.DeviceScene(desc)
        cam = hrt.default_camera(W / H)
        coh = coherent_rays(cam)
        inc = incoherent_rays(coh, dev.trace_rays(coh, "shade"))
        feat = torch.empty((H, W, hrt.FEATURE_FLOATS), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        lib = dev._lib

        def features():
            dev._check(lib.hrt_render_features(dev._h, C.byref(cam), W, H, 0, 0, 1, C.c_void_p(feat.data_ptr()), C.c_void_p(stream)))

        ms = timed(features, a.reps)
        rows.append(dict(scene=name, batch="coherent", mode="render_features(n=0)", form="-", rays=W * H, ms=ms, mrays_s=W * H / ms / 1e3))
        print(json.dumps(rows[-1]), flush=True)
        for batch, rays in (("coherent", coh), ("incoherent", inc)):
            for mode in ("closest", "shade", "occluded"):
                for form, flags in (("default", 0), ("no_lds_tree", hrt.FLAG_NO_LDS_TREE)):
                    ms = timed(lambda: dev.trace_rays(rays, mode, flags=flags), a.reps)
                    n = rays.shape[0]
                    rows.append(dict(scene=name, batch=batch, mode=mode, form=form, rays=n, ms=ms, mrays_s=n / ms / 1e3))
                    print(json.dumps(rows[-1]), flush=True)
        dev.close()
    print("\n| scene | batch | mode | tree | rays | ms | Mrays/s |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['batch']} | {r['mode']} | {r['form']} | {r['rays']} | {r['ms']:.3f} | {r['mrays_s']:.0f} |")


if __name__ == "__main__":
    main()
