"""Msamples/s of the radiance queries (hrt_trace_radiance) on one GPU, HIP-event timed, at 1920x1080 with 16 samples per ray:
  camera    the render's camera rays of sample 0 (hrt_camera_rays), in pixel order, traced with n_samples = 16; compared with
            hrt_render_tiles at 16 spp under each forced kernel form (HRT_FLAG_WAVE_KERNEL, _DUAL_KERNEL, _STREAM_KERNEL)
  baking    incoherent rays built with torch on the device from the SHADE records of the camera rays: origin p + 1e-4 n,
            directions n + a random unit vector (cosine-weighted about the normal, on the side the ray came from)
with the default flags and with HRT_FLAG_NO_LDS_TREE.  One JSON line per (scene, batch, form); a table at the end.  The default build
reads the tree from global memory, so both forms are the same there; a build with -DHRT_RADIANCE_STAGE_TREE (tools/variants.sh, loaded
with HRT_LIBNAME) stages the tree prefix in LDS unless HRT_FLAG_NO_LDS_TREE is given: that is the A/B of DESIGN section 5.

  python tools/radiance_bench.py [--scenes cornell_mesh backrooms_pool random_spheres] [--reps 10] [--spp 16]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hrt = importlib.import_module("hai719-raytracing_amd")

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


def baking_rays(dev, cam, seed=1):
    centre = hrt.camera_rays(cam, W, H, 0, seed)  # the hit points of the camera rays of sample 0 are all that is used
    shade = dev.trace_rays(centre, "shade")
    hit = shade[:, hrt.HIT_KIND].view(torch.int32) != 0
    r, s = centre[hit], shade[hit]
    p = r[:, 0:3] + s[:, 0:1] * r[:, 4:7]
    n = s[:, hrt.SHADE_NORMAL]
    n = torch.where((n * r[:, 4:7]).sum(1, keepdim=True) > 0, -n, n)  # face the incoming ray
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(p.shape, device="cuda", generator=g), dim=1)
    d = torch.nn.functional.normalize(n + u, dim=1)
    out = torch.empty((p.shape[0], 8), dtype=torch.float32, device="cuda")
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p + 1e-4 * n, 0.0, d, float("inf")
    return out.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_mesh", "backrooms_pool", "random_spheres"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    hrt.init(0)
    rows = []
    spp, seed = a.spp, 1

    def emit(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for name in a.scenes:
        host = hrt.HostScene().setup(name, W / H, 1)
        dev = hrt.DeviceScene(host.flatten())
        cam = hrt.default_camera(W / H)
        stream = torch.cuda.current_stream().cuda_stream
        tiles = torch.empty((hrt.tiles_total(W, H), 64, 3), dtype=torch.float32, device="cuda")
        for form, fl in (("wave", hrt.FLAG_WAVE_KERNEL), ("dual", hrt.FLAG_DUAL_KERNEL), ("stream", hrt.FLAG_STREAM_KERNEL)):
            try:
                ms = timed(lambda: dev.render_tiles(cam, W, H, spp, seed, fl, 0, 1, tiles.data_ptr(), stream), a.reps)
            except hrt.HrtError as e:  # a form that refuses the scene (the streaming kernel's 48 KiB of tables)
                print(json.dumps(dict(scene=name, what=f"hrt_render {form}", refused=str(e))), flush=True)
                continue
            dev.check_last_launch()
            emit(scene=name, batch="camera", what=f"hrt_render {form}", rays=W * H, spp=spp, ms=ms, msamples_s=W * H * spp / ms / 1e3)
        cam_rays = hrt.camera_rays(cam, W, H, 0, seed)
        bake = baking_rays(dev, cam)
        for batch, rays in (("camera", cam_rays), ("baking", bake)):
            out = torch.empty((rays.shape[0], 3), dtype=torch.float32, device="cuda")
            for form, fl in (("radiance", 0), ("radiance no_lds_tree", hrt.FLAG_NO_LDS_TREE)):
                ms = timed(lambda: dev.trace_radiance(rays, spp=spp, seed=seed, flags=fl, out=out), a.reps)
                n = rays.shape[0]
                emit(scene=name, batch=batch, what=form, rays=n, spp=spp, ms=ms, msamples_s=n * spp / ms / 1e3)
        dev.close()
    print("\n| scene | batch | what | rays | spp | ms | Msamples/s |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['batch']} | {r['what']} | {r['rays']} | {r['spp']} | {r['ms']:.3f} | {r['msamples_s']:.0f} |")


if __name__ == "__main__":
    main()
