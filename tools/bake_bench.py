"""Msamples/s of baking (hrt_bake_device) on one GPU, HIP-event timed: bake points at the SHADE hit points of the camera rays of a
1920x1080 frame (normal facing the incoming ray, bias 1e-4, time 0), 16 samples per point, three ways:
  fused      hrt_bake_device, one launch for all samples, no ray buffer
  composed   what a caller had before it: per sample hrt_bake_rays into an n x 32-byte buffer + hrt_trace_radiance(n_samples = 1),
             the outputs summed in torch and divided at the end -- the composition the fused bake equals bit for bit (CONTRACT A)
  torch      the "baking" column of tools/radiance_bench.py: directions sampled once with torch (n + a random unit vector), one
             hrt_trace_radiance launch with n_samples = 16 over those records (the sampler's own time included and separately)
The median (and the spread) of --reps timings after two warm-up runs, the four alternating within every repetition.  One JSON line per (scene, what); a table at the end; --out writes the rows as
a JSON file (profiles/bake_bench.json).

  python tools/bake_bench.py [--scenes cornell_mesh backrooms_pool random_spheres] [--reps 10] [--spp 16] [--out profiles/bake_bench.json]
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
BIAS = 1e-4


def timed(fns, reps):
    """Per function the median over `reps` runs of HIP-event time (ms) and the spread (min, max), after two warm-up runs each; the
    functions alternate within every repetition, so that what else the machine does falls on all of them alike."""
    for fn in fns:
        for _ in range(2):
            fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def bake_points(dev, cam, seed=1):
    """{P, 0, N, bias} at the hits of the camera rays of sample 0, N facing the incoming ray."""
    centre = hrt.camera_rays(cam, W, H, 0, seed)
    shade = dev.trace_rays(centre, "shade")
    hit = shade[:, hrt.HIT_KIND].view(torch.int32) != 0
    r, s = centre[hit], shade[hit]
    p = r[:, 0:3] + s[:, 0:1] * r[:, 4:7]
    n = s[:, hrt.SHADE_NORMAL]
    n = torch.where((n * r[:, 4:7]).sum(1, keepdim=True) > 0, -n, n)
    out = torch.empty((p.shape[0], 8), dtype=torch.float32, device="cuda")
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p, 0.0, n, BIAS
    return out.contiguous()


def torch_sampler(points, seed=1):
    """tools/radiance_bench.py's baking rays from the same points: origin P + bias N, direction normalize(N + random unit vector)."""
    p, n = points[:, 0:3], points[:, 4:7]
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(p.shape, device="cuda", generator=g), dim=1)
    d = torch.nn.functional.normalize(n + u, dim=1)
    out = torch.empty((p.shape[0], 8), dtype=torch.float32, device="cuda")
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p + BIAS * n, 0.0, d, float("inf")
    return out.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_mesh", "backrooms_pool", "random_spheres"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
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
        pts = bake_points(dev, cam)
        n = pts.shape[0]
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        acc = torch.empty_like(out)

        def composed():
            acc.zero_()
            for s in range(spp):
                acc.add_(dev.trace_radiance(hrt.bake_rays(pts, s, seed), spp=1, first_sample=s, seed=seed, out=out))
            acc.div_(float(spp))

        rays = torch_sampler(pts)
        fused_out = torch.empty_like(out)
        t = timed([lambda: dev.bake(pts, spp, seed=seed, out=fused_out), composed, lambda: torch_sampler(pts),
                   lambda: dev.trace_radiance(rays, spp=spp, seed=seed, out=out)], a.reps)
        dev.bake(pts, spp, seed=seed, out=fused_out)
        composed()
        same = bool(torch.equal(fused_out.view(torch.int32), acc.view(torch.int32)))
        both = tuple(x + y for x, y in zip(t[2], t[3]))
        for what, (ms, lo, hi) in (("fused", t[0]), ("composed", t[1]), ("torch sampler + radiance", both), ("radiance of torch rays", t[3])):
            emit(scene=name, what=what, points=n, spp=spp, ms=ms, ms_min=lo, ms_max=hi, msamples_s=n * spp / ms / 1e3, fused_equals_composed=same)
        dev.close()
    print("\n| scene | what | points | spp | ms | Msamples/s |\n|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['what']} | {r['points']} | {r['spp']} | {r['ms']:.3f} | {r['msamples_s']:.0f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(frame=[W, H], spp=spp, reps=a.reps, bias=BIAS, device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
