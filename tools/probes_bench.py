"""Light probes (hrt_probes_device) on one GPU, HIP-event timed: grids of 16x8x4 and 64x32x8 probes in the middle of the scene's
bounding box at 256 and 1024 samples per probe, two ways:
  fused      hrt_probes_device: one trace launch (a wave per probe and block of HRT_PROBE_BLOCK samples) and the small fold launch
  composed   what a caller had before it: per sample the uniform directions made in torch into an n x 32-byte ray buffer,
             hrt_trace_radiance(n_samples = 1), and the projection onto the nine basis functions in torch, summed and divided at
             the end (the same estimator; torch's random numbers, so not the same bits)
The median (and the spread) of --reps timings after two warm-up runs, the two alternating within every repetition.  One JSON line
per (scene, grid, spp, what); a table at the end; --out writes the rows as a JSON file (profiles/probes_bench.json).

A/B of the block size: for every library named by --variants (A/B builds of the same ABI with another -DHRT_PROBE_BLOCK,
  make -C hai719-raytracing_amd libhrt_var_probe256.so          (part of `make all`: tests/test_gpu_probe_cases.py loads it)
  make -C hai719-raytracing_amd libhrt_var_probe1024.so VARIANT=libhrt_var_probe1024.so VARIANT_FLAGS=-DHRT_PROBE_BLOCK=1024u
) the script starts itself once more with HRT_LIBNAME set and --fused-only, and adds that process's fused rows
tagged with the library.  The shipped library (libhrt.so) has the header's HRT_PROBE_BLOCK.

  python tools/probes_bench.py [--scenes cornell_mesh backrooms_pool random_spheres] [--reps 10] [--out profiles/probes_bench.json]
                               [--variants libhrt_var_probe256.so libhrt_var_probe1024.so]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hrt = importlib.import_module("hai719-raytracing_amd")

GRIDS = ((16, 8, 4), (64, 32, 8))
SPPS = (256, 1024)
C0, C1, C2, C3, C4 = 0.2820948, 0.48860251, 1.0925485, 0.31539157, 0.54627422


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


def scene_box(dev, cam):
    """The middle half, per axis, of the box round the first hits of a 64 x 36 frame: inside the scene, whatever its size."""
    centre = hrt.camera_rays(cam, 64, 36, 0, 1)
    shade = dev.trace_rays(centre, "shade")
    hit = shade[:, hrt.HIT_KIND].view(torch.int32) != 0
    p = (centre[hit][:, 0:3] + shade[hit][:, 0:1] * centre[hit][:, 4:7]).cpu().numpy()
    p = np.concatenate([p, centre[:1, 0:3].cpu().numpy()])
    lo, hi = np.percentile(p, 10, axis=0), np.percentile(p, 90, axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 4
    return (mid - half).tolist(), (mid + half).tolist()


def basis(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return torch.stack([torch.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * (3 * (z * z) - 1), C2 * (x * z),
                        C4 * (x * x - y * y)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_mesh", "backrooms_pool", "random_spheres"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", nargs="*", default=[])
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    lib = os.environ.get("HRT_LIBNAME", "libhrt.so")
    hrt.init(0)
    rows = []
    seed = 1

    def emit(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    for name in a.scenes:
        host = hrt.HostScene().setup(name, 16 / 9, 1)
        dev = hrt.DeviceScene(host.flatten())
        lo, hi = scene_box(dev, hrt.default_camera(16 / 9))
        for grid in GRIDS:
            probes = torch.from_numpy(hrt.probe_grid(lo, hi, *grid)).cuda()
            n = probes.shape[0]
            rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            rays[:, 0:4], rays[:, 7] = probes, float("inf")
            out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            acc = torch.empty((n, 9, 3), dtype=torch.float32, device="cuda")
            fused_out = torch.empty_like(acc)
            gen = torch.Generator(device="cuda").manual_seed(seed)
            for spp in SPPS:
                def composed():
                    acc.zero_()
                    for s in range(spp):
                        u = torch.rand((n, 2), device="cuda", generator=gen)
                        z = 1 - 2 * u[:, 0]
                        r, phi = torch.sqrt(torch.clamp(1 - z * z, min=0)), 6.2831855 * u[:, 1]
                        rays[:, 4], rays[:, 5], rays[:, 6] = r * torch.cos(phi), r * torch.sin(phi), z
                        dev.trace_radiance(rays, spp=1, first_sample=s, seed=seed, out=out)
                        acc.add_(basis(rays[:, 4:7])[:, :, None] * out[:, None, :])
                    acc.div_(float(spp))

                fns = [lambda: dev.probes(probes, spp, seed=seed, out=fused_out)] + ([] if a.fused_only else [composed])
                t = timed(fns, a.reps)
                for what, (ms, tlo, thi) in zip(("fused", "composed"), t):
                    emit(scene=name, lib=lib, grid=list(grid), probes=n, spp=spp, what=what, ms=ms, ms_min=tlo, ms_max=thi, msamples_s=n * spp / ms / 1e3)
                if not a.fused_only:  # the two estimate the same 27 numbers per probe: their difference is Monte-Carlo noise
                    emit(scene=name, lib=lib, grid=list(grid), probes=n, spp=spp, what="mean |fused - composed| / mean |fused|",
                         value=float((fused_out - acc).abs().mean() / fused_out.abs().mean()))
        dev.close()
    for variant in a.variants:  # a process each: the library is loaded once per process
        env = dict(os.environ, HRT_LIBNAME=variant)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-only", "--reps", str(a.reps), "--scenes"] + a.scenes,
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(f"{variant} FAILED ({r.returncode}): {r.stderr[-2000:]}", flush=True)
            continue
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                emit(**json.loads(line))
    if a.fused_only:
        return
    print("\n| scene | library | probes | spp | what | ms (min .. max) | Msamples/s |\n|---|---|---|---|---|---|---|")
    for r in rows:
        if "ms" in r:
            print(f"| {r['scene']} | {r['lib']} | {r['probes']} | {r['spp']} | {r['what']} | {r['ms']:.3f} ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) | {r['msamples_s']:.0f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(grids=[list(g) for g in GRIDS], spps=list(SPPS), reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
