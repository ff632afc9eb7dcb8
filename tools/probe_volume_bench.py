"""Probe volumes (hrt_probe_eval_device) on one GPU, HIP-event timed: 2 073 600 points (a 1080p frame's worth) looked up in grids
of 8 x 8 x 8, 32 x 16 x 32 and 64 x 64 x 64 probes, three ways:
  fused      hrt_probe_eval_device of the library loaded (libhrt.so: eight lanes to a point)
  fused A/B  the same from the A/B build with the other mapping (libhrt_var_probe_eval.so: a lane to a point), in a process of
             its own started by this script with HRT_LIBNAME set and --fused-only
  torch      what a caller had before: the cell and the weights in elementwise torch, eight gathers of 27 floats, and an einsum
             with the basis, on the same stream (no facing weights; agrees with the fused result to rounding, which is checked)
over three batches of points in cornell_mesh:
  texels     the 1920 x 1080 texel centres of the back wall (coherent: neighbours share their eight probes)
  shuffled   the same points in random order (incoherent)
  hits       the first hits of the 1920 x 1080 camera rays (trace_rays, mode "shade"), misses dropped and the rest repeated to size
Every timing is the time between two events round INNER back-to-back calls, divided by INNER; the median (min .. max) of --reps
such windows after two warm-up windows, the ways alternating within a repetition.  The plain and the facing rule are timed apart.

The quality figure users ask for, which has no threshold: a 16 x 16 x 16 grid traced at 1024 samples per probe, evaluated over the
64 x 64 floor lightmap, against scene.bake of the same texels at 1024 samples: relative RMSE with and without facing weights.  It
measures what nine SH coefficients and trilinear interpolation lose -- and the Monte-Carlo noise of both sides, so the bake is also
compared with itself under another seed, and the means over the lightmap with each other.

  python tools/probe_volume_bench.py [--reps 10] [--out profiles/probe_volume_bench.json] [--variants libhrt_var_probe_eval.so]
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

W, H = 1920, 1080
GRIDS = ((8, 8, 8), (32, 16, 32), (64, 64, 64))
INNER = 20
BOX = ((-3.4, -1.9, -1.9), (3.4, 1.9, 1.9))  # the room of cornell_mesh at 16:9 (x +-3.56, y +-2, z +-2), a little inside its walls
BACK_WALL, FLOOR = 5, 8                      # quads of the flattened scene: z = -2 and y = -2
C0, C1, C2, C3, C4 = 0.2820948, 0.48860251, 1.0925485, 0.31539157, 0.54627422
F_IRRADIANCE = (12.566371,) + (8.3775804,) * 3 + (3.1415927,) * 5


def timed(fns, reps):
    """Per function the median over `reps` windows of INNER calls of HIP-event time per call (ms) and the spread (min, max), after
    two warm-up windows each; the functions alternate within every repetition."""
    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / INNER
    for fn in fns:
        for _ in range(2):
            window(fn)
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(window(fn))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def torch_eval(lo, hi, counts, coeffs, pts):
    """The plain rule composed from torch operations: (n, 3)."""
    n = torch.tensor(counts, device="cuda")
    lo, hi = torch.tensor(lo, device="cuda"), torch.tensor(hi, device="cuda")
    s = n.float() / (hi - lo)
    P, N = pts[:, 0:3], pts[:, 4:7]
    Nn = N / N.norm(dim=1, keepdim=True)
    g = torch.minimum(((P - lo) * s - 0.5).clamp(min=0), (n - 1).float())
    i0f = g.floor()
    f = g - i0f
    i0 = i0f.long()
    i1 = torch.minimum(i0 + 1, n - 1)
    a = torch.zeros((pts.shape[0], 27), device="cuda")
    for m in range(8):
        c = [i1[:, k] if (m >> k) & 1 else i0[:, k] for k in range(3)]
        w = [f[:, k] if (m >> k) & 1 else 1 - f[:, k] for k in range(3)]
        a = a + ((w[0] * w[1]) * w[2])[:, None] * coeffs[(c[2] * counts[1] + c[1]) * counts[0] + c[0]]
    x, y, z = Nn[:, 0], Nn[:, 1], Nn[:, 2]
    Y = torch.stack([torch.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * (3 * (z * z) - 1), C2 * (x * z),
                     C4 * (x * x - y * y)], dim=1)
    F = torch.tensor(F_IRRADIANCE, device="cuda")
    return torch.einsum("nkc,nk->nc", a.view(-1, 9, 3), Y * F)


def batches(dev, desc, cam):
    n = W * H
    quads = hrt.scene_quads(desc)
    texels = torch.from_numpy(hrt.quad_points(quads[BACK_WALL], W, H)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    shuffled = texels[torch.randperm(n, device="cuda", generator=gen)].contiguous()
    rays = hrt.camera_rays(cam, W, H, 0, 1)
    shade = dev.trace_rays(rays, "shade")
    hit = shade[:, hrt.HIT_KIND].view(torch.int32) != 0
    hits = torch.zeros((int(hit.sum()), 8), device="cuda")
    hits[:, 0:3] = rays[hit][:, 0:3] + shade[hit][:, 0:1] * rays[hit][:, 4:7]
    hits[:, 4:7] = shade[hit][:, hrt.SHADE_NORMAL]
    hits = hits[torch.arange(n, device="cuda") % hits.shape[0]].contiguous()  # frame order kept; the tail repeats the head
    return {"texels": texels, "shuffled": shuffled, "hits": hits}


def quality(dev, desc, emit):
    counts, tw, spp = (16, 16, 16), 64, 1024
    coeffs = dev.probes(torch.from_numpy(hrt.probe_grid(*BOX, *counts)).cuda(), spp, seed=1)
    floor = torch.from_numpy(hrt.quad_points(hrt.scene_quads(desc)[FLOOR], tw, tw)).cuda()
    baked = dev.bake(floor, spp, seed=2)
    again = dev.bake(floor, spp, seed=3)  # the reference against itself: what of the figures below is its own Monte-Carlo noise
    emit(what="relative RMSE of bake against bake with another seed", scene="cornell_mesh", texels=[tw, tw], spp=spp,
         value=float(((again - baked) ** 2).mean().sqrt() / (baked ** 2).mean().sqrt()))
    with hrt.ProbeVolume(*BOX, *counts) as vol:
        vol.update(coeffs)
        for facing in (False, True):
            got = vol.eval(floor, facing=facing)
            rmse = float(((got - baked) ** 2).mean().sqrt() / (baked ** 2).mean().sqrt())
            emit(what="relative RMSE of eval against bake", scene="cornell_mesh", grid=list(counts), texels=[tw, tw], spp=spp, facing=facing, value=rmse)
            emit(what="mean of eval over the lightmap / mean of bake", scene="cornell_mesh", grid=list(counts), texels=[tw, tw], spp=spp, facing=facing,
                 value=float(got.mean() / baked.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", nargs="*", default=["libhrt_var_probe_eval.so"])
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    lib = os.environ.get("HRT_LIBNAME", "libhrt.so")
    hrt.init(0)
    rows = []

    def emit(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    host = hrt.HostScene().setup("cornell_mesh", W / H, 1)
    desc = host.flatten()
    dev = hrt.DeviceScene(desc)
    pts = batches(dev, desc, hrt.default_camera(W / H))
    n = W * H
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    for counts in GRIDS:
        count = counts[0] * counts[1] * counts[2]
        coeffs = torch.randn((count, 9, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(count))
        flat = coeffs.view(count, 27)
        with hrt.ProbeVolume(*BOX, *counts) as vol:
            vol.update(coeffs)
            for batch, p in pts.items():
                if not a.fused_only:  # the composition computes what the fused call computes, to rounding
                    ref, got = torch_eval(*BOX, counts, flat, p), vol.eval(p)
                    err = float((ref - got).abs().max() / got.abs().max())
                    assert err < 1e-4, (counts, batch, err)
                    emit(what="max |torch - fused| / max |fused|", grid=list(counts), batch=batch, value=err)
                fns = [lambda: vol.eval(p, out=out), lambda: vol.eval(p, facing=True, out=out)] + ([] if a.fused_only else [lambda: torch_eval(*BOX, counts, flat, p)])
                for what, (ms, tlo, thi) in zip(("fused", "fused, facing", "torch"), timed(fns, a.reps)):
                    emit(lib="torch" if what == "torch" else lib, grid=list(counts), probes=count, table_mb=count * 128 / 1e6, batch=batch, points=n, what=what,
                         ms=ms, ms_min=tlo, ms_max=thi, mpoints_s=n / ms / 1e3)
    if not a.fused_only:
        quality(dev, desc, emit)
    dev.close()
    for variant in a.variants if not a.fused_only else []:  # a process each: the library is loaded once per process
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-only", "--reps", str(a.reps)], env=dict(os.environ, HRT_LIBNAME=variant),
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(f"{variant} FAILED ({r.returncode}): {r.stderr[-2000:]}", flush=True)
            continue
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                emit(**json.loads(line))
    if a.fused_only:
        return
    print("\n| grid | packed MB | batch | what | library | ms per call (min .. max) | Mpoints/s |\n|---|---|---|---|---|---|---|")
    for r in sorted((r for r in rows if "ms" in r), key=lambda r: (r["probes"], r["batch"], r["what"], r["lib"])):
        print(f"| {'x'.join(map(str, r['grid']))} | {r['table_mb']:.2f} | {r['batch']} | {r['what']} | {r['lib']} | {r['ms']:.3f} ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) | {r['mpoints_s']:.0f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(points=n, grids=[list(g) for g in GRIDS], inner=INNER, reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
