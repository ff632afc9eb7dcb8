"""Probe visibility (hrt_probe_depth_device, hrt_probe_eval_visible_device) on one GPU, HIP-event timed, in cornell_mesh:

  probe_depth   8 x 8 x 8 and 16 x 16 x 16 grids at 256 and 1024 samples per probe, two ways:
      fused        hrt_probe_depth_device
      composed     what a caller had before: per sample hrt_probe_rays + hrt_trace_rays(closest), then the filter in torch (a
                   (probes, 64) matrix product per sample, accumulated); agrees with the fused sums to rounding, which is checked
  eval_visible  the three 2 073 600-point sets of tools/probe_volume_bench.py (texels, shuffled, hits) in 8 x 8 x 8, 32 x 16 x 32
                and 64 x 64 x 64 grids with random coefficients and moments: hrt_probe_eval_visible_device with facing weights
                against hrt_probe_eval_device with facing weights from the same library -- the cost of visibility
  quality       the floor-lightmap experiment of tools/probe_volume_bench.py (a 16 x 16 x 16 grid at 1024 samples against
                scene.bake of the 64 x 64 floor texels): the relative RMSE with and without visibility, no threshold

Timing is probe_volume_bench.timed: the median (min .. max) over --reps windows of back-to-back calls after two warm-up windows.

  python tools/probe_depth_bench.py [--reps 5] [--out profiles/probe_depth_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_volume_bench as pvb  # noqa: E402

hrt = pvb.hrt
W, H, BOX, FLOOR = pvb.W, pvb.H, pvb.BOX, pvb.FLOOR
DEPTH_GRIDS = ((8, 8, 8), (16, 16, 16))
DEPTH_SAMPLES = (256, 1024)


def r_max_of(counts):
    e = [(hi - lo) / c for lo, hi, c in zip(BOX[0], BOX[1], counts)]
    return 1.5 * float(np.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2))


def centres():
    """(64, 3) on the GPU, from the library's own host function."""
    return torch.from_numpy(np.stack([hrt.probe_depth_direction(e) for e in range(hrt.PROBE_DEPTH_TEXELS)])).cuda()


def composed_depth(dev, probes, spp, seed, r_max, c):
    """The sums from per-sample launches and a torch fold: (n, 64, 3)."""
    out = torch.zeros((probes.shape[0], 64, 3), device="cuda")
    for s in range(spp):
        rays = hrt.probe_rays(probes, s, seed)
        rec = dev.trace_rays(rays, "closest")
        hit = rec[:, hrt.HIT_KIND].view(torch.int32) != 0
        r = torch.where(hit, rec[:, hrt.HIT_T].clamp(max=r_max), torch.full_like(rec[:, 0], r_max))
        w = (rays[:, 4:7] @ c.T).clamp(min=0) ** 32
        out += torch.stack([w, w * r[:, None], w * (r * r)[:, None]], dim=2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hrt.init(0)
    rows = []

    def emit(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    host = hrt.HostScene().setup("cornell_mesh", W / H, 1)
    desc = host.flatten()
    dev = hrt.DeviceScene(desc)
    c = centres()
    # ---- probe_depth
    inner = pvb.INNER
    for counts in DEPTH_GRIDS:
        probes = torch.from_numpy(hrt.probe_grid(*BOX, *counts)).cuda()
        n, r_max = probes.shape[0], r_max_of(counts)
        out = torch.empty((n, 64, 3), device="cuda")
        for spp in DEPTH_SAMPLES:
            got, ref = dev.probe_depth(probes, spp, seed=1, r_max=r_max), composed_depth(dev, probes, spp, 1, r_max, c)
            err = float((ref - got).abs().max() / got.abs().max())
            assert err < 1e-4, (counts, spp, err)
            emit(what="max |composed - fused| / max |fused|", grid=list(counts), spp=spp, value=err)
            pvb.INNER = 4  # a fused call is milliseconds and a composed one thousands of launches: short windows
            (ms, lo, hi), = pvb.timed([lambda: dev.probe_depth(probes, spp, seed=1, r_max=r_max, out=out)], a.reps)
            emit(what="probe_depth, fused", grid=list(counts), probes=n, spp=spp, r_max=r_max, ms=ms, ms_min=lo, ms_max=hi, msamples_s=n * spp / ms / 1e3)
            pvb.INNER = 1
            (cms, clo, chi), = pvb.timed([lambda: composed_depth(dev, probes, spp, 1, r_max, c)], max(2, a.reps // 2))
            emit(what="probe_depth, composed", grid=list(counts), probes=n, spp=spp, r_max=r_max, ms=cms, ms_min=clo, ms_max=chi, msamples_s=n * spp / cms / 1e3,
                 fused_speedup=cms / ms)
    pvb.INNER = inner
    # ---- eval_visible against eval with facing weights
    pts = pvb.batches(dev, desc, hrt.default_camera(W / H))
    n = W * H
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    for counts in pvb.GRIDS:
        count = counts[0] * counts[1] * counts[2]
        gen = torch.Generator(device="cuda").manual_seed(count)
        coeffs = torch.randn((count, 9, 3), device="cuda", generator=gen)
        m1 = torch.rand((count, 64), device="cuda", generator=gen) * 2 + 0.2
        sums = torch.stack([torch.ones_like(m1), m1, m1 * m1 + 0.2 * torch.rand((count, 64), device="cuda", generator=gen)], dim=2).contiguous()
        with hrt.ProbeVolume(*BOX, *counts) as vol:
            vol.update(coeffs).update_depth(sums)
            for batch, p in pts.items():
                fns = [lambda: vol.eval(p, facing=True, out=out), lambda: vol.eval_visible(p, facing=True, out=out), lambda: vol.eval_visible(p, out=out)]
                res = pvb.timed(fns, a.reps)
                for what, (ms, lo, hi) in zip(("eval, facing", "eval_visible, facing", "eval_visible"), res):
                    emit(grid=list(counts), probes=count, moments_mb=count * 512 / 1e6, batch=batch, points=n, what=what, ms=ms, ms_min=lo, ms_max=hi,
                         mpoints_s=n / ms / 1e3, over_facing=ms / res[0][0])
    # ---- quality: the floor lightmap with and without visibility
    counts, tw, spp = (16, 16, 16), 64, 1024
    grid = torch.from_numpy(hrt.probe_grid(*BOX, *counts)).cuda()
    coeffs, sums = dev.probes(grid, spp, seed=1), dev.probe_depth(grid, spp, seed=1, r_max=r_max_of(counts))
    floor = torch.from_numpy(hrt.quad_points(hrt.scene_quads(desc)[FLOOR], tw, tw)).cuda()
    baked = dev.bake(floor, spp, seed=2)
    with hrt.ProbeVolume(*BOX, *counts) as vol:
        vol.update(coeffs).update_depth(sums)
        for what, got in (("eval", vol.eval(floor)), ("eval, facing", vol.eval(floor, facing=True)), ("eval_visible", vol.eval_visible(floor)),
                          ("eval_visible, facing", vol.eval_visible(floor, facing=True))):
            emit(what="relative RMSE against bake: " + what, scene="cornell_mesh", grid=list(counts), texels=[tw, tw], spp=spp, r_max=r_max_of(counts),
                 value=float(((got - baked) ** 2).mean().sqrt() / (baked ** 2).mean().sqrt()))
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(points=n, reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
