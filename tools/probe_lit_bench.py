"""Lit rays and probe relighting (hrt_probes_lit_device, hrt_trace_lit) on one GPU, HIP-event timed, in cornell_mesh:

  probes_lit   8 x 8 x 8 and 16 x 16 x 16 grids at 256 and 1024 samples per probe, against a volume of the same grid that holds one
               round of light, three ways:
      fused        hrt_probes_lit_device
      composed     what a caller had before: per sample hrt_probe_rays + hrt_trace_rays(shade) + hrt_probe_eval_device, then
                   emission / 6 + albedo x G and the SH fold in torch (no direct light: cornell_mesh has no lights); the
                   largest difference from the fused coefficients is reported
      probes       hrt_probes_device at the same counts from the same library: whole paths of up to six segments
  frame        hrt_trace_lit on the camera rays of one sample of a 1920 x 1080 frame (facing weights, with and without visibility)
               against hrt_trace_rays(shade) + hrt_probe_eval(_visible)_device on the same rays
  convergence  the floor-lightmap experiment of tools/probe_volume_bench.py (a 16 x 16 x 16 grid at 1024 samples against scene.bake
               of the 64 x 64 floor texels): the relative RMSE after 1 .. 8 rounds of relighting, beside that of the path-traced
               volume; no threshold

Timing is probe_volume_bench.timed: the median (min .. max) over --reps windows of back-to-back calls after two warm-up windows,
the functions alternated.

  python tools/probe_lit_bench.py [--reps 5] [--out profiles/probe_lit_bench.json]
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
GRIDS = ((8, 8, 8), (16, 16, 16))
SAMPLES = (256, 1024)
Y = (0.2820948, 0.48860251, 1.0925485, 0.31539157, 0.54627422)


def basis(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return torch.stack([torch.full_like(x, Y[0]), Y[1] * y, Y[1] * z, Y[1] * x, Y[2] * (x * y), Y[2] * (y * z), Y[3] * (3 * z * z - 1), Y[2] * (x * z),
                        Y[4] * (x * x - y * y)], dim=1)


def composed_value(dev, vol, rays, facing=False, visible=False, out=None):
    """emission / 6 + albedo x G of rays from hrt_trace_rays(shade) and the volume's look-up: (n, 3)."""
    rec = dev.trace_rays(rays, "shade")
    pts = torch.cat([rays[:, 0:3] + rec[:, 0:1] * rays[:, 4:7], rays[:, 3:4], rec[:, 4:7], torch.zeros_like(rec[:, 0:1])], dim=1)
    G = (vol.eval_visible if visible else vol.eval)(pts, facing=facing, out=out)
    diffuse = (rec[:, hrt.HIT_KIND].view(torch.int32) != 0) & (rec[:, hrt.SHADE_MATERIAL_TYPE].view(torch.int32) == 0)
    return rec[:, 12:15] / 6 + rec[:, 8:11] * torch.where(diffuse[:, None], G, torch.zeros_like(G))


def composed_probes(dev, vol, probes, spp, seed):
    """The coefficients from per-sample launches and a torch fold: (n, 9, 3).  Misses add the sky, which cornell_mesh's closed room
    never shows to a probe inside it."""
    out = torch.zeros((probes.shape[0], 9, 3), device="cuda")
    for s in range(spp):
        rays = hrt.probe_rays(probes, s, seed)
        out += basis(rays[:, 4:7])[:, :, None] * composed_value(dev, vol, rays)[:, None, :]
    return out / spp


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
    inner = pvb.INNER
    # ---- probes_lit: fused, composed, and whole paths
    for counts in GRIDS:
        probes = torch.from_numpy(hrt.probe_grid(*BOX, *counts)).cuda()
        n = probes.shape[0]
        out = torch.empty((n, 9, 3), device="cuda")
        with hrt.ProbeVolume(*BOX, *counts) as vol:
            vol.relight(dev, 256, 1)
            for spp in SAMPLES:
                got, ref = dev.probes_lit(probes, vol, spp, seed=1), composed_probes(dev, vol, probes, spp, 1)
                err = float((ref - got).abs().max() / got.abs().max())
                emit(what="max |composed - fused| / max |fused|", grid=list(counts), spp=spp, value=err)
                pvb.INNER = 4  # a fused call is milliseconds and a composed one thousands of launches: short windows
                (ms, lo, hi), (pms, plo, phi) = pvb.timed([lambda: dev.probes_lit(probes, vol, spp, seed=1, out=out),
                                                          lambda: dev.probes(probes, spp, seed=1, out=out)], a.reps)
                emit(what="probes_lit, fused", grid=list(counts), probes=n, spp=spp, ms=ms, ms_min=lo, ms_max=hi, msamples_s=n * spp / ms / 1e3)
                emit(what="probes (whole paths)", grid=list(counts), probes=n, spp=spp, ms=pms, ms_min=plo, ms_max=phi, msamples_s=n * spp / pms / 1e3,
                     over_probes_lit=pms / ms)
                pvb.INNER = 1
                (cms, clo, chi), = pvb.timed([lambda: composed_probes(dev, vol, probes, spp, 1)], max(2, a.reps // 2))
                emit(what="probes_lit, composed", grid=list(counts), probes=n, spp=spp, ms=cms, ms_min=clo, ms_max=chi, msamples_s=n * spp / cms / 1e3,
                     fused_speedup=cms / ms, ms_per_sample=cms / spp)
    pvb.INNER = inner
    # ---- the camera frame: one sample of 1080p
    cam = hrt.default_camera(W / H)
    rays = hrt.camera_rays(cam, W, H, 0, 1)
    npix = W * H
    out, scratch = torch.empty((npix, 3), device="cuda"), torch.empty((npix, 3), device="cuda")
    counts = (16, 16, 16)
    grid = torch.from_numpy(hrt.probe_grid(*BOX, *counts)).cuda()
    e = [(hi - lo) / c for lo, hi, c in zip(BOX[0], BOX[1], counts)]
    r_max = 1.5 * float(np.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2))
    with hrt.ProbeVolume(*BOX, *counts) as vol:
        vol.relight(dev, 1024, 4, depth_rmax=r_max)
        for visible in (False, True):
            ef = hrt.PROBE_EVAL_FACING | (hrt.LIT_VISIBLE if visible else 0)
            got, ref = dev.trace_lit(rays, vol, 1, eval_flags=ef), composed_value(dev, vol, rays, True, visible)
            err = float((ref - got).abs().max() / got.abs().max())
            emit(what="frame: max |composed - fused| / max |fused|", visible=visible, value=err)
            (ms, lo, hi), (cms, clo, chi) = pvb.timed([lambda: dev.trace_lit(rays, vol, 1, eval_flags=ef, out=out),
                                                      lambda: composed_value(dev, vol, rays, True, visible, out=scratch)], a.reps)
            emit(what="frame 1920 x 1080, trace_lit", visible=visible, rays=npix, ms=ms, ms_min=lo, ms_max=hi, mrays_s=npix / ms / 1e3)
            emit(what="frame 1920 x 1080, trace_rays(shade) + eval", visible=visible, rays=npix, ms=cms, ms_min=clo, ms_max=chi, mrays_s=npix / cms / 1e3,
                 fused_speedup=cms / ms)
    # ---- convergence: the floor lightmap after 1 .. 8 rounds
    tw, spp = 64, 1024
    floor = torch.from_numpy(hrt.quad_points(hrt.scene_quads(desc)[FLOOR], tw, tw)).cuda()
    baked = dev.bake(floor, spp, seed=2)
    rmse = lambda got: float(((got - baked) ** 2).mean().sqrt() / (baked ** 2).mean().sqrt())
    with hrt.ProbeVolume(*BOX, *counts) as vol:
        vol.update(dev.probes(grid, spp, seed=1))
        emit(what="relative RMSE against bake: path-traced volume", scene="cornell_mesh", grid=list(counts), texels=[tw, tw], spp=spp, value=rmse(vol.eval(floor)))
    with hrt.ProbeVolume(*BOX, *counts) as vol:
        vol.relight(dev, spp, 0)
        for k in range(1, 9):  # one more round on the volume as it stands, with that round's samples
            vol.update(dev.probes_lit(grid, vol, spp, first_sample=(k - 1) * spp, seed=1))
            emit(what="relative RMSE against bake: relit volume", rounds=k, scene="cornell_mesh", grid=list(counts), texels=[tw, tw], spp=spp,
                 value=rmse(vol.eval(floor)))
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
