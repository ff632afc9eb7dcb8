"""Lit paths (hrt_probes_lit_paths_device, hrt_trace_lit_paths) on one GPU, HIP-event timed, in cornell_mesh:

  probes_lit   a 16 x 16 x 16 grid at 1024 samples per probe against a volume of the same grid that holds one round of light:
      tail_after 1, 2, 3   hrt_probes_lit_paths_device: paths that follow mirror and glass and end in the volume at their K-th
                           diffuse hit
      one segment          hrt_probes_lit_device: what a caller has without a tail (the parent's kernel, unchanged)
      whole paths          hrt_probes_device at the same counts (the parent's kernel, unchanged)
    all five alternated in the same run, from the same library
  frame        hrt_trace_lit_paths(tail_after = 1) on the camera rays of one sample of a 1920 x 1080 frame (facing weights) against
               hrt_trace_lit on the same rays, alternated; the share of pixels the two differ on is reported (the pixels that see
               mirror or glass first)

Timing is probe_volume_bench.timed: the median (min .. max) over --reps windows of back-to-back calls after two warm-up windows,
the functions alternated.  Nothing here is a threshold.

  python tools/probe_lit_paths_bench.py [--reps 5] [--out profiles/probe_lit_paths_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_volume_bench as pvb  # noqa: E402

hrt = pvb.hrt
W, H, BOX = pvb.W, pvb.H, pvb.BOX
COUNTS, SPP, TAILS = (16, 16, 16), 1024, (1, 2, 3)


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

    dev = hrt.DeviceScene(hrt.HostScene().setup("cornell_mesh", W / H, 1).flatten())
    inner = pvb.INNER
    # ---- the fused update: K diffuse hits, one segment, whole paths
    probes = torch.from_numpy(hrt.probe_grid(*BOX, *COUNTS)).cuda()
    n = probes.shape[0]
    out = torch.empty((n, 9, 3), device="cuda")
    with hrt.ProbeVolume(*BOX, *COUNTS) as vol:
        vol.relight(dev, 256, 1)
        pvb.INNER = 4
        fns = [lambda K=K: dev.probes_lit(probes, vol, SPP, seed=1, out=out, tail_after=K) for K in TAILS]
        fns += [lambda: dev.probes_lit(probes, vol, SPP, seed=1, out=out), lambda: dev.probes(probes, SPP, seed=1, out=out)]
        t = pvb.timed(fns, a.reps)
        (sms, slo, shi), (pms, plo, phi) = t[len(TAILS)], t[len(TAILS) + 1]
        emit(what="probes_lit, one segment", grid=list(COUNTS), probes=n, spp=SPP, ms=sms, ms_min=slo, ms_max=shi, msamples_s=n * SPP / sms / 1e3)
        emit(what="probes (whole paths)", grid=list(COUNTS), probes=n, spp=SPP, ms=pms, ms_min=plo, ms_max=phi, msamples_s=n * SPP / pms / 1e3)
        for K, (ms, lo, hi) in zip(TAILS, t):
            emit(what="probes_lit, tail_after", tail_after=K, grid=list(COUNTS), probes=n, spp=SPP, ms=ms, ms_min=lo, ms_max=hi,
                 msamples_s=n * SPP / ms / 1e3, over_one_segment=ms / sms, over_whole_paths=ms / pms)
    pvb.INNER = inner
    # ---- the camera frame: one sample of 1080p
    rays = hrt.camera_rays(hrt.default_camera(W / H), W, H, 0, 1)
    npix = W * H
    out = torch.empty((npix, 3), device="cuda")
    ef = hrt.PROBE_EVAL_FACING
    with hrt.ProbeVolume(*BOX, *COUNTS) as vol:
        vol.relight(dev, 1024, 4)
        one, tail = dev.trace_lit(rays, vol, 1, eval_flags=ef), dev.trace_lit(rays, vol, 1, eval_flags=ef, tail_after=1)
        differ = float((one.view(torch.int32) != tail.view(torch.int32)).any(dim=1).float().mean())
        emit(what="frame: share of pixels where tail_after = 1 differs from one segment", value=differ)
        (ms, lo, hi), (oms, olo, ohi) = pvb.timed([lambda: dev.trace_lit(rays, vol, 1, eval_flags=ef, out=out, tail_after=1),
                                                  lambda: dev.trace_lit(rays, vol, 1, eval_flags=ef, out=out)], a.reps)
        emit(what="frame 1920 x 1080, trace_lit, one segment", rays=npix, ms=oms, ms_min=olo, ms_max=ohi, mrays_s=npix / oms / 1e3)
        emit(what="frame 1920 x 1080, trace_lit, tail_after = 1", rays=npix, ms=ms, ms_min=lo, ms_max=hi, mrays_s=npix / ms / 1e3, over_one_segment=ms / oms)
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
