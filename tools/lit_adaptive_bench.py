"""Adaptive lit frames (hrt_render_lit_adaptive_device) on one GPU, HIP-event timed, in cornell_mesh against a 16 x 16 x 16 volume
relit four rounds: a 1920 x 1080 frame through a thin lens, min / max 4 / 64 samples, at the threshold (found by bisection) that
gives a mean of about 12 samples per pixel; tail_after None (one segment) and 1.

Per tail: the adaptive frame's time, its mean count and the distribution of its tile counts, its RMSE against hrt_render_lit at 1024
samples -- beside uniform hrt_render_lit_device at the nearest equal count, timed in the same run, alternated, and its RMSE.
The rounds that add 16 and 32 samples (where the lanes of a fused path kernel drift apart over a launch's samples) are reported
separately, by difference: the same threshold with max_spp 16, 32 and 64 runs the same rounds up to that count, so the time of
max 32 minus max 16 is the round that adds 16 samples to the tiles still active at 16, and max 64 minus max 32 the one that adds 32.

Timing is probe_volume_bench.timed: the median (min .. max) over --reps windows of back-to-back calls after two warm-up windows,
the functions alternated.  Nothing here is a threshold.

  python tools/lit_adaptive_bench.py [--reps 5] [--out profiles/lit_adaptive_bench.json]
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
W, H, BOX = pvb.W, pvb.H, pvb.BOX
COUNTS, TAILS, MN, MX, MEAN = (16, 16, 16), (None, 1), 4, 64, 12.0
EF = hrt.PROBE_EVAL_FACING


def rmse(a, b):
    return float(((a - b) ** 2).mean().sqrt())


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
    lens = hrt.Lens(hrt.default_camera(W / H), "perspective", aperture=0.05, focus=4.0)
    npix = W * H
    inner = pvb.INNER
    pvb.INNER = 2
    with hrt.ProbeVolume(*BOX, *COUNTS) as vol:
        vol.relight(dev, 1024, 4)
        frame, flat = torch.zeros((H, W, 3), device="cuda"), torch.zeros((H, W, 3), device="cuda")
        for K in TAILS:
            kw = dict(eval_flags=EF, tail_after=K)

            def mean_of(thr, mx=MX):
                _, counts = dev.render_lit_adaptive(lens, vol, W, H, MN, mx, thr, seed=1, out=frame, **kw)
                torch.cuda.synchronize()
                c = counts.cpu().numpy().astype(np.uint32)
                pp = np.repeat(np.repeat(c, 8, axis=0), 8, axis=1)[:H, :W]
                return float(pp.mean()), c

            lo, hi = 1e-6, 10.0  # the mean count falls as the threshold rises: bisect in the logarithm
            for _ in range(24):
                thr = float(np.sqrt(lo * hi))
                m, _ = mean_of(thr)
                lo, hi = (thr, hi) if m > MEAN else (lo, thr)
            thr = float(np.sqrt(lo * hi))
            mean, counts = mean_of(thr)
            uni = max(1, int(round(mean)))
            ref = dev.render_lit(lens, vol, W, H, 1024, 2, out=torch.zeros((H, W, 3), device="cuda"), **kw).clone()
            fns = [lambda mx=mx: dev.render_lit_adaptive(lens, vol, W, H, MN, mx, thr, seed=1, out=frame, **kw) for mx in (16, 32, MX)]
            fns.append(lambda: dev.render_lit(lens, vol, W, H, uni, 1, out=flat, **kw))
            fns += [lambda n=n: dev.render_lit(lens, vol, W, H, n, 1, out=flat, **kw) for n in (16, 32)]
            t = pvb.timed(fns, a.reps)
            fns[2]()
            fns[3]()
            torch.cuda.synchronize()
            (ams, alo, ahi), (ums, ulo, uhi) = t[2], t[3]
            hist = {int(c): int(k) for c, k in zip(*np.unique(counts, return_counts=True))}
            emit(what="1920 x 1080 adaptive lit frame, 4 .. 64 samples", tail_after=K, threshold=thr, mean_spp=mean, tile_counts=hist, ms=ams, ms_min=alo,
                 ms_max=ahi, msamples_s=npix * mean / ams / 1e3, rmse_against_1024=rmse(frame, ref), over_uniform=ams / ums)
            emit(what="1920 x 1080 uniform lit frame at the nearest equal count", tail_after=K, spp=uni, ms=ums, ms_min=ulo, ms_max=uhi,
                 msamples_s=npix * uni / ums / 1e3, rmse_against_1024=rmse(flat, ref))
            for (mx_lo, k_lo), (mx_hi, k_hi), add, uk in (((16, 0), (32, 1), 16, 4), ((32, 1), (64, 2), 32, 5)):
                active = int(sum(v for c, v in hist.items() if c > mx_lo))
                ms = t[k_hi][0] - t[k_lo][0]
                emit(what=f"the round that adds {add} samples (max_spp {mx_hi} minus max_spp {mx_lo}, by difference of medians)", tail_after=K,
                     active_tiles=active, ms=ms, msamples_s=(active * 64 * add / ms / 1e3) if ms > 0 else None,
                     uniform_frame_ms_at_that_count=t[uk][0], uniform_msamples_s=npix * add / t[uk][0] / 1e3)
    pvb.INNER = inner
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(reps=a.reps, device=torch.cuda.get_device_name(0), library=os.environ.get("HRT_LIBNAME", "libhrt.so"), rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
