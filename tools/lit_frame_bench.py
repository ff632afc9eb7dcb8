"""Lit frames (hrt_render_lit_device, hrt_render_lit_views_device) on one GPU, HIP-event timed, in cornell_mesh against a 16 x 16 x 16
volume relit four rounds, facing weights:

  frame   a 1920 x 1080 frame through a thin lens, 1 and 16 samples, tail_after None (one segment), 1 and 2:
      fused        hrt_render_lit_device: one launch for all samples, no ray buffer
      composition  per sample hrt_lens_rays into a ray buffer, then hrt_trace_lit[_paths] of one sample into running sums (the
                   parent's kernels, unchanged) -- what a caller had before
    alternated in the same run, from the same library; the two are checked to give the same bits first
  views   64 views of 128 x 128 (an orbit of pinholes), 16 samples, tail_after None, 1 and 2: hrt_render_lit_views_device in one launch
          against 64 calls of hrt_render_lit_device, alternated

Timing is probe_volume_bench.timed: the median (min .. max) over --reps windows of back-to-back calls after two warm-up windows,
the functions alternated.  Nothing here is a threshold.

  python tools/lit_frame_bench.py [--reps 5] [--out profiles/lit_frame_bench.json]
  HRT_LIBNAME=libhrt_var_<name>.so python tools/lit_frame_bench.py --waves N --out <file>     one build of the launch-bound A/B
  python tools/lit_frame_bench.py --merge <file> <file> ... --out profiles/lit_frame_waves_ab.json
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_volume_bench as pvb  # noqa: E402

hrt = pvb.hrt
W, H, BOX = pvb.W, pvb.H, pvb.BOX
COUNTS, TAILS, SPPS = (16, 16, 16), (None, 1, 2), (1, 16)
VIEWS, VW, VH, VSPP = 64, 128, 128, 16
EF = hrt.PROBE_EVAL_FACING


def orbit(cam, degrees):
    """`cam` turned about the world's up axis through the origin."""
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    out = hrt.Camera.from_buffer_copy(cam)
    for name in ("eye", "right", "up", "forward"):
        x, z = getattr(cam, name)[0], getattr(cam, name)[2]
        getattr(out, name)[0], getattr(out, name)[2] = c * x + s * z, -s * x + c * z
    return out


def merge(files, out):
    runs = [json.load(open(f)) for f in files]
    rows = [dict(waves_per_simd=r["waves"], library=r["library"], **{k: v for k, v in row.items()}) for r in runs for row in r["rows"] if "ms" in row]
    with open(out, "w") as f:
        json.dump(dict(reps=runs[0]["reps"], device=runs[0]["device"], rows=rows), f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--waves", type=int, default=None, help="the waves per SIMD the loaded A/B build was made for (recorded, not set)")
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    hrt.init(0)
    rows = []

    def emit(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    dev = hrt.DeviceScene(hrt.HostScene().setup("cornell_mesh", W / H, 1).flatten())
    cam = hrt.default_camera(W / H)
    lens = hrt.Lens(cam, "perspective", aperture=0.05, focus=4.0)
    npix = W * H
    inner = pvb.INNER
    with hrt.ProbeVolume(*BOX, *COUNTS) as vol:
        vol.relight(dev, 1024, 4)
        # ---- the frame: fused against the composition
        fused_out, sums = torch.zeros((H, W, 3), device="cuda"), torch.zeros((npix, 3), device="cuda")

        def fused(spp, K):
            dev.render_lit(lens, vol, W, H, spp, 1, out=fused_out, accumulate=True, eval_flags=EF, tail_after=K)

        def composed(spp, K):
            for s in range(spp):
                dev.trace_lit(hrt.lens_rays(lens, W, H, s, 1), vol, 1, first_sample=s, seed=1, eval_flags=EF, out=sums, accumulate=True, tail_after=K)

        for K in TAILS:  # the same bits, before anything is timed
            fused_out.zero_(), sums.zero_()
            fused(3, K), composed(3, K)
            assert torch.equal(fused_out.view(npix, 3).view(torch.int32), sums.view(torch.int32)), K
        for spp in SPPS:
            pvb.INNER = 8 if spp == 1 else 2
            fns = [lambda K=K: fused(spp, K) for K in TAILS] + [lambda K=K: composed(spp, K) for K in TAILS]
            t = pvb.timed(fns, a.reps)
            for k, K in enumerate(TAILS):
                (fms, flo, fhi), (cms, clo, chi) = t[k], t[len(TAILS) + k]
                emit(what="frame 1920 x 1080, fused", family="hrt_lens_lit_paths_kernel" if K else "hrt_lens_lit_kernel", tail_after=K, spp=spp, ms=fms,
                     ms_min=flo, ms_max=fhi, msamples_s=npix * spp / fms / 1e3, over_composition=fms / cms)
                emit(what="frame 1920 x 1080, composition", tail_after=K, spp=spp, ms=cms, ms_min=clo, ms_max=chi, msamples_s=npix * spp / cms / 1e3)
        # ---- the batch: one launch against one call per view
        lenses = [hrt.Lens(orbit(hrt.default_camera(VW / VH), 360.0 * v / VIEWS)) for v in range(VIEWS)]
        seeds = list(range(1, VIEWS + 1))
        frames = torch.zeros((VIEWS, VH, VW, 3), device="cuda")

        def batch(K):
            dev.render_lit_views(lenses, vol, VW, VH, VSPP, seeds, out=frames, eval_flags=EF, tail_after=K)

        def singles(K):
            for v in range(VIEWS):
                dev.render_lit(lenses[v], vol, VW, VH, VSPP, seeds[v], out=frames[v], eval_flags=EF, tail_after=K)

        pvb.INNER = 2
        vt = TAILS
        t = pvb.timed([lambda K=K: batch(K) for K in vt] + [lambda K=K: singles(K) for K in vt], a.reps)
        items = VIEWS * VW * VH * VSPP
        for k, K in enumerate(vt):
            (bms, blo, bhi), (sms, slo, shi) = t[k], t[len(vt) + k]
            emit(what="64 views of 128 x 128, one launch", family="hrt_lens_views_lit_paths_kernel" if K else "hrt_lens_views_lit_kernel", tail_after=K,
                 spp=VSPP, ms=bms, ms_min=blo, ms_max=bhi, msamples_s=items / bms / 1e3, over_single_calls=bms / sms)
            emit(what="64 views of 128 x 128, 64 single calls", tail_after=K, spp=VSPP, ms=sms, ms_min=slo, ms_max=shi, msamples_s=items / sms / 1e3)
    pvb.INNER = inner
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(reps=a.reps, device=torch.cuda.get_device_name(0), library=os.environ.get("HRT_LIBNAME", "libhrt.so"), waves=a.waves, rows=rows),
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
