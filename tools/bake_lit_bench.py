"""Lit bakes (hrt_bake_lit_device) on one GPU, HIP-event timed, in cornell_mesh against a 16 x 16 x 16 volume relit four rounds: the
floor lightmap at 64 x 64 and at 512 x 512 texels, 16, 64 and 256 samples, tail_after None (one segment), 1 and 2:

  fused        hrt_bake_lit_device: one launch for all samples, no ray buffer
  composition  per sample hrt_bake_rays into a ray buffer, then hrt_trace_lit[_paths] of one sample into running sums (the parent's
               kernels, unchanged) -- what a caller had before; checked to give the same bits before anything is timed
  bake         hrt_bake_device at the same count: whole paths, no volume
alternated in the same run, from the same library.

Then the quality experiment of "Probe volumes": the relative RMSE of the 64 x 64 floor against hrt_bake at 1024 samples for
ProbeVolume.eval, for bake_lit at 16 / 64 / 256 samples per tail, and for bake at the same counts under another seed.

Timing is probe_volume_bench.timed: the median (min .. max) over --reps windows of back-to-back calls after two warm-up windows,
the functions alternated.  Nothing here is a threshold.

  python tools/bake_lit_bench.py [--reps 5] [--out profiles/bake_lit_bench.json]
  HRT_LIBNAME=libhrt_var_<name>.so python tools/bake_lit_bench.py --waves N --out <file>     one build of the launch-bound A/B
  python tools/bake_lit_bench.py --merge <file> <file> ... --out profiles/bake_lit_waves_ab.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_volume_bench as pvb  # noqa: E402

hrt = pvb.hrt
BOX, FLOOR = pvb.BOX, pvb.FLOOR
COUNTS, TAILS, SPPS, SIDES = (16, 16, 16), (None, 1, 2), (16, 64, 256), (64, 512)


def rel_rmse(got, ref):
    return float(((got - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--waves", type=int, default=None, help="the waves per SIMD the loaded A/B build was made for (recorded, not set): 512 x 512 only, no quality")
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    if a.merge:
        runs = [json.load(open(f)) for f in a.merge]
        merged = [dict(waves_per_simd=r["waves"], library=r["library"], **row) for r in runs for row in r["rows"] if row.get("family")]
        with open(a.out, "w") as f:
            json.dump(dict(reps=runs[0]["reps"], device=runs[0]["device"], rows=merged), f, indent=1)
            f.write("\n")
        return
    hrt.init(0)
    rows = []

    def emit(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    desc = hrt.HostScene().setup("cornell_mesh", pvb.W / pvb.H, 1).flatten()
    dev = hrt.DeviceScene(desc)
    floor = hrt.scene_quads(desc)[FLOOR]
    inner = pvb.INNER
    with hrt.ProbeVolume(*BOX, *COUNTS) as vol:
        vol.relight(dev, 1024, 4)
        for side in (SIDES if a.waves is None else SIDES[-1:]):
            pts = torch.from_numpy(hrt.quad_points(floor, side, side)).cuda()
            n = side * side
            fused_out, sums, baked = (torch.zeros((n, 3), device="cuda") for _ in range(3))

            def fused(spp, K):
                dev.bake_lit(pts, vol, spp, seed=1, out=fused_out, accumulate=True, tail_after=K)

            def composed(spp, K):
                for s in range(spp):
                    dev.trace_lit(hrt.bake_rays(pts, s, 1), vol, 1, first_sample=s, seed=1, out=sums, accumulate=True, tail_after=K)

            def bake(spp):
                dev.bake(pts, spp, seed=1, out=baked)

            for K in TAILS:  # the same bits, before anything is timed
                fused_out.zero_(), sums.zero_()
                fused(3, K), composed(3, K)
                assert torch.equal(fused_out.view(torch.int32), sums.view(torch.int32)), (side, K)
            for spp in SPPS:
                pvb.INNER = 1 if n * spp >= 2 ** 22 else 4
                fns = [lambda K=K: fused(spp, K) for K in TAILS] + [lambda K=K: composed(spp, K) for K in TAILS] + [lambda: bake(spp)]
                t = pvb.timed(fns, a.reps)
                bms, blo, bhi = t[-1]
                emit(what=f"floor {side} x {side}, bake", spp=spp, ms=bms, ms_min=blo, ms_max=bhi, msamples_s=n * spp / bms / 1e3)
                for k, K in enumerate(TAILS):
                    (fms, flo, fhi), (cms, clo, chi) = t[k], t[len(TAILS) + k]
                    emit(what=f"floor {side} x {side}, fused", family="hrt_bake_lit_paths_kernel" if K else "hrt_bake_lit_kernel", tail_after=K, spp=spp,
                         ms=fms, ms_min=flo, ms_max=fhi, msamples_s=n * spp / fms / 1e3, over_composition=fms / cms, over_bake=fms / bms)
                    emit(what=f"floor {side} x {side}, composition", tail_after=K, spp=spp, ms=cms, ms_min=clo, ms_max=chi, msamples_s=n * spp / cms / 1e3)
        # ---- quality: the 64 x 64 floor against bake at 1024 samples
        pts = torch.from_numpy(hrt.quad_points(floor, 64, 64)).cuda()
        ref = dev.bake(pts, 1024, seed=2)
        emit(what="relative RMSE against bake at 1024 samples: volume.eval", value=rel_rmse(vol.eval(pts), ref))
        emit(what="relative RMSE against bake at 1024 samples: volume.eval, facing", value=rel_rmse(vol.eval(pts, facing=True), ref))
        for spp in (SPPS if a.waves is None else ()):  # an A/B build is timed only
            emit(what="relative RMSE against bake at 1024 samples: bake under another seed", spp=spp, value=rel_rmse(dev.bake(pts, spp, seed=3), ref))
            for K in TAILS:
                emit(what="relative RMSE against bake at 1024 samples: bake_lit", tail_after=K, spp=spp,
                     value=rel_rmse(dev.bake_lit(pts, vol, spp, seed=3, tail_after=K), ref))
    pvb.INNER = inner
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(reps=a.reps, device=torch.cuda.get_device_name(0), library=os.environ.get("HRT_LIBNAME", "libhrt.so"), waves=a.waves, rows=rows),
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
