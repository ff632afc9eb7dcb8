"""Adaptive lens frames (hrt_render_lens_adaptive_device) against uniform lens frames (hrt_render_lens_device) on one GPU, at
1920x1080, min_spp 8, max_spp 64, HIP-event timed on the current stream, linear frames (no gamma):
  cornell_mesh     the thin lens (aperture 0.2, focused on the mesh at depth 6.7)
  random_spheres   the equirectangular panorama
Per case:
  1. round machinery overhead   adaptive at threshold 0 (every tile reaches max_spp through 5 rounds: gather, lens launch, judge,
                                compact, one 4-byte read-back each) against ONE uniform launch of max_spp samples -- the same samples,
                                the same bits.  The two are alternated, `--reps` times each after a warm-up; medians and their ratio.
  2. quality per sample         a threshold found by bisection that gives a mean of about max_spp / 2 samples per pixel: its time,
                                and its RMSE against a 1024-spp uniform reference of ANOTHER seed, beside the RMSE of uniform frames
                                at max_spp and at the uniform count nearest to the adaptive mean.
One JSON line per case, the table of DESIGN.md section 5 "Adaptive lens frames", and everything in --out (default
profiles/lens_adaptive_bench.json).  There is no pass / fail bar on these figures.

  python tools/lens_adaptive_bench.py [--reps 7] [--out profiles/lens_adaptive_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MN, MX, SEED, REF_SPP, REF_SEED = 1920, 1080, 8, 64, 1, 1024, 1000
CASES = [("cornell_mesh", "thin", dict(aperture=0.2, focus=6.7)), ("random_spheres", "equirect", dict(projection="equirect"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternated timed repetitions per side (the median is reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_adaptive_bench.json"))
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    hrt = importlib.import_module("hai719-raytracing_amd")
    hrt.init(0)
    cam = hrt.default_camera(W / H)
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def rmse(x, ref):
        return float(torch.sqrt(torch.mean((x - ref) ** 2)))

    rows = []
    for scene, lname, kw in CASES:
        dev = hrt.DeviceScene(hrt.HostScene().setup(scene, W / H, 1).flatten())
        lens = hrt.Lens(cam, **kw)
        uniform = lambda spp, seed=SEED: dev.render_lens(lens, W, H, spp, seed, out=frame)
        adaptive = lambda thr: dev.render_lens_adaptive(lens, W, H, MN, MX, thr, seed=SEED, out=frame)
        mean_of = lambda counts: float(counts.to(torch.float64).mean())  # over tiles: 1080p is whole tiles

        # 1. overhead of the rounds at threshold 0
        for _ in range(2):
            uniform(MX), adaptive(0.0)
        t_uni, t_ada = [], []
        for _ in range(a.reps):
            t_uni.append(timed(lambda: uniform(MX))[0])
            t_ada.append(timed(lambda: adaptive(0.0))[0])
        uni_ms, ada_ms = float(np.median(t_uni)), float(np.median(t_ada))

        # 2. the threshold whose mean count is about max / 2 (the mean falls as the threshold rises), by bisection on its logarithm
        lo, hi = 1e-4, 10.0
        for _ in range(12):
            mid = float(np.sqrt(lo * hi))
            m = mean_of(adaptive(mid)[1])
            lo, hi = (mid, hi) if m > MX / 2 else (lo, mid)
            if abs(m - MX / 2) <= 1.0:
                break
        thr = mid
        adaptive(thr)
        t_thr = []
        for _ in range(a.reps):
            ms, (_, counts) = timed(lambda: adaptive(thr))
            t_thr.append(ms)
        mean_spp = mean_of(counts)
        hist = {int(c): int(n) for c, n in zip(*np.unique(counts.cpu().numpy(), return_counts=True))}
        ref = uniform(REF_SPP, REF_SEED).clone()
        near = max(1, int(round(mean_spp)))
        e_ada = rmse(adaptive(thr)[0], ref)
        t_near = float(np.median([timed(lambda: uniform(near))[0] for _ in range(a.reps)]))
        e_near = rmse(uniform(near), ref)
        e_max = rmse(uniform(MX), ref)
        row = dict(scene=scene, lens=lname, w=W, h=H, min_spp=MN, max_spp=MX, reps=a.reps,
                   uniform_max_ms=uni_ms, uniform_max_min_max=[min(t_uni), max(t_uni)], adaptive_thr0_ms=ada_ms, adaptive_thr0_min_max=[min(t_ada), max(t_ada)],
                   overhead_ratio=ada_ms / uni_ms, threshold=thr, mean_spp=mean_spp, counts=hist, adaptive_ms=float(np.median(t_thr)),
                   adaptive_min_max=[min(t_thr), max(t_thr)], uniform_near_spp=near, uniform_near_ms=t_near, rmse_adaptive=e_ada, rmse_uniform_near=e_near,
                   rmse_uniform_max=e_max, reference=f"{REF_SPP} spp, seed {REF_SEED}")
        print(json.dumps(row), flush=True)
        rows.append(row)
        dev.close()
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/lens_adaptive_bench.py", rows=rows), f, indent=1)
        f.write("\n")
    print("\n| scene, lens | uniform 64 spp ms | adaptive thr 0 ms | ratio | threshold | mean spp | adaptive ms | RMSE adaptive | uniform n ms | RMSE uniform n | RMSE uniform 64 |\n"
          "|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']}, {r['lens']} | {r['uniform_max_ms']:.2f} | {r['adaptive_thr0_ms']:.2f} | {r['overhead_ratio']:.3f} | {r['threshold']:.4g} | "
              f"{r['mean_spp']:.1f} | {r['adaptive_ms']:.2f} | {r['rmse_adaptive']:.5f} | {r['uniform_near_ms']:.2f} (n = {r['uniform_near_spp']}) | "
              f"{r['rmse_uniform_near']:.5f} | {r['rmse_uniform_max']:.5f} |")


if __name__ == "__main__":
    main()
