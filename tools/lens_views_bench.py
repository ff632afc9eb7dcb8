"""Many small lens frames of one scene on one GPU: 64 views of 128 x 128 pixels, all equirectangular or all thin-lens, as
  batch          one hrt_render_lens_views_device call (frames stay on the device)
  lens_loop      64 hrt_render_lens_device calls on one stream: what there was before batched lens views.  Its kernels are the
                 ones the batch leaves instruction-identical, so it is the baseline
  pinhole_views  the same cameras as pinholes through one hrt_render_views_device call (the trace kernels' batch), for scale
Every variant is timed with events on the stream around work that ends in a stream synchronise; medians over --reps runs (at
least five) after two warm-up runs, the variants of a configuration alternating; the spread is min..max of the runs.  One JSON line
per (scene, lens, spp, variant); a table at the end.

No speed threshold is fixed in advance: the batch is expected not to be slower than the loop by more than the loop's own spread
(max - min of its runs).  The tool exits with status 1 if some configuration is.

  python tools/lens_views_bench.py [--scenes cornell_mesh random_spheres] [--spp 4 64] [--views 64] [--size 128] [--reps 9]
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


def orbit(cam, degrees):
    a = np.radians(degrees)
    c, s = np.cos(a), np.sin(a)
    out = hrt.Camera()
    for name in ("eye", "right", "up", "forward"):
        x, y, z = getattr(cam, name)
        getattr(out, name)[:] = (c * x + s * z, y, -s * x + c * z)
    out.fovy_deg, out.aspect, out.znear, out.zfar = cam.fovy_deg, cam.aspect, cam.znear, cam.zfar
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_mesh", "random_spheres"])
    ap.add_argument("--spp", nargs="+", type=int, default=[4, 64])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    hrt.init(0)
    n, w = a.views, a.size
    rows, slower = [], []
    for name in a.scenes:
        dev = hrt.DeviceScene(hrt.HostScene().setup(name, 1.0, 1).flatten())
        cam0 = hrt.default_camera(1.0)
        cams = [orbit(cam0, 360.0 * v / n) for v in range(n)]
        seeds = list(range(1, n + 1))
        stream = torch.cuda.current_stream()
        frames = torch.empty((n, w, w, 3), dtype=torch.float32, device="cuda")
        for lens_name, make in (("equirect", lambda c: hrt.Lens(c, "equirect")), ("thin", lambda c: hrt.Lens(c, aperture=0.1, focus=4.0))):
            lenses = [make(c) for c in cams]
            for spp in a.spp:
                def lens_loop():
                    for v in range(n):
                        dev.render_lens(lenses[v], w, w, spp, seeds[v], out=frames[v])

                variants = [("batch", lambda: dev.render_lens_views(lenses, w, w, spp, seeds, out=frames)),
                            ("lens_loop", lens_loop),
                            ("pinhole_views", lambda: dev.render_views(cams, w, w, spp, seeds=seeds, out=frames))]
                ms = {k: [] for k, _ in variants}
                for rep in range(a.reps + 2):  # two warm-up rounds; the variants alternate within a round
                    for k, fn in variants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        stream.synchronize()
                        e0.record(stream)
                        fn()
                        e1.record(stream)
                        stream.synchronize()
                        dev.check_last_launch()
                        if rep >= 2:
                            ms[k].append(e0.elapsed_time(e1))
                for k, _ in variants:
                    med = float(np.median(ms[k]))
                    r = dict(scene=name, lens=lens_name, spp=spp, variant=k, views=n, size=w, event_ms=med, event_ms_min=float(min(ms[k])),
                             event_ms_max=float(max(ms[k])), msamples_s=n * w * w * spp / med / 1e3)
                    rows.append(r)
                    print(json.dumps(r), flush=True)
                loop_spread = max(ms["lens_loop"]) - min(ms["lens_loop"])
                if np.median(ms["batch"]) > np.median(ms["lens_loop"]) + loop_spread:
                    slower.append(f"{name} {lens_name} {spp} spp: batch {np.median(ms['batch']):.3f} ms, loop {np.median(ms['lens_loop']):.3f} ms "
                                  f"with a spread of {loop_spread:.3f} ms")
        dev.close()
    print("\n| scene | lens | spp | variant | event ms (min..max) | Msamples/s |\n|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['lens']} | {r['spp']} | {r['variant']} | {r['event_ms']:.3f} ({r['event_ms_min']:.3f}..{r['event_ms_max']:.3f}) | {r['msamples_s']:.0f} |")
    for s in slower:
        print("SLOWER THAN THE LOOP BY MORE THAN ITS SPREAD: " + s)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
