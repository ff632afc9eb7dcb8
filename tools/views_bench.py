"""Many small frames of one scene on one GPU: 64 views of 128 x 128 pixels, as
  views        one hrt_render_views_device call (frames stay on the device)
  views_host   one hrt_render_views call (blocking, frames copied to the host)
  tiles_loop   64 hrt_render_tiles calls on one stream, then one synchronise (tile-major sums stay on the device): the best there
               was before batched views
  render_loop  64 blocking hrt_render calls (each copies its frame to the host)
and one 1024 x 1024 frame (the same number of pixels) with hrt_render_tiles as the ceiling.  Every variant is timed with the host
clock around work that ends in a stream synchronise (wall_ms: what the caller waits) and, for the asynchronous ones, with events on
the stream (event_ms); medians over --reps runs after two warm-up runs, the variants of a configuration alternating.  One JSON line
per (scene, spp, variant); a table at the end.

  python tools/views_bench.py [--scenes cornell_mesh random_spheres] [--spp 4 64] [--views 64] [--size 128] [--reps 9]
"""
import argparse
import importlib
import json
import os
import sys
import time

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
    hrt.init(0)
    n, w = a.views, a.size
    big = int(round((n * w * w) ** 0.5))  # one frame of the same pixel count (1024 for 64 x 128 x 128)
    rows = []
    for name in a.scenes:
        dev = hrt.DeviceScene(hrt.HostScene().setup(name, 1.0, 1).flatten())
        cam0 = hrt.default_camera(1.0)
        cams = [orbit(cam0, 360.0 * v / n) for v in range(n)]
        seeds = list(range(1, n + 1))
        stream = torch.cuda.current_stream()
        frames = torch.empty((n, w, w, 3), dtype=torch.float32, device="cuda")
        tiles = torch.empty((n, hrt.tiles_total(w, w), 64, 3), dtype=torch.float32, device="cuda")
        big_tiles = torch.empty((hrt.tiles_total(big, big), 64, 3), dtype=torch.float32, device="cuda")
        for spp in a.spp:
            def tiles_loop():
                for v in range(n):
                    dev.render_tiles(cams[v], w, w, spp, seeds[v], 0, 0, 1, tiles[v].data_ptr(), stream.cuda_stream)

            def render_loop():
                for v in range(n):
                    dev.render(cams[v], w, w, spp, seeds[v])

            variants = [("views", lambda: dev.render_views(cams, w, w, spp, seeds=seeds, out=frames), True, n * w * w),
                        ("views_host", lambda: dev.render_views(cams, w, w, spp, seeds=seeds), False, n * w * w),
                        ("tiles_loop", tiles_loop, True, n * w * w),
                        ("render_loop", render_loop, False, n * w * w),
                        (f"one_frame_{big}", lambda: dev.render_tiles(cam0, big, big, spp, 1, 0, 0, 1, big_tiles.data_ptr(), stream.cuda_stream), True, big * big)]
            wall = {k: [] for k, _, _, _ in variants}
            event = {k: [] for k, _, _, _ in variants}
            for rep in range(a.reps + 2):  # two warm-up rounds; the variants alternate within a round
                for k, fn, on_stream, _ in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    t0 = time.perf_counter()
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    stream.synchronize()
                    t1 = time.perf_counter()
                    dev.check_last_launch()
                    if rep >= 2:
                        wall[k].append((t1 - t0) * 1e3)
                        if on_stream:
                            event[k].append(e0.elapsed_time(e1))
            for k, _, on_stream, pixels in variants:
                wms = float(np.median(wall[k]))
                r = dict(scene=name, spp=spp, variant=k, pixels=pixels, wall_ms=wms, wall_ms_min=float(min(wall[k])), wall_ms_max=float(max(wall[k])),
                         event_ms=float(np.median(event[k])) if on_stream else None, msamples_s=pixels * spp / wms / 1e3)
                rows.append(r)
                print(json.dumps(r), flush=True)
        dev.close()
    print("\n| scene | spp | variant | wall ms (min..max) | event ms | Msamples/s (wall) |\n|---|---|---|---|---|---|")
    for r in rows:
        ev = "-" if r["event_ms"] is None else f"{r['event_ms']:.3f}"
        print(f"| {r['scene']} | {r['spp']} | {r['variant']} | {r['wall_ms']:.3f} ({r['wall_ms_min']:.3f}..{r['wall_ms_max']:.3f}) | {ev} | {r['msamples_s']:.0f} |")


if __name__ == "__main__":
    main()
