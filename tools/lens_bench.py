"""Frame time of the lens cameras (hrt_render_lens_device) on one GPU, HIP-event timed, at 1920x1080 with 16 samples per pixel:
  fused       the pinhole through the fused kernel (aperture 0): one launch, no ray buffer
  composed    what it replaces: per sample hrt_camera_rays + hrt_trace_radiance(n_samples = 1, HRT_RADIANCE_ACCUMULATE), 32 launches
              and a w*h*32-byte ray buffer -- run on ANOTHER checkout of the project, built (--baseline-root, e.g. the parent
              commit's), alternated with `fused` on the same card: each repetition is one child process per side (a process loads
              one library), so the two sides see the same drift.  Its event pair also covers the zero fill of the sums and the 16
              allocations of the ray buffer (torch's caching allocator: no device call after the warm-ups) -- what a caller of the
              composition pays, and a small bias in favour of `fused`
  render      hrt_render_tiles with HRT_FLAG_WAVE_KERNEL, for scale
  dof         fused with aperture 0.1, focus 4
  equirect    fused equirectangular panorama
Every child runs under its own timeout and the run stops at the first child that fails.  One JSON line per measurement, then per
scene: the medians, the run-to-run spread of `composed` (max - min over the repetitions), and whether fused <= composed + spread.

  python tools/lens_bench.py --baseline-root ../parent-checkout [--scenes cornell_mesh backrooms_pool random_spheres] [--reps 5]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, SEED = 1920, 1080, 16, 1


def child(scene, what, launches):
    import torch
    sys.path.insert(0, os.environ.get("LENS_BENCH_ROOT", ROOT))
    hrt = importlib.import_module("hai719-raytracing_amd")
    hrt.init(0)
    dev = hrt.DeviceScene(hrt.HostScene().setup(scene, W / H, 1).flatten())
    cam = hrt.default_camera(W / H)
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")

    def fused(lens):
        return lambda: dev.render_lens(lens, W, H, SPP, SEED, out=frame)

    def composed():
        acc = frame.view(W * H, 3)
        acc.zero_()
        for s in range(SPP):
            dev.trace_radiance(hrt.camera_rays(cam, W, H, s, SEED), spp=1, first_sample=s, seed=SEED, out=acc, accumulate=True)

    def render():
        tiles = torch.empty((hrt.tiles_total(W, H), 64, 3), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        return lambda: dev.render_tiles(cam, W, H, SPP, SEED, hrt.FLAG_WAVE_KERNEL, 0, 1, tiles.data_ptr(), stream)

    for name in what:
        fn = {"fused": lambda: fused(hrt.Lens(cam)), "composed": lambda: composed, "render": render,
              "dof": lambda: fused(hrt.Lens(cam, aperture=0.1, focus=4.0)), "equirect": lambda: fused(hrt.Lens(cam, "equirect"))}[name]()
        for _ in range(2):
            fn()
        times = []
        for _ in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        ms = float(np.median(times))
        print(json.dumps(dict(scene=scene, what=name, ms=ms, msamples_s=W * H * SPP / ms / 1e3, root=os.path.dirname(os.path.dirname(hrt.__file__)))), flush=True)
    if "render" in what:
        dev.check_last_launch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_mesh", "backrooms_pool", "random_spheres"])
    ap.add_argument("--reps", type=int, default=5, help="alternated repetitions of composed / fused")
    ap.add_argument("--launches", type=int, default=5, help="timed launches per measurement (the median is reported)")
    ap.add_argument("--baseline-root", required=True, help="root of the built checkout `composed` runs on")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1:], a.launches)

    def run(scene, what, root=None):
        env = dict(os.environ)
        if root:
            env["LENS_BENCH_ROOT"] = os.path.abspath(root)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(a.launches), "--child", scene] + what, env=env,
                           capture_output=True, text=True, timeout=a.timeout)
        if p.returncode != 0:
            sys.exit(f"child {scene} {what} failed ({p.returncode}); nothing more is started\n{p.stdout}\n{p.stderr}")
        rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        for r in rows:
            print(json.dumps(r), flush=True)
        return {r["what"]: r["ms"] for r in rows}

    table = []
    for scene in a.scenes:
        comp, fus, rest = [], [], {}
        for rep in range(a.reps):
            comp.append(run(scene, ["composed"], a.baseline_root)["composed"])
            got = run(scene, ["fused"] + (["render", "dof", "equirect"] if rep == a.reps - 1 else []))
            fus.append(got.pop("fused"))
            rest.update(got)
        spread = max(comp) - min(comp)
        row = dict(scene=scene, fused_ms=float(np.median(fus)), composed_ms=float(np.median(comp)), composed_spread_ms=spread,
                   fused_min_max=[min(fus), max(fus)], composed_min_max=[min(comp), max(comp)], **{k + "_ms": v for k, v in rest.items()})
        row["fused_not_slower"] = row["fused_ms"] <= row["composed_ms"] + spread
        print(json.dumps(row), flush=True)
        table.append(row)
    print("\n| scene | fused ms | composed ms (parent build) | spread of composed | hrt_render wave ms | dof ms | equirect ms | fused not slower |\n|---|---|---|---|---|---|---|---|")
    for r in table:
        print(f"| {r['scene']} | {r['fused_ms']:.2f} | {r['composed_ms']:.2f} | {r['composed_spread_ms']:.2f} | {r.get('render_ms', float('nan')):.2f} | "
              f"{r.get('dof_ms', float('nan')):.2f} | {r.get('equirect_ms', float('nan')):.2f} | {r['fused_not_slower']} |")
    if not all(r["fused_not_slower"] for r in table):
        sys.exit("the fused pinhole is slower than the composition it replaces beyond the composition's own spread")


if __name__ == "__main__":
    main()
