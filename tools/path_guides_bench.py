#!/usr/bin/env python3
"""Quality and cost of the path-feature guides (DESIGN.md section 5 "Path features") on one MI355X.

    python tools/path_guides_bench.py [--quick]          -> profiles/path_guides_bench.json

  quality   RMSE of the linear denoised frame against a 4096-spp render of its seed, for both filters (hrt_render_denoised,
            hrt_render_denoised_var, default parameters, features of min(spp, 16) samples), FIRST-HIT guides against PATH guides,
            on cornell_box, cornell_mesh and random_spheres at 4 / 16 / 64 spp, 480 x 270, seeds 1..4 (the seeds of the table of
            "Variance-guided denoising"); the same RMSE restricted to the pixels whose first hit, for the ray of sample 0 of seed 1,
            is mirror or glass; the noisy frame's RMSE beside them
  cost      hrt_render_features against hrt_render_path_features at 1920 x 1080 x 16 samples on the same scenes, alternated call by
            call in one loop on one build, torch events on the launch stream, median and spread of 10; and, for what direct_light
            costs a path-feature launch (it runs at every hit to keep the stream in step and its value is dropped), cornell_mesh
            against cornell_mesh with one light added, whose launch is the _lights build

    python tools/path_guides_bench.py --waves-ab          -> profiles/path_features_waves_ab.json

  the A/B of the launch bounds: for N in 2 .. 5 a fresh process per build hai719-raytracing_amd/libhrt_var_pf_wN.so (all three
  families at N waves per SIMD, built in hai719-raytracing_amd: make libhrt_var_pf_wN.so VARIANT=libhrt_var_pf_wN.so VARIANT_FLAGS="-DHRT_PATH_FEATURES_MIN_WAVES=N
  -DHRT_LENS_PATH_FEATURES_MIN_WAVES=N -DHRT_LENS_VIEWS_PATH_FEATURES_MIN_WAVES=N"), two rounds, the second in the reverse order
  of the first so that no build always runs first; per build the time of the record form on 1080p camera rays, of a 1080p x 16 frame and of 64
  views of 128 x 128 x 16 on cornell_mesh (no lights) and random_spheres (lights).  `--waves-one` is the child: one JSON line for
  the build HRT_LIBNAME names.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, REF_SPP, FEAT_SPP = 480, 270, 4096, 16
SCENES = ("cornell_box", "cornell_mesh", "random_spheres")
SEEDS = (1, 2, 3, 4)
SPPS = (4, 16, 64)


def rmse(a, b, mask=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


def ev_ms(torch, fns, reps=10):
    """Median and (min, max) in ms of each of `fns`, alternated call by call in one loop; two warm-up rounds."""
    s = torch.cuda.current_stream()
    out = [[] for _ in fns]
    for r in range(reps + 2):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn(s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if r >= 2:
                out[k].append(e0.elapsed_time(e1))
    return [{"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for t in out]


def build(hrt, name, w, h, light=False):
    host = hrt.HostScene().setup(name, w / h, 1)
    if light:
        host.add_light((0.0, 0.5, 0.0), 0.1, (1, 1, 1))
    return host, hrt.DeviceScene(host.flatten()), hrt.default_camera(w / h)


def quality(hrt, quick):
    res = {}
    for name in SCENES:
        host, dev, cam = build(hrt, name, W, H)
        first1, path1 = dev.render_features(cam, W, H, 0, 1, 1), dev.render_path_features(cam, W, H, 0, 1, 1)
        # which pixels look at mirror or glass: trace_rays("shade") on the rays of sample 0
        shade = dev.trace_rays(hrt.camera_rays(cam, W, H, 0, 1).cpu().numpy(), "shade").view(np.uint32).reshape(H, W, 16)
        spec = (shade[..., hrt.HIT_KIND] != hrt.KIND_MISS) & (shade[..., hrt.SHADE_MATERIAL_TYPE] != hrt.MAT_DIFFUSE)
        rows = {}
        for seed in (SEEDS[:1] if quick else SEEDS):
            ref, _ = dev.render(cam, W, H, 256 if quick else REF_SPP, seed)
            for spp in SPPS:
                fspp = min(spp, FEAT_SPP)
                noisy, _ = dev.render(cam, W, H, spp, seed)
                r = {"noisy": rmse(noisy, ref), "noisy_specular": rmse(noisy, ref, spec), "specular_pixels": int(spec.sum())}
                for filt, call in (("fixed", dev.render_denoised), ("var", dev.render_denoised_var)):
                    for guides in ("first", "diffuse"):
                        out = call(cam, W, H, spp, fspp, seed, 0, guides=guides)
                        r[f"{filt}_{guides}"] = rmse(out, ref)
                        r[f"{filt}_{guides}_specular"] = rmse(out, ref, spec)
                rows[f"seed{seed}_spp{spp}"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items()}
        # the means over the seeds, per spp
        mean = {}
        for spp in SPPS:
            ks = [k for k in rows if k.endswith(f"_spp{spp}")]
            mean[f"spp{spp}"] = {m: round(float(np.mean([rows[k][m] for k in ks])), 6) for m in rows[ks[0]] if m != "specular_pixels"}
            mean[f"spp{spp}"]["specular_pixels"] = rows[ks[0]]["specular_pixels"]
        res[name] = {"mean_over_seeds": mean, "per_seed": rows,
                     "pixels_where_the_guides_differ_at_1_sample": int((first1 != path1).any(axis=2).sum())}
        dev.close()
    return res


def cost(hrt, torch, quick):
    w, h, n = (1920, 1080, 16)
    lib = hrt.device_lib()
    res = {}
    cases = [(name, False) for name in SCENES] + [("cornell_mesh", True)]
    for name, light in cases:
        host, dev, cam = build(hrt, name, w, h, light)
        feat = torch.empty((h, w, 12), dtype=torch.float32, device="cuda")

        def first(st):
            assert lib.hrt_render_features(dev._h, C.byref(cam), w, h, 0, n, 1, feat.data_ptr(), st) == 0

        def path(st):
            assert lib.hrt_render_path_features(dev._h, C.byref(cam), w, h, 0, n, 1, feat.data_ptr(), st) == 0

        a, b = ev_ms(torch, (first, path), 3 if quick else 10)
        res[name + ("_plus_one_light" if light else "")] = {"first_hit": a, "path": b, "ratio": round(b["median_ms"] / a["median_ms"], 3),
                                                            "msamples_per_s_path": round(w * h * n / b["median_ms"] / 1e3, 1)}
        dev.close()
    plain, lit = res["cornell_mesh"]["path"]["median_ms"], res["cornell_mesh_plus_one_light"]["path"]["median_ms"]
    res["direct_light_cost"] = {"scene": "cornell_mesh, the same launch with one light added (the _lights build draws direct_light at every hit)",
                                "plain_ms": plain, "lights_ms": lit, "ratio": round(lit / plain, 3)}
    return res


def waves_one(hrt, torch):
    """The three families under the build HRT_LIBNAME names: one JSON line."""
    lib = hrt.device_lib()
    res = {"lib": os.environ.get("HRT_LIBNAME", "libhrt.so")}
    for name in ("cornell_mesh", "random_spheres"):
        w, h, n = 1920, 1080, 16
        host, dev, cam = build(hrt, name, w, h)
        lens = hrt.Lens(cam)
        feat = torch.empty((h, w, 12), dtype=torch.float32, device="cuda")
        rays = hrt.camera_rays(cam, w, h, 0, 1)
        cam_v = hrt.default_camera(1.0)
        views = (hrt.LensView * 64)()
        for v in range(64):
            views[v].lens, views[v].seed = hrt.Lens(cam_v, "equirect" if v % 2 else "perspective"), v + 1
        fv = torch.empty((64, 128, 128, 12), dtype=torch.float32, device="cuda")

        def record(st):
            assert lib.hrt_path_features(dev._h, rays.data_ptr(), None, w * h, 0, 1, 0, feat.data_ptr(), st) == 0

        def frame(st):
            assert lib.hrt_render_lens_path_features(dev._h, C.byref(lens), w, h, 0, n, 1, feat.data_ptr(), st) == 0

        def batch(st):
            assert lib.hrt_render_lens_views_path_features(dev._h, views, 64, 128, 128, 0, n, fv.data_ptr(), st) == 0

        r, f, b = ev_ms(torch, (record, frame, batch))
        res[name] = {"record_1080p_1_sample": r, "frame_1080p_16": f, "views_64x128x128_16": b}
        dev.close()
    print(json.dumps(res))


def waves_ab():
    """A fresh process per build, two rounds in opposite orders; the parent never opens the GPU."""
    rounds = []
    order = [2, 3, 4, 5]
    for r in range(2):
        for n in (order if r == 0 else order[::-1]):
            env = dict(os.environ, HRT_LIBNAME=f"libhrt_var_pf_w{n}.so")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--waves-one"], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"waves {n}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}")  # nothing more is started
            line = json.loads(p.stdout.strip().splitlines()[-1])
            line["waves"], line["round"] = n, r
            rounds.append(line)
    table = {}
    for name in ("cornell_mesh", "random_spheres"):
        for fam in ("record_1080p_1_sample", "frame_1080p_16", "views_64x128x128_16"):
            table[f"{name}/{fam}"] = {f"waves{n}": {"median_of_rounds_ms": round(float(np.median([x[name][fam]["median_ms"] for x in rounds if x["waves"] == n])), 4),
                                                  "rounds_ms": [x[name][fam]["median_ms"] for x in rounds if x["waves"] == n]} for n in order}
    out = {"what": "path-feature kernels at 2 .. 5 waves per SIMD (launch bounds), MI355X; see tools/path_guides_bench.py --waves-ab",
           "table": table, "runs": rounds}
    path = os.path.join(ROOT, "profiles", "path_features_waves_ab.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(table))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--waves-ab", action="store_true")
    ap.add_argument("--waves-one", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_guides_bench.json"))
    args = ap.parse_args()
    if args.waves_ab:
        return waves_ab()
    import torch
    hrt = importlib.import_module("hai719-raytracing_amd")
    hrt.init(0)
    if args.waves_one:
        return waves_one(hrt, torch)
    out = {"what": "path guides against first-hit guides, MI355X; see tools/path_guides_bench.py",
           "frame": [W, H], "ref_spp": 256 if args.quick else REF_SPP, "feature_spp": "min(spp, 16)", "seeds": list(SEEDS[:1] if args.quick else SEEDS),
           "cost": cost(hrt, torch, args.quick), "quality": quality(hrt, args.quick)}
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({"cost": out["cost"], "quality": {k: v["mean_over_seeds"] for k, v in out["quality"].items()}}))


if __name__ == "__main__":
    main()
