#!/usr/bin/env python3
"""Cost and quality of the denoiser ("Denoising"); prints ONE JSON line.

  time       hrt_render_features (n_samples 0 and 4) and hrt_denoise (the default parameters, and 1 and 8 iterations) at 1920x1080 and 3840x2160 on cornell_mesh,
             torch events on the launch stream, median of 10
  sweep      RMSE of the linear frame against a 4096-spp render, denoised / noisy, over a grid of parameters and of the feature
             samples (cornell_mesh and random_spheres, 480x270, 16 spp); `chosen` minimises the worse of the two ratios, each taken
             relative to its target (0.6 on cornell_mesh, 0.8 on random_spheres)
  quality    RMSE of noisy and denoised frames (defaults) at 4, 16 and 64 spp against the 4096-spp render, seed 1
  equal_time render + features + denoise at N spp against a plain render at the spp that takes the same wall time

    python tools/denoise_report.py [--quick]
"""
import argparse
import importlib
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hrt = importlib.import_module("hai719-raytracing_amd")

W, H, SEED, REF_SPP, FEAT_SPP = 480, 270, 1, 4096, 16  # features of every sample up to 16 (the sweep's choice)


def scene(name, w, h):
    host = hrt.HostScene().setup(name, w / h, 1)
    desc = host.flatten()
    return host, desc, hrt.DeviceScene(desc), hrt.default_camera(w / h)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def ev_ms(fn, reps=10):
    s = torch.cuda.current_stream()
    out = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn(s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out[2:]))


def timing():
    res = {}
    for (w, h) in ((1920, 1080), (3840, 2160)):
        _, _, dev, cam = scene("cornell_mesh", w, h)
        feat = torch.empty((h, w, 12), dtype=torch.float32, device="cuda")
        color = torch.rand((h, w, 3), dtype=torch.float32, device="cuda")
        scratch = torch.empty(hrt.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        lib = hrt.device_lib()
        r = {}
        for n in (0, 4):
            def f(st, n=n):
                assert lib.hrt_render_features(dev._h, torch_cam(cam), w, h, 0, n, SEED, feat.data_ptr(), st) == 0
            r[f"features_n{n}_ms"] = ev_ms(f)
        assert lib.hrt_render_features(dev._h, torch_cam(cam), w, h, 0, 4, SEED, feat.data_ptr(), None) == 0
        torch.cuda.synchronize()
        p = hrt.DenoiseParams()
        r[f"denoise_{p.iterations}it_ms"] = ev_ms(lambda st: hrt.denoise(color.data_ptr(), feat.data_ptr(), w, h, p, 0, scratch.data_ptr(), out.data_ptr(), st))
        for it in (1, 8):
            q = hrt.DenoiseParams(iterations=it)
            r[f"denoise_{it}it_ms"] = ev_ms(lambda st, q=q: hrt.denoise(color.data_ptr(), feat.data_ptr(), w, h, q, 0, scratch.data_ptr(), out.data_ptr(), st))
        res[f"{w}x{h}"] = {k: round(v, 4) for k, v in r.items()}
        dev.close()
    return res


def torch_cam(cam):
    import ctypes as C
    return C.byref(cam)


class Frames:
    """Noisy linear frames, features and the 4096-spp reference of one scene at W x H, with the denoiser on device pointers."""

    def __init__(self, name):
        self.host, self.desc, self.dev, self.cam = scene(name, W, H)
        self.ref, _ = self.dev.render(self.cam, W, H, REF_SPP, SEED)
        self.scratch = torch.empty(hrt.denoise_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        self.cache = {}

    def inputs(self, spp, fspp=FEAT_SPP):
        key = (spp, min(fspp, spp))
        if key not in self.cache:
            img, _ = self.dev.render(self.cam, W, H, spp, SEED)
            feat = self.dev.render_features(self.cam, W, H, 0, key[1], SEED)
            self.cache[key] = (img, torch.from_numpy(img).cuda(), torch.from_numpy(feat).cuda())
        return self.cache[key]

    def denoised(self, spp, p, fspp=FEAT_SPP):
        img, c, f = self.inputs(spp, fspp)
        hrt.denoise(c.data_ptr(), f.data_ptr(), W, H, p, 0, self.scratch.data_ptr(), self.out.data_ptr(), 0)
        torch.cuda.synchronize()
        return self.out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a smaller sweep")
    a = ap.parse_args()
    hrt.init(0)
    line = {"what": "denoise_report", "device": torch.cuda.get_device_name(0), "time": timing()}
    scenes = {n: Frames(n) for n in ("cornell_mesh", "random_spheres")}
    grid = dict(iterations=[3, 4, 5], sigma_color=[0.25, 0.5, 1.0, 2.0, 4.0, 8.0], sigma_normal=[0.05, 0.1, 0.3],
                sigma_albedo=[0.1, 0.2, 0.4], sigma_depth=[0.02, 0.05, 0.2])
    if a.quick:
        grid = dict(iterations=[5], sigma_color=[1.0], sigma_normal=[0.1, 0.5], sigma_albedo=[0.05], sigma_depth=[0.05])
    target = {"cornell_mesh": 0.6, "random_spheres": 0.8}
    sweep = []
    for fspp in (4, 16):
        for vals in itertools.product(*grid.values()):
            kw = dict(zip(grid.keys(), vals))
            p = hrt.DenoiseParams(**kw)
            ratios = {}
            for n, fr in scenes.items():
                img = fr.inputs(16, fspp)[0]
                ratios[n] = round(rmse(fr.denoised(16, p, fspp), fr.ref) / rmse(img, fr.ref), 4)
            sweep.append(dict(kw, feature_spp=fspp, **ratios, score=round(max(ratios[n] / target[n] for n in ratios), 4)))
    sweep.sort(key=lambda r: r["score"])
    line["sweep_16spp"] = sweep[:40]
    line["sweep_size"] = len(sweep)
    best = {k: sweep[0][k] for k in grid}
    line["chosen_feature_spp"] = sweep[0]["feature_spp"]
    line["chosen"] = best
    pbest = hrt.DenoiseParams(**best)
    pdef = hrt.DenoiseParams()
    line["defaults_in_build"] = {k: getattr(pdef, k) for k in grid}
    quality = {}
    for n, fr in scenes.items():
        q = {}
        for spp in (4, 16, 64):
            img = fr.inputs(spp)[0]
            q[str(spp)] = {"noisy": round(rmse(img, fr.ref), 5), "denoised": round(rmse(fr.denoised(spp, pdef), fr.ref), 5),
                           "denoised_chosen": round(rmse(fr.denoised(spp, pbest), fr.ref), 5),
                           "mean_rel": round(float(fr.denoised(spp, pdef).mean() / fr.ref.mean() - 1.0), 5),
                           "noisy_mean_rel": round(float(img.mean() / fr.ref.mean() - 1.0), 5)}
        quality[n] = q
    line["quality_rmse_480x270"] = quality
    eq = {}
    for n, fr in scenes.items():
        rows = []
        for spp in (4, 16):
            def wall(fn, reps=5):
                fn()
                t = []
                for _ in range(reps):
                    t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
                return float(np.median(t))
            td = wall(lambda: fr.dev.render_denoised(fr.cam, W, H, spp, min(FEAT_SPP, spp), SEED, 0, pdef))
            tp = wall(lambda: fr.dev.render(fr.cam, W, H, spp, SEED))
            m = spp
            while wall(lambda: fr.dev.render(fr.cam, W, H, m + max(1, m // 8), SEED)) <= td and m < 4096:
                m += max(1, m // 8)
            den = fr.dev.render_denoised(fr.cam, W, H, spp, min(FEAT_SPP, spp), SEED, 0, pdef)
            plain, _ = fr.dev.render(fr.cam, W, H, m, SEED)
            rows.append({"spp": spp, "denoised_ms": round(td * 1e3, 3), "plain_same_spp_ms": round(tp * 1e3, 3), "plain_equal_time_spp": m,
                         "denoised_rmse": round(rmse(den, fr.ref), 5), "plain_equal_time_rmse": round(rmse(plain, fr.ref), 5)})
        eq[n] = rows
    line["equal_time"] = eq
    print(json.dumps(line))


if __name__ == "__main__":
    main()
