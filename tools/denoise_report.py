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

With --var the line is the variance-guided filter's instead ("Variance-guided denoising"; hrt_denoise_var):

  time       hrt_denoise and hrt_denoise_var with the same iteration count (prefilter 0, 1, 2) at 1920x1080 and 3840x2160, alternated
             call by call in one loop, torch events on the launch stream, median of 10
  sweep      RMSE ratios denoised / noisy on cornell_mesh and random_spheres at 4, 16 and 64 spp (480x270, seed 1, features of every
             sample) over a grid of parameters; score = the worst of the six ratios relative to the fixed-width filter's ratio on the
             same frame, `chosen` minimises it
  quality    the twelve ratios (both filters, defaults) for seeds 1..4, each against the 4096-spp render of its seed, with the
             spread over the seeds; frame means and the variance map's mean at seed 1

    python tools/denoise_report.py --var [--quick]
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


def var_timing():
    res = {}
    s = torch.cuda.current_stream()
    for (w, h) in ((1920, 1080), (3840, 2160)):
        feat = torch.from_numpy(synthetic_guides(h, w)).cuda()
        color = torch.rand((h, w, 3), dtype=torch.float32, device="cuda")
        half = (color + 0.1 * (torch.rand((h, w, 3), dtype=torch.float32, device="cuda") - 0.5)).contiguous()
        scratch = torch.empty(max(hrt.denoise_scratch_bytes(w, h), hrt.denoise_var_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda")
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        var = torch.empty((h, w), dtype=torch.float32, device="cuda")
        old = hrt.DenoiseParams()
        calls = {f"denoise_{old.iterations}it_ms": lambda: hrt.denoise(color.data_ptr(), feat.data_ptr(), w, h, old, 0, scratch.data_ptr(), out.data_ptr(), s.cuda_stream)}
        for pre in (0, 1, 2):
            q = hrt.DenoiseVarParams(iterations=old.iterations, prefilter=pre)
            calls[f"denoise_var_{old.iterations}it_pre{pre}_ms"] = lambda q=q: hrt.denoise_var(
                color.data_ptr(), half.data_ptr(), feat.data_ptr(), w, h, q, 0, scratch.data_ptr(), out.data_ptr(), var.data_ptr(), s.cuda_stream)
        times = {k: [] for k in calls}
        for rep in range(12):  # alternated: every repetition times each call once
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                e1.synchronize()
                if rep >= 2:
                    times[k].append(e0.elapsed_time(e1))
        res[f"{w}x{h}"] = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    return res


def synthetic_guides(h, w):
    """Guides with regions and a depth ramp (the kernels' time does not depend on the scene, only on the taps that pass)."""
    f = np.zeros((h, w, 12), np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    region = (ys // 90 + xs // 120) % 4
    f[..., 0:3] = np.array([[0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.7, 0.7, 0.7], [0.1, 0.1, 0.9]], np.float32)[region]
    f[..., 3:6] = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [0.6, 0.8, 0]], np.float32)[region]
    f[..., 9] = 2.0 + (xs / w).astype(np.float32)
    f[..., 10] = 1
    return f


class VarFrames:
    """Noisy frames, their first halves, features and the 4096-spp reference of one scene and seed at W x H."""

    def __init__(self, name, seed):
        self.seed = seed
        self.host, self.desc, self.dev, self.cam = scene(name, W, H)
        self.ref, _ = self.dev.render(self.cam, W, H, REF_SPP, seed)
        self.scratch = torch.empty(max(hrt.denoise_scratch_bytes(W, H), hrt.denoise_var_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        self.var = torch.empty((H, W), dtype=torch.float32, device="cuda")
        self.cache = {}

    def inputs(self, spp):
        if spp not in self.cache:
            img, _ = self.dev.render(self.cam, W, H, spp, self.seed)
            half, _ = self.dev.render(self.cam, W, H, spp // 2, self.seed)
            feat = self.dev.render_features(self.cam, W, H, 0, spp, self.seed)
            self.cache[spp] = (img, rmse(img, self.ref), torch.from_numpy(img).cuda(), torch.from_numpy(half).cuda(), torch.from_numpy(feat).cuda())
        return self.cache[spp]

    def ratio_old(self, spp, p):
        img, rn, c, _, f = self.inputs(spp)
        hrt.denoise(c.data_ptr(), f.data_ptr(), W, H, p, 0, self.scratch.data_ptr(), self.out.data_ptr(), 0)
        torch.cuda.synchronize()
        return rmse(self.out.cpu().numpy(), self.ref) / rn

    def ratio_var(self, spp, p, frame=False):
        img, rn, c, ch, f = self.inputs(spp)
        hrt.denoise_var(c.data_ptr(), ch.data_ptr(), f.data_ptr(), W, H, p, 0, self.scratch.data_ptr(), self.out.data_ptr(), self.var.data_ptr(), 0)
        torch.cuda.synchronize()
        o = self.out.cpu().numpy()
        return (rmse(o, self.ref) / rn, o) if frame else rmse(o, self.ref) / rn


VAR_SCENES, VAR_SPPS = ("cornell_mesh", "random_spheres"), (4, 16, 64)


def var_main(quick):
    line = {"what": "denoise_var_report", "device": torch.cuda.get_device_name(0), "time": var_timing()}
    frames = {n: VarFrames(n, SEED) for n in VAR_SCENES}
    pold = hrt.DenoiseParams()
    old = {f"{n}/{spp}": frames[n].ratio_old(spp, pold) for n in VAR_SCENES for spp in VAR_SPPS}
    grid = dict(iterations=[4, 5], prefilter=[0, 1, 2, 3], sigma_variance=[1.0, 2.0, 4.0, 8.0, 16.0], variance_floor=[0.0, 1e-8, 1e-5, 1e-3])
    if quick:
        grid = dict(iterations=[4], prefilter=[2], sigma_variance=[4.0, 8.0], variance_floor=[1e-8])
    sweep = []
    for vals in itertools.product(*grid.values()):
        kw = dict(zip(grid.keys(), vals))
        p = hrt.DenoiseVarParams(**kw)
        ratios = {k: round(frames[k.split("/")[0]].ratio_var(int(k.split("/")[1]), p), 4) for k in old}
        sweep.append(dict(kw, **ratios, worst=max(ratios.values()), score=round(max(ratios[k] / old[k] for k in old), 4)))
    sweep.sort(key=lambda r: r["score"])
    line["sweep_size"] = len(sweep)
    line["sweep"] = sweep[:40]
    line["chosen"] = {k: sweep[0][k] for k in grid}
    pdef = hrt.DenoiseVarParams()
    line["defaults_in_build"] = {k: getattr(pdef, k) for k in ("iterations", "prefilter", "sigma_variance", "sigma_normal", "sigma_albedo",
                                                                 "sigma_depth", "variance_floor")}
    quality = {}
    for seed in (1, 2, 3, 4):
        fr = frames if seed == SEED else {n: VarFrames(n, seed) for n in VAR_SCENES}
        for n in VAR_SCENES:
            for spp in VAR_SPPS:
                q = quality.setdefault(f"{n}/{spp}", {"fixed": [], "variance": []})
                q["fixed"].append(round(fr[n].ratio_old(spp, pold), 4))
                r, o = fr[n].ratio_var(spp, pdef, frame=True)
                q["variance"].append(round(r, 4))
                if seed == SEED:
                    q["noisy_rmse"] = round(fr[n].inputs(spp)[1], 5)
                    q["mean_rel"] = round(float(o.mean() / fr[n].ref.mean() - 1.0), 5)
                    q["variance_map_mean"] = float(fr[n].var.mean().item())
        if seed != SEED:
            for f in fr.values():
                f.dev.close()
    for q in quality.values():
        for k in ("fixed", "variance"):
            q[k + "_spread"] = round(max(q[k]) - min(q[k]), 4)
    line["quality_ratio_480x270_seeds_1_to_4"] = quality
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a smaller sweep")
    ap.add_argument("--var", action="store_true", help="report on the variance-guided filter (hrt_denoise_var) instead")
    a = ap.parse_args()
    hrt.init(0)
    if a.var:
        return var_main(a.quick)
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
