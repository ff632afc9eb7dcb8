#!/usr/bin/env python3
"""Cost and quality of temporal accumulation ("Temporal accumulation"); prints ONE JSON line.

  time     hrt_temporal_accumulate at 1920x1080 on cornell_mesh frames (camera orbited by 1 degree between the two frames, default
           parameters), with and without the half frame, and under a still camera; torch events on the launch stream around one
           call, median of 10 after 3 warm-up calls; bytes = what a pixel reads and writes at most (four taps), over the time
  quality  random_spheres, 480x270, 64 spp, still camera, frames with seeds 1..4 accumulated through hrt_render_temporal: RMSE
           against a 4096-spp render (seed 1000) of every single frame, of the accumulated frame after each frame, and of both fed
           through hrt_denoise_var (defaults), as ratios to the single frame of the same seed; once with the features of the pixel
           centres (the same in every frame), of 16 and of all 64 samples (different in every frame)

    python tools/temporal_report.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
hrt = importlib.import_module("hai719-raytracing_amd")


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def scene(name, w, h):
    host = hrt.HostScene().setup(name, w / h, 1)
    return host, hrt.DeviceScene(host.flatten()), hrt.default_camera(w / h)


def timing():
    from test_gpu_temporal import orbit
    w, h = 1920, 1080
    host, dev, cam0 = scene("cornell_mesh", w, h)
    cam1 = orbit(hrt, cam0, 1.0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    frames = []
    for cam, seed in ((cam0, 1), (cam1, 2)):
        frames.append((up(dev.render(cam, w, h, 4, seed)[0]), up(dev.render(cam, w, h, 2, seed)[0]), up(dev.render_features(cam, w, h, 0, 4, seed))))
    (pc, pch, pf), (c, ch, f) = frames
    ph = torch.full((h, w), 3.0, dtype=torch.float32, device="cuda")
    out, outh, n = torch.empty_like(c), torch.empty_like(c), torch.empty_like(ph)
    s = torch.cuda.current_stream()
    p = hrt.TemporalParams()
    res = {}
    for label, cam, prev_cam, half in (("orbit_1deg_with_half", cam1, cam0, True), ("orbit_1deg_without_half", cam1, cam0, False),
                                       ("still_with_half", cam0, cam0, True), ("still_without_half", cam0, cam0, False)):
        def call():
            hrt.temporal_accumulate(cam, prev_cam, w, h, c.data_ptr(), ch.data_ptr() if half else 0, f.data_ptr(), pc.data_ptr(),
                                    pch.data_ptr() if half else 0, pf.data_ptr(), ph.data_ptr(), p, out.data_ptr(),
                                    outh.data_ptr() if half else 0, n.data_ptr(), s.cuda_stream)
        for _ in range(3):
            call()
        s.synchronize()
        ms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        own = 4 * (12 + 3 + (3 if half else 0))                       # the pixel's features (12 floats) and colour(s)
        tap = 4 * (12 + 3 + (3 if half else 0) + 1)                   # a tap's features, colour(s) and history
        wr = 4 * (3 + (3 if half else 0) + 1)
        bytes_max = w * h * (own + 4 * tap + wr)
        res[label] = {"ms_median_of_10": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "bytes_per_pixel_at_most": own + 4 * tap + wr, "gbps_at_most": round(bytes_max / med / 1e6, 1),
                      "mean_history_out": round(float(n.mean()), 3)}
    return res


def quality(fspp):
    w, h, spp = 480, 270, 64
    host, dev, cam = scene("random_spheres", w, h)
    ref, _ = dev.render(cam, w, h, 4096, 1000)
    tp, dp = hrt.TemporalParams(), hrt.DenoiseVarParams()
    plain, filtered = hrt.History(dev), hrt.History(dev)
    rows = []
    for seed in (1, 2, 3, 4):
        single, _ = dev.render(cam, w, h, spp, seed)
        single_f = dev.render_denoised_var(cam, w, h, spp, fspp, seed, 0, dp)
        acc, lens = dev.render_temporal(plain, cam, w, h, spp, fspp, seed, 0, tp, None)
        acc_f, _ = dev.render_temporal(filtered, cam, w, h, spp, fspp, seed, 0, tp, dp)
        rs = rmse(single, ref)
        rows.append({"seed": seed, "frames_accumulated": seed, "single_rmse": round(rs, 5), "single_filtered_ratio": round(rmse(single_f, ref) / rs, 4),
                     "accumulated_ratio": round(rmse(acc, ref) / rs, 4), "accumulated_filtered_ratio": round(rmse(acc_f, ref) / rs, 4),
                     "mean_history": round(float(lens.mean()), 3)})
    return rows


def main():
    hrt.init(0)
    line = {"tool": "temporal_report", "time_1920x1080": timing(), "quality_random_spheres_480x270_64spp": {f"feature_spp_{n}": quality(n) for n in (0, 16, 64)}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
