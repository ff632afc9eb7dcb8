"""The fused probe kernels and their per-sample pieces, run by whichever library HRT_LIBNAME names: tests/test_gpu_probe_cases.py starts
this with libhrt_var_probe256.so, the build whose sums run in blocks of 256 samples (a lane of an item then has up to four samples,
the loop a block of 64 passes once), and holds the fused outputs to tests/probe_ref.fold(..., block=256).

    python tests/probe_block_run.py OUT.npz

Per scene of SCENES, for the eight probes of tests/probe_cases.py at their own times: the per-sample series over SMAX samples -- the
basis values of hrt_probe_rays' directions and the one-sample outputs of trace_radiance, trace_lit and trace_lit(tail_after=2), none
of which depends on the block size -- the fused probes, probes_lit and probes_lit(tail_after=2) at every count of COUNTS, and one
pair of running sums."""
import importlib
import os
import sys

import numpy as np

F32 = np.float32
SCENES = ("cornell_mesh", "many_squares")
COUNTS = (65, 255, 256, 257, 513)  # 513 in blocks of 256: a lane with three samples in a block, then a block of one
SMAX = 513
RUNNING = (257, 256)
SEED, BIAS, TAIL = 5, 1e-3, 2
KINDS = {"probes": None, "lit": None, "lit_tail": TAIL}


def run(hrt):
    import probe_cases as pc
    import radiance_oracle as ro
    import test_gpu_lit_paths as lp
    import test_gpu_probe_lit as tl
    import test_gpu_probes as tp
    ef = tl.FACING | tl.VISIBLE
    got = {}
    for name in SCENES:
        dev = hrt.DeviceScene(ro.scene(hrt, name).desc)
        d_p = tp.on_gpu(pc.probes(hrt, name))
        vol, _, _ = tl.random_volume(hrt, pc.volume_box(hrt, name), 17)
        with vol:
            Y, v, deg = tp.series(hrt, dev, d_p, None, 0, SMAX, SEED)
            got[f"{name}__Y"], got[f"{name}__deg"], got[f"{name}__v_probes"] = Y, deg, v
            got[f"{name}__v_lit"] = tl.lit_series(hrt, dev, vol, d_p, None, 0, SMAX, SEED, 0, ef, BIAS)[1]
            got[f"{name}__v_lit_tail"] = lp.lit_path_series(hrt, dev, vol, d_p, None, 0, SMAX, SEED, 0, ef, BIAS, TAIL)[1]
            for S in COUNTS:
                got[f"{name}__probes__{S}"] = dev.probes(d_p, S, seed=SEED).cpu().numpy()
                got[f"{name}__lit__{S}"] = dev.probes_lit(d_p, vol, S, seed=SEED, eval_flags=ef, bias=BIAS).cpu().numpy()
                got[f"{name}__lit_tail__{S}"] = dev.probes_lit(d_p, vol, S, seed=SEED, eval_flags=ef, bias=BIAS, tail_after=TAIL).cpu().numpy()
            base = np.random.default_rng(3).uniform(0, 2, (len(d_p), 9, 3)).astype(F32)
            acc = tp.on_gpu(base)
            dev.probes(d_p, RUNNING[0], first_sample=0, seed=SEED, out=acc, accumulate=True)
            dev.probes(d_p, RUNNING[1], first_sample=RUNNING[0], seed=SEED, out=acc, accumulate=True)
            got[f"{name}__base"], got[f"{name}__running"] = base, acc.cpu().numpy()
        dev.close()
    return got


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    hrt = importlib.import_module("hai719-raytracing_amd")
    hrt.init(0)
    np.savez(sys.argv[1], **run(hrt))
    print("library", hrt.device_lib()._name)
