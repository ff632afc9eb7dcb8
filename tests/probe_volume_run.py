"""The matrix of tests/test_gpu_probe_volume.py's rule test, run by whichever library HRT_LIBNAME names: every grid, every flag
combination and every batch size, through ProbeVolume.update and ProbeVolume.eval on torch tensors.

    python tests/probe_volume_run.py OUT.npz     writes one array per case (the test starts this with the A/B library)

`matrix()` gives the inputs, the same in every process: they come from fixed seeds."""
import importlib
import os
import sys

import numpy as np

F32 = np.float32
BATCHES = (1, 7, 8, 9, 63, 65, 257, 1000)  # round the group, wave and workgroup sizes of both mappings
FLAGS = ((False, False), (True, False), (False, True), (True, True))  # (radiance, facing)


def matrix():
    """{grid name: (box, counts, coefficients (n, 9, 3), 1000 point records)}: random coefficients with negatives and mixed
    magnitudes; the points of test_probe_volume_abi.rule_points, repeated to 1000 and shuffled so that every batch size has of
    every kind."""
    import test_probe_volume_abi as abi
    out = {}
    for g, (name, (box, counts)) in enumerate(sorted(abi.GRIDS.items())):
        rng = np.random.default_rng(100 + g)
        n = int(np.prod(counts))
        coeffs = (rng.standard_normal((n, 9, 3)) * 10.0 ** rng.integers(-4, 5, (n, 9, 3))).astype(F32)
        pts = abi.rule_points(box, counts, seed=20 + g)[0]
        pts = np.resize(pts, (max(BATCHES), 8))[rng.permutation(max(BATCHES))]
        out[name] = (box, counts, coeffs, np.ascontiguousarray(pts, F32))
    return out


def run(hrt):
    """{"grid__<radiance><facing>__n": (n, 3) fp32} from the device."""
    import torch
    got = {}
    for name, (box, counts, coeffs, pts) in matrix().items():
        with hrt.ProbeVolume(*box, *counts) as vol:
            vol.update(torch.from_numpy(coeffs).to("cuda"))
            d_pts = torch.from_numpy(pts).to("cuda")
            for radiance, facing in FLAGS:
                for n in BATCHES:
                    r = vol.eval(d_pts[:n].contiguous(), radiance=radiance, facing=facing)
                    got[f"{name}__{int(radiance)}{int(facing)}__{n}"] = r.cpu().numpy()
    return got


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    hrt = importlib.import_module("hai719-raytracing_amd")
    hrt.init(0)
    np.savez(sys.argv[1], **run(hrt))
    print("library", hrt.device_lib()._name)
