"""The Python binding's refusals, text for text (hai719-raytracing_amd/__init__.py).

tests/golden/python_refusals.json maps a case name to the exact ValueError text.  It was recorded from the commit BEFORE the
binding's checks were collected into shared helpers, with this module's --write mode run on a built checkout of that commit:

    python tests/test_python_refusals.py --write <that checkout>/hai719-raytracing_amd/__init__.py

(never from the tree under test).  The test replays every case against the tree and compares the text for equality.

The file has 28 `raise ValueError` statements.  cpu_cases reach 20 of them without a GPU and without either library: after each
of these cases the freshly imported module has loaded neither (`_host is None and _dev is None`), which is what "every argument
check happens before `self` is touched" means.  lib_cases reach 3 more once libhrt.so is loaded (still no GPU).  The other five
cannot be reached without a GPU tensor or 2^31 rows: the two "at most 2^31 - 1" refusals, the torch `keys` / `out` refusals of
_radiance_batch and bake_rays (three statements) and render_lens_adaptive's "stats are the blocking form's".  The last four are
among gpu_cases: tests/test_gpu_lens_adaptive.py replays them, with their texts in the same golden file."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "python_refusals.json")
TREE_INIT = os.path.join(ROOT, "hai719-raytracing_amd", "__init__.py")


def _f32(*shape):
    return np.zeros(shape, dtype=np.float32)


def cpu_cases(hrt, torch):
    D, Camera = hrt.DeviceScene, hrt.Camera
    pts, L = _f32(4, 8), hrt.Lens(hrt.Camera())
    return {
        "lens_projection": lambda: hrt.Lens(Camera(), "pinhole"),
        "rays_mode": lambda: D.trace_rays(None, pts, mode="nearest"),
        "rays_torch": lambda: D.trace_rays(None, torch.zeros((4, 8))),
        "rays_shape": lambda: D.trace_rays(None, _f32(4, 7)),
        "rad_torch": lambda: D.trace_radiance(None, torch.zeros((4, 8), dtype=torch.float64)),
        "rad_shape": lambda: D.trace_radiance(None, _f32(4, 7)),
        "rad_keys": lambda: D.trace_radiance(None, pts, keys=np.zeros(3, np.uint32)),
        "rad_keys_dtype": lambda: D.trace_radiance(None, pts, keys=np.zeros(4, np.int64)),
        "rad_acc": lambda: D.trace_radiance(None, pts, first_sample=3, accumulate=True),
        "rad_out": lambda: D.trace_radiance(None, pts, out=_f32(4, 4)),
        "bake_torch": lambda: D.bake(None, torch.zeros((4, 8))),
        "bake_shape": lambda: D.bake(None, _f32(4, 7)),
        "bake_keys": lambda: D.bake(None, pts, keys=np.zeros(3, np.uint32)),
        "bake_acc": lambda: D.bake(None, pts, first_sample=3, accumulate=True),
        "bake_out": lambda: D.bake(None, pts, out=np.zeros((4, 3), np.float64)),
        "views_seeds": lambda: D.render_views(None, [Camera()] * 2, 8, 8, 1, seeds=[1]),
        "views_out": lambda: D.render_views(None, [Camera()] * 2, 8, 8, 1, out=torch.zeros((2, 8, 8, 3))),
        "lens_out_torch": lambda: D.render_lens(None, L, 16, 9, 1, out=torch.zeros((9, 16, 3))),
        "lens_out_np": lambda: D.render_lens(None, L, 16, 9, 1, out=_f32(9, 16, 4)),
        "lens_acc": lambda: D.render_lens(None, L, 16, 9, 1, first_sample=3, accumulate=True),
        "la_out": lambda: D.render_lens_adaptive(None, L, 16, 9, 4, 16, 0.5, out=_f32(9, 16, 3)),
        "lv_seeds": lambda: D.render_lens_views(None, [L, L], 16, 9, 1, seeds=[1]),
        "lvf_seeds": lambda: D.render_lens_views_features(None, [L], 16, 9, 0, 1, seeds=[1, 2]),
        "lv_out_torch": lambda: D.render_lens_views(None, [L, L], 16, 9, 1, out=torch.zeros((2, 9, 16, 3))),
        "lv_out_np": lambda: D.render_lens_views(None, [L, L], 16, 9, 1, out=_f32(1, 9, 16, 3)),
        "lv_acc": lambda: D.render_lens_views(None, [L], 16, 9, 1, first_sample=3, accumulate=True),
    }


def lib_cases(hrt, torch):
    return {
        "bake_rays_points": lambda: hrt.bake_rays(_f32(4, 8)),
        "mesh_points_positions": lambda: hrt.mesh_points(np.zeros((4, 2)), np.zeros((1, 3))),
        "mesh_points_indices": lambda: hrt.mesh_points(np.zeros((4, 3)), np.zeros((1, 4))),
    }


def gpu_cases(hrt, torch):
    D = hrt.DeviceScene
    pts, L = torch.zeros((4, 8), device="cuda"), hrt.Lens(hrt.Camera())
    keys3 = torch.zeros(3, dtype=torch.int32, device="cuda")
    return {
        "gpu_rad_keys": lambda: D.trace_radiance(None, pts, keys=keys3),
        "gpu_rad_out": lambda: D.trace_radiance(None, pts, out=torch.zeros((4, 4), device="cuda")),
        "gpu_bake_keys": lambda: D.bake(None, pts, keys=keys3),
        "gpu_bake_out": lambda: D.bake(None, pts, out=torch.zeros((4, 3), device="cpu")),
        "gpu_bake_rays_keys": lambda: hrt.bake_rays(pts, keys=keys3),
        "gpu_la_stats": lambda: D.render_lens_adaptive(None, L, 16, 9, 4, 16, 0.5, out=torch.zeros((9, 16, 3), device="cuda"),
                                                       stats=hrt.Stats()),
    }


def refusal(call):
    """The text of the ValueError `call` raises; anything else is reported as text that no golden entry has."""
    try:
        call()
    except ValueError as e:
        return str(e)
    except Exception as e:  # noqa: BLE001 -- the comparison fails on it, with the exception in the message
        return f"<{type(e).__name__}: {e}>"
    return "<nothing raised>"


def replay(init_path, groups):
    """{case: {"text": ..., "libs": whether a library was loaded by then}} of the package at init_path, freshly imported."""
    import torch
    spec = importlib.util.spec_from_file_location("hrt_refusals", init_path, submodule_search_locations=[os.path.dirname(init_path)])
    hrt = importlib.util.module_from_spec(spec)
    sys.modules["hrt_refusals"] = hrt
    spec.loader.exec_module(hrt)
    got = {}
    for group in groups:
        for name, call in {"cpu": cpu_cases, "lib": lib_cases, "gpu": gpu_cases}[group](hrt, torch).items():
            got[name] = {"group": group, "text": refusal(call), "libs": hrt._host is not None or hrt._dev is not None}
    return got


def test_every_refusal_has_the_recorded_text_and_comes_before_a_library_is_loaded(hrt):
    golden = json.load(open(GOLDEN))
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--replay", TREE_INIT, "cpu", "lib"], check=True,
                           capture_output=True, text=True)
    got = json.loads(child.stdout.splitlines()[-1])
    cpu = [k for k, v in got.items() if v["group"] == "cpu"]
    assert len(cpu) == 26 and len(got) == 29 and set(got) <= set(golden), sorted(set(got) - set(golden))
    wrong = {k: (v["text"], golden[k]) for k, v in got.items() if v["text"] != golden[k]}
    assert not wrong, wrong
    loaded = [k for k in cpu if got[k]["libs"]]
    assert not loaded, f"a library was loaded to refuse {loaded}"


if __name__ == "__main__":
    mode, init = sys.argv[1], sys.argv[2]
    if mode == "--replay":
        print(json.dumps(replay(init, sys.argv[3:])))
    elif mode == "--write":  # [file]: another golden file; cases that need a GPU are recorded where there is one
        import torch
        path = sys.argv[3] if len(sys.argv) > 3 else GOLDEN
        texts = json.load(open(path)) if os.path.exists(path) else {}
        new = replay(init, ["cpu", "lib"] + (["gpu"] if torch.cuda.is_available() else []))
        bad = {k: v["text"] for k, v in new.items() if v["text"].startswith("<")}
        assert not bad, bad
        texts.update({k: v["text"] for k, v in new.items()})
        json.dump(texts, open(path, "w"), indent=1, sort_keys=True)
        print(f"{path}: {len(new)} recorded, {len(texts)} in all")
    else:
        sys.exit("usage: test_python_refusals.py --replay INIT GROUP... | --write INIT [FILE]")
