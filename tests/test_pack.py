"""Scene packing without a GPU (csrc/hrt_pack.h pack_scene, through tests/pack/pack_check.cpp): the packed bytes and the refusals.

tests/golden/pack_hashes.json was RECORDED FROM THE COMMIT BEFORE the packing moved out of hrt_scene_create (its "recorded_from"),
by that commit's own code over the same cases, not from the code under test.  It pins the layout the kernels read: per array the
element count and the FNV-1a of the bytes, and every scalar of the scene header.  A later change that alters the packed layout ON
PURPOSE re-records the file with `pack_check <assets> hash all` / `refuse all` and says so in its description; any other difference
here is a bug.

pack_check is built with the address and undefined-behaviour sanitizers (make pack_check) and is an ordinary executable: a
refusal must come BEFORE the bad index is followed, so the sanitizers stay silent on every corrupted description too."""
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, PKG, ROOT

HRT_OK, HRT_ERR_INVALID = 0, -1
with open(os.path.join(GOLDEN, "pack_hashes.json")) as _f:
    RECORDED = json.load(_f)
VECTORS = ["tabs", "qfilter", "units", "tris", "planes", "colors", "vids", "images", "texels", "lights", "exceptions"]
HEADER = ["tab_quads", "tab_mats", "tab_spheres", "tab_meshes", "tab_sfilter", "tab_exc", "tab_rows", "exc_in_tabs", "qf_n", "sf_pairs", "sf_psize",
          "n_spheres", "n_quads", "n_meshes", "n_lights", "n_images", "n_kd_units", "dark_sky", "skybox_image", "any_motion", "prune_ok"]


@pytest.fixture(scope="module")
def pack_check():
    """{"hash": ..., "refuse": ...} as the program prints them, one run per mode."""
    subprocess.run(["make", "-s", "-C", PKG, "pack_check"], check=True)
    out = {}
    for mode in ("hash", "refuse"):
        r = subprocess.run([os.path.join(PKG, "pack_check"), os.path.join(ROOT, "assets"), mode, "all"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", f"pack_check {mode} all: exit {r.returncode}\n{r.stderr[-4000:]}"
        out[mode] = json.loads(r.stdout)
    return out


def test_cases_are_the_recorded_ones(pack_check):
    assert list(pack_check["hash"]) == list(RECORDED["hash"]) and list(pack_check["refuse"]) == list(RECORDED["refuse"])
    h = RECORDED["hash"]
    # the recording itself reaches the branches the cases are there for
    assert h["mesh_exc_long"]["header"]["exc_in_tabs"] == 0 and h["mesh_exc_long"]["vectors"]["exceptions"][0] > 1536
    assert h["mesh_irregular"]["header"]["exc_in_tabs"] == 1 and h["prune_off"]["header"]["prune_ok"] == 0
    assert h["spheres_odd"]["header"]["sf_pairs"] == 2 and h["spheres_odd"]["header"]["any_motion"] == 1
    assert all(n > 0 for n in h["quads"]["header"]["qf_n"])
    assert h["light_skybox"]["header"]["skybox_image"] == 2 and h["skybox_empty"]["header"]["skybox_image"] == -1
    assert h["mesh_colors"]["vectors"]["colors"][0] > 0 and h["mesh_colors"]["vectors"]["vids"][0] > 0
    assert all(set(v) == {"vectors", "header", "bound", "max_leaf"} and list(v["vectors"]) == VECTORS and list(v["header"]) == HEADER for v in h.values())


@pytest.mark.parametrize("case", list(RECORDED["hash"]))
def test_packed_bytes(pack_check, case):
    got, want = pack_check["hash"][case], RECORDED["hash"][case]
    assert "error" not in got, got
    for v in VECTORS:
        assert got["vectors"][v] == want["vectors"][v], f"{case}: {v} [count, fnv1a]"
    for k in HEADER:
        assert got["header"][k] == want["header"][k], f"{case}: header.{k}"
    assert got["bound"] == want["bound"] and got["max_leaf"] == want["max_leaf"]
    assert got == want


@pytest.mark.parametrize("case", list(RECORDED["refuse"]))
def test_refusal(pack_check, case):
    got, want = pack_check["refuse"][case], RECORDED["refuse"][case]
    assert want["base_rc"] == HRT_OK and want["rc"] == HRT_ERR_INVALID and want["error"]
    assert got["base_rc"] == HRT_OK, "the description the case corrupts must itself be accepted"
    assert got["rc"] == HRT_ERR_INVALID and got["error"] == want["error"]


def test_every_refusal_is_exercised_and_the_header_is_pure():
    with open(os.path.join(PKG, "csrc", "hrt_pack.h")) as f:
        src = f.read()
    texts = re.findall(r'refuse\(error, "([^"]+)"(\))?', src)  # (text, ")" when it is the whole message)
    assert len(texts) == 20
    seen = [r["error"] for r in RECORDED["refuse"].values()]
    for t, whole in texts:
        assert any(e == t if whole else e.startswith(t) for e in seen), f"no refusal case reaches: {t}"
    assert not re.search(r"\bhip[A-Z]\w*\s*\(|\bg_rt\b|getenv", src)
    assert re.findall(r'#include\s+([<"][^>"]+[>"])', src)[0] == '"hrt_device.h"' and src.count('#include "') == 1
