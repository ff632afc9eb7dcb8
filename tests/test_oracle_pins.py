"""The oracle against the reference's own code: committed golden vectors (generated from
oracle/_ref, i.e. the reference's Triangle.h / AABB.h / Functions.cpp / Vec3.h / Ray.h /
imageLoader.cpp compiled from /root/reference) and, where oracle/_ref is present, live.
Everything here is bit-exact: the restatement must BE the reference arithmetic."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "ref_kat.npz"))


def test_triangle_matches_reference_golden(oracle, kat):
    for tri, want in zip(kat["tri_prims"], kat["tri_out"]):
        got = oracle.kat("triangle", tri, kat["tri_rays"])
        assert np.array_equal(got, want)
    assert kat["tri_out"][0][:, 0].sum() > 100  # the vectors do exercise hits
    assert kat["tri_out"][1][:, 0].sum() == 0   # back-facing triangle: culled (Triangle.h:87-91)


def test_aabb_matches_reference_golden(oracle, kat):
    for box, want in zip(kat["aabb_prims"], kat["aabb_out"]):
        got = oracle.kat("aabb", box, kat["aabb_rays"])[:, 0]
        assert np.array_equal(got, want[:, 0])
    assert 0 < kat["aabb_out"][0].sum() < kat["aabb_rays"].shape[0]


def test_optics_match_reference_golden(oracle, kat):
    got = oracle.kat_optics(kat["optics_in"])
    assert np.array_equal(got, kat["optics_out"], equal_nan=True)


def test_random_stream_matches_reference_golden(oracle, kat):
    got = oracle.kat_random(kat["random_out"].shape[0], seed=int(kat["random_seed"][0]))
    assert np.array_equal(got, kat["random_out"])
    u = got[:, 0]
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.03
    assert np.allclose(np.linalg.norm(got[:, 1:], axis=1), 1.0, atol=1e-6)


def test_ray_normalisation_matches_reference_golden(oracle, kat):
    """Ray's constructor normalises (Line.h:13-16, Vec3.h:46): the oracle's `normalized`, through make_ray, against the
    directions the reference's own Ray produced."""
    assert np.array_equal(oracle.kat_normalize(kat["normalize_in"]), kat["normalize_out"])


def test_camera_rays_match_reference_golden(hrt, oracle, kat):
    """Row a2.  The golden rays come from the reference's gluInvertMatrix + screen_space_to_world_space_ray
    (matrixUtilities.h:53-74, 77-206) + Ray constructor on the GL matrices of 16 poses (4 default-pose aspect ratios, 12
    random rigid poses / fields of view).  The oracle restates the adjugate inverse term by term: inverses and rays are
    bit-identical."""
    assert kat["camera_rows"].shape[0] >= 16
    for row, want, inv in zip(kat["camera_rows"], kat["camera_rays"], kat["camera_inverses"]):
        cam = oracle.camera_from_row(hrt, row)
        assert np.array_equal(oracle.camera_rays(cam, kat["camera_uv"]), want)
        _, _, mvi, pri = oracle.camera_matrices(cam)
        assert np.array_equal(np.concatenate([mvi, pri]), inv)
    # the default pose: eye (0, 0, 6.1) looking down -Z (Camera.cpp:24-37, main.cpp:418)
    assert np.array_equal(kat["camera_rays"][0][:, :3], np.tile(np.float32([0, 0, 6.1]), (kat["camera_uv"].shape[0], 1)))


def test_oracle_kat_fixtures_are_reproduced(oracle):
    """Sphere / square vectors (tests/golden/oracle_kat.npz) are ORACLE output -- parity unpinned: Sphere.h and Square.h
    include <GL/glut.h> and cannot be compiled here.  This only checks that the oracle on this machine reproduces them;
    the GPU tests tie the device functions to the same vectors."""
    k = np.load(os.path.join(GOLDEN, "oracle_kat.npz"))
    for prim, want in zip(k["sphere_prims"], k["sphere_out"]):
        assert np.array_equal(oracle.kat("sphere", prim, k["sphere_rays"]), want)
    for prim, want in zip(k["quad_prims"], k["quad_out"]):
        assert np.array_equal(oracle.kat("quad", prim, k["quad_rays"]), want)
    assert k["sphere_out"][0][:, 0].sum() > 100 and k["quad_out"][0][:, 0].sum() > 100
    assert k["quad_out"][1][:, 0].sum() == 0 < k["quad_out"][2][:, 0].sum()  # back face: culled unless glass (Square.h:82)


def test_ppm_loader_matches_reference_golden(hrt):
    """Host-layer PPM loader == reference imageLoader.cpp (w, h, every byte) on every shipped image."""
    want = json.load(open(os.path.join(GOLDEN, "ref_ppm.json")))
    assert len(want) >= 5
    lib = hrt.host_lib()
    lib.hrt_host_ppm_info.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    for rel, info in want.items():
        w, h, s = C.c_int32(), C.c_int32(), C.c_uint64()
        assert lib.hrt_host_ppm_info(os.path.join(hrt.ASSET_ROOT, rel).encode(), C.byref(w), C.byref(h), C.byref(s)) == 0
        assert (w.value, h.value, f"{s.value:016x}") == (info["w"], info["h"], info["fnv1a"]), rel
    assert lib.hrt_host_ppm_info(b"/nonexistent.ppm", C.byref(w), C.byref(h), C.byref(s)) < 0


def test_live_reference_parts_when_present(hrt, oracle):
    """Random triangles, boxes, optics inputs and camera poses (tests/golden/ref_live.npz), bit-exact against what the
    reference's own code returns for them: the recorded outputs, and live where oracle/_ref is built."""
    g = np.load(os.path.join(GOLDEN, "ref_live.npz"))
    live = oracle.ref_parts() is not None
    rays = g["rays"]
    for tri, want in zip(g["tris"], g["tri_out"]):
        got = oracle.kat("triangle", tri, rays)
        assert np.array_equal(got, want)
        assert not live or np.array_equal(got, oracle.kat("triangle", tri, rays, use_ref=True))
    for box, want in zip(g["boxes"], g["aabb_out"]):
        got = oracle.kat("aabb", box, rays)
        assert np.array_equal(got, want)
        assert not live or np.array_equal(got, oracle.kat("aabb", box, rays, use_ref=True))
    inp = g["optics_in"]
    assert np.array_equal(oracle.kat_optics(inp), g["optics_out"])
    assert not live or np.array_equal(oracle.kat_optics(inp), oracle.kat_optics(inp, use_ref=True))
    uv = g["uv"]
    for row, want in zip(g["cameras"], g["camera_rays_out"]):
        cam = oracle.camera_from_row(hrt, row)
        assert np.array_equal(oracle.camera_rays(cam, uv), want)
        assert not live or np.array_equal(oracle.camera_rays(cam, uv), oracle.ref_camera_rays(cam, uv))


def test_oracle_renders_match_committed_images(hrt, oracle):
    """The oracle on this machine reproduces the committed oracle pixels (same compiler flags, no FMA)."""
    g = np.load(os.path.join(GOLDEN, "oracle_images.npz"))
    for name in ["cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool"]:
        w, h, spp, seed = (int(x) for x in g[name + "_shape"])
        host = hrt.HostScene().setup(name, w / h, 1)
        desc = host.flatten()
        cam = hrt.default_camera(w / h)
        sc = oracle.OracleScene(desc)
        img = sc.render(cam, w, h, spp, seed=seed, threads=0)
        assert np.allclose(img, g[name + "_render"], rtol=1e-5, atol=1e-6), name
        aov = sc.aov(cam, w, h)
        assert np.array_equal(aov["hit"][..., 1:], g[name + "_aov_hit"][..., 1:]), name


def test_oracle_thread_modes_agree(hrt, oracle):
    """Row pool, one-thread-per-scanline (main.cpp:232-238) and single thread give identical pixels."""
    host = hrt.HostScene().setup("cornell_box", 1.0, 1)
    desc = host.flatten()
    cam = hrt.default_camera(1.0)
    sc = oracle.OracleScene(desc)
    a = sc.render(cam, 32, 32, 2, seed=3, threads=1)
    b = sc.render(cam, 32, 32, 2, seed=3, threads=4)
    c = sc.render(cam, 32, 32, 2, seed=3, threads=-1)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    d = sc.render(cam, 32, 32, 2, seed=4, threads=4)
    assert not np.array_equal(a, d)


def test_path_stream_is_uniform_and_keyed(oracle):
    s = oracle.path_stream(1, 1000, 3, 4096)
    assert 0.0 <= s.min() and s.max() < 1.0
    assert abs(s.mean() - 0.5) < 0.02 and abs(s.var() - 1 / 12) < 0.01
    assert not np.array_equal(s, oracle.path_stream(1, 1001, 3, 4096))
    assert not np.array_equal(s, oracle.path_stream(1, 1000, 4, 4096))
    assert not np.array_equal(s, oracle.path_stream(2, 1000, 3, 4096))
    assert np.array_equal(s, oracle.path_stream(1, 1000, 3, 4096))
