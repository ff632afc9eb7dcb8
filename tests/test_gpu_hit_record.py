"""The streaming kernel's path record keeps a hit visit's state in one 64-byte half: ray, t and ONE word for the closest hit
(kind | index, or kind | mesh | soup slot).  What shade() reads beyond that -- the (u, v) of a square hit, the barycentrics of a
triangle hit -- is recomputed by the hit visit from the stored ray, the stored t and the one primitive (csrc/hrt_stream.hip
sp_hit_uv_square / sp_hit_uv_triangle).  The lane-per-pixel kernel keeps all of it in registers, so a recomputed value that
differs by one bit, a mesh or a soup slot decoded wrongly, or a time that is not the ray's changes a texel, a colour or a normal
and with it a pixel.  Every comparison here is bit for bit: the streaming form (FLAG_STREAM_KERNEL) against the lane-per-pixel
form (FLAG_WAVE_KERNEL) and against the streaming proof build (FLAG_EXACT_ONLY), which takes every square through quad_t from
scalar rows in index order where the shipped build refines the filter's candidates from per-lane rows.

hrt_scene_create refuses a soup that does not fit the word's 25 bits of soup slot by the meshes' counts, before it reads an
array -- but only after hrt_init, which needs a GPU, and a description that reaches that check needs no mesh data at all: the
refusal is tested here, on the GPU, with counts alone."""
import ctypes as C

import numpy as np
import pytest

from scene_util import describe_difference

pytestmark = pytest.mark.gpu


def forms_agree(gpu, host, w, h, spp, seed, what):
    """Renders the three forms; returns the streaming frame."""
    dev = gpu.DeviceScene(host.flatten())
    cam = gpu.default_camera(w / h)
    stream, _ = dev.render(cam, w, h, spp, seed=seed, flags=gpu.FLAG_STREAM_KERNEL)
    assert dev.last_kernel().startswith("hrt_wgstream_kernel"), dev.last_kernel()
    assert np.isfinite(stream).all() and stream.max() > 0, what
    lane, _ = dev.render(cam, w, h, spp, seed=seed, flags=gpu.FLAG_WAVE_KERNEL)
    assert dev.last_kernel().startswith("hrt_trace_kernel"), dev.last_kernel()
    assert np.array_equal(stream, lane), f"{what}: streaming vs lane-per-pixel: " + describe_difference(stream, lane)
    proof, _ = dev.render(cam, w, h, spp, seed=seed, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY)
    assert dev.last_kernel().startswith("hrt_wgstream_kernel") and "exact" in dev.last_kernel(), dev.last_kernel()
    assert np.array_equal(stream, proof), f"{what}: streaming vs its proof build: " + describe_difference(stream, proof)
    return stream


def textured_squares(gpu, lit):
    """Squares whose shading reads (u, v): an image texture with a normal map on the floor, a checker on the back wall, a
    normal-mapped side wall, an image on a MOVING square (its (u, v) depend on the ray's time), a textured glass square seen from
    the front and one seen from BEHIND (right x up points away from the camera: dotRN > 0, accepted because it is glass)."""
    M = gpu.Material.make
    rng = np.random.default_rng(21)
    s = gpu.HostScene()
    s.set_sky(False)
    tex = s.add_texture(rng.integers(0, 256, (17, 23, 3), dtype=np.uint8))
    tex2 = s.add_texture(rng.integers(0, 256, (9, 5, 3), dtype=np.uint8))
    nm = s.add_normal_map(rng.integers(96, 160, (8, 8, 3), dtype=np.uint8))
    if lit:
        s.add_light((0.5, 2.5, 2.0), 0.8)
    s.add_quad((-3, -1.2, -5), (1, 0, 0), (0, 0, 1), 6, 7, M(albedo=(1, 1, 1), texture_type=gpu.TEX_IMAGE, image=tex, normal_map=nm, tex_scale=(3, 2)))
    s.add_quad((-3, -1.2, -5), (1, 0, 0), (0, 1, 0), 6, 4, M(albedo=(0.9, 0.9, 0.9), texture_type=gpu.TEX_CHECKER, checker1=(0.9, 0.1, 0.1),
                                                             checker2=(0.1, 0.1, 0.9), tex_scale=(7, 5)))
    s.add_quad((-3, -1.2, 1), (0, 0, -1), (0, 1, 0), 6, 4, M(albedo=(0.7, 0.8, 0.6), normal_map=nm, tex_scale=(2, 2)))
    s.add_quad((0.6, -0.4, -2.5), (1, 0, 0), (0, 1, 0), 1.2, 1.0, M(albedo=(1, 1, 1), texture_type=gpu.TEX_IMAGE, image=tex2, tex_scale=(1, 1),
                                                                    motion=(0.0, 0.6, 0.0)))
    s.add_quad((-1.8, -0.8, -1.5), (1, 0, 0), (0, 1, 0), 1.2, 1.4, M(albedo=(0.6, 0.9, 0.9), type=gpu.MAT_GLASS, transparency=0.6, index_medium=1.3,
                                                                     texture_type=gpu.TEX_CHECKER, checker1=(1, 1, 0.6), checker2=(0.5, 1, 1), tex_scale=(4, 4)))
    s.add_quad((0.9, 0.2, -1.0), (-1, 0, 0), (0, 1, 0), 1.3, 1.1, M(albedo=(0.9, 0.7, 0.9), type=gpu.MAT_GLASS, transparency=0.5, index_medium=1.4,
                                                                    texture_type=gpu.TEX_IMAGE, image=tex, tex_scale=(2, 3)))
    s.add_quad((-0.5, 2.2, -3), (1, 0, 0), (0, 0, 1), 1.0, 1.0, M(emissive=True, light_color=(1, 0.9, 0.8), light_intensity=6.0,
                                                                  texture_type=gpu.TEX_CHECKER, checker1=(1, 0.5, 0.5), checker2=(0.5, 0.5, 1), tex_scale=(3, 3)))
    return s


@pytest.mark.parametrize("lit", [False, True])
def test_square_uv_is_recomputed_bit_for_bit(gpu, lit):
    forms_agree(gpu, textured_squares(gpu, lit), 64, 64, 8, 5, f"textured squares, lit={lit}")


def test_plain_walls(gpu):
    forms_agree(gpu, gpu.HostScene().setup("cornell_box", 1.0, 1), 64, 64, 8, 3, "cornell_box")


def test_triangle_barycentrics_are_recomputed_bit_for_bit(gpu):
    """Vertex-coloured meshes (color_type == 0: the colour is the barycentric mix of the triangle's three vertex colours).  The
    raccoon scene's two meshes have irregular triangles, which reach the hit through mesh_exceptions, not the tree."""
    host = gpu.HostScene().setup("raccoon", 96 / 54, 1)
    forms_agree(gpu, host, 96, 54, 8, 7, "raccoon")
    M = gpu.Material.make
    s = gpu.HostScene()
    s.set_sky(False)
    s.add_quad((-4, -1.5, -8), (1, 0, 0), (0, 0, 1), 8, 10, M(albedo=(0.8, 0.8, 0.8)))
    s.add_mesh_off("mesh/rubber_duck_colored.off", M(albedo=(0.9, 0.9, 0.9)))
    forms_agree(gpu, s, 96, 54, 8, 7, "rubber_duck_colored.off")


def test_more_meshes_than_a_queue_entry_carries(gpu):
    """Six meshes of different materials (diffuse, mirror, glass, face-coloured): beyond four the meshes to walk travel in the
    record's walk group, not in the T-queue entry, and a chunk of mesh hits mixes meshes -- the mesh in the hit word is per lane."""
    M = gpu.Material.make
    rng = np.random.default_rng(8)
    tet = np.array([[0, 0, 0], [1.2, 0, 0], [0.6, 1.2, 0.2], [0.6, 0.4, 1.2]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)
    mats = [M(albedo=(0.9, 0.3, 0.2)), M(albedo=(0.8, 0.8, 0.8), type=gpu.MAT_MIRROR), M(albedo=(0.7, 0.9, 0.9), type=gpu.MAT_GLASS, transparency=0.6, index_medium=1.4),
            M(albedo=(0.2, 0.8, 0.3)), M(albedo=(0.3, 0.3, 0.9), transparency=0.4), M(albedo=(0.9, 0.9, 0.2))]
    s = gpu.HostScene()
    s.set_sky(False)
    s.add_light((0.0, 3.0, 2.0), 0.8)
    s.add_quad((-5, -1.5, -8), (1, 0, 0), (0, 0, 1), 10, 10, M(albedo=(0.8, 0.8, 0.8)))
    for i, m in enumerate(mats):
        at = np.float32([-2.4 + 1.6 * (i % 3), -1.4 + 1.5 * (i // 3), -3.5 + 0.7 * (i % 2)])
        s.add_mesh(tet + at, tri, m, face_colors=rng.uniform(0.1, 1, (4, 3)).astype(np.float32) if i in (3, 5) else None)
    forms_agree(gpu, s, 64, 64, 8, 2, "six meshes")


def test_hit_word_round_trip(gpu):
    """kind | index (30 bits) for a sphere or a square, kind | mesh (5 bits) | soup slot (25 bits) for a mesh hit: every field at
    its ends, the device's pack against this statement of the layout and its unpack against the input."""
    top = (1 << 25) - 1   # HRT_MAX_SOUP_SLOTS - 1: the largest slot hrt_scene_create admits
    cases = [(0, 0, 0), (1, 0, 0), (1, 127, 0), (2, 0, 0), (2, 63, 0), (2, (1 << 30) - 1, 0), (1, (1 << 30) - 1, 0),
             (3, 0, 0), (3, 31, 0), (3, 0, top), (3, 31, top), (3, 31, 1), (3, 1, top - 1), (3, 17, 0x0155AAAA), (3, 10, 1 << 24)]
    a = np.array(cases, np.uint32)
    out = gpu.debug_kat(gpu.KAT_HITWORD, a.view(np.float32)).view(np.uint32)
    for (kind, index, slot), (word, k2, i2, s2) in zip(cases, out.tolist()):
        want = (3 << 30) | (index << 25) | slot if kind == 3 else (kind << 30) | index
        assert word == want, (kind, index, slot, hex(word), hex(want))
        assert (k2, i2, s2) == (kind, index, slot if kind == 3 else 0), (kind, index, slot, k2, i2, s2)


def test_mesh_31_of_32_is_decoded(gpu):
    """32 meshes, the most a scene may have: the last one's hits carry mesh 31 in the word."""
    M = gpu.Material.make
    tet = np.array([[0, 0, 0], [0.5, 0, 0], [0.25, 0.5, 0.1], [0.25, 0.2, 0.5]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)
    s = gpu.HostScene()
    s.set_sky(False)
    for i in range(31):   # small ones at the back, the last one large and in front: most mesh hits are mesh 31's
        s.add_mesh(tet + np.float32([-2.5 + 0.7 * (i % 8), -1.2 + 0.7 * (i // 8), -6.0]), tri, M(albedo=(0.3 + 0.02 * i, 0.5, 0.4)))
    s.add_mesh(tet * np.float32(3.0) + np.float32([-0.8, -0.8, -3.0]), tri, M(albedo=(0.9, 0.2, 0.2)),
               face_colors=np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]]))
    forms_agree(gpu, s, 64, 64, 8, 4, "32 meshes")


def test_a_soup_beyond_the_slot_field_is_refused_by_its_counts(gpu):
    """2^25 + 1 rows, stated by counts only (every array pointer NULL): refused with a message before any array is read."""
    lib = gpu.device_lib()

    class Mesh(C.Structure):   # include/hrt.h hrt_mesh
        _fields_ = [("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("positions", C.c_void_p), ("indices", C.c_void_p),
                    ("color_type", C.c_int32), ("vert_colors", C.c_void_p), ("face_colors", C.c_void_p), ("aabb_min", C.c_float * 3),
                    ("aabb_max", C.c_float * 3), ("material", C.c_int32), ("kd_root", C.c_uint32), ("kd_min", C.c_float * 3),
                    ("kd_max", C.c_float * 3), ("n_kd_units", C.c_uint32), ("kd_units", C.c_void_p), ("n_leaf_tris", C.c_uint32),
                    ("leaf_tris", C.c_void_p), ("n_exceptions", C.c_uint32), ("exceptions", C.c_void_p)]

    class Desc(C.Structure):   # include/hrt.h hrt_scene_desc
        _fields_ = [("n_materials", C.c_uint32), ("materials", C.c_void_p), ("n_spheres", C.c_uint32), ("spheres", C.c_void_p),
                    ("n_quads", C.c_uint32), ("quads", C.c_void_p), ("n_meshes", C.c_uint32), ("meshes", C.c_void_p),
                    ("n_lights", C.c_uint32), ("lights", C.c_void_p), ("n_images", C.c_uint32), ("images", C.c_void_p),
                    ("dark_sky", C.c_int32), ("skybox_image", C.c_int32)]

    meshes = (Mesh * 2)()
    meshes[0].n_triangles = 1 << 25
    meshes[0].n_leaf_tris = 1 << 25      # exactly the limit on its own ...
    meshes[1].n_triangles = 5
    meshes[1].n_exceptions = 1           # ... and one irregular triangle more
    d = Desc()
    d.n_meshes = 2
    d.meshes = C.cast(meshes, C.c_void_p)
    d.skybox_image = -1
    out = C.c_void_p()
    lib.hrt_scene_create.restype = C.c_int
    rc = lib.hrt_scene_create(C.byref(d), C.byref(out))
    msg = lib.hrt_last_error().decode()
    assert rc == -1 and out.value is None, (rc, msg)   # HRT_ERR_INVALID
    assert "HRT_MAX_SOUP_SLOTS" in msg and str((1 << 25) + 1) in msg, msg


@pytest.mark.parametrize("spp", [1, 4])
def test_units_as_small_as_the_pool_are_deterministic(gpu, spp):
    """cornell_mesh at 128x72 with 1 and 4 samples: work units no larger than the pool.  Twenty launches of the streaming form give
    one frame, and it is the lane-per-pixel form's and the proof build's."""
    w, h = 128, 72
    host = gpu.HostScene().setup("cornell_mesh", w / h, 1)
    dev = gpu.DeviceScene(host.flatten())
    cam = gpu.default_camera(w / h)
    first, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_STREAM_KERNEL)
    assert dev.last_kernel().startswith("hrt_wgstream_kernel")
    for k in range(19):
        again, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_STREAM_KERNEL)
        assert np.array_equal(first, again), f"launch {k + 2}: " + describe_difference(first, again)
    lane, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_WAVE_KERNEL)
    assert np.array_equal(first, lane), describe_difference(first, lane)
    proof, _ = dev.render(cam, w, h, spp, seed=13, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY)
    assert np.array_equal(first, proof), describe_difference(first, proof)
