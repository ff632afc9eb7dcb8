"""The parity and exactness bars of test_gpu_parity.py / test_gpu_exact.py along three axes they did not walk:

  * CAMERAS.  Every other render of the suite looks down -Z from (0, 0, 6.1).  In real use the pose comes from the reference's
    trackball, as float casts of an fp64 inverse modelview: a moved eye and a basis that is not exactly
    orthonormal.  Here: trackball orbits (walls seen from behind, zoomed in and out), exact axis-aligned bases at odd frame
    sizes (the centre pixel's ray has exact zero components), eyes inside the Cornell box, inside a mesh's root KD cell, ON its
    root split plane (a row of rays in the plane), inside a glass sphere, a far narrow frustum, a 150 degree one, one-row and
    one-column frames.  Scenes far from the origin and at other scales walk the filter margins (err_abs grows with |eye|).
  * CAMERA SWITCHES between launches on one hrt_scene: each frame must be the frame its own camera gives alone.
  * COLOURS above 1, and colours whose products overflow fp32: the exact path pruning must then be off (hrt_api.hip prune_ok).

Per (scene, pose): hrt_camera accepted, the four first-hit AOVs identical to the oracle, a small render within the stated 1e-6
bar, the shipped kernels bit for bit the proof builds (FLAG_EXACT_ONLY, and FLAG_MESH_BRUTE for meshes), all kernel forms equal.
"""
import ctypes as C

import numpy as np
import pytest

from scene_util import describe_difference, many_spheres, many_squares, open_box, overflow_scene, overlapping_soup, placed_camera
from test_gpu_parity import aov, assert_pixels_agree

pytestmark = pytest.mark.gpu

THREADS = 16                         # oracle threads (explicit: 0 means every hardware thread)
AOV_SIZE = (97, 55)                  # odd: the centre pixel's ray is u = v = 0.5 exactly
RENDER_SIZE, RENDER_SPP = (63, 35), 3
EXACT_SIZE, EXACT_SPP = (321, 181), 4
SCENE_ASPECT = 16 / 9                # the Cornell walls depend on it; one scene serves every frame size


class _Sphere(C.Structure):  # hrt_sphere (include/hrt.h)
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("material", C.c_int32)]


# ---------------------------------------------------------------------------------------------------------- poses
def _rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def camera_from_inverse_modelview(gpu, mi, aspect, fovy=45.0):
    """hrt_camera exactly as INTEGRATION.md fills it: float casts of the fp64 inverse modelview (row-major 4x4 here; its
    columns 0..2 are right, up, -forward, column 3 the eye) and Camera's perspective constants."""
    cam = gpu.Camera()
    for k in range(3):
        cam.right[k] = np.float32(mi[k, 0])
        cam.up[k] = np.float32(mi[k, 1])
        cam.forward[k] = np.float32(-mi[k, 2])
        cam.eye[k] = np.float32(mi[k, 3])
    cam.fovy_deg, cam.aspect, cam.znear, cam.zfar = fovy, aspect, 4.1, 10000.0
    return cam


def trackball_inverse(yaw=0.0, pitch=0.0, roll=0.0, dist=6.1, target=(0.0, 0.0, 0.0)):
    """fp64 inverse of modelview = translate(0, 0, -dist) . R . translate(-target): the default pose orbited about `target`."""
    r = _rot(2, roll) @ _rot(0, pitch) @ _rot(1, yaw)
    mi = np.eye(4)
    mi[:3, :3] = r.T
    mi[:3, 3] = np.asarray(target, np.float64) + r.T @ np.array([0.0, 0.0, dist])
    return mi


def look_inverse(eye, forward, up):
    """fp64 inverse modelview of an eye looking along `forward` (exact when the arguments are axis vectors)."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    mi = np.eye(4)
    mi[:3, 0], mi[:3, 1], mi[:3, 2], mi[:3, 3] = r, u, -f, np.asarray(eye, np.float64)
    return mi


AXES = {"+x": ((1, 0, 0), (0, 1, 0)), "-x": ((-1, 0, 0), (0, 1, 0)), "+y": ((0, 1, 0), (0, 0, -1)),
        "-y": ((0, -1, 0), (0, 0, 1)), "+z": ((0, 0, 1), (0, 1, 0)), "-z": ((0, 0, -1), (0, 1, 0))}

# name -> (inverse modelview, fovy, sizes or None for the defaults)
GENERIC_POSES = {
    "orbit_yaw35_pitch20": (trackball_inverse(35, 20), 45.0, None),
    "orbit_from_behind": (trackball_inverse(180, 10, 5), 45.0, None),           # the Cornell walls seen from their backs
    "orbit_zoomed_in_rolled": (trackball_inverse(-60, -25, 30, dist=3.0), 45.0, None),
    "orbit_zoomed_out": (trackball_inverse(15, 45, dist=14.0), 45.0, None),
    "far_narrow": (trackball_inverse(20, 10, dist=1000.0), 2.0, None),          # |eye| = 1e3, fovy 2 degrees
    "wide": (trackball_inverse(10, -5, dist=6.1), 150.0, None),
    "one_row": (trackball_inverse(25, 5), 45.0, (257, 1)),
    "one_column": (trackball_inverse(25, 5), 45.0, (1, 257)),
}
for _k, (_f, _u) in AXES.items():   # axis-aligned, exact basis, eye 6.1 back along the view axis
    GENERIC_POSES["axis" + _k] = (look_inverse(-6.1 * np.asarray(_f, np.float64), _f, _u), 45.0, None)


def _desc_struct(desc):
    from test_host_layer import SceneDesc
    return C.cast(desc, C.POINTER(SceneDesc)).contents


def _mesh(desc, m):
    from test_host_layer import MeshDesc
    return C.cast(_desc_struct(desc).meshes, C.POINTER(MeshDesc))[m]


def root_split(desc):
    """(split, axis) of the root of mesh 0's flattened tree (an inner nodelet: f32 split, u32 axis, left, right)."""
    m = _mesh(desc, 0)
    units = np.ctypeslib.as_array(C.cast(m.kd_units, C.POINTER(C.c_uint32)), shape=(m.n_kd_units, 4))
    return float(units[m.kd_root, 0:1].view(np.float32)[0]), int(units[m.kd_root, 1])


def scene_poses(gpu, name, desc):
    """Poses that depend on the scene: inside the box, inside a mesh's root KD cell / on its root split plane, inside glass."""
    out = {}
    if name in ("cornell_box", "cornell_mesh"):
        out["inside_box_corner"] = (look_inverse((-3.0, -1.6, 1.6), (5.0, 2.6, -3.1), (0, 1, 0)), 45.0, None)
    d = _desc_struct(desc)
    if d.n_meshes:
        m = _mesh(desc, 0)
        lo, hi = np.array(m.kd_min[:], np.float64), np.array(m.kd_max[:], np.float64)
        centre = (lo + hi) / 2
        out["inside_kd_root_cell"] = (look_inverse(centre, (0.3, -0.2, -1.0), (0, 1, 0)), 45.0, None)
        if not m.kd_root & 0x80000000:   # an inner root: eye ON its split plane, the camera's up along the split axis
            split, axis = root_split(desc)
            eye = centre.astype(np.float32).astype(np.float64)
            eye[axis] = split
            up = np.eye(3)[axis]
            fwd = -np.eye(3)[2] if axis != 2 else -np.eye(3)[0]
            out["on_kd_root_split_plane"] = (look_inverse(eye, fwd, up), 45.0, None)
    spheres = C.cast(d.spheres, C.POINTER(_Sphere))
    mats = C.cast(d.materials, C.POINTER(gpu.Material))
    glass = [spheres[i] for i in range(d.n_spheres) if mats[spheres[i].material].type == gpu.MAT_GLASS]
    if glass:
        g = max(glass, key=lambda s: s.radius)
        eye = np.array(g.center[:], np.float64) + 0.2 * g.radius
        out["inside_glass_sphere"] = (look_inverse(eye, (-0.2, 0.1, -1.0), (0, 1, 0)), 45.0, None)
    return out


# ---------------------------------------------------------------------------------------------------------- scenes
_CACHE = {}


def _scene(gpu, name):
    if name not in _CACHE:
        if name == "many_squares":
            host = many_squares(gpu, 70, 5)
        elif name == "many_spheres":
            host = many_spheres(gpu, 65, 2)
        else:
            host = gpu.HostScene().setup(name, SCENE_ASPECT, 1)
        desc = host.flatten()
        _CACHE[name] = (host, desc, gpu.DeviceScene(desc))
    return _CACHE[name]


VIEW_SCENES = ["cornell_box", "cornell_mesh", "backrooms_pool", "random_spheres", "many_squares", "many_spheres"]
SCENE_POSES = {"cornell_box": ["inside_box_corner", "inside_glass_sphere"],
               "cornell_mesh": ["inside_box_corner", "inside_kd_root_cell", "on_kd_root_split_plane", "inside_glass_sphere"],
               "backrooms_pool": ["inside_kd_root_cell", "on_kd_root_split_plane"],
               "random_spheres": ["inside_glass_sphere"], "many_squares": ["inside_kd_root_cell"],
               "many_spheres": ["inside_glass_sphere"]}
CASES = [(s, p) for s in VIEW_SCENES for p in list(GENERIC_POSES) + SCENE_POSES[s]]


def same_bits(a, b):
    """Identical frames, NaNs included (same NaN mask, same values elsewhere)."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def check_view(gpu, oracle, desc, dev, cam_at, what, has_mesh, sizes=None):
    """The whole bar for one scene and one pose.  cam_at(aspect) -> hrt_camera."""
    aw, ah = sizes or AOV_SIZE
    rw, rh = sizes or RENDER_SIZE
    ew, eh = sizes or EXACT_SIZE
    ref = oracle.OracleScene(desc)
    cam = cam_at(aw / ah)
    want = ref.aov(cam, aw, ah)
    for k, key in enumerate(("hit", "normal", "albedo", "emission")):
        got = aov(gpu, dev, cam, aw, ah, k)
        assert np.array_equal(got, want[key]), f"{what} AOV {key}: {describe_difference(got, want[key])}"
    cam = cam_at(rw / rh)
    img, _ = dev.render(cam, rw, rh, RENDER_SPP, seed=5)
    assert np.isfinite(img).all(), f"{what}: non-finite pixels"
    assert_pixels_agree(img, ref.render(cam, rw, rh, RENDER_SPP, seed=5, threads=THREADS), f"{what} (oracle)")
    cam = cam_at(ew / eh)
    frames = {}
    for form, label in ((gpu.FLAG_STREAM_KERNEL, "streaming"), (gpu.FLAG_WAVE_KERNEL, "lane-per-pixel")):
        a, _ = dev.render(cam, ew, eh, EXACT_SPP, seed=3, flags=form)
        b, _ = dev.render(cam, ew, eh, EXACT_SPP, seed=3, flags=form | gpu.FLAG_EXACT_ONLY)
        assert np.array_equal(a, b), f"{what} ({label}): filtered vs exact-only: {describe_difference(a, b)}"
        frames[label] = a
    assert np.array_equal(frames["streaming"], frames["lane-per-pixel"]), f"{what}: kernel forms: {describe_difference(frames['streaming'], frames['lane-per-pixel'])}"
    if has_mesh:
        c, _ = dev.render(cam, ew, eh, EXACT_SPP, seed=3, flags=gpu.FLAG_STREAM_KERNEL | gpu.FLAG_EXACT_ONLY | gpu.FLAG_MESH_BRUTE)
        assert np.array_equal(frames["streaming"], c), f"{what}: KD walk vs every triangle: {describe_difference(frames['streaming'], c)}"
        d, _ = dev.render(cam, ew, eh, EXACT_SPP, seed=3, flags=gpu.FLAG_DUAL_KERNEL)
        assert np.array_equal(frames["streaming"], d), f"{what}: two-stream kernel: {describe_difference(frames['streaming'], d)}"
    return frames["streaming"]


@pytest.mark.parametrize("name,pose", CASES)
def test_moved_cameras_keep_parity_and_exactness(gpu, oracle, name, pose):
    """Every (scene, pose): accepted by make_camera, first hits identical to the oracle, pixels within 1e-6, shipped == proof
    builds bit for bit, all kernel forms equal."""
    host, desc, dev = _scene(gpu, name)
    poses = dict(GENERIC_POSES, **scene_poses(gpu, name, desc))
    mi, fovy, sizes = poses[pose]
    if pose == "on_kd_root_split_plane":
        # the pose reaches what it is named for: the AOV rays of the centre row start ON the plane and stay in it
        split, axis = root_split(desc)
        aw, ah = AOV_SIZE
        cam = camera_from_inverse_modelview(gpu, mi, aw / ah, fovy)
        uv = np.stack([(np.arange(aw, dtype=np.float32) + np.float32(0.5)) / np.float32(aw),
                       np.full(aw, (np.float32(ah // 2) + np.float32(0.5)) / np.float32(ah), np.float32)], axis=1)
        rays = gpu.debug_kat(gpu.KAT_CAMERA, uv, cam=cam)
        assert (rays[:, axis] == np.float32(split)).all() and (rays[:, 3 + axis] == 0.0).all(), \
            f"centre row off the split plane: origin {rays[0, :3]}, direction components {np.unique(rays[:, 3 + axis])[:5]}"
    check_view(gpu, oracle, desc, dev, lambda aspect: camera_from_inverse_modelview(gpu, mi, aspect, fovy), f"{name} / {pose}",
               _desc_struct(desc).n_meshes > 0, sizes)


@pytest.mark.parametrize("name", ["cornell_mesh", "backrooms_pool"])
@pytest.mark.parametrize("pose", ["orbit_yaw35_pitch20", "orbit_from_behind"])
def test_moved_cameras_at_full_hd(gpu, name, pose):
    """As test_gpu_exact.py::FULL, from two trackball poses: 1920 x 1080 x 4 spp, shipped vs FLAG_EXACT_ONLY, both forms."""
    host, desc, dev = _scene(gpu, name)
    mi, fovy, _ = GENERIC_POSES[pose]
    w, h = 1920, 1080
    cam = camera_from_inverse_modelview(gpu, mi, w / h, fovy)
    for form, label in ((gpu.FLAG_STREAM_KERNEL, "streaming"), (gpu.FLAG_WAVE_KERNEL, "lane-per-pixel")):
        a, _ = dev.render(cam, w, h, 4, seed=3, flags=form)
        b, _ = dev.render(cam, w, h, 4, seed=3, flags=form | gpu.FLAG_EXACT_ONLY)
        assert np.isfinite(a).all() and a.max() > 0
        assert np.array_equal(a, b), f"{name} / {pose} ({label}) 1080p: filtered vs exact-only: {describe_difference(a, b)}"


# ---------------------------------------------------------------------------------------- far from the origin, other scales
PLACEMENTS = [("offset_1e2", (100.0, 50.0, -70.0), 1.0), ("offset_3e3", (3000.0, -1500.0, 2100.0), 1.0),
              ("scale_1e-2", None, 0.01), ("scale_1e2", None, 100.0)]


@pytest.mark.parametrize("kind", ["many_squares", "many_spheres", "soup"])
@pytest.mark.parametrize("label,offset,world_scale", PLACEMENTS)
def test_scenes_far_from_the_origin_and_at_other_scales(gpu, oracle, kind, label, offset, world_scale):
    """err_abs and the |ta| terms of the filter margins well outside the range the default scenes reach.  The reference's
    absolute EPSILON makes these frames differ from the unmoved ones (acne): parity is with the oracle on the same scene."""
    if kind == "many_squares":
        host = many_squares(gpu, 70, 5, offset=offset, world_scale=world_scale)
    elif kind == "many_spheres":
        host = many_spheres(gpu, 65, 2, offset=offset, world_scale=world_scale)
    else:
        host = overlapping_soup(gpu, offset=offset, world_scale=world_scale)
    desc = host.flatten()
    dev = gpu.DeviceScene(desc)
    check_view(gpu, oracle, desc, dev, lambda aspect: placed_camera(gpu, aspect, offset, world_scale), f"{kind} {label}",
               _desc_struct(desc).n_meshes > 0)


# -------------------------------------------------------------------------------------------------- camera switches
SWITCH_SIZE, SWITCH_SPP = (1920, 1080), 8


def _switch_setup(gpu):
    w, h = SWITCH_SIZE
    host = gpu.HostScene().setup("cornell_mesh", w / h, 1)
    desc = host.flatten()
    cam_a = gpu.default_camera(w / h)
    cam_b = camera_from_inverse_modelview(gpu, trackball_inverse(20, 10), w / h)
    return host, desc, cam_a, cam_b


def _tiles_alone(gpu, desc, cam, seed):
    """The tiles of one synchronous launch on a fresh scene."""
    import torch
    w, h = SWITCH_SIZE
    dev = gpu.DeviceScene(desc)
    buf = torch.zeros((gpu.tiles_total(w, h), 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, SWITCH_SPP, seed, 0, 0, 1, buf.data_ptr(), 0)
    torch.cuda.synchronize()
    dev.check_last_launch()
    return buf.cpu().numpy()


def test_camera_switch_between_launches_on_two_streams(gpu):
    """hrt_render_tiles with camera A on stream s1, then camera B on s2, no host wait: the copy of B's camera block must not
    land while A's launch still reads the block."""
    import torch
    host, desc, cam_a, cam_b = _switch_setup(gpu)
    want_a, want_b = _tiles_alone(gpu, desc, cam_a, 11), _tiles_alone(gpu, desc, cam_b, 12)
    w, h = SWITCH_SIZE
    dev = gpu.DeviceScene(desc)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.zeros((gpu.tiles_total(w, h), 64, 3), dtype=torch.float32, device="cuda")
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    dev.render_tiles(cam_a, w, h, SWITCH_SPP, 11, 0, 0, 1, a.data_ptr(), s1.cuda_stream)
    dev.render_tiles(cam_b, w, h, SWITCH_SPP, 12, 0, 0, 1, b.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    dev.check_last_launch()
    ga, gb = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(ga, want_a), f"camera A on s1: {describe_difference(ga, want_a)}"
    assert np.array_equal(gb, want_b), f"camera B on s2: {describe_difference(gb, want_b)}"


def test_camera_switches_on_one_stream(gpu):
    """A, B, A on one stream with no host wait: the staged host camera block is not read after it has been overwritten."""
    import torch
    host, desc, cam_a, cam_b = _switch_setup(gpu)
    want = [_tiles_alone(gpu, desc, c, s) for c, s in ((cam_a, 11), (cam_b, 12), (cam_a, 13))]
    w, h = SWITCH_SIZE
    dev = gpu.DeviceScene(desc)
    s1 = torch.cuda.Stream()
    bufs = [torch.zeros((gpu.tiles_total(w, h), 64, 3), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for buf, (cam, seed) in zip(bufs, ((cam_a, 11), (cam_b, 12), (cam_a, 13))):
        dev.render_tiles(cam, w, h, SWITCH_SPP, seed, 0, 0, 1, buf.data_ptr(), s1.cuda_stream)
    torch.cuda.synchronize()
    dev.check_last_launch()
    for k, (buf, ref) in enumerate(zip(bufs, want)):
        got = buf.cpu().numpy()
        assert np.array_equal(got, ref), f"launch {k} ({'ABA'[k]}): {describe_difference(got, ref)}"


def test_a_larger_batch_of_views_on_a_second_stream_grows_the_blocks_under_the_previous_batch(gpu):
    """hrt_render_views_device with one view on s1, then at once five on s2, no host wait: the scene's per-view blocks (and tile
    sums) must grow while the first batch's launch may still be reading the old ones.  Then two views on s1 again: the grown blocks
    reused across streams.  Every frame is hrt_render's bit for bit."""
    import torch
    w, h, spp = 16, 16, 2
    dev = gpu.DeviceScene(gpu.HostScene().setup("cornell_mesh", 1.0, 1).flatten())  # a scene of its own: its blocks start empty
    cams = [camera_from_inverse_modelview(gpu, trackball_inverse(15.0 * k, 4.0 * k), 1.0) for k in range(8)]
    seeds = [5 + 3 * k for k in range(8)]
    want = np.stack([dev.render(cam, w, h, spp, seed)[0] for cam, seed in zip(cams, seeds)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = torch.empty((8, h, w, 3), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        dev.render_views(cams[:1], w, h, spp, seeds[:1], out=got[:1])
    with torch.cuda.stream(s2):
        dev.render_views(cams[1:6], w, h, spp, seeds[1:6], out=got[1:6])
    torch.cuda.synchronize()
    dev.check_last_launch()
    first = got[:6].cpu().numpy()
    assert same_bits(first, want[:6]), describe_difference(first.reshape(-1, w, 3), want[:6].reshape(-1, w, 3))
    with torch.cuda.stream(s1):
        dev.render_views(cams[6:], w, h, spp, seeds[6:], out=got[6:])
    torch.cuda.synchronize()
    dev.check_last_launch()
    last = got[6:].cpu().numpy()
    assert same_bits(last, want[6:]), describe_difference(last.reshape(-1, w, 3), want[6:].reshape(-1, w, 3))


def test_aov_with_another_camera_while_a_launch_is_in_flight(gpu):
    """hrt_render_aov with camera B while a launch with camera A runs on a non-blocking stream: neither sees the other's camera."""
    import torch
    host, desc, cam_a, cam_b = _switch_setup(gpu)
    want_a = _tiles_alone(gpu, desc, cam_a, 11)
    w, h = SWITCH_SIZE
    aw, ah = AOV_SIZE
    want_aov = aov(gpu, gpu.DeviceScene(desc), cam_b, aw, ah, 0)
    dev = gpu.DeviceScene(desc)
    s1 = torch.cuda.Stream()
    a = torch.zeros((gpu.tiles_total(w, h), 64, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.render_tiles(cam_a, w, h, SWITCH_SPP, 11, 0, 0, 1, a.data_ptr(), s1.cuda_stream)
    got_aov = aov(gpu, dev, cam_b, aw, ah, 0)
    torch.cuda.synchronize()
    dev.check_last_launch()
    ga = a.cpu().numpy()
    assert np.array_equal(ga, want_a), f"camera A launch beside an AOV of camera B: {describe_difference(ga, want_a)}"
    assert np.array_equal(got_aov, want_aov), f"AOV of camera B beside a launch of camera A: {describe_difference(got_aov, want_aov)}"
    again, _ = dev.render(cam_a, 64, 36, 2, seed=4)   # and the trace launches' own camera block is still A's
    assert np.array_equal(again, gpu.DeviceScene(desc).render(cam_a, 64, 36, 2, seed=4)[0])


def test_camera_switch_on_a_multi_scene(gpu):
    """MultiScene.render (two slots sharing GPU 0) with A, then B: each frame is hrt_render's frame of its camera."""
    host, desc, cam_a, cam_b = _switch_setup(gpu)
    w, h = SWITCH_SIZE
    ms = gpu.MultiScene(desc, [0, 0])
    try:
        for cam, seed, label in ((cam_a, 11, "A"), (cam_b, 12, "B")):
            got, _ = ms.render(cam, w, h, SWITCH_SPP, seed=seed)
            want, _ = gpu.DeviceScene(desc).render(cam, w, h, SWITCH_SPP, seed=seed)
            assert np.array_equal(got, want), f"multi scene, camera {label}: {describe_difference(got, want)}"
    finally:
        ms.close()


# ------------------------------------------------------------------------------------------- colour range and pruning
def _in_range_scene(gpu, lit):
    M = gpu.Material.make
    s = open_box(gpu, (3.5, 2.0, 4.0), M(albedo=(0, 0, 0), emissive=True, light_color=(20, 18, 12), light_intensity=500.0),
             light=(20.0, 15.0, 10.0) if lit else None)
    rng = np.random.default_rng(31)
    s.add_quad((-1.5, -1.4, -3), (1, 0, 0.2), (0, 1, 0.1), 1.2, 1.0,
               M(albedo=(1, 1, 1), texture_type=gpu.TEX_CHECKER, checker1=(4, 0.5, 2), checker2=(0.2, 3.5, 4), tex_scale=(3, 3)))
    s.add_quad((0.6, -1.0, -2.0), (0, 1, 0), (0.3, 0, 1), 0.8, 0.8,
               M(albedo=(0, 0, 0), emissive=True, texture_type=gpu.TEX_CHECKER, checker1=(4, 4, 4), checker2=(1, 2, 3), light_intensity=2500.0))
    s.add_sphere((0.9, -0.9, -1.5), 0.5, M(albedo=(2.5, 3.9, 1.2)))
    s.add_sphere((-0.8, -0.7, -0.8), 0.45, M(albedo=(1.5, 1.5, 3.0), type=gpu.MAT_GLASS, transparency=0.7, index_medium=1.4))
    v = np.array([[-0.3, -1.5, -2.5], [0.5, -1.5, -2.5], [0.1, -0.6, -2.7], [0.1, -1.2, -1.9]], np.float32)
    t = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.uint32)
    s.add_mesh(v, t, M(albedo=(1, 1, 1)), face_colors=rng.uniform(0, 4, (4, 3)).astype(np.float32))
    return s


@pytest.mark.parametrize("lit", [False, True], ids=["unlit", "lit"])
def test_colours_above_one_keep_parity_and_exactness(gpu, oracle, lit):
    """Albedos, checker and face colours up to 4, emission products up to 1e4, light colours up to 20: every pixel finite,
    within 1e-6 of the oracle relative to |ref|, and the pruned kernels give the proof builds' bits."""
    desc = _in_range_scene(gpu, lit).flatten()
    dev = gpu.DeviceScene(desc)
    frame = check_view(gpu, oracle, desc, dev, lambda aspect: gpu.default_camera(aspect), f"colours above 1 ({'lit' if lit else 'unlit'})", True)
    assert np.isfinite(frame).all() and frame.max() > 10.0


@pytest.mark.parametrize("mechanism,lit", [("emission", False), ("emission", True), ("throughput", False)],
                         ids=["emission_overflow-unlit", "emission_overflow-lit", "throughput_overflow-unlit"])
def test_overflowing_colours_switch_the_pruning_off(gpu, monkeypatch, mechanism, lit):
    """Exact path pruning drops terms that are throughput x 0; that is exact only while no such product can be inf x 0 or
    0 x inf.  Where a colour product can overflow fp32 the pruned kernels must give the frame of the unpruned proof builds bit
    for bit, NaNs included, and the frame of a scene created with HRT_PRUNE=0.  No oracle comparison here: the recursion of the
    reference and the throughput form of the kernels overflow in different places, so NaN / inf land on different pixels."""
    host = overflow_scene(gpu, mechanism, lit)
    desc = host.flatten()
    dev = gpu.DeviceScene(desc)
    monkeypatch.setenv("HRT_PRUNE", "0")
    unpruned = gpu.DeviceScene(desc)
    monkeypatch.delenv("HRT_PRUNE")
    w, h, spp = 96, 54, 8
    cam = gpu.default_camera(w / h)
    for form, label in ((gpu.FLAG_STREAM_KERNEL, "streaming"), (gpu.FLAG_WAVE_KERNEL, "lane-per-pixel")):
        a, _ = dev.render(cam, w, h, spp, seed=2, flags=form)
        b, _ = dev.render(cam, w, h, spp, seed=2, flags=form | gpu.FLAG_EXACT_ONLY)
        c, _ = unpruned.render(cam, w, h, spp, seed=2, flags=form)
        assert not np.isfinite(b).all(), "the scene must overflow somewhere for this test to mean anything"
        assert same_bits(a, b), f"{mechanism} ({label}, {'lit' if lit else 'unlit'}): shipped vs exact-only: {describe_difference(a, b)}"
        assert same_bits(a, c), f"{mechanism} ({label}, {'lit' if lit else 'unlit'}): shipped vs HRT_PRUNE=0: {describe_difference(a, c)}"
