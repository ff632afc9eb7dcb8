"""Synthetic scenes shared by the GPU tests (host layer only: no GPU, no oracle)."""
import numpy as np


def _placement(offset, world_scale):
    """(point, length, motion) maps of a scene moved to `offset` and scaled by `world_scale` about the origin.  At the defaults
    they return their argument itself, so that the default scenes stay bit-identical."""
    if offset is None and world_scale == 1.0:
        return (lambda p: p), (lambda r: r), (lambda m: m)
    o = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
    k = float(world_scale)
    return (lambda p: tuple(float(x) for x in np.asarray(p, np.float64) * k + o)), (lambda r: float(r) * k), \
        (lambda m: tuple(float(x) * k for x in m))


def placed_camera(gpu, aspect, offset=None, world_scale=1.0):
    """default_camera moved with a scene placed by `offset` / `world_scale`."""
    cam = gpu.default_camera(aspect)
    at, _, _ = _placement(offset, world_scale)
    cam.eye[:] = at(tuple(cam.eye))
    return cam


def many_squares(gpu, n_quads, n_meshes, offset=None, world_scale=1.0):
    """A random cloud of small tilted squares (some glass, some mirror, some moving) over a floor, tetrahedra as meshes,
    one point light: exercises the 32-bit / 64-bit candidate masks of the square filter and the bypass beyond 64.
    `offset` / `world_scale` move and scale the whole scene (placed_camera moves the camera with it)."""
    M = gpu.Material.make
    at, ln, mv = _placement(offset, world_scale)
    rng = np.random.default_rng(100 + n_quads)
    s = gpu.HostScene()
    s.set_sky(False)
    s.add_light(at((0.0, 4.0, 3.0)), ln(1.0))
    s.add_quad(at((-6, -2, -8)), (1, 0, 0), (0, 0, 1), ln(12), ln(12), M(albedo=(0.8, 0.8, 0.8)))
    for i in range(n_quads - 1):
        c = rng.uniform((-3, -1.5, -6), (3, 2.0, -1))
        r = rng.normal(size=3); u = np.cross(r, rng.normal(size=3))
        kind = i % 5
        mat = M(albedo=tuple(rng.uniform(0.2, 1, 3)), type=gpu.MAT_GLASS if kind == 0 else (gpu.MAT_MIRROR if kind == 1 else gpu.MAT_DIFFUSE),
                transparency=0.5 if kind == 0 else 0.0, index_medium=1.4, motion=mv((0.0, 0.3, 0.0)) if kind == 2 else (0, 0, 0))
        s.add_quad(at(tuple(c)), tuple(r), tuple(u), ln(float(rng.uniform(0.3, 0.9))), ln(float(rng.uniform(0.3, 0.9))), mat)
    tet = np.array([[0, 0, 0], [0.6, 0, 0], [0.3, 0.6, 0.1], [0.3, 0.2, 0.6]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)
    for i in range(n_meshes):
        v = tet + rng.uniform((-3, -1.5, -5), (3, 1.5, -1.5)).astype(np.float32)
        s.add_mesh(v if offset is None and world_scale == 1.0 else np.array([at(p) for p in v], np.float32), tri, M(albedo=tuple(rng.uniform(0.2, 1, 3))))
    return s


def many_spheres(gpu, n, n_lights, dark=False, offset=None, world_scale=1.0):
    """A crowd of n spheres over a floor (mirror / glass / diffuse, some moving, some tiny, some overlapping, one enclosing the
    camera's side of the scene partly), n_lights point lights: exercises the packed pair filter of the closest-hit loop and of
    the shadow rays on both sides of its limits (8 <= n <= 128), odd counts (the last sphere pairs with itself) and far / near /
    tangent geometry.  `offset` / `world_scale` move and scale the whole scene."""
    M = gpu.Material.make
    at, ln, mv = _placement(offset, world_scale)
    rng = np.random.default_rng(7000 + 13 * n + n_lights)
    s = gpu.HostScene()
    s.set_sky(dark)
    for i in range(n_lights):
        s.add_light(at((float(rng.uniform(-4, 4)), float(rng.uniform(4, 9)), float(rng.uniform(-6, 3)))), ln(float(rng.uniform(0.5, 2.0))))
    s.add_quad(at((-40, -2, -60)), (1, 0, 0), (0, 0, 1), ln(80), ln(70), M(albedo=(0.7, 0.7, 0.7)))
    for i in range(n):
        kind = i % 4
        r = float(rng.choice([0.05, 0.3, 0.8, 1.5, 4.0], p=[0.1, 0.3, 0.3, 0.25, 0.05]))
        c = (float(rng.uniform(-12, 12)), float(-2 + r * rng.uniform(0.6, 1.4)), float(rng.uniform(-40, 1)))
        mat = M(albedo=tuple(rng.uniform(0.2, 1, 3)), type=gpu.MAT_GLASS if kind == 0 else (gpu.MAT_MIRROR if kind == 1 else gpu.MAT_DIFFUSE),
                transparency=0.6 if kind == 0 else (0.3 if kind == 3 else 0.0), index_medium=1.5,
                motion=mv((0.0, float(rng.uniform(0, 0.8)), 0.0)) if i % 3 == 0 else (0, 0, 0))
        s.add_sphere(at(c), ln(r), mat)
    return s


def overlapping_soup(gpu, nt=200, seed=1, scale=0.5, slivers=12, offset=None, world_scale=1.0):
    """A triangle soup on which the REFERENCE's builder degenerates (found by tools/fuzz_exact.py, round 3): triangles larger
    than their spacing straddle every median cut, the tree reaches depth 100 and drops triangles below it (KDTree.cpp:101), and
    because the cut is the median of UNCLIPPED bounds (:87-98) planes fall outside their nodes -- children stick out of their
    parents, and a leaf is then reached only through its own box AND those ancestors' (hrt_tri_exception::group).  With
    nt = 200, seed = 1: 117 dropped triangles, 12 797 (triangle, leaf) pairs, 27 711 box entries.  `scale` is the noise width of
    the triangles; `offset` / `world_scale` move and scale the whole scene."""
    at, ln, _ = _placement(offset, world_scale)
    rng = np.random.default_rng(1000 * nt + seed)
    centres = rng.normal(scale=1.0, size=(nt, 1, 3))
    v = (centres + rng.normal(scale=scale, size=(nt, 3, 3))).astype(np.float32)
    v[:slivers, 1] = v[:slivers, 0] + (v[:slivers, 2] - v[:slivers, 0]) * np.float32(0.5) + np.float32(1e-6)   # a few (near) collinear ones
    pos = v.reshape(-1, 3) + np.float32([0, 0.5, -4])
    if offset is not None or world_scale != 1.0:
        pos = np.array([at(p) for p in pos], np.float32)
    tri = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    s = gpu.HostScene()
    s.set_sky(False)
    s.add_quad(at((-6, -3, -10)), (1, 0, 0), (0, 0, 1), ln(12), ln(12), gpu.Material.make(albedo=(0.8, 0.8, 0.8)))
    s.add_quad(at((-1, 4, -5)), (1, 0, 0), (0, 0, 1), ln(2), ln(2), gpu.Material.make(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=8.0))
    s.add_mesh(pos, tri, gpu.Material.make(albedo=(0.7, 0.6, 0.5)), face_colors=rng.uniform(0.1, 1, (nt, 3)).astype(np.float32))
    return s


def same_nonfinite(a, b):
    """Per value: both sides non-finite in the same way (both NaN, or the same infinity)."""
    fa, fb = np.isfinite(a), np.isfinite(b)
    return ~fa & ~fb & ((np.isnan(a) & np.isnan(b)) | (a == b))


def describe_difference(a, b):
    """Text for an assertion message: how many pixels differ and by how much.  A pixel differs where a value differs,
    where exactly one side is non-finite, or where both are non-finite in different ways."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    both = np.isfinite(a64) & np.isfinite(b64)
    d = np.abs(np.where(both, a64, 0.0) - np.where(both, b64, 0.0))
    bad = (~((a64 == b64) | same_nonfinite(a64, b64))).any(axis=2)
    n = int(bad.sum())
    where = np.argwhere(bad)[:5].tolist()
    nf = int((~both & ~same_nonfinite(a64, b64)).any(axis=2).sum())
    text = f"{n} of {bad.size} pixels differ ({nf} of them non-finite on one side only or differently), max finite |diff| {d.max():.3g}, first at (y, x) {where}"
    same_nan = int(same_nonfinite(a64, b64).any(axis=2).sum())
    if same_nan:   # np.array_equal counts a NaN as unequal to itself: say so, a caller deciding with it fails on these alone
        text += f"; {same_nan} more pixels hold the same NaN / inf on both sides (not counted above; unequal to np.array_equal)"
    return text


def open_box(gpu, albedo, lamp, light=None, floor_albedo=None):
    """An open-fronted box of five diffuse walls, an emissive lamp square under its ceiling, an optional point light."""
    M = gpu.Material.make
    s = gpu.HostScene()
    s.set_sky(True)
    if light is not None:
        s.add_light((0.5, 1.2, 0.5), 0.4, light)
    fl = albedo if floor_albedo is None else floor_albedo
    s.add_quad((-2, -1.5, -4), (1, 0, 0), (0, 0, 1), 4, 6, M(albedo=fl))                     # floor
    s.add_quad((-2, 1.8, 2), (1, 0, 0), (0, 0, -1), 4, 6, M(albedo=albedo))                  # ceiling
    s.add_quad((-2, -1.5, -4), (1, 0, 0), (0, 1, 0), 4, 3.3, M(albedo=albedo))               # back
    s.add_quad((-2, -1.5, 2), (0, 0, -1), (0, 1, 0), 6, 3.3, M(albedo=albedo))               # left
    s.add_quad((2, -1.5, -4), (0, 0, 1), (0, 1, 0), 6, 3.3, M(albedo=albedo))                # right
    s.add_quad((-1.5, 1.75, -3.0), (1, 0, 0), (0, 0, 1), 3.0, 3.0, lamp)                     # lamp, facing down
    return s


def overflow_scene(gpu, mechanism, lit):
    """A box whose colour products overflow fp32 (tests/test_gpu_views.py): mechanism "emission" (an infinite lamp over a black
    floor; `lit` adds a point light) or "throughput" (albedos of 1e8)."""
    M = gpu.Material.make
    if mechanism == "emission":
        # (a) a black floor below a lamp whose light_color x light_intensity overflows fp32: a path off the floor has throughput
        # 0 and then meets an infinite emission -- 0 x inf = NaN unless the path ends where its throughput became 0
        return open_box(gpu, (0.7, 0.7, 0.7), M(albedo=(0, 0, 0), emissive=True, light_color=(1e30, 1e30, 1e30), light_intensity=1e10),
                        light=(1.0, 1.0, 1.0) if lit else None, floor_albedo=(0, 0, 0))
    # (b) albedos of 1e8: after five bounces the throughput is 1e40 = inf, and a last segment that ends on a non-emitting wall or
    # in the dark sky adds inf x 0 = NaN unless it is pruned
    return open_box(gpu, (1e8, 1e8, 1e8), M(albedo=(0, 0, 0), emissive=True, light_color=(1, 1, 1), light_intensity=5.0))
