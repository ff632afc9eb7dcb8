"""The inputs of tests/test_probe_cases.py (CPU) and tests/test_gpu_probe_cases.py (GPU): probe records at NON-ZERO TIMES on the scenes
the radiance queries are held to the oracle on, a set of FAR probes whose rays do meet the scene, and the oracle's value for both.

Everything here is made WITHOUT a GPU: the probes start from the oracle's own first hits (radiance_oracle.Scene.hits()), the far keys
are picked with the NumPy rule (probe_ref.directions), and the scene's bound is read off the flattened description.  So the CPU test
can state, on the very inputs the GPU test traces, that the times move what the probes see, that the far rays hit, and how many tie
rays there are.

PER SCENE, eight probe records {P, time} (probes()):
  0..4  p + 0.25 n for oracle first-hit points p with shading normal n,
  5     p + 1e-3 d: just BEHIND a first hit (radiance_oracle.interior's construction: inside glass and meshes, behind walls),
  6, 7  degenerate: a NaN coordinate, and an infinite time.
The six live probes have six different times -- 0, 0.5, the largest float below 1 and three uniform draws -- so that a time dropped,
taken from another probe of the batch or carried over from the wave's previous item changes what a moving scene returns.

THE FAR SET (far_set()): one position farther than 16 x (bound + 1) from the origin -- the far-origin rule of
csrc/hrt_rays.hip query_margin, bound = csrc/hrt_pack.h scene_bound restated in bound() -- repeated 64 times under 64 keys at
n_samples = 1.  From there a uniform direction practically never meets the scene (a part in a few thousand of the sphere), so the
keys are CHOSEN: of the candidate keys 0 .. 2^21 - 1 in ascending order, the first AIMED keys whose ray of sample 0 passes within
half the scene's radius of its centre, and 16 stray ones whose ray misses the centre by more than twice the radius (centre and
radius: of the box round the description's points, box()).  A tetrahedron of many_squares or edge_scene subtends about 1e-6 of the
sphere from there, so no key below 2^21 need meet one: MESH_KEYS are keys found by mesh_keys() over 2^24 candidates whose ray
passes within a mesh's own bounding sphere and, by the oracle, hits the mesh; they take the last places among the aimed."""
import ctypes as C

import numpy as np

import probe_ref
import radiance_oracle as ro

F32, U32 = np.float32, np.uint32
SCENES = ro.EXTRA + ["random_spheres"]
STATIC = ("skybox",)     # nothing in it moves: the times cannot matter there
SEED = ro.SEED
S = 65                   # a full block of 64 and a second block of one
LIVE, DEGENERATE = slice(0, 6), slice(6, 8)
FAR_TIME = F32(0.625)
AIMED, STRAY, CANDIDATES = 48, 16, 1 << 21
# Per scene: the seed of the hit points the probes start from -- one of the seeds 1 .. 24 with the most probes whose band 0 the
# oracle changes with the time (5 of the 5 at a time other than 0; 3 on many_squares, whose moving squares are small), to be
# changed when a batch exceeds radiance_oracle.tie_cap (none did) -- r_max of the depth comparisons, between the depths that
# occur from these probes, and the direction the far probe lies in: a square is hit from its front only, and the floors of these scenes but random_spheres' face down, so the probe lies on the side
# from which the oracle gives the aimed rays the most hits; on the two scenes with meshes, among 250 random directions the one
# with the most hits from which a tetrahedron is not hidden behind the floor.
PROBE_SEED = {"many_squares": 6, "many_spheres": 3, "edge_scene": 14, "skybox": 4, "dark_spheres": 10, "random_spheres": 6, "cornell_mesh": 7}
R_MAX = {"many_squares": 2.5, "many_spheres": 6.0, "edge_scene": 3.0, "skybox": 2.0, "dark_spheres": 6.0, "random_spheres": 6.0,
         "cornell_mesh": 1.5}
FAR_DIR = {"many_squares": (0.73, -0.6, -0.33), "many_spheres": (0.4, -1.0, 0.4), "edge_scene": (0.2, 0.16, 0.97), "skybox": (0.4, -1.0, 0.0),
           "dark_spheres": (0.4, -1.0, 0.4), "random_spheres": (0.4, 1.0, 0.4)}
# the first four keys of mesh_keys(hrt, name, 1 << 24) whose first segment the oracle gives as a mesh hit
MESH_KEYS = {"many_squares": (2728345, 3176523, 5426323, 9614461), "edge_scene": (229215, 542882, 684038, 1693961)}


# ----------------------------------------------------------------------------------------------------------- the description
class _Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("material", C.c_int32)]


class _Light(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3)]


class _Mesh(C.Structure):
    """``hrt_mesh`` (include/hrt.h), whole: the array is walked by its size."""
    _fields_ = [("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("positions", C.POINTER(C.c_float)), ("indices", C.c_void_p),
                ("color_type", C.c_int32), ("vert_colors", C.c_void_p), ("face_colors", C.c_void_p), ("aabb_min", C.c_float * 3),
                ("aabb_max", C.c_float * 3), ("material", C.c_int32), ("kd_root", C.c_uint32), ("kd_min", C.c_float * 3),
                ("kd_max", C.c_float * 3), ("n_kd_units", C.c_uint32), ("kd_units", C.c_void_p), ("n_leaf_tris", C.c_uint32),
                ("leaf_tris", C.c_void_p), ("n_exceptions", C.c_uint32), ("exceptions", C.c_void_p)]


def _desc(hrt, desc):
    class Desc(C.Structure):
        _fields_ = [("n_materials", C.c_uint32), ("materials", C.POINTER(hrt.Material)), ("n_spheres", C.c_uint32), ("spheres", C.POINTER(_Sphere)),
                    ("n_quads", C.c_uint32), ("quads", C.POINTER(hrt.Quad)), ("n_meshes", C.c_uint32), ("meshes", C.POINTER(_Mesh)),
                    ("n_lights", C.c_uint32), ("lights", C.POINTER(_Light))]
    return C.cast(desc, C.POINTER(Desc)).contents


def _mesh_vertices(m):
    return np.ctypeslib.as_array(m.positions, shape=(m.n_vertices, 3)).astype(np.float64)


def bound(hrt, desc):
    """csrc/hrt_pack.h scene_bound: the largest distance of any scene point from the origin, in double, rounded to fp32."""
    D = _desc(hrt, desc)
    b = 0.0
    mlen = lambda i: float(np.linalg.norm(np.array(D.materials[i].motion[:], np.float64)))
    for i in range(D.n_spheres):
        sp = D.spheres[i]
        b = max(b, float(np.linalg.norm(np.array(sp.center[:], np.float64))) + abs(float(sp.radius)) + mlen(sp.material))
    for i in range(D.n_quads):
        q = D.quads[i]
        v0, v1, v3 = (np.array(v[:], np.float64) for v in (q.v0, q.v1, q.v3))
        for p in (v0, v1, v3, v1 + v3 - v0):
            b = max(b, float(np.linalg.norm(p)) + mlen(q.material))
    for i in range(D.n_meshes):
        b = max(b, float(np.linalg.norm(_mesh_vertices(D.meshes[i]) * 1.00001, axis=1).max()))
    for i in range(D.n_lights):
        b = max(b, float(np.linalg.norm(np.array(D.lights[i].pos[:], np.float64))) + abs(float(D.lights[i].radius)))
    return float(F32(b))


def box(hrt, desc):
    """(centre, radius, [(centre, radius) of every mesh]) of the axis-aligned box round the description's points at rest: sphere
    extents, quad corners, mesh vertices.  Every point of the scene lies within `radius` (half the diagonal) of `centre`, up to
    its motion (below 1 on these scenes)."""
    D = _desc(hrt, desc)
    pts, meshes = [], []
    for i in range(D.n_spheres):
        c, r = np.array(D.spheres[i].center[:], np.float64), abs(float(D.spheres[i].radius))
        pts += [c - r, c + r]
    for i in range(D.n_quads):
        q = D.quads[i]
        v0, v1, v3 = (np.array(v[:], np.float64) for v in (q.v0, q.v1, q.v3))
        pts += [v0, v1, v3, v1 + v3 - v0]
    for i in range(D.n_meshes):
        v = _mesh_vertices(D.meshes[i])
        pts += [v.min(axis=0), v.max(axis=0)]
        meshes.append(((v.min(axis=0) + v.max(axis=0)) / 2, float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)) / 2)))
    pts = np.array(pts)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return (lo + hi) / 2, float(np.linalg.norm(hi - lo) / 2), meshes


# ------------------------------------------------------------------------------------------------------------------- probes
_probes, _far = {}, {}


def times(rng):
    """The six times of the live probes: no two equal, the fixed ones between the draws."""
    u = rng.uniform(0.05, 0.95, 3).astype(F32)
    return np.array([u[0], 0.0, u[1], np.nextafter(F32(1), F32(0)), 0.5, u[2]], F32)


def probes(hrt, name):
    """The eight probe records of scene `name` (the module's text): the same array on every call."""
    if name not in _probes:
        sc = ro.scene(hrt, name)
        p, n, _, d = sc.hits()
        assert len(p) >= 16, f"{name}: too few hit points"
        rng = np.random.default_rng([PROBE_SEED[name], sum(name.encode())])
        i = rng.choice(len(p), 6, replace=False)
        rec = np.empty((8, 4), F32)
        rec[0:5, 0:3] = p[i[:5]] + 0.25 * n[i[:5]]
        rec[5, 0:3] = p[i[5]] + 1e-3 * d[i[5]]
        rec[0:6, 3] = times(rng)
        rec[6] = (np.nan, 1.0, 2.0, 0.25)
        rec[7] = (0.5, 0.25, -1.0, np.inf)
        _probes[name] = rec
    return _probes[name].copy()


def keys(name, with_keys):
    """None, or radiance_oracle.random_keys for the eight probes (0 and 0xFFFFFFFF among them)."""
    return ro.random_keys(8, np.random.default_rng([11, sum(name.encode())])) if with_keys else None


def volume_box(hrt, name):
    """The box of the probe volumes the lit comparisons use on scene `name`: round the live probes, one unit wider on every side."""
    p = probes(hrt, name)[LIVE, 0:3]
    return tuple(float(x) for x in p.min(axis=0) - F32(1)), tuple(float(x) for x in p.max(axis=0) + F32(1))


def line_distance(o, d, c):
    """Distance of the points c from the lines o + t d (d unit), and t of the nearest point: in double."""
    v = np.asarray(c, np.float64) - np.asarray(o, np.float64)
    t = (v * d).sum(axis=-1)
    return np.linalg.norm(v - t[..., None] * d, axis=-1), t


def far_position(hrt, name):
    """(position in fp32, its distance from the origin, bound, far threshold 16 x (bound + 1))."""
    sc = ro.scene(hrt, name)
    b = bound(hrt, sc.desc)
    far = 16.0 * (b + 1.0)
    u = np.asarray(FAR_DIR[name], np.float64)
    pos = (1.0625 * far * u / np.linalg.norm(u)).astype(F32)
    return pos, float(np.linalg.norm(pos.astype(np.float64))), b, far


def far_r_max(hrt, name):
    """r_max of the far set's depth comparisons: the distance from the far probe to the scene's centre, so that the aimed rays hit
    on either side of it."""
    sc = ro.scene(hrt, name)
    return float(F32(np.linalg.norm(far_position(hrt, name)[0].astype(np.float64) - box(hrt, sc.desc)[0])))


def far_set(hrt, name):
    """(probe records (64, 4), keys (64,) uint32, aimed mask (64,)): the far position under AIMED chosen keys whose ray of sample 0
    passes within half the scene's radius of its centre -- the last of them MESH_KEYS[name], aimed at a mesh -- and STRAY whose ray
    misses the centre by more than twice the radius; aimed and stray interleaved (every fourth key a stray one)."""
    if name not in _far:
        sc = ro.scene(hrt, name)
        pos, _, _, _ = far_position(hrt, name)
        centre, radius, _ = box(hrt, sc.desc)
        cand = np.arange(CANDIDATES, dtype=np.uint64).astype(U32)
        d = probe_ref.directions(SEED, cand, 0).astype(np.float64)
        dist, t = line_distance(pos.astype(np.float64), d, centre)
        mesh = np.array(MESH_KEYS.get(name, ()), U32)
        aimed = cand[(dist < radius / 2) & (t > 0) & ~np.isin(cand, mesh)][:AIMED - len(mesh)]
        stray = cand[(dist > 2 * radius) | (t <= 0)][:STRAY]
        assert len(aimed) + len(mesh) == AIMED and len(stray) == STRAY, (name, len(aimed), len(stray))
        aimed = np.concatenate([aimed, mesh]).astype(U32)
        k, is_aimed = np.empty(64, U32), np.ones(64, bool)
        is_aimed[3::4] = False
        k[is_aimed], k[~is_aimed] = aimed, stray
        rec = np.empty((64, 4), F32)
        rec[:, 0:3], rec[:, 3] = pos, FAR_TIME
        _far[name] = (rec, k, is_aimed)
    return tuple(a.copy() for a in _far[name])


def mesh_keys(hrt, name, candidates, chunk=1 << 20):
    """How MESH_KEYS were found: the keys below `candidates`, ascending, whose ray of sample 0 from the far position passes within
    a mesh's bounding sphere AND within half the scene's radius of its centre.  Five seconds for 2^24 keys: not run by a test."""
    sc = ro.scene(hrt, name)
    pos = far_position(hrt, name)[0].astype(np.float64)
    centre, radius, meshes = box(hrt, sc.desc)
    out = []
    for k0 in range(0, candidates, chunk):
        cand = np.arange(k0, min(candidates, k0 + chunk), dtype=np.uint64).astype(U32)
        d = probe_ref.directions(SEED, cand, 0).astype(np.float64)
        ok = line_distance(pos, d, centre)[0] < radius / 2
        near = np.zeros(len(cand), bool)
        for c, r in meshes:
            dist, t = line_distance(pos, d, c)
            near |= (dist < r) & (t > 0)
        out += cand[ok & near].tolist()
    return out


# --------------------------------------------------------------------------------------------------------------------- oracle
def rule_records(p, keys, first, count=S):
    """The NumPy rule's ray records of samples first .. first + count - 1: (count, n, 8) fp32."""
    return np.stack([probe_ref.rays(p, s, SEED, keys)[0] for s in range(first, first + count)])


def oracle_values(sc, records, keys, first):
    """Per sample the value the device is held to under the tie rule (radiance_oracle.expected: REF_TREE off the tie rays, ROPE_TREE
    on them, the tie rays of every sample's batch within the cap): records (count, n, 8) -> values (count, n, 3), ties (count, n)."""
    vs, ties = [], []
    for j, rec in enumerate(records):
        v, tie = ro.expected(sc, rec, keys=keys, first_sample=first + j, n_samples=1, seed=SEED)
        vs.append(v)
        ties.append(tie)
    return np.stack(vs), np.stack(ties)


def first_segments(sc, records, keys, first):
    """Per sample and probe the oracle's first segment of the path of that record: (kind, t, triangle) each (count, n), kind 0 for a
    miss and for a degenerate record, and the tie mask -- the samples on which the oracle's two mesh modes disagree about the
    segment, which are held to the ROPE_TREE one (the walk the device runs)."""
    import oracle_lib
    count, n = records.shape[:2]
    k = np.arange(n, dtype=U32) if keys is None else np.asarray(keys, U32)
    out = {}
    for mode in (oracle_lib.MESH_REF_TREE, oracle_lib.MESH_ROPE_TREE):
        o = sc.oracle(mode)
        kind, t, tri = np.zeros((count, n), np.int64), np.zeros((count, n), F32), np.full((count, n), -1, np.int64)
        for j in range(count):
            for i in range(n):
                rec = records[j, i]
                if not np.isfinite(rec[0:7]).all() or not rec[4:7].any():
                    continue
                row = o.trace_ray_path(rec, int(k[i]), first + j, SEED, cap=1)[0]
                kind[j, i], t[j, i], tri[j, i] = int(row[7]), row[9], int(row[10])
        out[mode] = (kind, t, tri)
    ref, rope = out[oracle_lib.MESH_REF_TREE], out[oracle_lib.MESH_ROPE_TREE]
    tie = (ref[0] != rope[0]) | (ref[1].view(U32) != rope[1].view(U32))
    return np.where(tie, rope[0], ref[0]), np.where(tie, rope[1], ref[1]), np.where(tie, rope[2], ref[2]), tie


def depths(kind, t, r_max):
    """r of the depth fold: fminf(t, r_max) of a hit, r_max of a miss."""
    return np.where(kind != 0, np.fmin(t, F32(r_max)), F32(r_max)).astype(F32)


def chain(count, block=None):
    """D: the fp32 operations on the longest chain of probe_ref.fold(...) / count -- the product Y x v, a lane's additions within
    a block, the six halvings, the additions of the blocks, the division."""
    block = probe_ref.BLOCK if block is None else block
    return 1 + -(-min(count, block) // 64) + 6 + -(-count // block) + 1


def coefficient_tolerance(Y, v, deg, block=None):
    """The bound on |fold(Y, v_device) - fold(Y, v_oracle)| / S per coefficient and channel, (n, 9, 3) in double: the project's
    bar for a sample, 1e-6 max(1, |v|), through sums that do the same additions in the same order on both
    sides, each operation of the chain rounding by at most 2^-24 of a partial sum no larger than sum_j |Y_jk| max(1, |v_jc|)."""
    count = len(v)
    Ya = np.abs(np.asarray(Y, np.float64))[:, :, :, None]
    va = np.maximum(1.0, np.abs(np.asarray(v, np.float64)))[:, :, None, :]
    live = ~np.asarray(deg, bool)[:, :, None, None]
    return (1e-6 + chain(count, block) * 2.0 ** -24) * (Ya * va * live).sum(axis=0) / count
