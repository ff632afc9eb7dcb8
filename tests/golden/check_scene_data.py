"""Scene DATA of the host layer against the reference's own set-up code, read WHERE IT LIES (build container only).

    python tests/golden/check_scene_data.py            # pass / fail per scene
    python tests/golden/check_scene_data.py --write    # and record the reference's objects in tests/golden/ref_scene_data.npz

Only the resulting DATA is recorded (object positions, sizes, materials, transformed mesh vertices), none of the reference's
text; tests/test_scene_data_against_reference.py checks the host layer against that record.

Why: host/scene*.cpp was transcribed by hand from Scene.h's setup_* functions, and both the oracle and the GPU path are fed
by it -- a slip in a literal would be invisible to every parity test.  This script reads
/root/reference/src/Scene.h at run time, interprets the statements of the set-up functions the BASELINE configurations use
(setup_cornell_box, setup_backrooms_pool, the fixed part of setup_random_spheres) with a small statement interpreter, and
compares the resulting objects -- square vertices after all transforms, tangent frames as setQuad leaves them, sphere
centres and radii, transformed mesh vertices, every Material field the path reads, lights, texture bindings -- with the
hrt_scene_desc the host layer flattens for the same scene.  The semantics it needs (setQuad, translate / scale / rotate_*,
centerAndScaleToUnit, addBox) are the documented behaviour of Square.h:31-63, Mesh.h:173-224, Mesh.cpp:93-105 and
Scene.h:92-146, evaluated in float64; agreement is asked to 2e-5 absolute (fp32 transform chains).

Known, documented differences it accounts for: the pool's `flamingo_float_colored.off` and `sky.ppm` are missing upstream
blobs: the host layer loads `flamingo_float.off` and no skybox; setup_random_spheres' 79 random spheres come
from the host layer's own seeded generator (N13) and are not compared.
"""
import ctypes as C
import importlib
import json
import math
import os
import re
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
TOL = 2e-5


# ---------------------------------------------------------------- the reference's objects, as far as set-up code touches them
def V3(*a):
    a = [float(x) for x in a]
    return np.array(a * 3 if len(a) == 1 else a, np.float64)


class Material:
    def __init__(self):
        self.diffuse_material = V3(0); self.specular_material = V3(0); self.ambient_material = V3(0); self.shininess = 0.0
        self.motion_blur_translation = V3(0); self.index_medium = 1.0; self.transparency = 0.0
        self.type = "Material_Diffuse_Blinn_Phong"; self.texture_type = "Texture_None"
        self.checkerboard_color1 = V3(0); self.checkerboard_color2 = V3(0); self.texture_scale_x = 1.0; self.texture_scale_y = 1.0
        self.emissive = False; self.light_color = V3(0); self.light_intensity = 0.0
        self.image = -1; self.normals = -1; self.has_normal_map = False

    def copy(self):
        m = Material(); m.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()}); return m

    def set_texture(self, ref): self.image = ref[1]
    def set_normals(self, ref): self.normals = ref[1]; self.has_normal_map = True


class Mesh:
    def __init__(self):
        self.v = np.zeros((0, 3)); self.tris = np.zeros((0, 3), np.int64); self.material = Material(); self.off = None

    def translate(self, t): self.v = self.v + t
    def scale(self, s): self.v = self.v * s
    def _rot(self, m): self.v = self.v @ np.array(m, np.float64).T
    def rotate_x(self, a):
        a = a * math.pi / 180.0; self._rot([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    def rotate_y(self, a):
        a = a * math.pi / 180.0; self._rot([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    def rotate_z(self, a):
        a = a * math.pi / 180.0; self._rot([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    def rotate(self, ang): self.rotate_x(ang[0]); self.rotate_y(ang[1]); self.rotate_z(ang[2])
    def build_arrays(self): pass
    def recomputeNormals(self): pass

    def loadOFF(self, path, assets):
        self.off = path
        alt = {"mesh/flamingo_float_colored.off": "mesh/flamingo_float.off"}.get(path, path)  # missing upstream blob
        lines = [l for l in open(os.path.join(assets, alt)).read().split("\n") if l.strip() and not l.lstrip().startswith("#")]
        head = lines[0].split()
        k = 1
        if len(head) >= 3 and head[0] in ("OFF", "COFF"): counts = head[1:]     # "OFF nv nf ne" on one line
        else: counts = lines[1].split(); k = 2
        nv, nf = int(counts[0]), int(counts[1])
        self.v = np.array([[float(x) for x in l.split()[:3]] for l in lines[k:k + nv]], np.float64)   # COFF: colours follow the position
        self.tris = np.array([[int(x) for x in l.split()[1:4]] for l in lines[k + nv:k + nv + nf]], np.int64)

    def centerAndScaleToUnit(self):   # Mesh.cpp:93-105
        c = self.v.mean(axis=0)
        self.v = (self.v - c) / np.linalg.norm(self.v - c, axis=1).max()


class Sphere(Mesh):
    def __init__(self): super().__init__(); self.m_center = V3(0); self.m_radius = 0.0


class Square(Mesh):
    def __init__(self): super().__init__(); self.m_right_vector = V3(0); self.m_up_vector = V3(0)

    def setQuad(self, bl, rv, uv, w=1.0, h=1.0):   # Square.h:31-63
        self.m_right_vector = rv / np.linalg.norm(rv) * w
        self.m_up_vector = uv / np.linalg.norm(uv) * h
        self.v = np.array([bl, bl + self.m_right_vector, bl + self.m_right_vector + self.m_up_vector, bl + self.m_up_vector])


class Light:
    def __init__(self): self.pos = V3(0); self.radius = 0.0; self.material = V3(0)


class Scene:
    def __init__(self, assets):
        self.assets = assets; self.meshes, self.spheres, self.squares, self.lights = [], [], [], []
        self.textures, self.normals = [], []; self.dark_sky = True; self.skybox = None


# ---------------------------------------------------------------- a statement interpreter for the shapes the set-up code uses
def strip_comments(s):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))


def function_body(src, name):
    i = src.index("void " + name + "(")
    j = src.index("{", i); d = 0
    for k in range(j, len(src)):
        d += src[k] == "{"; d -= src[k] == "}"
        if d == 0: return strip_comments(src[j + 1:k])
    raise ValueError(name)


def to_py(expr):
    e = re.sub(r"(\d+\.\d*|\.\d+|\d+)f\b", r"\1", expr)
    e = re.sub(r"&\s*textures\[(\w+)\]", r"('tex', \1)", e)
    e = re.sub(r"&\s*normals\[(\w+)\]", r"('nm', \1)", e)
    e = re.sub(r"\bVec3\b", "V3", e)
    e = re.sub(r"\btrue\b", "True", e); e = re.sub(r"\bfalse\b", "False", e)
    e = re.sub(r"\b(Material_\w+|Texture_\w+|LightType_\w+)\b", r"'\1'", e)
    return e


def run(body, scene, env):
    """Executes the straight-line statements of a set-up body; returns at the first `for` whose bound is not a literal (the
    random part of setup_random_spheres)."""
    stmts = [re.sub(r"\s+", " ", x).strip() for x in re.split(r"[;{}]", body)]
    stmts = [x for x in stmts if x]
    kinds = {"squares": Square, "spheres": Sphere, "meshes": Mesh, "lights": Light}
    ev = lambda e: eval(to_py(e), {"V3": V3, "math": math, "M_PI": math.pi}, env)
    i = 0
    while i < len(stmts):
        st = stmts[i]; i += 1
        m = re.match(r"(\w+)\.resize\( ?\1\.size\(\) \+ 1 ?\)$", st)
        if m: getattr(scene, m.group(1)).append(kinds[m.group(1)]()); continue
        m = re.match(r"(Square|Sphere|Mesh|Light) ?& ?(\w+) = (\w+)(\[\3\.size\(\) - 1\]|\.back\(\))$", st)
        if m: env[m.group(2)] = getattr(scene, m.group(3))[-1]; continue
        m = re.match(r"int (\w+) = load_(texture|normal_map)\(\"([^\"]*)\"\)$", st)
        if m:
            lst = scene.textures if m.group(2) == "texture" else scene.normals
            lst.append(m.group(3)); env[m.group(1)] = len(lst) - 1; continue
        if st in ("clear()", "computeKDTrees()") or st.startswith("skybox =") or st.startswith("loadSkybox("): continue
        m = re.match(r"(?:float|int|double) (\w+) = (.+)$", st)
        if m:
            if "random_float" in m.group(2) or "rand()" in m.group(2): return
            env[m.group(1)] = ev(m.group(2)); continue
        m = re.match(r"Vec3 (\w+) = (.+)$", st)
        if m: env[m.group(1)] = ev(m.group(2)); continue
        m = re.match(r"Material (\w+) = Material\(\)$", st)
        if m: env[m.group(1)] = Material(); continue
        if st == "std::vector<Material> materials": env["materials"] = []; continue
        m = re.match(r"materials\.push_back\((\w+)\)$", st)
        if m: env["materials"].append(env[m.group(1)].copy()); continue
        if st.startswith("for (int i ="):
            bound = re.match(r"i < (\w+)$", stmts[i]); i += 2  # "i < N", "i++)"
            if not bound or not bound.group(1).isdigit(): return   # the random part: not reference DATA (N13)
            nxt = stmts[i]; i += 1
            for _ in range(int(bound.group(1))):
                mm = re.match(r"materials\.push_back\((\w+)\)$", nxt); assert mm, nxt
                env["materials"].append(env[mm.group(1)].copy())
            continue
        m = re.match(r"bool faces\[6\] =$", st)
        if m: env["faces"] = [x.strip() == "true" for x in stmts[i].split(",")]; i += 1; continue
        m = re.match(r"addBox\((.+)\)$", st)
        if m: add_box(scene, env, *[a.strip() for a in split_args(m.group(1))]); continue
        m = re.match(r"dark_sky = (\w+)$", st)
        if m: scene.dark_sky = m.group(1) == "true"; continue
        m = re.match(r"(\w+)((?:\.\w+)+) = (.+)$", st)          # field assignment
        if m and m.group(1) in env:
            if "random_float" in m.group(3): return
            obj = env[m.group(1)]; path = m.group(2).strip(".").split(".")
            for p in path[:-1]: obj = getattr(obj, p)
            if path[-1] in ("powerCorrection", "isInCamSpace", "type") and isinstance(obj, Light): continue
            setattr(obj, path[-1], ev(m.group(3))); continue
        m = re.match(r"(\w+)((?:\.\w+)+)\((.*)\)$", st)          # method call
        if m and m.group(1) in env:
            obj = env[m.group(1)]; path = m.group(2).strip(".").split(".")
            for p in path[:-1]: obj = getattr(obj, p)
            args = [ev(a) for a in split_args(m.group(3))] if m.group(3).strip() else []
            if path[-1] == "loadOFF": obj.loadOFF(args[0], scene.assets)
            else: getattr(obj, path[-1])(*args)
            continue
        raise ValueError("statement shape not understood: " + st)


def split_args(s):
    out, d, cur = [], 0, ""
    for ch in s:
        if ch == "," and d == 0: out.append(cur); cur = ""; continue
        d += ch in "(["; d -= ch in ")]"; cur += ch
    if cur.strip(): out.append(cur)
    return out


def add_box(scene, env, materials, faces, pos, rotation, size="1.", facing_out="true"):
    """Scene::addBox, Scene.h:92-146: the faces' setQuad / rotate calls are read from the reference's own text."""
    src = strip_comments(open(os.path.join(REF, "src", "Scene.h")).read())
    i = src.index("void addBox("); body = src[src.index("{", i):src.index("void draw", i) if "void draw" in src[i:] else i + 6000]
    local = dict(env); local["size"] = eval(to_py(size), {}, env)
    ev = lambda e: eval(to_py(e), {"V3": V3}, local)
    for name in ("base_bottom_left", "base_right_vector", "base_up_vector"):
        local[name] = ev(re.search(name + r" = ([^;]+);", body).group(1))
    first = len(scene.squares)
    for k in range(6):
        blk = re.search(r"if \(faces\[%d\]\) ?\{(.*?)nfaces\+\+" % k, body, re.S).group(1)
        if not env[faces][k]: continue
        sq = Square(); scene.squares.append(sq)
        for call in re.findall(r"square\.(\w+)\(([^;]*)\);", blk):
            getattr(sq, call[0])(*[ev(a) for a in split_args(call[1])])
    for j, sq in enumerate(scene.squares[first:]):
        sq.translate(env[pos]); sq.material = env[materials][j].copy()


# ---------------------------------------------------------------- comparison with the host layer's flattened description
class Quad(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("v1", C.c_float * 3), ("v3", C.c_float * 3), ("t", C.c_float * 3), ("b", C.c_float * 3), ("mat", C.c_int32)]
class Sph(C.Structure):
    _fields_ = [("c", C.c_float * 3), ("r", C.c_float), ("mat", C.c_int32)]
class Lgt(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3)]


def reference_scene(ref_fn, aspect):
    """The objects the reference's set-up function `ref_fn` creates, interpreted from its Scene.h (needs the reference)."""
    src = open(os.path.join(REF, "src", "Scene.h")).read()
    sc = Scene(os.path.join(ROOT, "assets"))
    run(function_body(src, ref_fn), sc, {"aspect_ratio": aspect})
    return sc


# ---------------------------------------------------------------- the same objects as a committed fixture (GOLDEN)
# GOLDEN holds, per (set-up function, aspect ratio), what reference_scene() produced: every sphere, square, mesh and light with
# the Material fields listed above (float64, exact), mesh vertices after their transforms as arrays, the texture and normal-map
# lists and dark_sky.  Written by `python tests/golden/check_scene_data.py --write` where the reference is present; read by
# tests/test_scene_data_against_reference.py, which therefore needs nothing outside the repository.
GOLDEN = os.path.join(HERE, "ref_scene_data.npz")


def golden_key(ref_fn, aspect):
    return f"{ref_fn} {aspect:.9g}"


def _plain(x):
    return x.tolist() if isinstance(x, np.ndarray) else x


def _material_data(m):
    return {k: _plain(v) for k, v in m.__dict__.items()}


def scene_data(sc, key):
    """(json-able description, {array name: array}) of a Scene."""
    meshes, arrays = [], {}
    for i, m in enumerate(sc.meshes):
        arrays[f"{key}/mesh{i}"] = np.asarray(m.v, np.float64)
        meshes.append({"off": m.off, "material": _material_data(m.material)})
    d = {"spheres": [{"m_center": _plain(s.m_center), "m_radius": s.m_radius, "material": _material_data(s.material)} for s in sc.spheres],
         "squares": [{"v": _plain(np.asarray(q.v, np.float64)), "m_right_vector": _plain(q.m_right_vector), "m_up_vector": _plain(q.m_up_vector),
                      "material": _material_data(q.material)} for q in sc.squares],
         "meshes": meshes,
         "lights": [{"pos": _plain(l.pos), "radius": l.radius, "material": _plain(l.material)} for l in sc.lights],
         "textures": list(sc.textures), "normals": list(sc.normals), "dark_sky": sc.dark_sky}
    return d, arrays


def write_golden(scenes):
    meta, arrays = {}, {}
    for ref_fn, aspect in scenes:
        key = golden_key(ref_fn, aspect)
        meta[key], a = scene_data(reference_scene(ref_fn, aspect), key)
        arrays.update(a)
    np.savez_compressed(GOLDEN, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)


def golden_scene(ref_fn, aspect):
    """The Scene of `ref_fn` at `aspect` as GOLDEN recorded it."""
    key = golden_key(ref_fn, aspect)
    with np.load(GOLDEN, allow_pickle=False) as g:
        d = json.loads(str(g["meta"]))[key]
        verts = {k: g[k] for k in g.files if k.startswith(key + "/")}

    def material(md):
        m = Material()
        for k, v in md.items():
            setattr(m, k, np.array(v, np.float64) if isinstance(v, list) else v)
        return m
    sc = Scene(os.path.join(ROOT, "assets"))
    for s in d["spheres"]:
        o = Sphere(); o.m_center = np.array(s["m_center"], np.float64); o.m_radius = s["m_radius"]; o.material = material(s["material"])
        sc.spheres.append(o)
    for q in d["squares"]:
        o = Square(); o.v = np.array(q["v"], np.float64); o.m_right_vector = np.array(q["m_right_vector"], np.float64)
        o.m_up_vector = np.array(q["m_up_vector"], np.float64); o.material = material(q["material"])
        sc.squares.append(o)
    for i, md in enumerate(d["meshes"]):
        o = Mesh(); o.off = md["off"]; o.v = verts[f"{key}/mesh{i}"]; o.material = material(md["material"])
        sc.meshes.append(o)
    for l in d["lights"]:
        o = Light(); o.pos = np.array(l["pos"], np.float64); o.radius = l["radius"]; o.material = np.array(l["material"], np.float64)
        sc.lights.append(o)
    sc.textures, sc.normals, sc.dark_sky = list(d["textures"]), list(d["normals"]), d["dark_sky"]
    return sc


def check(name, ref_fn, setup_name, aspect, hrt, sc=None):
    """Compares the host layer's flattened `setup_name` scene with the reference's objects: `sc` when given (golden_scene()),
    otherwise interpreted from the reference's Scene.h."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_layer import MeshDesc, SceneDesc
    if sc is None:
        sc = reference_scene(ref_fn, aspect)
    host = hrt.HostScene().setup(setup_name, aspect, 1); desc = host.flatten()
    d = C.cast(desc, C.POINTER(SceneDesc)).contents
    mats = C.cast(d.materials, C.POINTER(hrt.Material))
    fails = []
    def near(a, b, what):
        a = np.atleast_1d(np.asarray(a, np.float64)); b = np.atleast_1d(np.asarray(b, np.float64))
        if a.shape != b.shape or not np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))): fails.append(f"{what}: host {a.tolist()} reference {b.tolist()}")
    def material(hm, rm, what):
        near(hm.albedo[:], rm.diffuse_material, what + " diffuse_material"); near(hm.transparency, rm.transparency, what + " transparency")
        near(hm.index_medium, rm.index_medium, what + " index_medium"); near(hm.motion[:], rm.motion_blur_translation, what + " motion")
        if hm.type != ["Material_Diffuse_Blinn_Phong", "Material_Glass", "Material_Mirror"].index(rm.type): fails.append(what + " type")
        if hm.texture_type != ["Texture_None", "Texture_Checkerboard", "Texture_Image"].index(rm.texture_type): fails.append(what + " texture_type")
        near(hm.tex_scale_x, rm.texture_scale_x, what + " texture_scale_x"); near(hm.tex_scale_y, rm.texture_scale_y, what + " texture_scale_y")
        near(hm.checker1[:], rm.checkerboard_color1, what + " checker1"); near(hm.checker2[:], rm.checkerboard_color2, what + " checker2")
        if bool(hm.emissive) != bool(rm.emissive): fails.append(what + " emissive")
        if rm.emissive: near(hm.light_color[:], rm.light_color, what + " light_color"); near(hm.light_intensity, rm.light_intensity, what + " light_intensity")
        if rm.texture_type == "Texture_Image" and hm.image != rm.image: fails.append(f"{what} texture binding: host {hm.image} reference {rm.image}")
        want_nm = len(sc.textures) + rm.normals if rm.has_normal_map else -1
        if hm.normal_map != want_nm: fails.append(f"{what} normal-map binding: host {hm.normal_map} reference {want_nm}")
    n_ref_spheres = len(sc.spheres)
    if name != "random_spheres" and (d.n_spheres, d.n_quads, d.n_meshes, d.n_lights) != (len(sc.spheres), len(sc.squares), len(sc.meshes), len(sc.lights)):
        fails.append(f"object counts: host {(d.n_spheres, d.n_quads, d.n_meshes, d.n_lights)} reference {(len(sc.spheres), len(sc.squares), len(sc.meshes), len(sc.lights))}")
    sp = C.cast(d.spheres, C.POINTER(Sph)); qd = C.cast(d.quads, C.POINTER(Quad)); lg = C.cast(d.lights, C.POINTER(Lgt)); ms = C.cast(d.meshes, C.POINTER(MeshDesc))
    for i, s in enumerate(sc.spheres[:min(n_ref_spheres, d.n_spheres)]):
        near(sp[i].c[:], s.m_center, f"sphere {i} centre"); near(sp[i].r, s.m_radius, f"sphere {i} radius"); material(mats[sp[i].mat], s.material, f"sphere {i}")
    for i, q in enumerate(sc.squares[:d.n_quads]):
        near(qd[i].v0[:], q.v[0], f"square {i} vertex 0"); near(qd[i].v1[:], q.v[1], f"square {i} vertex 1"); near(qd[i].v3[:], q.v[3], f"square {i} vertex 3")
        near(qd[i].t[:], q.m_right_vector, f"square {i} m_right_vector"); near(qd[i].b[:], q.m_up_vector, f"square {i} m_up_vector")
        material(mats[qd[i].mat], q.material, f"square {i}")
    for i, m in enumerate(sc.meshes[:d.n_meshes]):
        pos = np.ctypeslib.as_array(C.cast(ms[i].positions, C.POINTER(C.c_float)), shape=(ms[i].n_vertices, 3))
        if pos.shape != m.v.shape: fails.append(f"mesh {i} ({m.off}) vertex count: host {pos.shape[0]} reference {m.v.shape[0]}")
        elif np.abs(pos - m.v).max() > 5 * TOL: fails.append(f"mesh {i} ({m.off}) transformed vertices differ by {np.abs(pos - m.v).max():.3g}")
        material(mats[ms[i].material], m.material, f"mesh {i}")
    for i, l in enumerate(sc.lights[:d.n_lights]):
        near(lg[i].pos[:], l.pos, f"light {i} pos"); near(lg[i].radius, l.radius, f"light {i} radius"); near(lg[i].color[:], l.material, f"light {i} material")
    if name != "backrooms_pool" and bool(d.dark_sky) != sc.dark_sky: fails.append("dark_sky")
    compared = f"{min(n_ref_spheres, d.n_spheres)} spheres, {min(len(sc.squares), d.n_quads)} squares, {min(len(sc.meshes), d.n_meshes)} meshes, {min(len(sc.lights), d.n_lights)} lights"
    return compared, fails


SCENES = (("cornell_box", "setup_cornell_box", "cornell_box", 16 / 9), ("cornell_box (1:1)", "setup_cornell_box", "cornell_box", 1.0),
          ("backrooms_pool", "setup_backrooms_pool", "backrooms_pool", 16 / 9), ("random_spheres", "setup_random_spheres", "random_spheres", 16 / 9))


def main():
    """Checks against the reference's Scene.h where it is present (`--write`: and records GOLDEN from it), else against GOLDEN."""
    live = os.path.isdir(os.path.join(REF, "src"))
    if "--write" in sys.argv:
        if not live:
            print("reference absent: cannot write " + os.path.relpath(GOLDEN, ROOT)); return 1
        write_golden([(ref_fn, aspect) for _, ref_fn, _, aspect in SCENES])
    hrt = importlib.import_module("hai719-raytracing_amd")
    bad = 0
    print("against " + ("the reference's set-up code" if live else os.path.relpath(GOLDEN, ROOT)))
    for name, ref_fn, setup, aspect in SCENES:
        compared, fails = check(name.split(" ")[0], ref_fn, setup, aspect, hrt, None if live else golden_scene(ref_fn, aspect))
        print(f"{name}: {'PASS' if not fails else 'FAIL'} ({compared})")
        for f in fails[:20]: print("   " + f)
        bad += bool(fails)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
