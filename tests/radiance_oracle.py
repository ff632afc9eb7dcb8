"""What tests/test_oracle_radiance.py (CPU) and tests/test_gpu_radiance_oracle.py (GPU) share: the scenes, the families of
non-camera rays, and the oracle's value for them under the tie rule.

Every ray here is made WITHOUT a GPU: the hit points the families start from are the oracle's own first hits
(OracleScene.aov, which tests/test_gpu_rays.py holds the device's SHADE records to).  So the CPU test can count the tie rays of
exactly the batches the GPU test traces.

THE TIE RULE.  A mesh ray may be settled differently by the reference-shaped tree (MESH_REF_TREE) and by the rope walk the device
runs (MESH_ROPE_TREE): exact ties between two triangles and rays in a split plane, DESIGN section 5 "Ray queries".  A ray is a
tie ray exactly when the oracle's two modes disagree on its value bit-wise.  Off the tie rays the device is held to the REF_TREE
value, on them to the ROPE_TREE value; `tie_cap` bounds how many there may be."""
import numpy as np

import oracle_lib
import test_gpu_rays as qr
from scene_util import many_spheres, many_squares

F32 = np.float32
U32 = np.uint32
THREADS = 8          # workers of oracle_radiance (the tests stay at or below 16)
W, H = 37, 23        # the frame whose pixel-centre first hits are the families' hit points
SEED = 2 ** 63 + 12345
EXTRA = ["many_squares", "many_spheres", "edge_scene", "skybox", "dark_spheres"]
SLOW = ("flamingo_pond", "raccoon")  # about 1 ms per path on the CPU: the smallest batches


def tie_cap(n):
    """The cap tests/test_gpu_rays.py uses for triangle ties."""
    return max(1, n // 100)


# --------------------------------------------------------------------------------------------------------------------- scenes
def skybox_scene(hrt):
    """The skybox-image scene of test_gpu_parity.test_skybox_image_lookup."""
    M = hrt.Material.make
    rng = np.random.default_rng(8)
    s = hrt.HostScene()
    sky = rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)
    sky[:, :, 2] = np.linspace(0, 255, 64).astype(np.uint8)[None, :]
    s.set_skybox(sky)
    s.add_sphere((-0.9, 0.0, -1.0), 0.8, M(albedo=(0.9, 0.9, 0.9), type=hrt.MAT_MIRROR))
    s.add_sphere((0.9, 0.1, -0.5), 0.6, M(albedo=(1, 1, 1), type=hrt.MAT_GLASS, transparency=0.9, index_medium=1.5))
    s.add_quad((-2, -1.2, -3), (1, 0, 0.1), (0, 0.2, 1), 4, 4, M(albedo=(0.7, 0.6, 0.5)))
    return s


class Scene:
    """A host scene, its flattened description and the default camera of a w x h frame, and the oracle in both mesh modes (built on
    first use)."""

    def __init__(self, hrt, name, w, h):
        self.name, self.w, self.h = name, w, h
        if name == "many_squares":
            self.host = many_squares(hrt, 20, 2)       # one light, gradient sky, moving squares, two meshes
        elif name == "many_spheres":
            self.host = many_spheres(hrt, 12, 2)       # two lights, gradient sky, moving spheres
        elif name == "dark_spheres":
            self.host = many_spheres(hrt, 12, 1, dark=True)
        elif name == "edge_scene":
            self.host = qr.edge_scene(hrt)[0]          # no light, gradient sky, a moving sphere, a glass square, a tetrahedron
        elif name == "skybox":
            self.host = skybox_scene(hrt)
        else:
            self.host = hrt.HostScene().setup(name, w / h, 1)
        self.desc = self.host.flatten()
        self.cam = hrt.default_camera(w / h)
        self._oracle = {}
        self._hits = None

    def oracle(self, mode=oracle_lib.MESH_REF_TREE):
        if mode not in self._oracle:
            self._oracle[mode] = oracle_lib.OracleScene(self.desc, mode)
        return self._oracle[mode]

    def hits(self):
        """(p, n, kind, d) of the pixel-centre rays that hit: point and shading normal in float64, hit kind, incoming direction."""
        if self._hits is None:
            rays = qr.pixel_centre_rays(self.cam, self.w, self.h)
            rec = AovDevice(self).trace_rays(rays, "shade")
            p, n, _, kind = qr.hit_points(AovDevice(self, rec), rays)
            self._hits = (p, n, kind, rays[qr.bits(rec)[:, 1] != 0, 4:7].astype(np.float64))
        return self._hits


class AovDevice:
    """Stands in for a DeviceScene where qr.hit_points asks for the SHADE records of the pixel-centre rays of the scene's frame: t,
    kind and shading normal from the oracle's first-hit AOVs."""

    def __init__(self, scene, records=None):
        self.scene, self.records = scene, records

    def trace_rays(self, rays, mode):
        sc = self.scene
        assert mode == "shade" and len(rays) == sc.w * sc.h
        if self.records is None:
            aov = sc.oracle().aov(sc.cam, sc.w, sc.h)
            hit = aov["hit"].reshape(-1, 3)
            rec = np.zeros((sc.w * sc.h, 16), F32)
            rec[:, 0] = hit[:, 0]
            rec.view(U32)[:, 1] = hit[:, 1].astype(U32)
            rec[:, 4:7] = aov["normal"].reshape(-1, 3)
            self.records = rec
        return self.records


_scenes = {}


def scene(hrt, name, w=W, h=H):
    if (name, w, h) not in _scenes:
        _scenes[name, w, h] = Scene(hrt, name, w, h)
    return _scenes[name, w, h]


# ------------------------------------------------------------------------------------------------------------------- families
def batch_size(name, family):
    """400..900 rays, never a multiple of 64, the slow scenes at the low end."""
    n = 401 + 2 * FAMILIES.index(family) if name in SLOW else 523 + 37 * FAMILIES.index(family)
    assert 400 <= n <= 900 and n % 64
    return n


def _pick(sc, n, rng):
    p, nrm, kind, d = sc.hits()
    assert len(p) >= 16, f"{sc.name}: too few hit points"
    i = rng.integers(0, len(p), n)
    return p[i], nrm[i], kind[i], d[i]


def baking(sc, n, rng):
    """1e-4 off the surface on the side the ray came from, cosine-like lobe: test_gpu_radiance.baking_rays' construction, at random times."""
    p, nrm, _, d = _pick(sc, n, rng)
    nrm = np.where((nrm * d).sum(1, keepdims=True) > 0, -nrm, nrm)
    return qr.make_rays(p + 1e-4 * nrm, qr.unit(nrm + qr.unit(rng.normal(size=nrm.shape))), rng.uniform(0, 1, n))


def interior(sc, n, rng):
    """Origins 1e-3 BEHIND the first hit, random directions: inside glass and mirror spheres, inside closed meshes, behind walls."""
    p, _, _, d = _pick(sc, n, rng)
    return qr.make_rays(p + 1e-3 * d, qr.unit(rng.normal(size=p.shape)), rng.uniform(0, 1, n))


def far(sc, n, rng):
    """Origins 1e4 and 1e6 away, aimed at hit points; one ray in eight in a random direction instead."""
    p, _, _, _ = _pick(sc, n, rng)
    R = np.where(np.arange(n) % 2 == 0, 1e4, 1e6)[:, None]
    o = p + R * qr.unit(rng.normal(size=p.shape))
    d = qr.unit(p - o)
    stray = np.arange(n) % 8 == 7
    d[stray] = qr.unit(rng.normal(size=(int(stray.sum()), 3)))
    return qr.make_rays(o, d, rng.uniform(0, 1, n))


def grazing(sc, n, rng):
    """qr.hard_rays' axis-parallel rays (two zero components, and one), rays in the plane of a hit square or triangle through the hit
    point, and rays from the hit point along its surface, both ways."""
    p, nrm, kind, _ = _pick(sc, n, rng)
    o, d = np.empty_like(p), np.empty_like(p)
    t1 = qr.unit(np.cross(nrm, rng.normal(size=p.shape)))
    for i in range(n):
        how, ax = i % 6, (i // 6) % 3
        e = np.zeros(3); e[ax] = 1.0
        if how >= 3 and kind[i] < 2:  # a sphere has no plane: the axis-parallel forms instead
            how -= 3
        if how == 0:
            o[i], d[i] = p[i] - 3.0 * e, e
        elif how == 1:
            o[i], d[i] = p[i] + 3.0 * e, -e
        elif how == 2:
            g = rng.normal(size=3); g[ax] = 0.0
            g = qr.unit(g)
            o[i], d[i] = p[i] - 2.0 * g, g
        elif how == 3:
            o[i], d[i] = p[i] - 1.5 * t1[i], t1[i]
        else:
            o[i], d[i] = p[i], t1[i] if how == 4 else -t1[i]
    return qr.make_rays(o, d, rng.uniform(0, 1, n))


def nonunit(sc, n, rng):
    """Directions scaled by 1e-3, 0.1, 10 and 1e3, towards hit points from 0.5 .. 3 away."""
    p, _, _, _ = _pick(sc, n, rng)
    u = qr.unit(rng.normal(size=p.shape))
    o = p + rng.uniform(0.5, 3.0, (n, 1)) * u
    scale = np.array([1e-3, 0.1, 10.0, 1e3])[np.arange(n) % 4][:, None]
    return qr.make_rays(o, -u * scale, rng.uniform(0, 1, n))


FAMILIES = ["baking", "interior", "far", "grazing", "nonunit"]
_MAKERS = {"baking": baking, "interior": interior, "far": far, "grazing": grazing, "nonunit": nonunit}
_rays = {}


def rays(hrt, name, family):
    """The batch of (scene, family): the same array on every call."""
    if (name, family) not in _rays:
        rng = np.random.default_rng([FAMILIES.index(family), sum(name.encode())])
        _rays[name, family] = _MAKERS[family](scene(hrt, name), batch_size(name, family), rng)
    return _rays[name, family].copy()


def random_keys(n, rng):
    """Random 32-bit keys with 0 and 0xFFFFFFFF among them, and one key in five repeated from elsewhere in the batch."""
    k = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32)
    k[rng.integers(0, n)] = 0
    k[rng.integers(0, n)] = 0xFFFFFFFF
    again = rng.choice(n, n // 5, replace=False)
    k[again] = k[rng.integers(0, n, again.size)]
    k[0], k[n - 1] = 0, 0xFFFFFFFF
    return k


# --------------------------------------------------------------------------------------------------------------------- oracle
_values = {}


def oracle_pair(sc, batch, cache_key=None, **kw):
    """(REF_TREE value, ROPE_TREE value, tie mask) of OracleScene.radiance(batch, **kw)."""
    if cache_key is not None and cache_key in _values:
        return _values[cache_key]
    ref = sc.oracle(oracle_lib.MESH_REF_TREE).radiance(batch, threads=THREADS, **kw)
    rope = sc.oracle(oracle_lib.MESH_ROPE_TREE).radiance(batch, threads=THREADS, **kw)
    tie = (qr.bits(ref) != qr.bits(rope)).any(axis=1)
    if cache_key is not None:
        _values[cache_key] = (ref, rope, tie)
    return ref, rope, tie


def expected(sc, batch, cache_key=None, **kw):
    """The value the device is held to, and the tie mask: REF_TREE off the tie rays, ROPE_TREE on them; the tie rays within the cap."""
    ref, rope, tie = oracle_pair(sc, batch, cache_key, **kw)
    assert tie.sum() <= tie_cap(len(batch)), f"{sc.name}: {int(tie.sum())} tie rays of {len(batch)}"
    return np.where(tie[:, None], rope, ref), tie


def family_expected(hrt, name, family, S=3, normalize=False):
    """expected() of (scene, family) at keys None, samples [0, S), SEED: computed once per process."""
    return expected(scene(hrt, name), rays(hrt, name, family), cache_key=(name, family, S, normalize), n_samples=S, seed=SEED,
                    normalize=normalize)


def worst(got, want):
    """Largest |got - want| / max(1, |want|) over the values finite on both sides."""
    a, r = got.astype(np.float64), want.astype(np.float64)
    both = np.isfinite(a) & np.isfinite(r)
    return float((np.abs(np.where(both, a - r, 0.0)) / np.maximum(1.0, np.abs(np.where(both, r, 0.0)))).max()) if a.size else 0.0
