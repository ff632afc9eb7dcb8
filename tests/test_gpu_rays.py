"""Ray queries on caller rays (include/hrt.h hrt_trace_rays), bit for bit: camera rays against hrt_render_aov and the oracle's AOVs,
every closest-hit query of the oracle's paths (bounce rays off surfaces, motion-blur times), the shading of sampled rays against
hrt_render_features, tmax at and around the hit, the shipped kernel against the proof builds on far, axis-parallel, grazing and
edge rays, normalisation, degenerate rays, batch shapes up to 8 M rays, and queries beside a render of the same scene."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
INF = F32(np.inf)
SCENES = ["cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool", "single_sphere", "single_square", "mesh",
          "rt_in_a_weekend", "debug_refraction", "flamingo", "raccoon", "flamingo_pond", "flamingo_lake"]
EXACT, BRUTE, NO_LDS = 64, 128, 2
MISS = np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF], U32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def build(gpu, name, w, h):
    host = gpu.HostScene().setup(name, w / h, 1)
    desc = host.flatten()
    return host, desc, gpu.DeviceScene(desc), gpu.default_camera(w / h)


def make_rays(o, d, time=0.0, tmax=np.inf):
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    r = np.empty((o.shape[0], 8), F32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, time, d, tmax
    return r


def pixel_centre_rays(cam, w, h):
    y, x = np.mgrid[0:h, 0:w]
    uv = np.stack([(x.ravel().astype(F32) + F32(0.5)) / F32(w), (y.ravel().astype(F32) + F32(0.5)) / F32(h)], axis=1)
    cr = oracle_lib.camera_rays(cam, uv)
    return make_rays(cr[:, 0:3], cr[:, 3:6])


def aov(gpu, dev, cam, w, h, which):
    lib = gpu.device_lib()
    lib.hrt_render_aov.argtypes = [C.c_void_p, C.POINTER(gpu.Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    out = np.empty((h, w, 3), F32)
    assert lib.hrt_render_aov(dev._h, C.byref(cam), w, h, which, out.ctypes.data) == 0, lib.hrt_last_error()
    return out.reshape(-1, 3)


def path_queries(o, cam, w, h, pairs, seed, cap=8):
    """Every recorded closest-hit query of the oracle's paths: (rays, expected CLOSEST records as u32)."""
    rows = [oracle_lib.trace_path(o, cam, w, h, x, y, s, seed, cap) for x, y, s in pairs]
    rows = np.concatenate([r for r in rows if len(r)])
    rays = make_rays(rows[:, 0:3], rows[:, 3:6], rows[:, 6])
    kind = rows[:, 7].astype(U32)
    want = np.empty((rows.shape[0], 4), U32)
    want[:, 0] = bits(rows[:, 9])
    want[:, 1] = kind
    want[:, 2] = np.where(kind != 0, rows[:, 8].astype(np.int64), 0xFFFFFFFF).astype(U32)
    want[:, 3] = np.where(kind == 3, rows[:, 10].astype(np.int64), 0xFFFFFFFF).astype(U32)
    return rays, want


def sample_pairs(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [(int(x), int(y), int(s)) for x, y, s in zip(rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, 64, n))]


def tie_rows(got, want):
    """Rows that differ only in the triangle of a mesh hit, at the same t: an exact tie between two triangles of one mesh (shared edge
    or vertex), which the reference's tree settles by its own test order and the rope walk of the device by its own (the oracle's
    rope-tree mode picks what the device picks; hrt_render_aov shows the same pixels).  DESIGN section 5 "Ray queries"."""
    same = (got[:, 0] == want[:, 0]) & (got[:, 1] == want[:, 1]) & (got[:, 2] == want[:, 2])
    return same & (want[:, 1] == 3) & (got[:, 3] != want[:, 3])


def check_records(got, want, what, ties=False):
    got = bits(got)
    diff = (got != want).any(axis=1)
    if ties:  # against the oracle: exact triangle ties are allowed, and must stay rare
        tie = tie_rows(got, want)
        assert tie.sum() <= max(1, (want[:, 1] == 3).sum() // 100), f"{what}: {int(tie.sum())} triangle ties"
        diff &= ~tie
    bad = np.flatnonzero(diff)
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} records differ, first {bad[:4].tolist()}: got {got[bad[:2]].tolist()} want {want[bad[:2]].tolist()}"


# ------------------------------------------------------------------------------------------------------------- 1. camera rays
@pytest.mark.parametrize("name", SCENES)
def test_camera_rays_equal_render_aov_and_the_oracle(gpu, name):
    w, h = 37, 23
    _, desc, dev, cam = build(gpu, name, w, h)
    rays = pixel_centre_rays(cam, w, h)
    rec = dev.trace_rays(rays, "shade")
    ru = bits(rec)
    kind = ru[:, 1]
    ident = np.where(kind == 3, ru[:, 3], ru[:, 2]).astype(np.int64)
    hit = np.stack([rec[:, 0], kind.astype(F32), np.where(kind != 0, ident, -1).astype(F32)], axis=1)
    got = {"hit": hit, "normal": rec[:, 4:7], "albedo": rec[:, 8:11], "emission": rec[:, 12:15]}
    ref = oracle_lib.OracleScene(desc).aov(cam, w, h)
    for which, key in enumerate(["hit", "normal", "albedo", "emission"]):
        assert np.array_equal(bits(got[key]), bits(aov(gpu, dev, cam, w, h, which))), f"{name} {key}: differs from hrt_render_aov"
    # against the oracle by value, as the parity tests compare hrt_render_aov with it; the id may differ only on an exact triangle tie
    rh = ref["hit"].reshape(-1, 3)
    want = np.stack([bits(rh[:, 0]), rh[:, 1].astype(U32), np.where(rh[:, 1] != 0, rh[:, 2].astype(np.int64), 0xFFFFFFFF).astype(U32),
                     np.zeros(len(rh), U32)], axis=1)
    got4 = np.stack([ru[:, 0], kind, np.where(kind != 0, ident, 0xFFFFFFFF).astype(U32), np.zeros(len(ru), U32)], axis=1)
    want[:, 3], got4[:, 3] = want[:, 2], got4[:, 2]  # the id of a mesh hit is its triangle: a tie shows in the last column
    want[want[:, 1] == 3, 2] = got4[want[:, 1] == 3, 2] = 0
    check_records(got4.view(F32), want, f"{name} hit vs the oracle", ties=True)
    tie = tie_rows(got4, want)
    for key in ("normal", "albedo", "emission"):
        assert np.array_equal(got[key][~tie], ref[key].reshape(-1, 3)[~tie]), f"{name} {key}: differs from the oracle"
    miss = kind == 0
    assert (ru[miss, 4:] == 0).all() and (ru[miss, :4] == MISS).all(), f"{name}: a miss record is not the defined one"
    assert (ru[(kind == 1) | (kind == 2), 3] == 0xFFFFFFFF).all()
    check_records(dev.trace_rays(rays, "closest"), ru[:, :4], f"{name} CLOSEST vs SHADE")
    assert np.array_equal(dev.trace_rays(rays, "occluded"), (kind != 0).astype(U32)), f"{name}: OCCLUDED != (kind != 0)"


# --------------------------------------------------------------------------------------------------------------- 2. path rays
@pytest.mark.parametrize("name", SCENES)
def test_every_closest_hit_query_of_the_oracle_paths(gpu, name):
    w, h = 37, 23
    _, desc, dev, cam = build(gpu, name, w, h)
    o = oracle_lib.OracleScene(desc)
    rays, want = path_queries(o, cam, w, h, sample_pairs(w, h, 300, 11), seed=9)
    assert (want[:, 1] != 0).any(), "no hit among the queries"
    check_records(dev.trace_rays(rays, "closest"), want, f"{name} CLOSEST vs oracle_trace_path", ties=True)
    if name in ("rt_in_a_weekend", "random_spheres"):
        assert np.unique(rays[:, 3]).size > 50, "motion-blur times expected"


# --------------------------------------------------------------------------------------------------- 3. shading of sampled rays
@pytest.mark.parametrize("name", SCENES)
def test_shading_of_sampled_rays_equals_render_features(gpu, name):
    w, h, seed = 19, 11, 5
    _, desc, dev, cam = build(gpu, name, w, h)
    o = oracle_lib.OracleScene(desc)
    for s in (0, 3):
        rows = np.stack([oracle_lib.trace_path(o, cam, w, h, x, y, s, seed, cap=1)[0] for y in range(h) for x in range(w)])
        rec = dev.trace_rays(make_rays(rows[:, 0:3], rows[:, 3:6], rows[:, 6]), "shade")
        rec = np.where(rec == 0, F32(0), rec)  # -0.0 in a record compares as +0.0: the feature sums start from +0
        f = dev.render_features(cam, w, h, s, 1, seed).reshape(-1, 12)
        kind = bits(rec)[:, 1]
        got = np.concatenate([rec[:, 8:11], rec[:, 4:7], rec[:, 12:15], rec[:, 0:1], (kind != 0).astype(F32)[:, None]], axis=1)
        assert np.array_equal(bits(got), bits(f[:, :11])), f"{name} sample {s}: SHADE differs from render_features"


# --------------------------------------------------------------------------------------------------------------------- 4. tmax
@pytest.mark.parametrize("name", SCENES)
def test_tmax_cuts_exactly_at_the_hit(gpu, name):
    w, h = 37, 23
    _, desc, dev, cam = build(gpu, name, w, h)
    rays, want = path_queries(oracle_lib.OracleScene(desc), cam, w, h, sample_pairs(w, h, 120, 3), seed=2)
    t = want[:, 0].view(F32)
    rng = np.random.default_rng(4)
    variants = [np.full_like(t, INF), t, np.nextafter(t, INF), np.nextafter(t, F32(0)), t / F32(2), np.full_like(t, F32(1e-5)),
                rng.uniform(0, 2, t.size).astype(F32) * np.maximum(t, F32(1e-3)), rng.exponential(3.0, t.size).astype(F32)]
    for k, tmax in enumerate(variants):
        r = rays.copy()
        r[:, 7] = tmax
        keep = (want[:, 1] != 0) & (t < tmax)
        exp = np.where(keep[:, None], want, MISS)
        check_records(dev.trace_rays(r, "closest"), exp, f"{name} tmax variant {k}", ties=True)
        assert np.array_equal(dev.trace_rays(r, "occluded"), keep.astype(U32)), f"{name} tmax variant {k}: OCCLUDED"


# ------------------------------------------------------------------------------------------------------------- 5. proof builds
def hit_points(dev, rays):
    rec = dev.trace_rays(rays, "shade")
    hit = bits(rec)[:, 1] != 0
    p = rays[hit, 0:3].astype(np.float64) + rec[hit, 0:1].astype(np.float64) * rays[hit, 4:7].astype(np.float64)
    return p, rec[hit, 4:7].astype(np.float64), rays[hit, 3], bits(rec)[hit, 1]


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def hard_rays(dev, cam, w, h, seed):
    """Far origins (1e4, 1e6), axis-parallel directions, grazing rays in the planes of hit squares and triangles, rays from hit
    points along their surface, non-unit directions."""
    rng = np.random.default_rng(seed)
    p, n, _, kind = hit_points(dev, pixel_centre_rays(cam, w, h))
    tm = rng.uniform(0, 1, len(p)).astype(F32)  # motion-blur times
    out = []
    for R in (1e4, 1e6):  # far origins aimed at hit points, and some random directions
        u = unit(rng.normal(size=p.shape))
        o = p + R * u
        out.append(make_rays(o, unit(p - o), tm))
        out.append(make_rays(o[:64], unit(rng.normal(size=(min(64, len(o)), 3)))))
    for ax in range(3):  # axis-parallel: two zero components, and one
        e = np.zeros(3); e[ax] = 1.0
        out.append(make_rays(p - 3.0 * e, np.tile(e, (len(p), 1)), tm))
        out.append(make_rays(p + 3.0 * e, np.tile(-e, (len(p), 1)), tm))
        d = unit(rng.normal(size=p.shape)); d[:, ax] = 0.0
        d = unit(d)
        out.append(make_rays(p - 2.0 * d, d, tm))
    flat = kind >= 2  # squares and triangles: rays in their plane through the hit point, and from it along the surface
    t1 = unit(np.cross(n[flat], rng.normal(size=(int(flat.sum()), 3))))
    out.append(make_rays(p[flat] - 1.5 * t1, t1, tm[flat]))
    nd = rng.normal(size=p.shape) * rng.choice([1e-3, 0.1, 10.0, 1e3], size=(len(p), 1))  # non-unit directions
    out.append(make_rays(p - nd, nd, tm))
    n_before = sum(len(r) for r in out)
    out.append(make_rays(p[flat], t1, tm[flat]))  # last: from the hit point along the surface (see assert_builds_agree)
    out.append(make_rays(p[flat], -t1, tm[flat]))
    rays = np.concatenate(out)
    on_surface = np.zeros(len(rays), bool)
    on_surface[n_before:] = True
    return rays, on_surface


def edge_scene(gpu):
    """Squares with known corners (an axis-aligned floor and wall, tilted squares), a tetrahedron and a sphere."""
    M = gpu.Material.make
    s = gpu.HostScene()
    s.set_sky(False)
    quads = [((-4, -2, -8), (1, 0, 0), (0, 0, 1), 8.0, 8.0), ((-4, -2, -8), (1, 0, 0), (0, 1, 0), 8.0, 5.0),
             ((0.5, -1, -4), (0.8, 0.0, 0.6), (0.0, 1.0, 0.0), 1.5, 1.0), ((-2, 0, -5), (0.6, 0.64, 0.48), (-0.8, 0.48, 0.36), 1.0, 1.2)]
    for i, (bl, r, u, wd, ht) in enumerate(quads):
        s.add_quad(bl, r, u, wd, ht, M(albedo=(0.5, 0.6, 0.7), type=gpu.MAT_GLASS if i == 3 else gpu.MAT_DIFFUSE, index_medium=1.5))
    tet = np.array([[-1, -1, -3], [0.5, -1, -3.2], [-0.3, 0.4, -3.1], [-0.2, -0.4, -2.2]], np.float32)
    s.add_mesh(tet, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32), M(albedo=(0.9, 0.2, 0.2)))
    s.add_sphere((1.5, -1.2, -2.5), 0.8, M(albedo=(0.2, 0.9, 0.2), motion=(0.0, 0.3, 0.0)))
    return s, quads, tet


def edge_rays(quads, tet, seed):
    rng = np.random.default_rng(seed)
    out = []
    for bl, r, u, wd, ht in quads:
        bl, r, u = np.array(bl, np.float64), unit(np.array(r, np.float64)), unit(np.array(u, np.float64))
        corners = [bl, bl + wd * r, bl + ht * u, bl + wd * r + ht * u]
        for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):  # origins on the edges, directions everywhere and along the plane
            s = rng.uniform(0, 1, (200, 1))
            o = corners[a] + s * (corners[b] - corners[a])
            out.append(make_rays(o, unit(rng.normal(size=o.shape)), rng.uniform(0, 1, 200)))
            g = unit(rng.normal(size=(200, 1)) * r + rng.normal(size=(200, 1)) * u)
            out.append(make_rays(o - 2.0 * g, g))
            out.append(make_rays(o, g))
    for a, b, c in ((0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)):
        v0, v1, v2 = tet[a].astype(np.float64), tet[b].astype(np.float64), tet[c].astype(np.float64)
        wts = rng.dirichlet((1, 1, 1), 200)
        q = wts @ np.stack([v0, v1, v2])
        g = unit(rng.normal(size=(200, 1)) * (v1 - v0) + rng.normal(size=(200, 1)) * (v2 - v0))  # grazing, in the triangle's plane
        out.append(make_rays(q - 3.0 * g, g))
        e = v0 + rng.uniform(0, 1, (200, 1)) * (v1 - v0)  # through the triangle's edges
        out.append(make_rays(e + unit(rng.normal(size=(200, 3))) * 4.0, unit(e - (e + unit(rng.normal(size=(200, 3))) * 4.0))))
    return np.concatenate(out)


def assert_builds_agree(dev, rays, what, on_surface=None):
    # Two kinds of ray reach the limits of the rope walk that every kernel form shares (DESIGN section 5 "Ray queries"): a ray with a
    # zero direction component can lie IN a split plane of the KD-tree, and a ray that starts on a triangle and runs along its surface
    # meets that triangle at t ~ 0 in one cell and not in the other.  The walk (shipped and EXACT alike) then follows one side and the
    # brute-force test may pick differently.  Those rays are held to EXACT and NO_LDS only; every other ray to all the proof builds.
    in_plane = (rays[:, 4:7] == 0).any(axis=1)
    if on_surface is not None:
        in_plane |= on_surface
    for mode in ("closest", "shade", "occluded"):
        base = bits(dev.trace_rays(rays, mode))
        for flags in (EXACT, EXACT | BRUTE, NO_LDS, EXACT | NO_LDS):
            got = bits(dev.trace_rays(rays, mode, flags=flags))
            neq = got != base if got.ndim == 1 else (got != base).any(axis=1)
            if flags & BRUTE:
                neq &= ~in_plane
            bad = np.flatnonzero(neq)
            assert bad.size == 0, f"{what} {mode} flags {flags}: {bad.size} of {len(rays)} records differ from the shipped kernel, first rays {rays[bad[:2]].tolist()}"


@pytest.mark.parametrize("name", SCENES)
def test_shipped_kernel_equals_the_proof_builds_on_hard_rays(gpu, name):
    w, h = 37, 23
    _, desc, dev, cam = build(gpu, name, w, h)
    rays, on_surface = hard_rays(dev, cam, w, h, seed=len(name))
    assert_builds_agree(dev, rays, name, on_surface)


def test_shipped_kernel_equals_the_proof_builds_on_square_edges(gpu):
    host, quads, tet = edge_scene(gpu)
    dev = gpu.DeviceScene(host.flatten())
    rays = edge_rays(quads, tet, seed=1)
    assert (bits(dev.trace_rays(rays, "closest"))[:, 1] != 0).mean() > 0.05
    assert_builds_agree(dev, rays, "edge scene")


# ---------------------------------------------------------------------------------------------------------------- 6. normalise
@pytest.mark.parametrize("name", ["cornell_mesh", "rt_in_a_weekend", "backrooms_pool"])
def test_normalize_flag_equals_directions_normalised_by_the_device(gpu, name):
    w, h = 37, 23
    _, desc, dev, cam = build(gpu, name, w, h)
    rays, _ = path_queries(oracle_lib.OracleScene(desc), cam, w, h, sample_pairs(w, h, 100, 8), seed=4)
    rng = np.random.default_rng(6)
    raw = rays.copy()
    raw[:, 4:7] *= rng.choice([1e-3, 0.37, 3.0, 1e3], size=(len(raw), 1)).astype(F32) * rng.uniform(0.5, 2, (len(raw), 3)).astype(F32)
    pre = raw.copy()
    pre[:, 4:7] = gpu.debug_kat(gpu.KAT_NORMALIZE, raw[:, 4:7])
    for mode in ("closest", "shade", "occluded"):
        assert np.array_equal(bits(dev.trace_rays(raw, mode, normalize=True)), bits(dev.trace_rays(pre, mode))), f"{name} {mode}"


# --------------------------------------------------------------------------------------------------------------- 7. degenerate
def test_degenerate_rays_give_the_miss_record_and_leave_the_batch_alone(gpu):
    w, h = 37, 23
    _, desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    good = pixel_centre_rays(cam, w, h)
    nan, inf = F32(np.nan), INF
    bad_rows = []
    for col in range(7):  # o, time, d: NaN, +inf, -inf one component at a time
        for v in (nan, inf, -inf):
            r = good[col * 3 % len(good)].copy(); r[col] = v; bad_rows.append(r)
    for z in ((0, 0, 0), (-0.0, 0, -0.0)):
        r = good[5].copy(); r[4:7] = z; bad_rows.append(r)
    for tm in (nan, F32(0), F32(-0.0), F32(-1), -inf, F32(-1e-30)):
        r = good[7].copy(); r[7] = tm; bad_rows.append(r)
    bad = np.array(bad_rows, F32)
    mixed = np.concatenate([good, bad])
    order = np.random.default_rng(1).permutation(len(mixed))
    mixed = mixed[order]
    is_bad = order >= len(good)
    for mode in ("closest", "shade", "occluded"):
        ref = bits(dev.trace_rays(good, mode))
        got = bits(dev.trace_rays(mixed, mode))
        for flags in (0, EXACT):
            got_f = bits(dev.trace_rays(mixed, mode, flags=flags))
            if mode == "occluded":
                assert (got_f[is_bad] == 0).all()
            elif mode == "closest":
                assert (got_f[is_bad] == MISS).all()
            else:
                assert (got_f[is_bad, :4] == MISS).all() and (got_f[is_bad, 4:] == 0).all()
        assert np.array_equal(got[~is_bad], ref[order[~is_bad]]), f"{mode}: good rays changed beside degenerate ones"
    # a direction whose length under- or overflows is degenerate only under HRT_RAYS_NORMALIZE
    tiny = good[:4].copy(); tiny[:, 4:7] = F32(1e-30)
    assert (bits(dev.trace_rays(tiny, "closest", normalize=True)) == MISS).all()


# ------------------------------------------------------------------------------------------------------------ 8. batch shapes
def test_batch_shapes(gpu):
    import torch
    w, h = 64, 36
    _, desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = cus * 256 * 8 + 1  # a multiple of any resident grid's capacity, plus one
    base = pixel_centre_rays(cam, w, h)
    rays = np.concatenate([base] * (big // len(base) + 1))[:big]
    rays[:, 4:7] = gpu.debug_kat(gpu.KAT_NORMALIZE, rays[:, 4:7] + np.random.default_rng(0).normal(0, 0.05, (big, 3)).astype(F32))
    full = {m: bits(dev.trace_rays(rays, m)) for m in ("closest", "shade", "occluded")}
    sub = np.arange(0, big, 37)
    for m in full:
        assert np.array_equal(bits(dev.trace_rays(rays[sub], m, flags=EXACT)), full[m][sub]), m
    for n in (1, 63, 64, 65, 255, 257, 4097):
        for m in full:
            assert np.array_equal(bits(dev.trace_rays(rays[:n], m)), full[m][:n]), (n, m)
    # n == 0: OK, nothing launched, the output untouched
    out = torch.full((16, 4), 7.0, device="cuda")
    r = torch.from_numpy(rays[:4].copy()).cuda()
    lib = gpu.device_lib()
    for q in (0, 1, 2):
        assert lib.hrt_trace_rays(dev._h, C.c_void_p(r.data_ptr()), 0, q, 0, C.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert dev.trace_rays(np.zeros((0, 8), F32), "shade").shape == (0, 16)


def test_eight_million_rays_on_backrooms_pool(gpu):
    import torch
    w, h = 1920, 1080
    _, desc, dev, cam = build(gpu, "backrooms_pool", w, h)
    y, x = np.mgrid[0:h, 0:w]
    uvs = []
    for jx, jy in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):
        uvs.append(np.stack([(x.ravel().astype(F32) + F32(jx)) / F32(w), (y.ravel().astype(F32) + F32(jy)) / F32(h)], axis=1))
    cr = oracle_lib.camera_rays(cam, np.concatenate(uvs))
    rays = torch.from_numpy(make_rays(cr[:, 0:3], cr[:, 3:6])).cuda()
    assert rays.shape[0] == 4 * w * h
    sub = torch.arange(0, rays.shape[0], 1009, device="cuda")
    for m in ("closest", "shade", "occluded"):
        full = dev.trace_rays(rays, m)
        want = dev.trace_rays(rays[sub].contiguous(), m, flags=EXACT)
        torch.cuda.synchronize()
        assert torch.equal(full[sub].view(torch.int32), want.view(torch.int32)), m
        if m == "closest":
            assert (full[:, 1].view(torch.int32) != 0).float().mean().item() > 0.5


# --------------------------------------------------------------------------------------------------------------- 9. streams
def test_queries_on_a_second_stream_beside_a_render_of_the_same_scene(gpu):
    import torch
    w, h, spp, seed = 480, 270, 8, 3
    _, desc, dev, cam = build(gpu, "cornell_mesh", w, h)
    rays_np = pixel_centre_rays(cam, w, h)
    rays_np = np.concatenate([rays_np, hard_rays(dev, gpu.default_camera(64 / 36), 64, 36, 1)[0]])
    rays = torch.from_numpy(rays_np).cuda()
    tiles = gpu.tiles_total(w, h)
    want_t = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, want_t.data_ptr(), 0)
    dev.check_last_launch()
    want = {m: dev.trace_rays(rays, m) for m in ("closest", "shade", "occluded")}
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t = torch.zeros_like(want_t)
    torch.cuda.synchronize()
    dev.render_tiles(cam, w, h, spp, seed, 0, 0, 1, t.data_ptr(), s1.cuda_stream)
    with torch.cuda.stream(s2):
        got = {m: dev.trace_rays(rays, m) for m in ("closest", "shade", "occluded")}
    torch.cuda.synchronize()
    dev.check_last_launch()
    for m in want:
        assert torch.equal(got[m].view(torch.int32), want[m].view(torch.int32)), f"{m} beside a render"
    assert torch.equal(t.view(torch.int32), want_t.view(torch.int32)), "the render changed beside queries"
