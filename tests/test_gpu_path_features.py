"""Path features on the GPU (include/hrt.h "Path features").  Every comparison but the oracle's chains (5) is on bits.

1. CONTRACT B: the record agrees with the tail record of path_tails(tail_after = 1, bias = 0), also in the proof builds;
2. CONTRACT A: where the first hit is diffuse, or the ray misses, the record is trace_rays("shade")'s, and a pixel all of whose
   samples are such has the bits of render_lens_features / render_features;
3. CONTRACT C: the frames are the fold (tests/path_features_ref.py) of lens_rays and path_features, for every lens, in a batch, and
   through a camera;
4. a mirror seen by hand-made rays: what the feature is for;
5. depth and emission along chains, against the CPU oracle's paths shaded segment by segment;
6. the guided renders are denoise / denoise_var of the same frames with render_path_features;
7. the command-line tool;
8. repeated calls leave no live device resource.
Frames are 19 x 11 = 209 pixels: the last wave is partial, and in a batch waves straddle views."""
import os
import subprocess

import numpy as np
import pytest

import lit_paths_ref as lp
import oracle_lib
import path_features_ref as pf
import radiance_oracle
import test_gpu_denoise_var as tdv
import test_gpu_lens as tlens
import test_gpu_rays as qr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W, H = 19, 11
NPIX = W * H
EXACT, BRUTE = 64, 128
FIRST, S, SEED = 3, 5, 11
SCENES = ["cornell_mesh", "random_spheres", "skybox"]
# What contract B can say of the emission: cornell_mesh has no lights and a dark sky (E / 6 is the tail's a on every path); the
# skybox scene has no lights but a sky, which the tail record adds where a path ends in a miss (a reached path never does);
# random_spheres has lights, whose direct term is in the tail's a and not in E.
EMISSION = {"cornell_mesh": "all", "skybox": "reached", "random_spheres": None}
bits = qr.bits

_cases, _rays = {}, {}


def case(gpu, name):
    """(device scene, camera, description, the lenses by name) of a scene, built once."""
    if name not in _cases:
        if name == "skybox":
            desc = radiance_oracle.skybox_scene(gpu).flatten()
            dev, cam = gpu.DeviceScene(desc), gpu.default_camera(W / H)
        else:
            _, desc, dev, cam = qr.build(gpu, name, W, H)
        lenses = {k: v for k, v in tlens.lenses(gpu, cam).items() if k in ("pinhole", "thin", "equirect")}
        lenses["fisheye200"] = gpu.Lens(cam, "fisheye", extent=200.0)
        _cases[name] = (dev, cam, desc, lenses)
    return _cases[name]


def lens_rays(gpu, name, lname, s, seed=SEED):
    """hrt_lens_rays(lens, W, H, s, seed) of a case's lens as a NumPy array, made once and left unchanged."""
    key = (name, lname, s, seed)
    if key not in _rays:
        _rays[key] = gpu.lens_rays(case(gpu, name)[3][lname], W, H, s, seed).cpu().numpy()
    return _rays[key]


def ray_sets(gpu, name, lnames, samples):
    """(label, rays, sample) of the lens rays of the named lenses at `samples`; for the skybox scene, whose default camera sees
    little but sky, also the project's own non-camera rays from inside the scene and from its surfaces (radiance_oracle.rays)."""
    sets = [(lname, lens_rays(gpu, name, lname, s), s) for lname in lnames for s in samples]
    if name == "skybox":
        sets += [(family, radiance_oracle.rays(gpu, "skybox", family), s) for family in ("interior", "baking") for s in samples]
    return sets


def traced(rays):
    return (rays[:, 4:7] != 0).any(axis=1)


def first_hits(gpu, ru):
    """(hit, first hit diffuse, first hit mirror or glass) of SHADE records as words."""
    hit = ru[:, gpu.HIT_KIND] != gpu.KIND_MISS
    diffuse = hit & (ru[:, gpu.SHADE_MATERIAL_TYPE] == gpu.MAT_DIFFUSE)
    return hit, diffuse, hit & ~diffuse


# ------------------------------------------------------------------------------------------------- 1. contract B: the tail record
@pytest.mark.parametrize("flags", [0, EXACT, EXACT | BRUTE])
@pytest.mark.parametrize("name", SCENES)
def test_the_record_agrees_with_the_tail_record_of_the_same_path(gpu, name, flags):
    dev = case(gpu, name)[0]
    seen = np.zeros(3, int)  # reached, unreached, reached after two or more segments
    for label, rays, s in ray_sets(gpu, name, ("pinhole", "equirect"), range(S)):
        n = len(rays)
        keys = radiance_oracle.random_keys(n, np.random.default_rng(5))
        T = dev.path_tails(rays, 1, s, seed=SEED, keys=keys, flags=flags)
        R = dev.path_features(rays, s, seed=SEED, keys=keys, flags=flags)
        assert R.shape == (n, 12) and R.dtype == F32
        albedo, normal, coverage, a = pf.from_tail(T)
        _, _, seg, reached, _ = lp.split(T)
        what = (name, flags, label, s)
        assert np.array_equal(bits(R[:, pf.ALBEDO]), bits(albedo)), what
        assert np.array_equal(bits(R[:, pf.NORMAL]), bits(normal)), what
        assert np.array_equal(bits(R[:, pf.COVERAGE]), bits(coverage)) and not bits(R[:, 11]).any(), what
        assert not bits(R[~reached][:, [0, 1, 2, 3, 4, 5, 9]]).any(), (what, "an unreached path keeps nothing but E")
        assert (R[reached, pf.DEPTH] > 0).all(), what
        if EMISSION[name]:
            where = reached if EMISSION[name] == "reached" else np.ones(n, bool)
            assert np.array_equal(bits(R[where, pf.EMISSION] / F32(6)), bits(a[where])), (what, "E / 6.f is the tail's a")
        seen += (int(reached.sum()), int((~reached).sum()), int((reached & (seg >= 2)).sum()))
    print(f"{name}, flags {flags}: reached {seen[0]}, unreached {seen[1]}, reached after two or more segments {seen[2]}")
    # Without both kinds of path, and without chains that reach the tail, the comparison shows nothing.  The skybox scene's square
    # is seen from one side only and lies under the spheres: no chain off its mirror or through its glass ever reaches it, so there
    # the chains are the unreached ones (the sky is not in E); cornell_mesh and random_spheres have the chains that reach.
    assert seen[0] >= 20 and seen[1] >= 10 and (seen[2] >= 5 or name == "skybox"), (name, seen.tolist())


def test_keys_samples_the_torch_form_and_degenerate_rays(gpu):
    import torch
    dev = case(gpu, "cornell_mesh")[0]
    rays = lens_rays(gpu, "cornell_mesh", "pinhole", 0).copy()
    rays[7, 4:7] = 0
    rays[100, 0] = np.nan
    base = dev.path_features(rays, 2, seed=SEED)
    assert not bits(base[[7, 100]]).any(), "a degenerate ray gives twelve zeros"
    keys = np.arange(NPIX, dtype=U32)[::-1].copy()
    flipped = dev.path_features(rays[::-1].copy(), 2, seed=SEED, keys=keys)
    assert np.array_equal(bits(flipped[::-1]), bits(base)), "the key, not the position in the batch, names the stream"
    big = torch.full((NPIX + 2, 12), 7.0, dtype=torch.float32, device="cuda")
    got = dev.path_features(torch.from_numpy(rays).cuda(), 2, seed=SEED, out=big[1:NPIX + 1])
    torch.cuda.synchronize()
    assert isinstance(got, torch.Tensor) and np.array_equal(bits(got.cpu().numpy()), bits(base))
    assert (big[0] == 7.0).all() and (big[NPIX + 1] == 7.0).all(), "nothing is written outside the batch"
    for b in (1, 63, 64, 65):
        assert np.array_equal(bits(dev.path_features(rays[:b], 2, seed=SEED)), bits(base[:b])), b
    assert dev.path_features(np.zeros((0, 8), F32)).shape == (0, 12)


# ----------------------------------------------------------------------------------------------- 2. contract A: first-hit values
@pytest.mark.parametrize("name", SCENES)
def test_a_diffuse_first_hit_or_a_miss_gives_the_first_hit_values(gpu, name):
    dev, cam, _, lenses = case(gpu, name)
    firsts = np.zeros(3, int)  # first hits over the lenses and samples: diffuse, mirror or glass, none
    for lname in ("pinhole", "thin", "equirect"):
        qualifies = np.ones(NPIX, bool)
        for s in range(FIRST, FIRST + S):
            rays = lens_rays(gpu, name, lname, s)
            ru = bits(dev.trace_rays(rays, "shade"))
            rec = ru.view(F32)
            hit, diffuse, specular = first_hits(gpu, ru)
            R = dev.path_features(rays, s, seed=SEED)
            want = np.zeros((NPIX, 12), F32)
            want[:, pf.ALBEDO], want[:, pf.NORMAL], want[:, pf.EMISSION] = rec[:, gpu.SHADE_ALBEDO], rec[:, gpu.SHADE_NORMAL], rec[:, gpu.SHADE_EMISSION]
            want[:, pf.DEPTH], want[:, pf.COVERAGE] = rec[:, gpu.HIT_T], 1
            want[~hit] = 0
            ok = diffuse | ~hit
            assert np.array_equal(bits(R[ok]), bits(want[ok])), (name, lname, s)
            firsts += (int(diffuse.sum()), int(specular.sum()), int((~hit).sum()))
            qualifies &= ok
        got = dev.render_lens_path_features(lenses[lname], W, H, FIRST, S, SEED).reshape(NPIX, 12)
        first = dev.render_lens_features(lenses[lname], W, H, FIRST, S, SEED).reshape(NPIX, 12)
        same = (bits(got) == bits(first)).all(axis=1)
        print(f"{name}, {lname}: {int(qualifies.sum())} of {NPIX} pixels have only diffuse first hits or misses; the frames differ on {int((~same).sum())}")
        assert qualifies.sum() >= 20 and (~qualifies).sum() >= 2, (name, lname)
        assert same[qualifies].all(), (name, lname, np.flatnonzero(~same & qualifies)[:8].tolist())
        assert (~same[~qualifies]).any(), (name, lname, "behind mirror and glass the features differ")
        if lname == "pinhole":
            assert np.array_equal(bits(first), bits(dev.render_features(cam, W, H, FIRST, S, SEED).reshape(NPIX, 12)))
    assert firsts[0] >= 20 and firsts[1] >= 2 and firsts[2] >= 2, (name, firsts.tolist(), "all three kinds of first hit are among the rays")


# ----------------------------------------------------------------------------------------------- 3. contract C: the frame forms
def folded(gpu, name, lname, first, n, seed):
    dev = case(gpu, name)[0]
    recs, mask = [], []
    for s in range(first, first + n):
        rays = lens_rays(gpu, name, lname, s, seed)
        recs.append(dev.path_features(rays, s, seed=seed))
        mask.append(traced(rays))
    return pf.fold(np.stack(recs), np.stack(mask)), np.stack(mask)


@pytest.mark.parametrize("name", SCENES)
def test_the_frame_is_the_fold_of_lens_rays_and_path_features(gpu, name):
    dev, cam, _, lenses = case(gpu, name)
    for lname, lens in lenses.items():
        want, mask = folded(gpu, name, lname, FIRST, S, SEED)
        got = dev.render_lens_path_features(lens, W, H, FIRST, S, SEED)
        assert got.shape == (H, W, 12) and np.isfinite(got).all() and got.any()
        bad = np.flatnonzero((bits(got.reshape(NPIX, 12)) != bits(want)).any(axis=1))
        assert bad.size == 0, (name, lname, bad[:8].tolist())
        if lname == "fisheye200":
            outside = ~mask.any(axis=0)
            # the circle is inscribed in the frame's height: it covers pi * H / (4 * W) = 0.455 of the frame, the rest lies outside
            assert 8 <= outside.sum() <= int(NPIX * (1 - np.pi * H / (4 * W)))
            assert not bits(got.reshape(NPIX, 12)[outside]).any() and got.reshape(NPIX, 12)[~outside].any()
            assert (mask.any(axis=0) & ~mask.all(axis=0)).any(), "the rim crosses pixels: some have samples on both sides"
    pin = dev.render_lens_path_features(lenses["pinhole"], W, H, FIRST, S, SEED)
    assert np.array_equal(bits(dev.render_path_features(cam, W, H, FIRST, S, SEED)), bits(pin)), "a camera is its pinhole lens"
    one = dev.render_lens_path_features(lenses["pinhole"], W, H, FIRST, 1, SEED).reshape(NPIX, 12)
    assert np.array_equal(bits(one), bits(F32(0) + dev.path_features(lens_rays(gpu, name, "pinhole", FIRST), FIRST, seed=SEED)))


@pytest.mark.parametrize("name", SCENES)
def test_frame_v_of_a_batch_is_the_single_frame_of_view_v_with_its_seed(gpu, name):
    dev, _, _, lenses = case(gpu, name)
    names, seeds = ["fisheye200", "thin", "equirect"], [SEED, 2 ** 40 + 3, 7]
    got = dev.render_lens_views_path_features([lenses[k] for k in names], W, H, FIRST, S, seeds)
    assert got.shape == (3, H, W, 12)
    for v, (lname, seed) in enumerate(zip(names, seeds)):
        single = dev.render_lens_path_features(lenses[lname], W, H, FIRST, S, seed)
        assert np.array_equal(bits(got[v]), bits(single)), (name, v, lname)
        if seed != SEED:
            assert not np.array_equal(bits(single), bits(dev.render_lens_path_features(lenses[lname], W, H, FIRST, S, SEED)))
    assert dev.render_lens_views_path_features([], W, H, FIRST, S).shape == (0, H, W, 12)
    with pytest.raises(gpu.HrtError, match="n_samples must be positive"):
        dev.render_lens_path_features(lenses["thin"], W, H, 0, 0, SEED)


# ------------------------------------------------------------------------------------------- 4. a mirror seen by hand-made rays
def test_a_mirror_shows_the_walls_it_reflects_and_first_hit_features_show_the_mirror(gpu):
    """A mirror quad in z = 0 (x, y in [-1, 1], facing +z) and a diffuse wall in x = 2 facing -x, made of two quads of different
    albedo that meet at y = 0, under a dark sky.  Rays from x <= -1, z > 0 towards points of the mirror are reflected onto the wall
    (the construction of test_gpu_lit_paths.test_a_planar_mirror_sends_the_tail_to_the_reflected_point)."""
    s = gpu.HostScene()
    s.set_sky(True)
    m, a1, a2 = (0.9, 0.8, 0.7), (0.6, 0.5, 0.4), (0.2, 0.3, 0.9)
    s.add_quad((-1.0, -1.0, 0.0), (1, 0, 0), (0, 1, 0), 2.0, 2.0, gpu.Material.make(albedo=m, type=gpu.MAT_MIRROR))
    s.add_quad((2.0, -3.0, 0.0), (0, 0, 1), (0, 1, 0), 6.0, 3.0, gpu.Material.make(albedo=a1))
    s.add_quad((2.0, 0.0, 0.0), (0, 0, 1), (0, 1, 0), 6.0, 3.0, gpu.Material.make(albedo=a2))
    dev = gpu.DeviceScene(s.flatten())
    rng = np.random.default_rng(4)
    n = 97
    to = np.stack([rng.uniform(0.2, 0.9, n), rng.uniform(-0.5, 0.5, n), np.zeros(n)], axis=1)
    o = np.stack([rng.uniform(-1.5, -1.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 1.0, n)], axis=1)
    rays = qr.make_rays(o, (to - o) / np.linalg.norm(to - o, axis=1, keepdims=True))
    first = bits(dev.trace_rays(rays, "shade"))
    rec = first.view(F32)
    assert (first[:, gpu.HIT_KIND] == gpu.KIND_SQUARE).all() and (first[:, gpu.SHADE_MATERIAL_TYPE] == gpu.MAT_MIRROR).all()
    assert np.array_equal(bits(rec[:, gpu.SHADE_ALBEDO]), bits(np.tile(np.asarray(m, F32), (n, 1)))), "first-hit features: the one albedo m everywhere"
    w1 = (F32(1) * np.asarray(m, F32)) * np.asarray(a1, F32)
    w2 = (F32(1) * np.asarray(m, F32)) * np.asarray(a2, F32)
    for flags in (0, EXACT):
        R = dev.path_features(rays, 5, seed=3, flags=flags)
        is1 = (bits(R[:, pf.ALBEDO]) == bits(w1)).all(axis=1)
        is2 = (bits(R[:, pf.ALBEDO]) == bits(w2)).all(axis=1)
        assert (is1 ^ is2).all() and is1.sum() >= 10 and is2.sum() >= 10, (flags, int(is1.sum()), int(is2.sum()))
        assert np.array_equal(bits(R[:, pf.NORMAL]), bits(np.tile(np.array([-1, 0, 0], F32), (n, 1)))), "the wall's normal, not the mirror's"
        assert (R[:, pf.COVERAGE] == 1).all() and not bits(R[:, pf.EMISSION]).any() and not bits(R[:, 11]).any()
        assert (R[:, pf.DEPTH] > rec[:, gpu.HIT_T]).all(), "the depth is the length of the chain, not the distance to the mirror"
        # which wall: the reflection of d is (dx, dy, -dz), and it meets x = 2 at y = my + (2 - mx) dy / dx
        d64, o64 = rays[:, 4:7].astype(np.float64), rays[:, 0:3].astype(np.float64)
        hit = o64 + (-o64[:, 2] / d64[:, 2])[:, None] * d64
        y = hit[:, 1] + (2.0 - hit[:, 0]) * d64[:, 1] / d64[:, 0]
        clear = np.abs(y) > 1e-3
        assert np.array_equal(is2[clear], y[clear] > 0), "the albedo is that of the wall the reflection meets"


# --------------------------------------------------------------------------------------- 5. depth and emission along the chains
@pytest.mark.parametrize("name", ["skybox", "cornell_mesh"])
def test_depth_and_emission_along_chains_follow_the_oracles_paths(gpu, name):
    """The oracle's path of (ray, key, sample) as closest-hit queries (OracleScene.trace_ray_path), every segment shaded by
    trace_rays("shade") -- emission, albedo, t, type, normal -- and the NumPy rule over them.  The oracle's scattered rays are not
    promised to carry the device's bits, so the bound is the project's parity bar: radiance_oracle.worst <= 1e-6
    (tests/test_gpu_parity.assert_pixels_agree).  cornell_mesh is held to radiance_oracle.expected's tie rule: a ray on which the
    oracle's two mesh modes give different records is a tie ray, held to the rope walk's record, and there are at most
    radiance_oracle.tie_cap(n) of them.
    Measured on MI355X: skybox 302 chains, none reaches a diffuse hit (its square lies under the spheres and is seen from one side
    only: these are the chains that end in the sky, which E leaves out), worst 0.000e+00, 302 of 302 records equal on bits;
    cornell_mesh 68 chains, all 68 reach a diffuse hit, worst 0.000e+00, 68 of 68 records equal on bits, 0 tie rays (cap 1)."""
    dev, _, desc, _ = case(gpu, name)
    modes = (oracle_lib.MESH_REF_TREE, oracle_lib.MESH_ROPE_TREE) if name == "cornell_mesh" else (oracle_lib.MESH_REF_TREE,)
    oracles = [oracle_lib.OracleScene(desc, mode) for mode in modes]
    got, want = [], [[] for _ in modes]
    for _, rays, s in ray_sets(gpu, name, ("pinhole",), range(4)):
        _, _, specular = first_hits(gpu, bits(dev.trace_rays(rays, "shade")))
        chain = np.flatnonzero(specular)  # paths of two or more segments
        R = dev.path_features(rays, s, seed=SEED)
        got.append(R[chain])
        for k, oracle in enumerate(oracles):
            rows = [oracle.trace_ray_path(rays[i], int(i), s, SEED)[:pf.MAXBOUNCES] for i in chain]
            flat = np.concatenate(rows)
            rec = dev.trace_rays(qr.make_rays(flat[:, 0:3], flat[:, 3:6], flat[:, 6]), "shade")
            ru = bits(rec)
            starts = np.cumsum([0] + [len(r) for r in rows])
            for j in range(len(chain)):
                segs = [None if ru[q, gpu.HIT_KIND] == gpu.KIND_MISS else
                        (int(ru[q, gpu.SHADE_MATERIAL_TYPE]), rec[q, gpu.SHADE_ALBEDO], rec[q, gpu.SHADE_EMISSION], rec[q, gpu.HIT_T], rec[q, gpu.SHADE_NORMAL])
                        for q in range(starts[j], starts[j + 1])]
                assert len(segs) >= 2, "a specular first hit is followed"
                want[k].append(pf.record(segs))
    got, want = np.concatenate(got), [np.stack(w) for w in want]
    n = len(got)
    tie = (bits(want[0]) != bits(want[-1])).any(axis=1)
    held = np.where(tie[:, None], want[-1], want[0])
    worst = radiance_oracle.worst(got, held)
    exact = int((bits(got) == bits(held)).all(axis=1).sum())
    reached = int((got[:, pf.COVERAGE] == 1).sum())
    print(f"{name}: {n} chains of two or more segments, {reached} reach a diffuse hit; worst {worst:.3e}, {exact} of {n} records equal on bits, "
          f"{int(tie.sum())} tie rays (cap {radiance_oracle.tie_cap(n)})")
    assert n >= 20 and (reached >= 5 or name == "skybox")
    assert tie.sum() <= radiance_oracle.tie_cap(n)
    assert (got[:, pf.DEPTH][got[:, pf.COVERAGE] == 1] > 0).all()
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------------------- 6. the guided renders
def dev_denoise(gpu, c, f, flags, p):
    """hrt_denoise on NumPy arrays -> the frame as a NumPy array."""
    import torch
    c, f = (torch.from_numpy(np.ascontiguousarray(a, F32)).cuda() for a in (c, f))
    h, w = c.shape[0], c.shape[1]
    scratch = torch.empty(gpu.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    gpu.denoise(c.data_ptr(), f.data_ptr(), w, h, p, flags, scratch.data_ptr(), out.data_ptr(), st.cuda_stream)
    st.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["cornell_box", "random_spheres"])
def test_the_guided_renders_are_the_filters_on_path_features(gpu, name):
    w, h, spp, fspp, seed = 57, 31, 4, 2, 5
    _, _, dev, cam = qr.build(gpu, name, w, h)
    p, pv = gpu.DenoiseParams(), gpu.DenoiseVarParams()
    img, _ = dev.render(cam, w, h, spp, seed)
    half, _ = dev.render(cam, w, h, spp // 2, seed)
    f_first, f_path = dev.render_features(cam, w, h, 0, fspp, seed), dev.render_path_features(cam, w, h, 0, fspp, seed)
    assert not np.array_equal(bits(f_first), bits(f_path)), "the scene has mirror or glass in view"
    for flags in (0, gpu.FLAG_GAMMA):
        what = (name, flags)
        fixed = dev.render_denoised(cam, w, h, spp, fspp, seed, flags, p, guides="diffuse")
        assert np.array_equal(bits(fixed), bits(dev_denoise(gpu, img, f_path, flags, p))), what
        var, vmap = dev.render_denoised_var(cam, w, h, spp, fspp, seed, flags, pv, variance=True, guides="diffuse")
        parts, vparts = tdv.dev_denoise_var(gpu, img, half, f_path, flags, **tdv.params_dict(pv))
        assert np.array_equal(bits(var), bits(parts)) and np.array_equal(bits(vmap), bits(vparts)), what
        # "first" is the existing call, and the existing call is still the filter on first-hit features
        old = dev.render_denoised(cam, w, h, spp, fspp, seed, flags, p)
        assert np.array_equal(bits(dev.render_denoised(cam, w, h, spp, fspp, seed, flags, p, guides="first")), bits(old)), what
        assert np.array_equal(bits(old), bits(dev_denoise(gpu, img, f_first, flags, p))) and not np.array_equal(bits(old), bits(fixed)), what
        old_var = dev.render_denoised_var(cam, w, h, spp, fspp, seed, flags, pv)
        assert np.array_equal(bits(dev.render_denoised_var(cam, w, h, spp, fspp, seed, flags, pv, guides="first")), bits(old_var)), what
        assert not np.array_equal(bits(old_var), bits(var)), what
    # HRT_GUIDES_FIRST_HIT through the new entry points gives the existing functions' bits
    out = np.empty((h, w, 3), F32)
    dev._check(dev._lib.hrt_render_denoised_guides(dev._h, cam, w, h, spp, fspp, seed, 0, gpu.GUIDES_FIRST_HIT, p, out.ctypes.data, None))
    assert np.array_equal(bits(out), bits(dev.render_denoised(cam, w, h, spp, fspp, seed, 0, p)))
    dev._check(dev._lib.hrt_render_denoised_var_guides(dev._h, cam, w, h, spp, 0, seed, 0, gpu.GUIDES_FIRST_HIT, pv, out.ctypes.data, None, None))
    assert np.array_equal(bits(out), bits(dev.render_denoised_var(cam, w, h, spp, 0, seed, 0, pv)))
    with pytest.raises(gpu.HrtError, match="feature_spp must be at least 1 with HRT_GUIDES_FIRST_DIFFUSE"):
        dev.render_denoised(cam, w, h, spp, 0, seed, guides="diffuse")
    st = gpu.Stats()
    dev.render_denoised(cam, w, h, spp, fspp, seed, 0, p, st, guides="diffuse")
    assert st.kernel_ms > 0 and st.samples == w * h * spp


# ------------------------------------------------------------------------------------------------------------------ 7. the CLI
def cli(tmp_path, args, scene="cornell_box", w=57, h=31, spp=4):
    out = tmp_path / "out.ppm"
    r = subprocess.run([os.path.join(PKG, "raytracer"), "--scene", scene, "--w", str(w), "--h", str(h), "--spp", str(spp), "--seed", "5", "--out", str(out),
                        "--assets", os.path.join(ROOT, "assets")] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return out.read_bytes()


def test_the_cli_writes_the_guided_frames_the_library_computes(gpu, tmp_path):
    w, h, spp, fspp, seed = 57, 31, 4, 2, 5
    _, _, dev, cam = qr.build(gpu, "cornell_box", w, h)
    mine = tmp_path / "mine.ppm"
    for filt, render in (("--denoise", dev.render_denoised), ("--denoise-var", dev.render_denoised_var)):
        plain = cli(tmp_path, [filt, str(fspp)])
        assert cli(tmp_path, [filt, str(fspp), "--denoise-guides", "first"]) == plain, (filt, "first-hit guides are the default")
        guided = cli(tmp_path, [filt, str(fspp), "--denoise-guides", "diffuse"])
        assert guided != plain, filt
        gpu.write_ppm(str(mine), render(cam, w, h, spp, fspp, seed, gpu.FLAG_GAMMA, guides="diffuse"))
        assert guided == mine.read_bytes(), filt
        gpu.write_ppm(str(mine), render(cam, w, h, spp, fspp, seed, gpu.FLAG_GAMMA))
        assert plain == mine.read_bytes(), filt
    # with --lens: the frame, the features and the filter of that lens
    import torch
    lens = gpu.Lens(cam, "fisheye", extent=200.0)
    frame = dev.render_lens(lens, w, h, spp, seed, out=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")).cpu().numpy()
    for guides, features in (("first", dev.render_lens_features), ("diffuse", dev.render_lens_path_features)):
        got = cli(tmp_path, ["--lens", "fisheye", "--lens-extent", "200", "--denoise", str(fspp), "--denoise-guides", guides])
        gpu.write_ppm(str(mine), dev_denoise(gpu, frame, features(lens, w, h, 0, fspp, seed), gpu.FLAG_GAMMA, gpu.DenoiseParams()))
        assert got == mine.read_bytes(), guides


# -------------------------------------------------------------------------------------------------------------- 8. resources
def test_path_feature_calls_give_back_what_they_took(gpu):
    import torch
    torch.cuda.synchronize()
    before = gpu.live_resources()
    _, _, dev, cam = qr.build(gpu, "cornell_box", W, H)
    lenses = [gpu.Lens(cam), gpu.Lens(cam, "equirect")]
    rays = gpu.lens_rays(lenses[0], W, H, 0, SEED)
    dev.path_features(rays, 0, seed=SEED)
    dev.render_path_features(cam, W, H, 0, 2, SEED)
    dev.render_lens_path_features(lenses[1], W, H, 0, 2, SEED)
    dev.render_lens_views_path_features(lenses, W, H, 0, 2)
    dev.render_denoised(cam, W, H, 2, 1, SEED, guides="diffuse")
    dev.render_denoised_var(cam, W, H, 2, 1, SEED, guides="diffuse")
    torch.cuda.synchronize()
    held = gpu.live_resources()
    for _ in range(3):
        assert dev.path_features(rays, 0, seed=SEED).any() and dev.path_features(rays.cpu().numpy(), 1, seed=SEED).any()
        dev.render_path_features(cam, W, H, 0, 2, SEED)
        dev.render_lens_path_features(lenses[1], W, H, 0, 2, SEED)
        dev.render_lens_views_path_features(lenses, W, H, 0, 2)
        dev.render_denoised(cam, W, H, 2, 1, SEED, guides="diffuse")
        dev.render_denoised_var(cam, W, H, 2, 1, SEED, guides="diffuse")
        torch.cuda.synchronize()
        assert gpu.live_resources() == held, "repeated calls take nothing more"
    dev.close()
    assert gpu.live_resources() == before
