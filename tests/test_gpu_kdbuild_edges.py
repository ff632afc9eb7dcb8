"""hrt_kd_build_gpu (csrc/hrt_kdbuild.hip) at the places where a level-by-level device build can part from the host's recursion:
candidate counts around one workgroup's 256 and references around the 256-wide LDS tiles, ties across workgroups, lists and
axes, signed zeros, cells without extent, areas that underflow or overflow, depth limits, levels of thousands of open nodes.
Every mesh is synthetic and seeded (tests/kd_meshes.py).  Two routes:
  * hrt_kd_build_gpu called directly on hrt_kd_build_input arrays made here, its nodes compared by a walk from the root with
    tests/kd_ref.py's (inputs the mesh layer never gives: exact signed zeros, bounds on the cell faces, references spanning the
    whole cell, cube cells);
  * through the host layer: the device-built flattened arrays must equal the host builder's (and, for small meshes, the numpy
    statement's), and a frame rendered from either tree is the same bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest

import kd_meshes as km
import kd_ref
from test_kd_ref import mesh_trees, same_trees, trees

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def dev_fn(gpu):
    return C.cast(gpu.device_lib().hrt_kd_build_gpu, C.c_void_p).value


def check_direct(dev_fn, ids, lo, hi, cl, ch, leaf_max, max_depth, ct=1.0, ci=1.5, eb=0.8, reps=1):
    """Device nodes == kd_ref nodes (walked from the roots); on a difference, the cost table of the first node that differs."""
    want_nodes, want_tris, want_depth = kd_ref.build(ids, lo, hi, cl, ch, leaf_max, max_depth, ct, ci, eb)
    for _ in range(reps):
        rc, nodes, tris, root, depth = kd_ref.call_builder(dev_fn, ids, lo, hi, cl, ch, leaf_max, max_depth, ct, ci, eb)
        assert rc == 0
        d = kd_ref.first_difference((want_nodes, want_tris, 0), (nodes, tris, root))
        assert d is None, f"{d[1]}\n{kd_ref.explain(d[0], ids, lo, hi, cl, ch, ct, ci, eb)}"
        assert depth == want_depth and len(nodes) == len(want_nodes)
    return want_nodes


def direct_soup(pos, tri):
    lo, hi, cl, ch = kd_ref.soup_refs(pos, tri)
    return np.arange(len(lo), dtype=np.uint32), lo, hi, cl, ch


# ---- hrt_kd_build_gpu called directly


@pytest.mark.parametrize("n", [127, 128, 129, 255, 256, 257, 512, 513])
def test_counts_around_a_workgroup_and_an_lds_tile(dev_fn, n):
    """2n candidates per (node, axis) around 256 and 512 (one and two workgroups, the lists split inside or at the edge of
    one), n references around the 256-wide LDS tiles (a last tile of 1 or 255).  leaf_max = n - 1 searches only the root,
    leaf_max = 1 the whole tree."""
    ids, lo, hi, cl, ch = direct_soup(*km.soup(n, 100 + n))
    check_direct(dev_fn, ids, lo, hi, cl, ch, n - 1, 30)
    nodes = check_direct(dev_fn, ids, lo, hi, cl, ch, 1, 30)
    assert nodes[0]["axis"] >= 0
    # the same references with shuffled ids and order, a few bounds moved onto the cell faces and two references spanning
    # the whole cell (never a candidate inside it; always on both sides)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    lo2, hi2 = lo[perm].copy(), hi[perm].copy()
    lo2[:5] = cl
    hi2[5:10] = ch
    lo2[10:12], hi2[10:12] = cl, ch
    check_direct(dev_fn, (ids[perm] * 7 + 3).astype(np.uint32), lo2, hi2, cl, ch, 1, 30)


TIE_CONSTANTS = [(1.0, 1.5, 0.8), (1.0, 1.5, 0.0), (1.0, 1.5, 1.0), (-1.0, 1e-12, 0.8), (0.0, 1.0, 0.5)]


@pytest.mark.parametrize("consts", TIE_CONSTANTS, ids=["default", "eb0", "eb1", "all_tie", "ct0"])
def test_ties_on_a_lattice_across_workgroups(dev_fn, consts):
    """Identical triangles on an integer lattice in a cell of integer faces: equal costs at many positions of both lists, in
    different workgroups (384 references: 768 candidates per axis, three workgroups)."""
    pos, tri = km.lattice(8, 8, 6)
    lo, hi, _, _ = kd_ref.soup_refs(pos, tri)
    cl, ch = np.full(3, -5, f32), np.full(3, 5, f32)
    ids = np.arange(len(lo), dtype=np.uint32)
    for leaf_max, max_depth in ((1, 12), (64, 40), (200, 3)):
        check_direct(dev_fn, ids, lo, hi, cl, ch, leaf_max, max_depth, *consts)


@pytest.mark.parametrize("consts", TIE_CONSTANTS, ids=["default", "eb0", "eb1", "all_tie", "ct0"])
def test_ties_across_axes_and_lists(dev_fn, consts):
    """A cube-symmetric set in a cube cell prices x, y and z the same (dyadic coordinates: exact), so axis 0 must win; its
    mirror symmetry prices a lower bound at p and an upper bound at -p the same, so the lower-bound list must win.  The slabs of
    shared_planes end exactly where the next ones start."""
    ids, lo, hi, _, _ = direct_soup(*km.cube_symmetric(12, 5))
    cl, ch = np.full(3, -5, f32), np.full(3, 5, f32)
    nodes = check_direct(dev_fn, ids, lo, hi, cl, ch, 1, 10, *consts)
    root = kd_ref.refs_at("", ids, lo, hi, cl, ch, *consts)
    per_axis = [kd_ref.best_on_axis(cl, ch, root[3], root[4], a, f32(consts[0]), f32(consts[1]), f32(consts[2]), f32(consts[1]) * f32(len(ids)))
                for a in range(3)]
    if per_axis[0][2]:
        assert per_axis[0][0] == per_axis[1][0] == per_axis[2][0] and nodes[0]["axis"] == 0  # the tie is real; x wins it
    ids, lo, hi, _, _ = direct_soup(*km.shared_planes(5, 6))
    check_direct(dev_fn, ids, lo, hi, np.array([-6, -2, -2], f32), np.array([6, 2, 2], f32), 1, 12, *consts)


def test_signed_zero_inputs_build_one_tree(dev_fn):
    """Bounds of exactly -0.0 and +0.0 on the planes that win, in orders that put either sign first: three device builds of each
    order equal each other and the statement's (+0.0 everywhere)."""
    for neg in (True, False):
        ids, lo, hi, _, _ = direct_soup(*km.signed_zero(300, 3, neg))
        assert (lo.view(np.uint32) == 0x80000000).any() or (hi.view(np.uint32) == 0x80000000).any()
        cl, ch = np.full(3, -1.5, f32), np.full(3, 1.5, f32)
        for order in (np.arange(len(ids)), np.arange(len(ids))[::-1]):
            nodes = check_direct(dev_fn, ids[order], lo[order], hi[order], cl, ch, 2, 20, reps=3)
            zero = nodes[(nodes["axis"] >= 0) & (nodes["split"] == 0)]["split"]
            assert len(zero) > 0 and (zero.view(np.uint32) == 0).all()


@pytest.mark.parametrize("case", ["planar_cell", "tiny_1e-19", "huge_1e18", "huge_1e19", "far_1e6", "flat_cell_eb0"])
def test_extents_and_scales(dev_fn, case):
    """A cell without extent on z; areas below the 1e-30 clamp and in denormals; areas and costs of inf and NaN; bounds 1e6 from
    the origin that round to the same fp32 values."""
    eb = 0.8
    if case in ("planar_cell", "flat_cell_eb0"):
        ids, lo, hi, cl, ch = direct_soup(*km.planar(300, 1))
        cl[2] = ch[2] = 0.0
        eb = 0.0 if case == "flat_cell_eb0" else eb
    elif case == "tiny_1e-19":
        ids, lo, hi, _, _ = direct_soup(*km.soup(300, 2, scale=1e-19))
        cl, ch = (lo.min(axis=0) - f32(1e-22)).astype(f32), (hi.max(axis=0) + f32(1e-22)).astype(f32)  # (the host layer pads by 1e-4)
        a = kd_ref.area(cl, ch)
        assert a < 1e-30  # the clamp is in play, the children's areas in denormals
    elif case.startswith("huge"):
        ids, lo, hi, cl, ch = direct_soup(*km.soup(300, 3, scale=float(case.split("_")[1])))
    else:
        ids, lo, hi, cl, ch = direct_soup(*km.soup(400, 4, size=0.02, offset=1e6))
        assert len(np.unique(lo[:, 0])) < len(lo)
    for leaf_max in (1, 4):
        check_direct(dev_fn, ids, lo, hi, cl, ch, leaf_max, 25, 1.0, 1.5, eb)
        check_direct(dev_fn, ids, lo, hi, cl, ch, leaf_max, 25, 1.0, 1.5, 0.0)


# ---- through the host layer


def host_and_gpu(gpu, pos, tri, leaf_max=0, max_depth=0, statement=False):
    want = mesh_trees(gpu, pos, tri, None, leaf_max, max_depth)
    got = mesh_trees(gpu, pos, tri, "gpu", leaf_max, max_depth)
    assert same_trees(want, got) is None, same_trees(want, got)
    if statement:
        ref = mesh_trees(gpu, pos, tri, kd_ref.make_builder(), leaf_max, max_depth)
        assert same_trees(want, ref) is None, same_trees(want, ref)
    return want


LAYER_FAMILIES = [("soup_513", lambda: km.soup(513, 1)), ("lattice", lambda: km.lattice(10, 8, 6)), ("cube_symmetric", lambda: km.cube_symmetric(20, 2)),
                  ("shared_planes", lambda: km.shared_planes(8, 3)), ("planar", lambda: km.planar(600, 4)),
                  ("tiny_1e-19", lambda: km.soup(500, 5, scale=1e-19)), ("huge_1e18", lambda: km.soup(500, 6, scale=1e18)),
                  ("huge_1e19", lambda: km.soup(500, 7, scale=1e19)), ("far_1e6", lambda: km.soup(800, 8, size=0.02, offset=1e6)),
                  ("long_thin", lambda: km.long_thin(2000, 150, 9))]


@pytest.mark.parametrize("eb", [None, "0", "1"])
@pytest.mark.parametrize("family", LAYER_FAMILIES, ids=[f[0] for f in LAYER_FAMILIES])
def test_families_through_the_host_layer(gpu, monkeypatch, family, eb):
    if eb is not None:
        monkeypatch.setenv("HRT_KD_EB", eb)
    pos, tri = family[1]()
    for leaf_max in (1, 4):
        host_and_gpu(gpu, pos, tri, leaf_max, 0, statement=len(tri) <= 1000)


@pytest.mark.parametrize("env", [{"HRT_KD_CT": "-1", "HRT_KD_CI": "1e-12"}, {"HRT_KD_CI": "0.01"}, {"HRT_KD_CT": "0", "HRT_KD_EB": "0"}],
                         ids=["all_tie", "ci_small", "ct0_eb0"])
def test_cost_constants_that_make_ties(gpu, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for pos, tri in (km.lattice(8, 6, 4), km.cube_symmetric(10, 3), km.soup(300, 4)):
        host_and_gpu(gpu, pos, tri, 1, 10, statement=True)


def test_signed_zero_through_the_host_layer(gpu):
    """The same triangles with either sign of zero first: three device builds each, all equal to the host's tree."""
    base = None
    for neg in (True, False):
        pos, tri = km.signed_zero(600, 11, neg)
        want = mesh_trees(gpu, pos, tri, None, 2, 0)
        for _ in range(3):
            got = mesh_trees(gpu, pos, tri, "gpu", 2, 0)
            assert same_trees(want, got) is None, same_trees(want, got)
        base = base or want
        assert same_trees(base, want) is None


def test_depth_and_leaf_limits_with_growing_levels(gpu):
    """Long thin triangles across the mesh: every split copies them to both sides, so a level's references grow, then shrink."""
    pos, tri = km.long_thin(3000, 300, 21)
    for leaf_max in (1, 2, 4, 64):
        for max_depth in (1, 2, 3, 40, 0):
            host_and_gpu(gpu, pos, tri, leaf_max, max_depth)


def test_a_soup_with_levels_of_thousands_of_nodes(gpu, dev_fn):
    """150 000 triangles (about five times the flamingo's): levels of more than 1024 open nodes.  Build times are printed."""
    pos, tri = km.soup(150000, 31, size=0.004)
    ids, lo, hi, cl, ch = direct_soup(pos, tri)
    t0 = time.perf_counter()
    rc, nodes, _, root, _ = kd_ref.call_builder(dev_fn, ids, lo, hi, cl, ch, 4, 30)
    t_direct = time.perf_counter() - t0
    assert rc == 0
    width, level = [], [root]
    while level:
        width.append(len(level))
        nxt = nodes[level]
        inner = nxt[nxt["axis"] >= 0]
        level = np.concatenate([inner["left"], inner["right"]]).tolist()
    assert max(width) > 1024, width
    t0 = time.perf_counter()
    want = mesh_trees(gpu, pos, tri, None)
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = mesh_trees(gpu, pos, tri, "gpu")
    t_gpu = time.perf_counter() - t0
    assert same_trees(want, got) is None, same_trees(want, got)
    print(f"150k soup: widest level {max(width)} nodes, {len(width)} levels; hrt_kd_build_gpu {t_direct * 1e3:.0f} ms; "
          f"flatten with the host builder {t_host * 1e3:.0f} ms, with the GPU builder {t_gpu * 1e3:.0f} ms")


@pytest.mark.parametrize("seed", range(40))
def test_random_soups(gpu, monkeypatch, seed):
    """The KD part of tools/fuzz_plumbing.py, seeded: random soups, leaf_max, max_depth and cost constants."""
    pos, tri, leaf_max, max_depth, env = km.random_case(seed)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    host_and_gpu(gpu, pos, tri, leaf_max, max_depth, statement=seed % 4 == 0)


@pytest.mark.parametrize("family", ["lattice", "signed_zero", "long_thin", "far_1e6"])
def test_renders_from_either_tree_are_identical(gpu, family):
    pos, tri = {"lattice": lambda: km.lattice(6, 6, 4), "signed_zero": lambda: km.signed_zero(400, 5, True),
                "long_thin": lambda: km.long_thin(1500, 100, 6), "far_1e6": lambda: km.soup(500, 7, size=0.02, offset=1e6)}[family]()
    if family == "far_1e6":
        pos = (pos - f32(1e6)).astype(f32) * f32(0.5)  # (rounded to the grid 1e6 imposes, then brought into view)
    else:
        pos = (pos * f32(0.5 / max(1.0, float(np.abs(pos).max())))).astype(f32)
    frames = []
    for builder in (None, "gpu"):
        s = gpu.HostScene().setup("cornell_box", 1.0, 1)
        s.set_kd_params(leaf_max=2)
        s.set_kd_builder(builder)
        s.add_mesh(pos, tri, gpu.Material.make())
        desc = s.flatten()
        frames.append((trees(desc), gpu.DeviceScene(desc).render(gpu.default_camera(1.0), 64, 64, 2, seed=3)[0]))
    assert same_trees(frames[0][0], frames[1][0]) is None
    assert np.array_equal(frames[0][1], frames[1][1])
