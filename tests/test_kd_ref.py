"""tests/kd_ref.py, the numpy statement of the KD build rule, pinned without a GPU before the GPU tests use it as their reference:
a hand-worked cost table, the host builder's flattened arrays with the statement plugged in as the builder (every mesh family of
tests/kd_meshes.py at small sizes, several cost constants), and tests/golden/kd_trees.json, the host builder's trees of every mesh
of the configurations and demo scenes.  A change to the host's rule has to show up as a deliberate update of that file:
    python tests/test_kd_ref.py --write"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kd_meshes as km  # noqa: E402
import kd_ref  # noqa: E402

f32 = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kd_trees.json")
SCENES = ["cornell_box", "cornell_mesh", "random_spheres", "mesh_in_box", "backrooms_pool", "single_sphere", "single_square", "mesh",
          "rt_in_a_weekend", "debug_refraction", "flamingo", "raccoon", "flamingo_pond"]


def trees(desc):
    """(units (n, 4), leaf ids, root, root lo, root hi) of every mesh of a flattened scene."""
    from test_host_layer import MeshDesc, SceneDesc
    d = C.cast(desc, C.POINTER(SceneDesc)).contents
    out = []
    for m in range(d.n_meshes):
        mesh = C.cast(d.meshes, C.POINTER(MeshDesc))[m]
        units = np.ctypeslib.as_array(C.cast(mesh.kd_units, C.POINTER(C.c_uint32)), shape=(mesh.n_kd_units, 4)).copy() if mesh.n_kd_units else np.zeros((0, 4), np.uint32)
        leaf = np.ctypeslib.as_array(C.cast(mesh.leaf_tris, C.POINTER(C.c_uint32)), shape=(mesh.n_leaf_tris,)).copy() if mesh.n_leaf_tris else np.zeros(0, np.uint32)
        out.append((units, leaf, int(mesh.kd_root), tuple(np.float32(mesh.kd_min[:]).view(np.uint32).tolist()),
                    tuple(np.float32(mesh.kd_max[:]).view(np.uint32).tolist())))
    return out


def same_trees(a, b):
    """None, or what differs first between two lists of trees()."""
    if len(a) != len(b):
        return f"{len(a)} meshes != {len(b)}"
    for m, (x, y) in enumerate(zip(a, b)):
        if x[2:] != y[2:]:
            return f"mesh {m}: root / root cell differ"
        if x[0].shape != y[0].shape or not np.array_equal(x[0], y[0]):
            n = int((x[0] != y[0]).any(axis=1).sum()) if x[0].shape == y[0].shape else -1
            return f"mesh {m}: units differ ({len(x[0])} vs {len(y[0])} units, {n} differ)"
        if not np.array_equal(x[1], y[1]):
            return f"mesh {m}: leaf triangle lists differ"
    return None


def digest(tree):
    units, leaf, root, lo, hi = tree
    return {"units": len(units), "units_sha256": hashlib.sha256(units.astype("<u4").tobytes()).hexdigest(),
            "leaf_tris": len(leaf), "leaf_tris_sha256": hashlib.sha256(leaf.astype("<u4").tobytes()).hexdigest(), "root": root,
            "root_lo_bits": list(lo), "root_hi_bits": list(hi)}


def scene_digests(hrt):
    return {name: [digest(t) for t in trees(hrt.HostScene().setup(name, 16 / 9, 1).flatten())] for name in SCENES}


def mesh_trees(hrt, pos, tri, builder, leaf_max=0, max_depth=0):
    s = hrt.HostScene()
    s.set_kd_params(leaf_max=leaf_max, max_depth=max_depth)
    s.set_kd_builder(builder)
    s.add_mesh(pos, tri, hrt.Material.make())
    return trees(s.flatten())


# ---- one node by hand


def test_cost_table_of_one_node_by_hand():
    """Cell [0,5] x [0,1] x [0,1], ct 1, ci 1.5, eb 0.8.  A spans x [0,1], B x [2,5]; both fill y and z.  Cell area 2(5+1+5) = 22.
    Inside the cell on x: the lower bound 2 and the upper bound 1 (0 and 5 are on its faces); y and z have none.
      p = 2 (list 0): nl = 1, nr = 1, L = [0,2] area 2(2+1+2) = 10, R = [2,5] area 2(3+1+3) = 14: 1 + 1.5/22 * 24
      p = 1 (list 1): nl = 1, nr = 1, L = [0,1] area 6,              R = [1,5] area 2(4+1+4) = 18: 1 + 1.5/22 * 24
    The same cost, bit for bit, below the leaf cost 1.5 * 2 = 3: the lower-bound list is visited first, so x = 2 wins although
    the other plane lies lower."""
    lo = np.array([[0, 0, 0], [2, 0, 0]], f32)
    hi = np.array([[1, 1, 1], [5, 1, 1]], f32)
    cl, ch = np.zeros(3, f32), np.array([5, 1, 1], f32)
    lists, pos, nl, nr, cost = kd_ref.axis_table(cl, ch, lo, hi, 0, 1.0, 1.5, 0.8)
    want = f32(1) + (f32(1.5) * (f32(1) / f32(22))) * f32(24)
    assert lists.tolist() == [0, 1] and pos.tolist() == [2.0, 1.0] and nl.tolist() == [1, 1] and nr.tolist() == [1, 1]
    assert cost.view(np.uint32).tolist() == [want.view(np.uint32)] * 2 and abs(float(want) - (1 + 1.5 / 22 * 24)) < 1e-6
    for a in (1, 2):
        assert len(kd_ref.axis_table(cl, ch, lo, hi, a, 1.0, 1.5, 0.8)[1]) == 0
    assert kd_ref.best_split(cl, ch, lo, hi, f32(1), f32(1.5), f32(0.8)) == (0, f32(2))
    nodes, tris, depth = kd_ref.build([7, 9], lo, hi, cl, ch, 1, 10)
    assert nodes["axis"].tolist() == [0, -1, -1] and nodes["split"][0] == 2 and tris.tolist() == [7, 9] and depth == 1
    # A third triangle C at x [3, 4] makes x = 2 empty on neither side and moves the best plane: the upper bound 4 now has
    # nl = 3 (0, 2 and 3 are below it), nr = 1 (B ends at 5) -- and with eb = 0 every plane with an empty side costs 0.
    lo3 = np.vstack([lo, [3, 0, 0]]).astype(f32)
    hi3 = np.vstack([hi, [4, 1, 1]]).astype(f32)
    lists, pos, nl, nr, cost = kd_ref.axis_table(cl, ch, lo3, hi3, 0, 1.0, 1.5, 0.0)
    assert pos.tolist() == [2, 3, 1, 4] and nl.tolist() == [1, 2, 1, 3] and nr.tolist() == [2, 2, 2, 1]
    assert (cost > 0).all()  # no plane has an empty side here
    assert "winner" in kd_ref.node_table(cl, ch, lo3, hi3, f32(1), f32(1.5), f32(0.0))


def test_a_nan_cost_never_wins_and_a_tie_with_the_leaf_loses():
    """Areas of inf make 0 * inf = NaN in the cost of an empty side (eb 0); the leaf cost is the bar, not a tie."""
    lo = np.array([[-3e38, 0, 0], [1e38, 0, 0]], f32)
    hi = np.array([[-1e38, 1, 1], [3e38, 1, 1]], f32)
    cl, ch = np.array([-3.2e38, 0, 0], f32), np.array([3.2e38, 1, 1], f32)
    _, _, _, _, cost = kd_ref.axis_table(cl, ch, lo, hi, 0, 1.0, 1.5, 0.0)
    assert np.isnan(cost).any()
    assert kd_ref.best_split(cl, ch, lo, hi, f32(1), f32(1.5), f32(0.0)) in (None, (0, f32(-1e38)), (0, f32(1e38)))
    # ct = ci * n exactly: a plane priced at the leaf cost does not split
    lo = np.array([[0, 0, 0], [2, 0, 0]], f32)
    hi = np.array([[1, 1, 1], [3, 1, 1]], f32)
    assert kd_ref.best_split(np.zeros(3, f32), np.array([3, 1, 1], f32), lo, hi, f32(3), f32(1.5), f32(1.0)) is None


def test_signed_zero_bounds_are_positive_zero():
    """-0.0 and +0.0 are one candidate, stored as +0.0 whichever reference carries which."""
    lo = np.array([[-1, -1, -1], [-0.0, -1, -1], [0.0, -1, -1], [0.5, -1, -1]], f32)
    hi = np.array([[-0.0, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]], f32)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        nodes, _, _ = kd_ref.build(np.arange(4)[order], lo[order], hi[order], [-1, -1, -1], [1, 1, 1], 1, 3)
        assert (nodes["axis"] >= 0).any()
        zero = nodes["split"][(nodes["axis"] >= 0) & (nodes["split"] == 0)]
        assert len(zero) and (zero.view(np.uint32) == 0).all()
        assert (np.concatenate([nodes["lo"].ravel(), nodes["hi"].ravel()]).view(np.uint32) != 0x80000000).all()


def test_the_tree_walk_reports_the_first_node_that_differs():
    pos, tri = km.soup(60, 3)
    lo, hi, cl, ch = kd_ref.soup_refs(pos, tri)
    ids = np.arange(len(lo))
    a = kd_ref.build(ids, lo, hi, cl, ch, 2, 20)
    assert kd_ref.first_difference((a[0], a[1], 0), (a[0], a[1], 0)) is None
    b = a[0].copy()
    inner = np.nonzero(b["axis"] >= 0)[0]
    k = int(inner[-1])
    b["split"][k] = np.nextafter(b["split"][k], f32(np.inf))
    path, why = kd_ref.first_difference((a[0], a[1], 0), (b, a[1], 0))
    assert "split" in why
    # the path leads to node k
    n = 0
    for step in path:
        n = int(a[0]["right" if step == "R" else "left"][n])
    assert n == k
    assert "winner" in kd_ref.explain(path, ids, lo, hi, cl, ch)


# ---- the statement equals the host builder


def _families():
    yield "soup_300", km.soup(300, 1), (0, 0)
    yield "soup_129_root_only", km.soup(129, 2), (128, 0)
    yield "soup_257_leaf1", km.soup(257, 3), (1, 0)
    yield "clustered_2000", km.clustered(2000, 4), (0, 0)
    yield "lattice_8x4x3", km.lattice(8, 4, 3), (1, 0)
    yield "cube_symmetric", km.cube_symmetric(10, 5), (1, 0)
    yield "shared_planes", km.shared_planes(4, 6), (1, 0)
    yield "signed_zero_neg_first", km.signed_zero(90, 7, True), (2, 0)
    yield "signed_zero_pos_first", km.signed_zero(90, 7, False), (2, 0)
    yield "planar", km.planar(200, 8), (2, 0)
    yield "tiny_1e-19", km.soup(200, 9, scale=1e-19), (2, 0)
    yield "huge_1e19", km.soup(200, 10, scale=1e19), (2, 0)
    yield "far_1e6", km.soup(300, 11, size=0.02, offset=1e6), (2, 0)
    yield "long_thin", km.long_thin(400, 60, 12), (1, 0)
    yield "depth_1", km.soup(200, 13), (1, 1)
    yield "depth_3", km.soup(200, 14), (1, 3)


FAMILIES = list(_families())


@pytest.mark.parametrize("eb", [None, "0", "1"])
@pytest.mark.parametrize("case", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_the_statement_builds_the_host_builders_tree(hrt, monkeypatch, case, eb):
    _, (pos, tri), (leaf_max, max_depth) = case
    if eb is not None:
        monkeypatch.setenv("HRT_KD_EB", eb)
    want = mesh_trees(hrt, pos, tri, None, leaf_max, max_depth)
    got = mesh_trees(hrt, pos, tri, kd_ref.make_builder(), leaf_max, max_depth)
    assert same_trees(want, got) is None, same_trees(want, got)


@pytest.mark.parametrize("env", [{"HRT_KD_CT": "-1", "HRT_KD_CI": "1e-12"}, {"HRT_KD_CI": "0.01"}, {"HRT_KD_CT": "0", "HRT_KD_EB": "0.5"},
                                 {"HRT_KD_CT": "2.5", "HRT_KD_CI": "3", "HRT_KD_EB": "1"}], ids=["all_tie", "ci_small", "ct0", "ct_high"])
def test_the_statement_follows_the_cost_constants(hrt, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for pos, tri in (km.lattice(6, 3, 2), km.soup(150, 21)):
        want = mesh_trees(hrt, pos, tri, None, 2, 6)
        got = mesh_trees(hrt, pos, tri, kd_ref.make_builder(), 2, 6)
        assert same_trees(want, got) is None, same_trees(want, got)


@pytest.mark.parametrize("seed", range(8))
def test_the_statement_on_random_soups(hrt, monkeypatch, seed):
    pos, tri, leaf_max, max_depth, env = km.random_case(seed)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = mesh_trees(hrt, pos, tri, None, leaf_max, max_depth)
    got = mesh_trees(hrt, pos, tri, kd_ref.make_builder(), leaf_max, max_depth)
    assert same_trees(want, got) is None, (env, leaf_max, max_depth, same_trees(want, got))


def test_the_host_layer_hands_builders_no_negative_zero(hrt):
    """hrt_kd_builder_fn: -0.0 in a mesh reaches a builder as +0.0 (so the same tree comes out whatever the references' order)."""
    seen = []
    inner = kd_ref.make_builder()

    @kd_ref.BUILDER_FN
    def spy(inp, out, user):
        i = inp.contents
        n = i.n_refs
        seen.append(np.concatenate([np.ctypeslib.as_array(i.lo, shape=(3 * n,)), np.ctypeslib.as_array(i.hi, shape=(3 * n,))]).copy())
        return inner(inp, out, user)

    for neg in (True, False):
        pos, tri = km.signed_zero(30, 1, neg)
        assert (pos.view(np.uint32) == 0x80000000).any()
        mesh_trees(hrt, pos, tri, spy, 2, 0)
    assert len(seen) == 2 and all((s == 0).any() and not (s.view(np.uint32) == 0x80000000).any() for s in seen)
    a = mesh_trees(hrt, *km.signed_zero(30, 1, True), None, 2, 0)
    b = mesh_trees(hrt, *km.signed_zero(30, 1, False), None, 2, 0)
    assert same_trees(a, b) is None  # the same triangles with the signs of their zeros swapped: the same tree


# ---- the host builder's trees of the configurations and demo scenes


def test_the_host_builders_trees_match_the_fixture(hrt):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = scene_digests(hrt)
    assert sorted(got) == sorted(want["scenes"])
    for name in SCENES:
        assert got[name] == want["scenes"][name], f"{name}: the host builder's tree changed (update {os.path.basename(FIXTURE)} only on purpose)"


if __name__ == "__main__" and "--write" in sys.argv:
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    h = importlib.import_module("hai719-raytracing_amd")
    with open(FIXTURE, "w") as f:
        json.dump({"about": "host builder (host/kdtree.cpp) trees of every mesh of the scenes at their default KD parameters: "
                            "SHA-256 of the flattened 16-byte units and of the leaf triangle list (little-endian uint32), root ref, "
                            "root cell bits; tests/test_kd_ref.py --write", "scenes": scene_digests(h)}, f, indent=1)
        f.write("\n")
