"""Plain numpy statement of the KD build rule of host/kdtree.cpp (Builder::build / best_split / best_on_axis), shared by the KD
tests.  It takes the fields of include/hrt.h hrt_kd_build_input as arrays and returns hrt_kd_build_node records plus the leaves'
triangle ids; tests/test_kd_ref.py checks it against the host builder and hand-worked costs, the GPU tests against
hrt_kd_build_gpu.

The rule, in fp32 with no contraction and in the host's order of operations:
  * a node of <= leaf_max references, or at depth max_depth, is a leaf;
  * per axis 0, 1, 2: the candidates are the references' lower bounds, ascending and deduplicated, then their upper bounds, the
    same way; only a plane strictly inside the cell counts; with inv_area = 1 / max(area(cell), 1e-30),
        cost = ct + ci * inv_area * (area(L) * nl + area(R) * nr),   then cost *= eb when nl == 0 or nr == 0,
    nl = #(lo < p), nr = #(hi > p), area(box) = 2 * (dx * dy + dy * dz + dz * dx);
  * a plane wins only if its cost is strictly below the best so far, starting from the leaf cost ci * n (a NaN never wins);
    the axes are reduced in order with the same strict `<`;
  * a reference goes left if lo < p or hi <= p (its hi clipped to p), right if hi > p or lo >= p (its lo clipped to p).
Bounds of -0.0 are +0.0 (hrt_kd_builder_fn): the host layer hands a builder no negative zero, so that a plane at zero has one
bit pattern whatever order the references come in."""
import ctypes as C

import numpy as np

f32 = np.float32
NODE = np.dtype([("axis", "<i4"), ("split", "<f4"), ("left", "<i4"), ("right", "<i4"), ("lo", "<f4", 3), ("hi", "<f4", 3),
                 ("first_tri", "<u4"), ("n_tris", "<u4")])  # hrt_kd_build_node, 48 bytes


class In(C.Structure):
    _fields_ = [("n_refs", C.c_uint32), ("ids", C.POINTER(C.c_uint32)), ("lo", C.POINTER(C.c_float)), ("hi", C.POINTER(C.c_float)),
                ("cell_lo", C.c_float * 3), ("cell_hi", C.c_float * 3), ("leaf_max", C.c_uint32), ("max_depth", C.c_uint32),
                ("cost_traverse", C.c_float), ("cost_intersect", C.c_float), ("empty_bonus", C.c_float)]


class Out(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_uint32), ("tris", C.c_void_p), ("n_tris", C.c_uint32), ("root", C.c_int32),
                ("depth", C.c_uint32)]


BUILDER_FN = C.CFUNCTYPE(C.c_int, C.POINTER(In), C.POINTER(Out), C.c_void_p)
assert NODE.itemsize == 48


def _libc():
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.restype = None
    libc.free.argtypes = [C.c_void_p]
    return libc


def area(lo, hi):
    """Box::area on (..., 3) arrays, fp32, left to right."""
    dx, dy, dz = (f32(hi[..., k]) - f32(lo[..., k]) for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(2) * ((dx * dy + dy * dz) + dz * dx)


def positive_zero(a):
    """-0.0 -> +0.0 (every other value, NaN included, unchanged)."""
    a = np.array(a, dtype=f32)
    a[a == 0] = f32(0)
    return a


def axis_table(cell_lo, cell_hi, lo, hi, a, ct, ci, eb):
    """Every candidate of axis `a` of one node in the host's visiting order: (list, pos, nl, nr, cost) arrays, candidates outside
    the cell dropped.  list 0 = lower bounds, 1 = upper bounds."""
    cell_lo = np.asarray(cell_lo, f32)
    cell_hi = np.asarray(cell_hi, f32)
    n = len(lo)
    mins = np.sort(np.asarray(lo, f32)[:, a])
    maxs = np.sort(np.asarray(hi, f32)[:, a])

    def dedup(v):  # the host's `!= last` over a sorted list (the first of equal values stays)
        keep = np.ones(len(v), bool)
        keep[1:] = v[1:] != v[:-1]
        return v[keep]

    cl, cm = dedup(mins), dedup(maxs)
    lists = np.concatenate([np.zeros(len(cl), np.int64), np.ones(len(cm), np.int64)])
    pos = np.concatenate([cl, cm]).astype(f32)
    inside = (pos > cell_lo[a]) & (pos < cell_hi[a])
    lists, pos = lists[inside], pos[inside]
    nl = np.searchsorted(mins, pos, side="left")
    nr = n - np.searchsorted(maxs, pos, side="right")
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        a_cell = area(cell_lo, cell_hi)
        inv_area = f32(1) / (a_cell if not (a_cell < f32(1e-30)) else f32(1e-30))  # std::max(area, 1e-30f): NaN stays NaN
        Llo = np.broadcast_to(cell_lo, (len(pos), 3)).copy()
        Lhi = np.broadcast_to(cell_hi, (len(pos), 3)).copy()
        Rlo, Rhi = Llo.copy(), Lhi.copy()
        Lhi[:, a] = pos
        Rlo[:, a] = pos
        cost = f32(ct) + (f32(ci) * inv_area) * (area(Llo, Lhi) * nl.astype(f32) + area(Rlo, Rhi) * nr.astype(f32))
        cost = np.where((nl == 0) | (nr == 0), cost * f32(eb), cost).astype(f32)
    return lists, pos, nl, nr, cost


def best_on_axis(cell_lo, cell_hi, lo, hi, a, ct, ci, eb, leaf_cost):
    """(cost, pos, found): the first candidate whose cost is below every earlier one and below leaf_cost."""
    _, pos, _, _, cost = axis_table(cell_lo, cell_hi, lo, hi, a, ct, ci, eb)
    ok = np.where(cost < leaf_cost, cost, np.inf)  # NaN and costs not below the leaf never win
    if not len(ok) or not (ok.min() < np.inf):
        return leaf_cost, f32(0), False
    i = int(np.argmin(ok))  # the first of the minima: the strict `<` loop keeps it
    return cost[i], pos[i], True


def best_split(cell_lo, cell_hi, lo, hi, ct, ci, eb):
    """(axis, pos) of the split, or None for a leaf (not counting leaf_max / max_depth)."""
    leaf_cost = f32(ci) * f32(len(lo))
    best, out = leaf_cost, None
    for a in range(3):
        c, p, found = best_on_axis(cell_lo, cell_hi, lo, hi, a, ct, ci, eb, leaf_cost)
        if found and c < best:
            best, out = c, (a, p)
    return out


def node_table(cell_lo, cell_hi, lo, hi, ct, ci, eb):
    """The cost table of one node as text: every candidate of every axis, the leaf cost and the winner."""
    leaf_cost = f32(ci) * f32(len(lo))
    rows = [f"cell {list(map(float, cell_lo))} .. {list(map(float, cell_hi))}, {len(lo)} refs, leaf cost {leaf_cost!r}"]
    for a in range(3):
        lists, pos, nl, nr, cost = axis_table(cell_lo, cell_hi, lo, hi, a, ct, ci, eb)
        for k in range(len(pos)):
            rows.append(f"  axis {a} list {lists[k]} pos {pos[k]!r} ({pos[k].view(np.uint32):#010x}) nl {nl[k]} nr {nr[k]} cost {cost[k]!r}")
    rows.append(f"  winner: {best_split(cell_lo, cell_hi, lo, hi, ct, ci, eb)}")
    return "\n".join(rows)


def build(ids, lo, hi, cell_lo, cell_hi, leaf_max, max_depth, ct=1.0, ci=1.5, eb=0.8):
    """The host's tree for one hrt_kd_build_input.  ids (n,), lo / hi (n, 3); max_depth as given (the host layer resolves 0).
    Returns (nodes: NODE array, preorder from the root = 0, tris: uint32 array, depth reached)."""
    ids = np.asarray(ids, np.uint32)
    lo = positive_zero(np.asarray(lo, f32).reshape(-1, 3))
    hi = positive_zero(np.asarray(hi, f32).reshape(-1, 3))
    ct, ci, eb = f32(ct), f32(ci), f32(eb)
    nodes, tris = [], []
    depth_reached = [0]

    def rec(cl, ch, ids, lo, hi, depth):
        depth_reached[0] = max(depth_reached[0], depth)
        me = len(nodes)
        rec_ = np.zeros((), NODE)
        rec_["lo"], rec_["hi"] = cl, ch
        rec_["left"] = rec_["right"] = -1
        nodes.append(rec_)
        s = None if (len(ids) <= leaf_max or depth >= max_depth) else best_split(cl, ch, lo, hi, ct, ci, eb)
        if s is None:
            rec_["axis"] = -1
            rec_["first_tri"] = sum(len(t) for t in tris)
            rec_["n_tris"] = len(ids)
            tris.append(np.sort(ids))
            return me
        a, p = s
        rec_["axis"], rec_["split"] = a, p
        to_left = (lo[:, a] < p) | (hi[:, a] <= p)
        to_right = (hi[:, a] > p) | (lo[:, a] >= p)
        lhi = hi[to_left].copy()
        lhi[:, a] = np.where(p < lhi[:, a], p, lhi[:, a])   # std::min(hi, p)
        rlo = lo[to_right].copy()
        rlo[:, a] = np.where(rlo[:, a] < p, p, rlo[:, a])   # std::max(lo, p)
        lch, rcl = ch.copy(), cl.copy()
        lch[a] = p
        rcl[a] = p
        rec_["left"] = rec(cl, lch, ids[to_left], lo[to_left], lhi, depth + 1)
        rec_["right"] = rec(rcl, ch, ids[to_right], rlo, hi[to_right], depth + 1)
        return me

    rec(np.array(cell_lo, f32), np.array(cell_hi, f32), ids, lo, hi, 0)
    out = np.array(nodes, dtype=NODE)
    t = np.concatenate(tris).astype(np.uint32) if tris else np.zeros(0, np.uint32)
    return out, t, depth_reached[0]


def make_builder():
    """A hrt_kd_builder_fn (ctypes callback) that builds with `build`: HostScene.set_kd_builder(make_builder())."""
    libc = _libc()

    @BUILDER_FN
    def fn(inp, out, user):
        try:
            i = inp.contents
            n = i.n_refs
            ids = np.ctypeslib.as_array(i.ids, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            lo = np.ctypeslib.as_array(i.lo, shape=(n, 3)).copy() if n else np.zeros((0, 3), f32)
            hi = np.ctypeslib.as_array(i.hi, shape=(n, 3)).copy() if n else np.zeros((0, 3), f32)
            nodes, tris, depth = build(ids, lo, hi, i.cell_lo[:], i.cell_hi[:], i.leaf_max, i.max_depth, i.cost_traverse,
                                       i.cost_intersect, i.empty_bonus)
            pn = libc.malloc(max(nodes.nbytes, 1))
            pt = libc.malloc(max(tris.nbytes, 1))
            C.memmove(pn, nodes.ctypes.data, nodes.nbytes)
            if len(tris):
                C.memmove(pt, tris.ctypes.data, tris.nbytes)
            o = out.contents
            o.nodes, o.n_nodes, o.tris, o.n_tris, o.root, o.depth = pn, len(nodes), pt, len(tris), 0, depth
            return 0
        except Exception:  # (an exception cannot cross the C boundary: the host layer reports the failure)
            import traceback
            traceback.print_exc()
            return -1

    return fn


def call_builder(fn, ids, lo, hi, cell_lo, cell_hi, leaf_max, max_depth, ct=1.0, ci=1.5, eb=0.8):
    """Call a hrt_kd_builder_fn (e.g. libhrt.so's hrt_kd_build_gpu) on arrays made here; the output is copied and freed with libc
    free.  Returns (rc, nodes: NODE array, tris, root, depth)."""
    ids = np.ascontiguousarray(ids, np.uint32)
    lo = np.ascontiguousarray(lo, f32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, f32).reshape(-1, 3)
    i = In()
    i.n_refs = len(ids)
    i.ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
    i.lo = lo.ctypes.data_as(C.POINTER(C.c_float))
    i.hi = hi.ctypes.data_as(C.POINTER(C.c_float))
    for a in range(3):
        i.cell_lo[a], i.cell_hi[a] = float(f32(cell_lo[a])), float(f32(cell_hi[a]))
    i.leaf_max, i.max_depth = leaf_max, max_depth
    i.cost_traverse, i.cost_intersect, i.empty_bonus = ct, ci, eb
    o = Out()
    f = fn if isinstance(fn, BUILDER_FN) else BUILDER_FN(C.cast(fn, C.c_void_p).value)
    rc = f(C.byref(i), C.byref(o), None)
    libc = _libc()
    nodes = np.zeros(0, NODE)
    tris = np.zeros(0, np.uint32)
    try:
        if rc == 0:
            nodes = np.frombuffer(C.string_at(o.nodes, o.n_nodes * NODE.itemsize), dtype=NODE).copy()
            tris = np.frombuffer(C.string_at(o.tris, o.n_tris * 4), dtype=np.uint32).copy() if o.n_tris else tris
    finally:
        libc.free(o.nodes)
        libc.free(o.tris)
    return rc, nodes, tris, int(o.root), int(o.depth)


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


def first_difference(a, b):
    """Walk two builders' trees from their roots (their numberings differ: the host's is preorder, the device's level by level).
    a, b: (nodes, tris, root).  Returns None when they are the same tree (axes, split bits, cell bits, every leaf's ids), or
    (path, text): the path from the root ('' = the root, then 'L' / 'R') to the first node where they part, and what differs."""
    (na, ta, ra), (nb, tb, rb) = a, b
    stack = [("", ra, rb)]
    while stack:
        path, i, j = stack.pop()
        x, y = na[i], nb[j]
        why = []
        if int(x["axis"]) != int(y["axis"]):
            why.append(f"axis {int(x['axis'])} != {int(y['axis'])}")
        if not np.array_equal(_bits(x["lo"]), _bits(y["lo"])) or not np.array_equal(_bits(x["hi"]), _bits(y["hi"])):
            why.append(f"cell {x['lo']}..{x['hi']} != {y['lo']}..{y['hi']}")
        if int(x["axis"]) >= 0 and int(y["axis"]) >= 0:
            if _bits(x["split"]) != _bits(y["split"]):
                why.append(f"split {float(x['split'])!r} ({int(_bits(x['split'])):#010x}) != {float(y['split'])!r} ({int(_bits(y['split'])):#010x})")
        elif int(x["axis"]) < 0 and int(y["axis"]) < 0:
            la = np.sort(ta[x["first_tri"]:x["first_tri"] + x["n_tris"]])
            lb = np.sort(tb[y["first_tri"]:y["first_tri"] + y["n_tris"]])
            if not np.array_equal(la, lb):
                why.append(f"leaf ids {la[:16]}{'...' if len(la) > 16 else ''} != {lb[:16]}{'...' if len(lb) > 16 else ''}")
        if why:
            return path, "; ".join(why)
        if int(x["axis"]) >= 0:
            stack.append((path + "R", int(x["right"]), int(y["right"])))
            stack.append((path + "L", int(x["left"]), int(y["left"])))
    return None


def refs_at(path, ids, lo, hi, cell_lo, cell_hi, ct=1.0, ci=1.5, eb=0.8):
    """The cell and references (as `build` partitions them) of the node at `path`, for node_table."""
    lo = positive_zero(np.asarray(lo, f32).reshape(-1, 3))
    hi = positive_zero(np.asarray(hi, f32).reshape(-1, 3))
    ids = np.asarray(ids, np.uint32)
    cl, ch = np.array(cell_lo, f32), np.array(cell_hi, f32)
    for step in path:
        s = best_split(cl, ch, lo, hi, f32(ct), f32(ci), f32(eb))
        if s is None:
            break
        a, p = s
        if step == "L":
            m = (lo[:, a] < p) | (hi[:, a] <= p)
            ids, lo, hi = ids[m], lo[m], hi[m].copy()
            hi[:, a] = np.where(p < hi[:, a], p, hi[:, a])
            ch = ch.copy()
            ch[a] = p
        else:
            m = (hi[:, a] > p) | (lo[:, a] >= p)
            ids, lo, hi = ids[m], lo[m].copy(), hi[m]
            lo[:, a] = np.where(lo[:, a] < p, p, lo[:, a])
            cl = cl.copy()
            cl[a] = p
    return cl, ch, ids, lo, hi


def explain(path, ids, lo, hi, cell_lo, cell_hi, ct=1.0, ci=1.5, eb=0.8):
    """The cost table of the node at `path`, as `build` sees it."""
    cl, ch, _, l, h = refs_at(path, ids, lo, hi, cell_lo, cell_hi, ct, ci, eb)
    return f"node at path '{path}':\n" + node_table(cl, ch, l, h, f32(ct), f32(ci), f32(eb))


def soup_refs(positions, indices):
    """Reference bounds of a triangle soup as the host layer makes them (every triangle regular): lo, hi (n, 3) and the padded root
    cell, from positions ALREADY scaled."""
    p = np.asarray(positions, f32)[np.asarray(indices, np.int64)]  # (n, 3 vertices, 3)
    lo = p.min(axis=1)
    hi = p.max(axis=1)
    rl, rh = lo.min(axis=0), hi.max(axis=0)
    pad = f32(1e-4) * np.maximum(f32(1), np.maximum(np.abs(rl), np.abs(rh)))
    return lo, hi, (rl - pad).astype(f32), (rh + pad).astype(f32)
