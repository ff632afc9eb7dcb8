"""The squares' no-division filter (csrc/hrt_kernels.hip quad_filter, quad_filter_axis) lets through every square the exact
test hits.  The filter only chooses which squares go through the exact arithmetic, so it may be as loose as it likes and must
never be tighter: column 7 of the quad kinds of hrt_debug_kat ("the shipped filter lets the square through") has to be 1
wherever column 0 ("quad_t / quad_t_rcp hits") is 1, on every ray, with no case left out.

Squares: one in each axis plane with each normal sign, one carrying the 3e-8 residues a rotation by 90 degrees leaves, glass
(in an axis plane and tilted), one rotated off the axes (the general, four-row form), sides of 1e-3 and of 1e3.  Rays, about
2e5 per square from a fixed seed: uniform directions from origins inside and outside the square's neighbourhood, rays aimed at
the square from either side (back-facing ones on plain and on glass squares among them), hit points within +-8 ulp of each edge
and corner, |d_K| at par (1 +- 2^-20), at 0 and at -0, origins on the plane and at t = 9e-6 (1 +- 2^-20).

A filter that let nothing through would pass the implication on a ray set without hits, so a NumPy restatement of
Square::intersect (fp32, the folded constants of hrt_pack.h fold_quad) counts the exact hits of every ray set on the CPU: at
least a thousand per square."""
import numpy as np
import pytest

F32 = np.float32
C90 = float(F32(np.cos(np.pi / 2)))  # -4.37e-8: what rotate_x / rotate_y by 90 degrees leave where a zero belongs


def _rot90_y(p):
    """A point turned by 90 degrees about y in fp32, as the set-up code turns a wall: residues of a few 1e-8 stay behind."""
    x, y, z = (F32(v) for v in p)
    c, s = F32(C90), F32(1.0)
    return (float(c * x + s * z), float(y), float(-s * x + c * z))


SQUARES = {  # v0, v1, v3, glass
    "z_plus": ((-1, -1, 0.5), (1, -1, 0.5), (-1, 1, 0.5), 0),
    "z_minus": ((-1, -1, 0.5), (-1, 1, 0.5), (1, -1, 0.5), 0),
    "x_plus": ((0.25, -1, -1), (0.25, 1, -1), (0.25, -1, 1), 0),
    "x_minus": ((0.25, -1, -1), (0.25, -1, 1), (0.25, 1, -1), 0),
    "y_plus": ((-1, -0.75, -1), (-1, -0.75, 1), (1, -0.75, -1), 0),
    "y_minus": ((-1, -0.75, -1), (1, -0.75, -1), (-1, -0.75, 1), 0),
    "residues": (_rot90_y((-1, -1, 0.5)), _rot90_y((1, -1, 0.5)), _rot90_y((-1, 1, 0.5)), 0),
    "glass_axis": ((-1, -1, 0.5), (1, -1, 0.5), (-1, 1, 0.5), 1),
    "glass_tilted": ((-1, -0.5, 0.2), (0.7, -0.2, 0.9), (-1.3, 1.1, 0.4), 1),
    "tilted": ((-1, -0.5, 0.2), (0.7, -0.2, 0.9), (-1.3, 1.1, 0.4), 0),
    "side_1e-3": ((0, 0, 0), (1e-3, 0, 0), (0, 1e-3, 0), 0),
    "side_1e3": ((-500, -500, 0), (500, -500, 0), (-500, 500, 0), 0),
}
N_UNIFORM, N_AIMED, N_EDGE, N_PAR, N_NEAR = 40000, 60000, 50000, 30000, 20000
PAR = 8.0 * 4e-7  # hrt_pack.h build_quad_filter for a square exactly in an axis plane; the residues' square has a little more


def _ulps(x, k):
    """float32 x moved by k units in the last place (k an integer array)."""
    x = np.ascontiguousarray(x, F32)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, np.int64(-(1 << 31)) - i, i) + k       # to a monotone integer line and back
    i = np.where(i < 0, np.int64(-(1 << 31)) - i, i)
    return i.astype(np.int32).view(F32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ray_set(name):
    """(n, 7) float32 rays {origin, direction, time} for one square; the device normalises the direction."""
    v0, v1, v3, _ = SQUARES[name]
    v0, v1, v3 = (np.array([float(F32(c)) for c in p]) for p in (v0, v1, v3))
    rng = np.random.default_rng(sum(map(ord, name)))
    R, U = v1 - v0, v3 - v0
    size = max(np.linalg.norm(R), np.linalg.norm(U))
    nrm = _unit(np.cross(R, U))
    Rh, Uh = _unit(R), _unit(U)
    centre = v0 + 0.5 * (R + U)
    at = lambda uv: v0 + uv[:, :1] * R + uv[:, 1:] * U
    parts = []
    # uniform directions, origins inside and outside
    o = centre + rng.uniform(-3, 3, (N_UNIFORM, 3)) * size
    o[: N_UNIFORM // 2] = centre + rng.uniform(-0.6, 0.6, (N_UNIFORM // 2, 3)) * size
    parts.append((o, _unit(rng.normal(size=(N_UNIFORM, 3)))))
    # aimed at the plane of the square from either side: most inside, some past the edges
    tgt = at(rng.uniform(-0.25, 1.25, (N_AIMED, 2)))
    o = tgt + rng.normal(size=(N_AIMED, 3)) * size * rng.choice([0.05, 1.0, 3.0], (N_AIMED, 1))
    parts.append((o, tgt - o))
    # hit points within +-8 ulp of each edge and corner
    uv = rng.uniform(0, 1, (N_EDGE, 2))
    side = rng.integers(0, 4, N_EDGE)
    uv[side == 0, 0] = 0; uv[side == 1, 0] = 1; uv[side == 2, 1] = 0; uv[side == 3, 1] = 1
    uv[: N_EDGE // 5] = rng.integers(0, 2, (N_EDGE // 5, 2))  # the corners
    tgt = _ulps(at(uv).astype(F32), rng.integers(-8, 9, (N_EDGE, 3))).astype(np.float64)
    away = rng.normal(size=(N_EDGE, 3))
    away[:, :] = np.where((away @ nrm)[:, None] < 0, -away, away)  # front side, so that the exact test accepts them
    away[N_EDGE // 2:] *= rng.choice([-1.0, 1.0], (N_EDGE - N_EDGE // 2, 1))
    o = (tgt + _unit(away) * size * rng.choice([0.3, 2.0], (N_EDGE, 1))).astype(F32).astype(np.float64)
    parts.append((o, tgt - o))
    # nearly parallel: d.n at +-par (1 +- 2^-20), at 0 and at -0, towards points of the square
    dn = rng.choice([PAR * (1 + 2.0 ** -20), PAR * (1 - 2.0 ** -20), PAR, 0.0, 1e-9], N_PAR) * rng.choice([-1.0, 1.0], N_PAR)
    phi = rng.uniform(0, 2 * np.pi, N_PAR)
    d = (np.cos(phi) * np.sqrt(1 - dn * dn))[:, None] * Rh + (np.sin(phi) * np.sqrt(1 - dn * dn))[:, None] * Uh + dn[:, None] * nrm
    d32 = d.astype(F32)
    k = int(np.argmax(np.abs(nrm)))
    if abs(nrm[k]) == 1.0:  # an axis plane: the component itself, signed zeros included
        d32[:, k] = (dn * nrm[k]).astype(F32)
        d32[dn == 0.0, k] = np.where(rng.integers(0, 2, int((dn == 0.0).sum())) == 0, F32(0.0), F32(-0.0))
    tgt = at(rng.uniform(-0.1, 1.1, (N_PAR, 2)))
    o = tgt - d * (size * rng.uniform(0.01, 2.0, (N_PAR, 1)))
    parts.append((o, d32))
    # origins on the plane and at t = 9e-6 (1 +- 2^-20), and at the accepted 1e-5
    tgt = at(rng.uniform(0.02, 0.98, (N_NEAR, 2)))
    d = _unit(rng.normal(size=(N_NEAR, 3)))
    d = np.where((d @ nrm)[:, None] > 0, -d, d)                # front-facing
    t = rng.choice([0.0, 9e-6 * (1 + 2.0 ** -20), 9e-6 * (1 - 2.0 ** -20), 1e-5 * (1 + 2.0 ** -20), 1.2e-5, 1e-4], (N_NEAR, 1))
    parts.append((tgt - t * d, d))
    o = np.concatenate([p[0] for p in parts]).astype(F32)
    d = np.concatenate([np.asarray(p[1], F32) for p in parts])
    return np.concatenate([o, d, rng.uniform(0, 1, (len(o), 1)).astype(F32)], axis=1)


def exact_hits_numpy(name, rays):
    """Square::intersect in fp32 on the constants fold_quad folds (hrt_kernels.hip quad_t): which rays hit."""
    v0, v1, v3, glass = SQUARES[name]
    v0, v1, v3 = (np.array(p, F32) for p in (v0, v1, v3))
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    length = lambda a: F32(np.sqrt(np.float64(dot(a, a))))
    R, U = v1 - v0, v3 - v0
    c = np.array([R[1] * U[2] - R[2] * U[1], R[2] * U[0] - R[0] * U[2], R[0] * U[1] - R[1] * U[0]], F32)
    n = (c / length(c)).astype(F32)
    lr, lu, D = length(R), length(U), dot(v0, n)
    o, d = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(all="ignore"):
        L = np.sqrt(dot(d, d).astype(np.float64)).astype(F32)
        d = (d / L[:, None]).astype(F32)
        den = dot(d, n)
        t = (D - dot(o, n)) / den
        ok = (den != 0) & ((den < 0) | bool(glass)) & (t > F32(1e-5))
        q = (o + t[:, None] * d) - v0
        p1, p2 = dot(q, R) / lr, dot(q, U) / lu
        ok &= (p1 <= lr) & (p1 >= 0) & (p2 <= lu) & (p2 >= 0)
    return ok


@pytest.fixture(scope="module")
def ray_sets():
    return {name: ray_set(name) for name in SQUARES}


@pytest.mark.parametrize("name", list(SQUARES))
def test_the_ray_set_hits_the_square_often_enough(name, ray_sets):
    rays = ray_sets[name]
    assert 1.8e5 <= len(rays) <= 2.2e5
    hits = int(exact_hits_numpy(name, rays).sum())
    assert hits >= 1000, f"{name}: only {hits} exact hits among {len(rays)} rays"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["KAT_QUAD", "KAT_QUAD_RCP"])
@pytest.mark.parametrize("name", list(SQUARES))
def test_the_filter_lets_every_exact_hit_through(gpu, name, kind, ray_sets):
    v0, v1, v3, glass = SQUARES[name]
    prim = np.array([*v0, *v1, *v3, 0, 0, 0, glass], F32)
    rays = ray_sets[name]
    out = gpu.debug_kat(getattr(gpu, kind), rays, prim=prim)
    hit, through = out[:, 0] == 1.0, out[:, 7] == 1.0
    print(f"{name} {kind}: {int(hit.sum())} exact hits, {int(through.sum())} let through, of {len(rays)} rays")
    assert hit.sum() >= 1000, f"{name}: only {int(hit.sum())} exact hits on the device"
    lost = hit & ~through
    assert not lost.any(), f"{name} {kind}: the filter drops {int(lost.sum())} rays the exact test hits, first {rays[np.flatnonzero(lost)[:3]].tolist()}"
