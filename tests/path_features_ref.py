"""THE RULE of path features (include/hrt.h "Path features") in NumPy: the record of one path from the surfaces its segments meet
(`record`), the fold of the records of a pixel's samples (`fold`), and what a tail record of hrt_path_tails(tail_after = 1) says of
the same path (`from_tail`).

Everything is fp32 in the order the header writes (NumPy neither fuses nor reassociates).  The path itself -- closest hits, shading,
scattering -- is the integrator's and is not restated: the inputs are per-segment surfaces (hrt_trace_rays in SHADE mode gives them)
or per-sample records (hrt_path_features gives them)."""
import numpy as np

import lit_paths_ref as lp

F32, U32 = np.float32, np.uint32
FEATURE_FLOATS = 12
MAXBOUNCES = lp.MAXBOUNCES
DIFFUSE = lp.DIFFUSE
ALBEDO, NORMAL, EMISSION, DEPTH, COVERAGE = slice(0, 3), slice(3, 6), slice(6, 9), 9, 10


def record(segments):
    """Steps 1-5 for one path.  `segments`: what its segments meet, in order, at most MAXBOUNCES of them -- None for a miss, else
    (type, albedo (3,), emission (3,), t, normal (3,)).  A list that ends before a miss, a diffuse hit or MAXBOUNCES segments is a
    path the caller cut short.  -> (12,) float32."""
    assert len(segments) <= MAXBOUNCES
    thr, E, depth = np.ones(3, F32), np.zeros(3, F32), F32(0)
    out = np.zeros(FEATURE_FLOATS, F32)
    for seg in segments:
        if seg is None:
            break                                   # a miss ends the path unreached; the sky is not added
        typ, albedo, emission, t, normal = seg
        E = E + thr * np.asarray(emission, F32)
        depth = F32(depth + F32(t))
        thr = thr * np.asarray(albedo, F32)
        if typ == DIFFUSE:                          # reached, without scattering
            out[ALBEDO], out[NORMAL], out[DEPTH], out[COVERAGE] = thr, np.asarray(normal, F32), depth, F32(1)
            break
    out[EMISSION] = E                               # an unreached path keeps the emitters seen on the way
    return out


def fold(records, traced=None):
    """The frame form: records (n_samples, ..., 12) of the samples in ascending order -> their sum from +0, in order, over
    float32(n_samples).  `traced` (n_samples, ...) bool: False where the lens made no ray -- that sample adds nothing and counts in
    the divisor."""
    records = np.asarray(records, F32)
    total = np.zeros(records.shape[1:], F32)
    for s in range(records.shape[0]):
        if traced is None:
            total = total + records[s]
        else:
            total = np.where(np.asarray(traced[s], bool)[..., None], total + records[s], total)
    return total / F32(records.shape[0])


def from_tail(T):
    """CONTRACT B: (albedo (n, 3), normal (n, 3), coverage (n,), E / 6.f (n, 3)) that tail records (n, 16) of
    hrt_path_tails(tail_after = 1, bias = 0) give for the path-feature records of the same rays, keys, sample and seed."""
    pts, thr, _, reached, a = lp.split(T)
    return thr, pts[:, 4:7], reached.astype(F32), a
