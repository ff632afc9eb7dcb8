"""THE RULE of lit paths (include/hrt.h "Lit paths") in NumPy, from the path's own tail records: the value of one sample
(`sample_value`), what a path that meets given surfaces does (`walk`), and the pieces of a tail record (`split`).

Everything is fp32 in the order the header writes (NumPy neither fuses nor reassociates).  The path itself -- closest hits, shading,
direct light, scattering -- is the integrator's and is not restated: the inputs here are the tail records hrt_path_tails writes
(`a` = rad / 6.f, `thr`, the point record and the word) and the look-up G of the point records (the volume's own eval /
eval_visible, or probe_lit_ref.gather).  The samples of a ray are probe_lit_ref.ray_output, the fold of a probe probe_ref.fold."""
import numpy as np

F32, U32 = np.float32, np.uint32
TAIL_FLOATS, TAIL_WORD, REACHED = 16, 11, 0x80000000
MAXBOUNCES = 6
DIFFUSE = 0  # Surface::type of a diffuse material; 1 is glass, 2 mirror


def split(T):
    """(point records (n, 8), thr (n, 3), segments (n,), reached (n,), a (n, 3)) of tail records (n, 16)."""
    T = np.ascontiguousarray(T, F32)
    assert T.ndim == 2 and T.shape[1] == TAIL_FLOATS
    word = T.view(U32)[:, TAIL_WORD]
    assert not (word & ~U32(REACHED | 0xFF)).any() and (T.view(U32)[:, 15] == 0).all(), "bits 8..30 of the word and float 15 are zero"
    return T[:, 0:8], T[:, 8:11], (word & U32(0xFF)).astype(np.int64), (word & U32(REACHED)) != 0, T[:, 12:15]


def sample_value(T, G):
    """Steps 4 and 5: value = a where the tail was not reached, (a) + thr * G elsewhere; a = rad / 6.f is already in the record."""
    _, thr, _, reached, a = split(T)
    G = np.asarray(G, F32)
    with np.errstate(all="ignore"):
        return np.where(reached[:, None], a + thr * G, a).astype(F32)


def walk(types, K):
    """What the rule does with a path whose segments meet surfaces of `types` in order (None: the segment misses; the list is as
    long as the unshortened path, at most MAXBOUNCES): (segments traced, tail reached)."""
    assert 1 <= K <= MAXBOUNCES and len(types) <= MAXBOUNCES
    diffuse = 0
    for j, t in enumerate(types):
        if t is None:
            return j + 1, False          # a miss ends the path
        if t == DIFFUSE:
            diffuse += 1
            if diffuse == K:
                return j + 1, True       # the tail, without scattering
    return len(types), False             # the bounces ran out
