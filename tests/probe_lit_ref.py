"""THE RULE of lit rays (include/hrt.h "Lit rays") in NumPy: the value of one sample from what the integrator's own device
functions return for its first hit (`sample_value`), the samples of a ray (`ray_output`), the hysteresis update (`blend`) and the
furnace series the end-to-end test compares with (`furnace`).

Everything is fp32 in the order the header writes (NumPy neither fuses nor reassociates).  The hit itself -- closest hit, shading,
direct light -- is the trace path's and is not restated: the inputs here are `head` = rad / 6.f per channel after step 4 (what a lit
ray returns against a volume of zeros), the albedo, and per ray whether the surface is diffuse and what the look-up G of the point
record {p, time, n, bias} gives (probe_volume_ref.evaluate or probe_depth_ref.evaluate_visible)."""
import numpy as np

import probe_depth_ref as pd
import probe_volume_ref as pv

F32, U32 = np.float32, np.uint32
FACING, LIT_VISIBLE, RADIANCE = 2, 4, 1
DIFFUSE = 0  # Surface::type of a diffuse material; 1 is glass, 2 mirror


def point_records(o, d, t, normal, time, bias):
    """The tail's point records {p, time, n, bias}: p = o + t * d in fp32, n the shaded normal as it is."""
    o, d, t = np.asarray(o, F32), np.asarray(d, F32), np.asarray(t, F32)
    pts = np.zeros((len(o), 8), F32)
    with np.errstate(all="ignore"):
        pts[:, 0:3] = o + t[:, None] * d
    pts[:, 3] = np.asarray(time, F32)
    pts[:, 4:7] = np.asarray(normal, F32)
    pts[:, 7] = F32(bias)
    return pts


def gather(lo, hi, counts, coeffs, mom, pts, eval_flags):
    """G of step 5 for point records: the plain look-up, or with LIT_VISIBLE the visible one; always the irradiance form."""
    assert not eval_flags & RADIANCE and not eval_flags & ~(FACING | LIT_VISIBLE), "refused"
    facing = bool(eval_flags & FACING)
    if eval_flags & LIT_VISIBLE:
        return pd.evaluate_visible(lo, hi, counts, coeffs, mom, pts, False, facing)
    return pv.evaluate(lo, hi, counts, coeffs, pts, False, facing)


def sample_value(head, albedo, diffuse, G):
    """Step 5: value = (rad / 6.f) + thr * G per channel, thr = 1 * albedo; G = 0 where the surface is not diffuse or the ray
    missed (`diffuse` False)."""
    head, albedo, G = np.asarray(head, F32), np.asarray(albedo, F32), np.asarray(G, F32)
    G = np.where(np.asarray(diffuse, bool)[:, None], G, F32(0)).astype(F32)
    thr = (F32(1) * albedo).astype(F32)
    with np.errstate(all="ignore"):
        return (head + thr * G).astype(F32)


def ray_output(values, n_samples=None, base=None):
    """Step 6: values (S, n, 3) in ascending sample order -> the mean, or with `base` (n, 3) the running sums."""
    values = np.asarray(values, F32)
    total = np.zeros(values.shape[1:], F32) if base is None else np.asarray(base, F32).copy()
    for v in values:
        total = total + v
    if base is not None:
        return total.astype(F32)
    return (total / F32(len(values) if n_samples is None else n_samples)).astype(F32)


def blend(packed, coeffs, keep):
    """hrt_probe_volume_blend on the 27 coefficients: p = (keep * p) + ((1.f - keep) * c)."""
    p, c, k = np.asarray(packed, F32), np.asarray(coeffs, F32), F32(keep)
    assert 0 <= k < 1, "refused"
    with np.errstate(all="ignore"):
        return ((k * p) + ((F32(1) - k) * c)).astype(F32)


def furnace(e, rho, rounds):
    """Band 0 over Y0 of a closed diffuse room of albedo rho and emission e (hrt_trace_radiance's units: / 6) after `rounds`
    rounds of relighting from zero: (e / 6) (1 - rho^K) / (1 - rho)."""
    return (e / 6.0) * (1.0 - rho ** rounds) / (1.0 - rho)
