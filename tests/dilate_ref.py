"""Reference for the time dilation (tgms_dilate_batch*), shared by test_dilate_host.py and
test_gpu_dilate.py.  NumPy only.  The contract of include/tgms.h is free of conditioning: it
speaks about the OUTPUT coefficients, so the check takes bounds_ref.records and
thrust_ref.records of the output (both independent of the library's derivative ladder) and holds
them against the limits; no reference dilation is searched for.  The closed forms are those of
single rest-to-rest segments (bounds_ref.rest_to_rest, thrust_ref.a_peak)."""
import numpy as np

import bounds_ref as R
import thrust_ref as TR
from extrema_ref import ORACLE_TOL

INF = float("inf")
NONE, SPEED, ACCEL, JERK, THRUST_HIGH, THRUST_LOW, TILT = range(7)
CAPPED, NONFINITE, MASK, EVALS_SHIFT = 1, 16, 0xFF, 8


def scale_coeffs(so, T, C, s):
    """(T', C') of the batch dilated by s [B]: T_i' = s T_i, c_k' = c_k / s^k."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    per_seg = np.repeat(np.asarray(s, dtype=np.float64), np.diff(so))
    return per_seg * T, C * (1.0 / per_seg)[:, None, None] ** np.arange(8)


def quantities(so, T_out, C_out, g=TR.G0):
    """[B, 6] v_peak a_peak j_peak f_max f_min tilt_max of the output, from the references."""
    rb, rt = R.records(so, T_out, C_out), TR.records(so, T_out, C_out, g)
    return np.c_[rb[:, 6:9], rt[:, 1], rt[:, 0], rt[:, 2]]


def excesses(q, lim):
    """[B, 6] how far each quantity of `quantities` is past its limit, in the units of the
    contract's right-hand sides: relative for v, a, j, f_max; (f_lo - f_min) / F for f_min; (tilt -
    tilt_max) f_min / F for the tilt.  <= 1e-9 everywhere is "feasible"; the column of the active
    limit within +-1e-9 is "tight" (the f_min column as (f_lo - f_min) / f_lo there)."""
    v_max, a_max, j_max, f_lo, f_hi, tilt = lim
    F, f_min = q[:, 3], q[:, 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.c_[q[:, 0] / v_max - 1, q[:, 1] / a_max - 1, q[:, 2] / j_max - 1, F / f_hi - 1,
                  (f_lo - f_min) / F if f_lo > 0 else np.full(len(q), -INF),
                  (q[:, 5] - tilt) * f_min / F]
    return e


def check_contract(so, T_out, C_out, scale, active, flags, lim, s_lo, g=TR.G0, tol=ORACLE_TOL, label=""):
    """"Feasible" and "tight" of include/tgms.h on every usable, uncapped row; lim = (v_max,
    a_max, j_max, f_lo, f_hi, tilt_max) with inf (f_lo: 0) for unchecked.  Prints and returns the
    worst feasible excess, the worst tight deviation and the active code the reference sees per
    row (the limit the output is closest to; NONE where scale == s_lo)."""
    scale, active, flags = np.asarray(scale), np.asarray(active), np.asarray(flags) & MASK
    q = quantities(so, T_out, C_out, g)
    e = excesses(q, lim)
    ok = flags == 0
    assert np.isfinite(scale[ok]).all() and (scale[ok] >= s_lo).all()
    worst_feas = e[ok].max() if ok.any() else -INF
    col = {SPEED: 0, ACCEL: 1, JERK: 2, THRUST_HIGH: 3, THRUST_LOW: 4, TILT: 5}
    tight = np.zeros(len(scale))
    seen = np.full(len(scale), NONE)
    for b in np.flatnonzero(ok):
        assert (active[b] == NONE) == (scale[b] == s_lo), (b, active[b], scale[b])
        if active[b] == NONE:
            continue
        d = e[b].copy()
        d[4] = (lim[3] - q[b, 4]) / lim[3] if lim[3] > 0 else -INF  # f_min: relative to its limit
        tight[b] = abs(d[col[int(active[b])]])
        seen[b] = [SPEED, ACCEL, JERK, THRUST_HIGH, THRUST_LOW, TILT][int(np.argmax(d))]
    print("dilate contract %s: %d rows, feasible excess %.3g, tight deviation %.3g (tol %.1g)"
          % (label, int(ok.sum()), worst_feas, tight.max(), tol))
    assert worst_feas <= tol, (int(np.argmax(np.where(ok, e.max(axis=1), -INF))), worst_feas)
    assert tight.max() <= tol, (int(tight.argmax()), float(tight.max()))
    return worst_feas, float(tight.max()), seen


# ---- closed forms on bounds_ref.rest_to_rest: the expected scale of one limit alone ----

def peaks(d, T):
    """v, a, j peaks of rest_to_rest(d, T)."""
    return 35.0 / 16.0 * abs(d) / T, TR.a_peak(d, T), 52.5 * abs(d) / T ** 3


def s_horizontal_fmax(a_pk, f_hi, g):
    return (a_pk ** 2 / (f_hi ** 2 - g ** 2)) ** 0.25


def s_horizontal_tilt(a_pk, theta, g):
    return np.sqrt(a_pk / (g * np.tan(theta)))


def s_vertical_fmax(a_pk, f_hi, g):
    return np.sqrt(a_pk / (f_hi - g))


def s_vertical_fmin(a_pk, f_lo, g):
    return np.sqrt(a_pk / (g - f_lo))


def s_kinematic(pk, v_max=INF, a_max=INF, j_max=INF):
    """max(v_peak / v_max, sqrt(a_peak / a_max), cbrt(j_peak / j_max))."""
    return max(pk[0] / v_max, np.sqrt(pk[1] / a_max), np.cbrt(pk[2] / j_max))
