"""Reference for the continuous thrust and tilt bounds (tgms_thrust_batch*), shared by
test_thrust_ref.py, test_thrust_host.py and test_gpu_thrust.py.  NumPy only, independent of the
library's derivative ladder, built on bounds_ref's pieces.

Per segment, in np.longdouble and in u = t / T: E = T^2 (p'' + g e_z), three polynomials of
degree 5.  Candidates are u = 0, u = 1, the 4,097-point grid (a floor: a root np.roots missed
cannot move the reference by more than O(h^2)), the stationary points of ||E||^2 and the roots
of G = E_z H' - 2 H E_z' (H = E_x^2 + E_y^2), both from bounds_ref._candidates (np.roots on the
trimmed polynomial, Newton-polished in longdouble); G goes in as the derivative of its own
antiderivative.  Values are longdouble sqrt / arctan2 of the axis polynomials at the
candidates.  A record is f_min, f_max, tilt_max (m/s^2, m/s^2, rad)."""
import numpy as np

from bounds_ref import GRID, LD, _candidates, _deriv, _polyval
from extrema_ref import ORACLE_TOL

G0 = 9.80665


def _force_polys(c, T, g):
    """E [3][6] (ascending, longdouble) of one segment: c [3][8] on t in [0, T]."""
    a = np.asarray(c, dtype=LD) * LD(T) ** np.arange(8, dtype=LD)
    e = np.stack([_deriv(_deriv(a[ax])) for ax in range(3)])
    e[2, 0] += LD(g) * LD(T) ** 2
    return e


def _antiderivative(q):
    return np.concatenate([np.zeros(1, dtype=LD), q / np.arange(1, len(q) + 1, dtype=LD)])


def tilt_poly(e):
    """G = E_z H' - 2 H E_z', ascending; its degree-14 coefficient cancels (kept: ~1e-19 relative)."""
    H = np.convolve(e[0], e[0]) + np.convolve(e[1], e[1])
    return np.convolve(e[2], _deriv(H)) - 2 * np.convolve(H, _deriv(e[2]))


def _values(e, T, u):
    x, y, z = (_polyval(e[ax], u) / LD(T) ** 2 for ax in range(3))
    return np.sqrt(x * x + y * y + z * z), np.arctan2(np.sqrt(x * x + y * y), z)


def segment_record(c, T, g, grid_only=False):
    """(f_min, f_max, tilt_max) of one segment as longdouble."""
    e = _force_polys(c, T, g)
    cand = [GRID]
    if not grid_only:
        cand.append(_candidates(sum(np.convolve(e[ax], e[ax]) for ax in range(3))))
        cand.append(_candidates(_antiderivative(tilt_poly(e))))
    f, th = _values(e, T, np.concatenate(cand))
    return f.min(), f.max(), th.max()


def records(so, T, C, g=G0, grid_only=False):
    """[B, 3] reference records f_min f_max tilt_max of a CSR batch (float64)."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    ref = np.empty((len(so) - 1, 3))
    for b in range(len(so) - 1):
        segs = np.array([segment_record(C[s], T[s], g, grid_only) for s in range(int(so[b]), int(so[b + 1]))])
        ref[b] = [float(segs[:, 0].min()), float(segs[:, 1].max()), float(segs[:, 2].max())]
    return ref


def evaluate(so, T, C, b, t, g=G0):
    """(||f||, theta) of trajectory b at its global time t in [0, D_b], as floats: the segment
    is the one whose closed interval [knot_m, knot_m + T_m] holds t (the last such one), knots by
    the left-to-right float64 prefix sum the library uses."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    s0, s1 = int(so[b]), int(so[b + 1])
    knot, seg, k0 = 0.0, s0, 0.0
    for s in range(s0, s1):
        if t >= knot:
            seg, k0 = s, knot
        knot += T[s]
    u = np.clip((LD(t) - LD(k0)) / LD(T[seg]), 0, 1)
    f, th = _values(_force_polys(C[seg], T[seg], g), T[seg], np.array([u], dtype=LD))
    return float(f[0]), float(th[0])


def contract_errors(rec, ref):
    """The three ratios of include/tgms.h's accuracy block, each to be <= 1e-9: the errors of
    f_min^2 and f_max^2 over F^2 and of tilt_max over F / f_min (F, f_min the reference's)."""
    rec, ref = np.asarray(rec), np.asarray(ref)
    F2 = ref[:, 1] ** 2
    e_lo = np.abs(rec[:, 0] ** 2 - ref[:, 0] ** 2) / F2
    e_hi = np.abs(rec[:, 2] ** 2 - ref[:, 1] ** 2) / F2
    with np.errstate(divide="ignore", invalid="ignore"):
        e_tilt = np.where(ref[:, 0] > 0, np.abs(rec[:, 4] - ref[:, 2]) / (ref[:, 1] / ref[:, 0]), 0.0)
    return e_lo, e_hi, e_tilt


def check_contract(rec, ref, g=G0, tol=ORACLE_TOL):
    """|f_min^2 - true^2| <= tol F^2, |f_max^2 - true^2| <= tol F^2 and, where f_min > 0,
    |tilt_max - true| <= tol F / f_min.  rec [B, 6] (the library's), ref [B, 3]; g only labels
    the printed line."""
    rec = np.asarray(rec)
    assert rec.shape == (ref.shape[0], 6) and np.isfinite(rec).all()
    e_lo, e_hi, e_tilt = contract_errors(rec, ref)
    print("thrust vs reference (g = %g): f_min^2 %.3g F^2, f_max^2 %.3g F^2, tilt %.3g F / f_min rad"
          % (g, e_lo.max(), e_hi.max(), e_tilt.max()))
    assert (e_lo <= tol).all(), (int(e_lo.argmax()), float(e_lo.max()))
    assert (e_hi <= tol).all(), (int(e_hi.argmax()), float(e_hi.max()))
    assert (e_tilt <= tol).all(), (int(e_tilt.argmax()), float(e_tilt.max()))


def check_times(so, T, C, rec, ref, g=G0, tol=ORACLE_TOL):
    """Every t_* lies in [0, D_b], and the reference quantity evaluated there matches the stored
    value within the contract (on the squares for the thrust, F / f_min for the tilt)."""
    from extrema_ref import durations
    D = durations(so, T)
    rec = np.asarray(rec)
    for b in range(len(so) - 1):
        F, fmin = ref[b, 1], ref[b, 0]
        for col in (1, 3, 5):
            assert 0.0 <= rec[b, col] <= D[b], (b, col, rec[b, col], D[b])
        assert abs(evaluate(so, T, C, b, rec[b, 1], g)[0] ** 2 - rec[b, 0] ** 2) <= tol * F * F, (b, "f_min")
        assert abs(evaluate(so, T, C, b, rec[b, 3], g)[0] ** 2 - rec[b, 2] ** 2) <= tol * F * F, (b, "f_max")
        if fmin > 0:
            assert abs(evaluate(so, T, C, b, rec[b, 5], g)[1] - rec[b, 4]) <= tol * F / fmin, (b, "tilt")


def a_peak(d, T):
    """Peak |acceleration| of bounds_ref.rest_to_rest: 84 / (5 sqrt 5) |d| / T^2."""
    return 84.0 / (5.0 * np.sqrt(5.0)) * abs(d) / T ** 2
