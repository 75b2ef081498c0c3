"""Reference for the continuous feasibility bounds (tgms_bounds_batch*), shared by
test_bounds_host.py and test_gpu_bounds.py.  NumPy only, and independent of the library's
derivative ladder: per segment and quantity the polynomial in u = t / T, then the best of
  - the values at 0, at 1 and at every candidate stationary point: the real roots of the
    derivative from np.roots (companion-matrix eigenvalues) on the trimmed derivative, kept
    when inside [-1e-6, 1 + 1e-6], polished by four Newton steps in np.longdouble, clamped to
    [0, 1], the quantity evaluated there in np.longdouble;
  - a 4,097-point uniform evaluation, a floor: a root np.roots missed cannot lower the
    reference by more than O(h^2).
A record is pmin[3] pmax[3] v_peak a_peak j_peak, as the library's first nine entries."""
from fractions import Fraction

import numpy as np

from extrema_ref import ORACLE_TOL

LD = np.longdouble
GRID = np.linspace(0.0, 1.0, 4097).astype(LD)


def _polyval(c, u):
    """sum_k c[k] u^k in longdouble (c ascending)."""
    s = np.zeros_like(u, dtype=LD) + c[-1]
    for k in range(len(c) - 2, -1, -1):
        s = s * u + c[k]
    return s


def _deriv(c):
    return c[1:] * np.arange(1, len(c), dtype=LD)


def _candidates(q):
    """Stationary points of the polynomial q (ascending longdouble coefficients) in [0, 1]."""
    d1 = _deriv(q)
    d = np.asarray(d1, dtype=np.float64)
    while len(d) and d[-1] == 0.0:
        d = d[:-1]
    if len(d) < 2:
        return np.zeros(0, dtype=LD)
    r = np.roots(d[::-1])
    r = r[np.abs(r.imag) <= 1e-6].real
    r = r[(r >= -1e-6) & (r <= 1.0 + 1e-6)].astype(LD)
    d2 = _deriv(d1)
    for _ in range(4):
        f, g = _polyval(d1, r), _polyval(d2, r)
        ok = g != 0
        r = np.where(ok, r - f / np.where(ok, g, 1), r)
    return np.clip(r, 0, 1)


def segment_record(c, T):
    """(lo[3], hi[3], n2[3]) of one segment: c [3][8] on t in [0, T]; n2 = max |p^(q)|^2."""
    a = np.asarray(c, dtype=LD) * LD(T) ** np.arange(8, dtype=LD)  # coefficients in u
    lo, hi, n2 = np.empty(3), np.empty(3), np.empty(3)
    for ax in range(3):
        u = np.concatenate([GRID, _candidates(a[ax])])
        v = _polyval(a[ax], u)
        lo[ax], hi[ax] = float(v.min()), float(v.max())
    e = a
    for q in range(3):
        e = np.stack([_deriv(e[ax]) for ax in range(3)])  # T^(q+1) p^(q+1) in u
        sq = sum(np.convolve(e[ax], e[ax]) for ax in range(3))
        u = np.concatenate([GRID, _candidates(sq)])
        v = sum(_polyval(e[ax], u) ** 2 for ax in range(3))
        n2[q] = float(v.max() / LD(T) ** (2 * (q + 1)))
    return lo, hi, n2


def records(so, T, C):
    """[B, 9] reference records of a CSR batch."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    ref = np.empty((len(so) - 1, 9))
    for b in range(len(so) - 1):
        segs = [segment_record(C[s], T[s]) for s in range(int(so[b]), int(so[b + 1]))]
        ref[b, 0:3] = np.min([s[0] for s in segs], axis=0)
        ref[b, 3:6] = np.max([s[1] for s in segs], axis=0)
        ref[b, 6:9] = np.sqrt(np.max([s[2] for s in segs], axis=0))
    return ref


def check_contract(ext, ref, tol=ORACLE_TOL):
    """include/tgms.h: extents within tol x max|p| of the reference, peaks within tol relative."""
    ext = np.asarray(ext)
    assert ext.shape == (ref.shape[0], 10) and np.isfinite(ext).all()
    pmax = np.abs(ref[:, 0:6]).max(axis=1)
    err_p = np.abs(ext[:, 0:6] - ref[:, 0:6]).max(axis=1) / pmax
    err_k = (np.abs(ext[:, 6:9] - ref[:, 6:9]) / ref[:, 6:9]).max(axis=1)
    print("bounds vs reference: extents %.3g x max|p|, peaks %.3g relative" % (err_p.max(), err_k.max()))
    assert (err_p <= tol).all(), (int(err_p.argmax()), float(err_p.max()))
    assert (err_k <= tol).all(), (int(err_k.argmax()), float(err_k.max()))


# ---- the batches both test files use ----

def ragged48(seed=48):
    """48 trajectories covering every M in 1..16 three times (shuffled), with the waypoints
    and times of synthetic.ragged_batch: (so, W [S+48,3], T [S])."""
    from trajectory_generator_ros2_amd import synthetic as S
    rng = np.random.default_rng(seed)
    Ms = rng.permutation(np.tile(np.arange(1, 17), 3)).astype(np.int32)
    so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    n_seg, n_w = int(so[-1]), int(so[-1]) + 48
    W = np.c_[rng.uniform(-5, 5, n_w), rng.uniform(-5, 5, n_w), rng.uniform(0.5, 5, n_w)]
    rows = np.arange(n_seg) + np.repeat(np.arange(48), Ms)
    T = np.clip(np.linalg.norm(W[rows + 1] - W[rows], axis=1) / S.V_NOMINAL, S.T_MIN, S.T_MAX)
    return so, W, T


def end_derivs48(seed=49):
    """Non-zero start and final v, a, j for the 48 trajectories: [48, 18]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (48, 18)) * np.repeat([1.0, 0.5, 0.25, 1.0, 0.5, 0.25], 3)


def rest_to_rest(p0, d, T, axis=0):
    """M = 1, rest to rest: p = p0 + d (35 u^4 - 84 u^5 + 70 u^6 - 20 u^7) on `axis`, the other
    axes constant.  Returns (so, T [1], C [1,3,8], peaks) with the closed-form peaks
    v = 35/16 |d| / T, a = 84 / (5 sqrt 5) |d| / T^2, j = 105/2 |d| / T^3."""
    C = np.zeros((1, 3, 8))
    C[0, :, 0] = p0
    for j, k in ((4, 35.0), (5, -84.0), (6, 70.0), (7, -20.0)):
        C[0, axis, j] = d * k / T ** j
    peaks = np.array([35.0 / 16.0 * abs(d) / T, 84.0 / (5.0 * np.sqrt(5.0)) * abs(d) / T ** 2,
                      52.5 * abs(d) / T ** 3])
    return np.array([0, 1], np.int32), np.array([T]), C, peaks


OVERSHOOT_ROOTS = [Fraction(1, 8), Fraction(5, 8), Fraction(3, 4), Fraction(7, 8), Fraction(15, 16), Fraction(31, 32)]


def overshoot():
    """M = 1, T = 2: dx/du = k prod (u - r_i) with the six roots above and k = 105/4, integrated
    exactly from x(0) = 1; y linear, z constant.  Every coefficient is a dyadic rational, so
    the fp64 input is the exact polynomial.  Returns (so, T, C, pmin [3], pmax [3]) with the
    exact rational extents rounded to fp64."""
    k, x0, T = Fraction(105, 4), Fraction(1), 2
    v = [Fraction(1)]  # prod (u - r_i), ascending
    for r in OVERSHOOT_ROOTS:
        v = [(v[i - 1] if i else 0) - r * (v[i] if i < len(v) else 0) for i in range(len(v) + 1)]
    x = [x0] + [k * v[j] / (j + 1) for j in range(7)]
    C = np.zeros((1, 3, 8))
    for j in range(8):
        cj = x[j] / T ** j
        C[0, 0, j] = float(cj)
        assert Fraction(C[0, 0, j]) == cj  # exactly representable
    C[0, 1, 0], C[0, 1, 1] = -0.75, 0.5  # y = -0.75 + t/2: [-0.75, 0.25]
    C[0, 2, 0] = 2.0
    vals = [sum(x[j] * u ** j for j in range(8)) for u in [Fraction(0), Fraction(1)] + OVERSHOOT_ROOTS]
    pmin = np.array([float(min(vals)), -0.75, 2.0])
    pmax = np.array([float(max(vals)), 0.25, 2.0])
    assert max(vals) > max(vals[0], vals[1]) + Fraction(1, 25)  # x peaks at u = 1/8, 4 % past both ends
    return np.array([0, 1], np.int32), np.array([float(T)]), C, pmin, pmax
