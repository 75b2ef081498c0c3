"""Reference for the continuous body-rate bound (tgms_rate_batch*), shared by test_rate_ref.py,
test_rate_host.py and test_gpu_rate.py.  NumPy only, independent of the library's derivative
ladder, built on bounds_ref's and thrust_ref's pieces.

Per segment, in u = t / T: E = T^2 (p'' + g e_z), three polynomials of degree 5, E' = T^3 p''',
and omega^2 = ||E x E'||^2 / (T^2 ||E||^4), evaluated from the axis polynomials.  Its maximum
over [0, 1] is found two independent ways:
  (a) roots: G = N' D - 2 N D' with N = ||E x E'||^2 and D = ||E||^2 from np.convolve, its real
      roots from np.roots (companion-matrix eigenvalues) through bounds_ref._candidates (kept
      when inside [-1e-6, 1 + 1e-6], Newton-polished in np.longdouble), with u = 0 and u = 1;
      values in np.longdouble;
  (b) samples: 200,001 uniform samples in float64, then a golden-section search in
      np.longdouble around every local maximum of the samples.
The reference value is the larger of the two; `segment_omega2` returns both so that
test_rate_ref.py can hold them against each other."""
import functools
import os

import numpy as np

import bounds_ref as R
import thrust_ref as TR
from bounds_ref import LD, _candidates, _deriv
from extrema_ref import ORACLE_TOL
from thrust_ref import G0, _antiderivative, _force_polys

SAMPLES = 200001
CHUNK = 8192  # samples evaluated at a time: the temporaries stay in cache
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("ragged", "end_derivs", "extreme")


def _horner(c, u):
    """sum_k c[k] u^k in u's dtype (c ascending)."""
    s = np.zeros_like(u) + c[-1]
    for k in range(len(c) - 2, -1, -1):
        s = s * u + c[k]
    return s


def _omega2(e, T, u):
    """omega^2 at u (array) from the axis polynomials e [3][6], in u's dtype."""
    dt = u.dtype.type
    e = e.astype(dt)
    f = [_horner(e[ax], u) for ax in range(3)]
    d = [_horner(_deriv(e[ax]).astype(dt), u) for ax in range(3)]
    cx, cy, cz = f[1] * d[2] - f[2] * d[1], f[2] * d[0] - f[0] * d[2], f[0] * d[1] - f[1] * d[0]
    n2 = cx * cx + cy * cy + cz * cz
    den = (f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) ** 2 * dt(T) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n2 == 0, dt(0), n2 / den)


def rate_poly(e):
    """G = N' D - 2 N D', ascending, 26 coefficients.  The degree-9 coefficient of E x E' is 5
    a_5 b_5 - 5 b_5 a_5 = 0 identically and is dropped: left in as rounding noise it would be the
    leading coefficient the companion matrix divides by."""
    d = [_deriv(e[ax]) for ax in range(3)]
    cr = [(np.convolve(e[(ax + 1) % 3], d[(ax + 2) % 3]) - np.convolve(e[(ax + 2) % 3], d[(ax + 1) % 3]))[:9]
          for ax in range(3)]
    N = sum(np.convolve(c, c) for c in cr)
    D = sum(np.convolve(e[ax], e[ax]) for ax in range(3))
    return np.convolve(_deriv(N), D) - 2 * np.convolve(N, _deriv(D))


def _golden(e, T, lo, hi, iters=40):
    """Golden-section maximisation of omega^2 on each [lo_i, hi_i] (longdouble arrays).  The
    brackets are 1e-5 wide and omega^2 is stationary at the maximum: 40 steps leave 4e-14 in u."""
    r = (np.sqrt(LD(5)) - 1) / 2
    a, b, n = lo.copy(), hi.copy(), len(lo)
    for _ in range(iters):
        c, d = b - r * (b - a), a + r * (b - a)
        f = _omega2(e, T, np.concatenate([c, d]))
        left = f[:n] > f[n:]
        b, a = np.where(left, d, b), np.where(left, a, c)
    u = (a + b) / 2
    return u, _omega2(e, T, u)


def segment_omega2(c, T, g):
    """((w2, u) by roots, (w2, u) by samples) of one segment: c [3][8] on t in [0, T]."""
    e = _force_polys(c, T, g)
    ua = np.concatenate([np.array([0, 1], dtype=LD), _candidates(_antiderivative(rate_poly(e)))])
    wa = _omega2(e, T, ua)
    ia = int(np.argmax(wa))
    us = np.linspace(0.0, 1.0, SAMPLES)
    ws = np.concatenate([_omega2(e, T, us[i:i + CHUNK]) for i in range(0, SAMPLES, CHUNK)])
    top = np.flatnonzero((ws[1:-1] > ws[:-2]) & (ws[1:-1] >= ws[2:])) + 1  # a plateau counts once, at its left end
    ub = np.array([0, 1], dtype=LD)
    wb = _omega2(e, T, ub)
    if len(top):
        ur, wr = _golden(e, T, us[top - 1].astype(LD), us[top + 1].astype(LD))
        ub, wb = np.concatenate([ub, ur]), np.concatenate([wb, wr])
    ib = int(np.argmax(wb))
    return (wa[ia], ua[ia]), (wb[ib], ub[ib])


def segments(so, T, C, g=G0):
    """Per segment of a CSR batch: w2_roots [S], w2_samples [S] (longdouble) and the u [S] of the
    larger of the two."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    S = int(so[-1])
    wa, wb, u = np.empty(S, dtype=LD), np.empty(S, dtype=LD), np.empty(S)
    for s in range(S):
        (wa[s], ua), (wb[s], ub) = segment_omega2(C[s], T[s], g)
        u[s] = float(ua if wa[s] >= wb[s] else ub)
    return wa, wb, u


def records(so, T, C, g=G0):
    """(omega_max [B], seg_omega [S], seg_u [S]) of a CSR batch as float64: the larger of the two
    ways per segment, the maximum over a trajectory's segments."""
    wa, wb, u = segments(so, T, C, g)
    seg = np.sqrt(np.maximum(wa, wb)).astype(np.float64)
    return np.array([seg[so[b]:so[b + 1]].max() for b in range(len(so) - 1)]), seg, u


def evaluate(so, T, C, b, t, g=G0):
    """omega of trajectory b at its global time t in [0, D_b] (thrust_ref.evaluate's rule for the
    segment), as a float."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    knot, seg, k0 = 0.0, int(so[b]), 0.0
    for s in range(int(so[b]), int(so[b + 1])):
        if t >= knot:
            seg, k0 = s, knot
        knot += T[s]
    u = np.clip((LD(t) - LD(k0)) / LD(T[seg]), 0, 1)
    return float(np.sqrt(_omega2(_force_polys(C[seg], T[seg], g), T[seg], np.array([u], dtype=LD))[0]))


def scale(so, T, C, g=G0):
    """F J / m^2 [B] of include/tgms.h's accuracy block: F = f_max and m = f_min of
    thrust_ref.records, J = j_peak of bounds_ref.records."""
    th, bo = TR.records(so, T, C, g), R.records(so, T, C)
    assert (th[:, 0] > 0).all()
    return th[:, 1] * bo[:, 8] / th[:, 0] ** 2


@functools.lru_cache(maxsize=None)
def fixture(name, g=G0):
    """A golden batch with its reference, computed once and shared: so, T, C, omega [B], seg [S],
    seg_u [S], scale [B] (read-only arrays)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    so, T, C = z["seg_offsets"].astype(np.int32), z["seg_times"].copy(), z["coeffs"].copy()
    wa, wb, u = segments(so, T, C, g)
    seg = np.sqrt(np.maximum(wa, wb)).astype(np.float64)
    omega = np.array([seg[so[b]:so[b + 1]].max() for b in range(len(so) - 1)])
    out = dict(so=so, T=T, C=C, w2_roots=wa, w2_samples=wb, omega=omega, seg=seg, seg_u=u, scale=scale(so, T, C, g))
    for a in out.values():
        a.setflags(write=False)
    return out


def contract_errors(rec, seg_rec, fx):
    """|omega_max - true| / (F J / m^2) per trajectory, and the same ratio per segment row with
    its trajectory's F J / m^2; each to be <= 1e-9."""
    rec, seg_rec = np.asarray(rec), np.asarray(seg_rec)
    e_traj = np.abs(rec[:, 0] - fx["omega"]) / fx["scale"]
    e_seg = np.abs(seg_rec[:, 0] - fx["seg"]) / np.repeat(fx["scale"], np.diff(fx["so"]))
    return e_traj, e_seg


def check_contract(rec, seg_rec, fx, label, tol=ORACLE_TOL, g=G0):
    """The accuracy block of include/tgms.h on a fixture, with what the records promise about
    each other: every time in range, omega evaluated at the stored times reproduces the stored
    values, and the maximum over a trajectory's rows is its omega_max to the bit."""
    so, T, C = fx["so"], fx["T"], fx["C"]
    rec, seg_rec = np.asarray(rec), np.asarray(seg_rec)
    assert rec.shape == (len(so) - 1, 2) and seg_rec.shape == (so[-1], 2)
    assert np.isfinite(rec).all() and np.isfinite(seg_rec).all()
    e_traj, e_seg = contract_errors(rec, seg_rec, fx)
    print("rate vs reference (%s): omega_max %.3g, segment rows %.3g x F J / m^2" % (label, e_traj.max(), e_seg.max()))
    assert (e_traj <= tol).all(), (int(e_traj.argmax()), float(e_traj.max()))
    assert (e_seg <= tol).all(), (int(e_seg.argmax()), float(e_seg.max()))
    assert (seg_rec[:, 1] >= 0).all() and (seg_rec[:, 1] <= T).all()
    for b in range(len(so) - 1):
        rows = seg_rec[so[b]:so[b + 1]]
        assert rows[:, 0].max() == rec[b, 0]
        D = 0.0
        for x in T[so[b]:so[b + 1]]:
            D += x
        assert 0.0 <= rec[b, 1] <= D
        assert abs(evaluate(so, T, C, b, rec[b, 1], g) - rec[b, 0]) <= tol * fx["scale"][b], b


def closed_form(a=-3.0, k=4.0, T=1.5, p0=(0.3, -1.0, 2.0)):
    """One segment with p_x = p0 + a t^2 / 2 + k t^3 / 6, a < 0 < k: f = (a + k t, 0, g), p''' =
    (k, 0, 0), omega = g k / ((a + k t)^2 + g^2), largest where a + k t = 0: k / g at t = -a / k,
    inside (0, T).  Returns (so, T [1], C [1,3,8], t_peak)."""
    assert 0.0 < -a / k < T
    C = np.zeros((1, 3, 8))
    C[0, :, 0] = p0
    C[0, 0, 2], C[0, 0, 3] = a / 2.0, k / 6.0
    return np.array([0, 1], np.int32), np.array([T]), C, -a / k
