"""The three transforming calls (tgms_dilate_batch*, tgms_cut_batch*, tgms_corridor_split_batch*)
on the constructed polynomials of poly_zoo.py, shared by test_transform_zoo_host.py and
test_gpu_transform_zoo.py.  Their own test files feed them minimum-snap solves; here the input
has its extremum exactly on a knot, trailing zero coefficients, a free-falling arc, and every
expected value is a closed form or a fractions.Fraction value rounded once.

Every check_* takes a backend `be`:
    be.dilate(so, T, C, lim, s_lo, s_hi, g)      -> (scale, active, flags, T_out, C_out)
    be.cut(so, W, T, C, t_cut, min_frac, ED)     -> Solver.cut's tuple
    be.corridor(so, T, C, faces, fo, r)          -> Solver.corridor's tuple
    be.split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac) -> Solver.corridor_split's
    be.solve / be.bounds / be.thrust / be.separation: the Solver's
    be.dilate_records(...)  the dilate call, then bounds and thrust of its own output
    be.cut_then(...)        the cut call, then one analysis call on its own output
Host below wraps a Solver(host=True); the GPU file's Device keeps the buffers of the last two on
the device from end to end.  lim = (v_max, a_max, j_max, f_lo, f_hi, tilt) as in dilate_ref.

Tolerances are the header's 1e-9 (TOL), the bounds of cut_ref / split_ref / test_split_host, or
derived beside their use; none comes from an output."""
import functools
from fractions import Fraction as Fr
from math import comb

import numpy as np

import bounds_ref as R
import cut_ref as CR
import dilate_ref as DR
import poly_zoo as Z
import split_ref as SR
import thrust_ref as TR
from extrema_ref import bit_equal
from test_poly_zoo_host import (BALL, CHEB, CUBIC, DEF4, HOLD, KP2, KP3, LIN, PARTNER, TOUCH, zoo, zoo_reference)

TOL = 1e-9
G = Z.G
INF = float("inf")
S_HI = 100.0
LD = np.longdouble
ACC = 105.0 / 32.0   # |p''| of knot_peak on its knot (poly_zoo.knot_peak: q''(1) / T^2 = -32 k / 4)
LIM6 = (3.0, 6.0, 30.0, 4.0, 16.0, 0.5)  # all six finite: test_dilate_host.LIM
WORST = {}  # label -> the largest observed fraction of its bound, printed by the checks


def note(label, value, bound):
    """Record and print an observed value beside its bound, in the style of check_contract."""
    value = float(value)
    WORST[label] = max(WORST.get(label, 0.0), value)
    print("transform zoo %s: %.3g (bound %.3g)" % (label, value, bound))


def fr(x):
    return Fr(float(x))


# ---- the zoo with waypoints ----

def end_point(c, T):
    """p(T) of one segment [3, 8], in Fraction, rounded once."""
    return np.array([float(Z._val([fr(x) for x in c[ax]], fr(T))) for ax in range(3)])


def waypoints(so, T, C):
    """[S + B, 3]: every segment's c_0 and the last segment's end, the layout of the solve."""
    W = []
    for b in range(len(so) - 1):
        W += [C[s, :, 0] for s in range(so[b], so[b + 1])] + [end_point(C[so[b + 1] - 1], T[so[b + 1] - 1])]
    return np.array(W)


@functools.lru_cache(maxsize=None)
def zoo_w():
    """((so, T, C), W, exact) of the ten zoo rows."""
    (so, T, C), ex = zoo()
    W = waypoints(so, T, C)
    W.setflags(write=False)
    return (so, T, C), W, ex


def rows(batch, W, which):
    """The trajectories `which` of a batch with their waypoints."""
    so = batch[0]
    wp = np.concatenate([np.arange(so[b] + b, so[b + 1] + b + 1) for b in which])
    return Z.take(batch, list(which)), np.asarray(W)[wp]


class Host:
    """The backend protocol on a Solver's host-pointer calls."""

    def __init__(self, solver):
        self.s = solver

    def dilate(self, so, T, C, lim, s_lo, s_hi=S_HI, g=G):
        from test_dilate_host import limits_of
        lk, lt = limits_of(lim)
        return self.s.dilate(so, T, C, g, lk, lt, s_lo, s_hi)

    def cut(self, so, W, T, C, tc, mf=0.0, ED=None):
        return self.s.cut(so, W, T, C, tc, mf, ED)

    def corridor(self, so, T, C, faces, fo, r=0.0):
        return self.s.corridor(so, T, C, faces, fo, r)

    def split(self, so, W, T, C, faces, fo, seg_rec, seg_face, r=0.0, mode=SR.PULL, min_frac=0.1):
        return self.s.corridor_split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac)

    def solve(self, so, W, T, ED=None):
        return self.s.solve(so, W, T, ED)

    def bounds(self, so, T, C):
        return self.s.bounds(so, T, C)

    def thrust(self, so, T, C, g):
        return self.s.thrust(so, T, C, g)

    def separation(self, so, T, C, pairs, t0):
        return self.s.separation(so, T, C, pairs, t0)

    def dilate_records(self, so, T, C, lim, s_lo, g=G):
        out = self.dilate(so, T, C, lim, s_lo, S_HI, g)
        return out, self.bounds(so, out[3], out[4])[0], self.thrust(so, out[3], out[4], g)[0]

    def cut_then(self, so, W, T, C, tc, kind, g=G, pairs=None):
        out = self.cut(so, W, T, C, tc, 0.0)
        so2, _, T2, _, C2, _, t0, _ = out
        if kind == "bounds":
            return out, self.bounds(so2, T2, C2)[0]
        if kind == "thrust":
            return out, self.thrust(so2, T2, C2, g)[0]
        return out, self.separation(so2, T2, C2, pairs, t0)[0]


# =====================================================================================
# A. dilate
# =====================================================================================

def one_limit(**kw):
    lim = dict(v=INF, a=INF, j=INF, f_lo=0.0, f_hi=INF, tilt=INF)
    lim.update(kw)
    return tuple(lim[k] for k in ("v", "a", "j", "f_lo", "f_hi", "tilt"))


def s_tolerance(kind, s, lim=None, dfds=None):
    """The relative tolerance on s from the header's tight clause to first order, doubled for the
    record's own 1e-9 (the clause speaks of records taken by calls that carry 1e-9 themselves).
    With e = 1e-9:
      speed  v / s = v_max (1 + e)                 ds / s = e
      accel  a / s^2 = a_max (1 + e)               ds / s = e / 2
      jerk   j / s^3 = j_max (1 + e)               ds / s = e / 3
      f_hi   F^2 = a^2 / s^4 + g^2 = f_hi^2 (1 + e)^2: 2 F dF = -4 a^2 / s^5 ds, so with a^2 / s^4 =
             f_hi^2 - g^2:  ds / s = e f_hi^2 / (2 (f_hi^2 - g^2))
      tilt   theta = atan(a / (s^2 g)) within e F / f_min rad; the hold and the ends have f = g, so
             f_min = g and F = g / cos(theta); d theta / ds = -sin(2 theta) / s:
             ds / s = e / (cos(theta) sin(2 theta))
      f_lo   a general crossing: |f_min - f_lo| <= e f_lo and dfds = |d f_min / d s| at s from the
             closed form: ds / s = e f_lo / (s dfds)"""
    e = TOL
    if kind == DR.SPEED:
        t = e
    elif kind == DR.ACCEL:
        t = e / 2
    elif kind == DR.JERK:
        t = e / 3
    elif kind == DR.THRUST_HIGH:
        t = e * lim ** 2 / (2 * (lim ** 2 - G ** 2))
    elif kind == DR.TILT:
        t = e / (np.cos(lim) * np.sin(2 * lim))
    else:
        t = e * lim / (s * dfds)
    return 2 * t


def _closed(be, what, so, T, C, lim, want, code, tol, s_lo=0.5, g=G):
    s, act, fl, T_out, C_out = be.dilate(so, T, C, lim, s_lo, S_HI, g)
    assert (fl & DR.MASK == 0).all() and np.isfinite(s).all(), (what, fl)
    assert s_lo < want < S_HI
    assert act[0] == code, (what, act[0], code)
    rel = abs(s[0] / want - 1.0)
    note("%s dilate closed form %s, |s / s* - 1|" % (what, ("", "speed", "accel", "jerk", "f_max", "f_min", "tilt")[code]),
         rel, tol)
    assert rel <= tol, (what, code, s[0], want, rel, tol)
    assert bit_equal(T_out, s[0] * np.asarray(T))  # seg_times_out = s T_i, one product
    return s[0]


def check_dilate_knot_peak(be, what):
    """The peak acceleration, and with it f_max and the tilt, sits exactly on an interior knot: a
    search or a peak that leaves the knot's end out returns a smaller s."""
    (so, T, C), W, ex = zoo_w()
    out = {}
    for r in (KP2, KP3):
        b, _ = rows((so, T, C), W, [r])
        f_hi, th, a_max = 10.0, 0.25, 2.0
        out[r, "f_hi"] = _closed(be, what, *b, one_limit(f_hi=f_hi), DR.s_horizontal_fmax(ACC, f_hi, G), DR.THRUST_HIGH,
                                 s_tolerance(DR.THRUST_HIGH, None, f_hi))
        out[r, "tilt"] = _closed(be, what, *b, one_limit(tilt=th), DR.s_horizontal_tilt(ACC, th, G), DR.TILT,
                                 s_tolerance(DR.TILT, None, th))
        out[r, "a"] = _closed(be, what, *b, one_limit(a=a_max), np.sqrt(ACC / a_max), DR.ACCEL,
                              s_tolerance(DR.ACCEL, None))
    return out


def check_dilate_deficient(be, what):
    """Trailing zero coefficients: s = peak / limit (root, cube root) from the exact peaks; a peak
    that is exactly 0 gives s == s_lo to the bit, NONE and one evaluation, so c_0 (and for the
    constant-velocity row c_1) must not leak into a higher peak."""
    (so, T, C), W, ex = zoo_w()
    pk = ex["deficient"]["ext"][:, 6:9]
    s_lo, out = 0.5, {}
    for col, (name, code, root) in enumerate((("v", DR.SPEED, 1), ("a", DR.ACCEL, 2), ("j", DR.JERK, 3))):
        for n, r in enumerate((DEF4, LIN, BALL, CUBIC, HOLD)):
            b, _ = rows((so, T, C), W, [r])
            limit = 0.25 if pk[n, col] == 0.0 else pk[n, col] / 2.0  # s* = 2, sqrt 2, cbrt 2: inside (s_lo, s_hi)
            lim = one_limit(**{name: limit})
            if pk[n, col] == 0.0:
                s, act, fl, T_out, C_out = be.dilate(*b, lim, s_lo, S_HI, G)
                assert s[0] == s_lo and act[0] == DR.NONE and fl[0] == 1 << DR.EVALS_SHIFT, (r, name, s, act, fl)
                assert bit_equal(T_out, s_lo * b[1])
            else:
                want = (pk[n, col] / limit) ** (1.0 / root)
                out[r, name] = _closed(be, "%s row %d" % (what, r), *b, lim, want, code, s_tolerance(code, None), s_lo)
    return out


def _cubic_crossing(f_lo):
    """The lambda at which the cubic piece of deficient row 0 meets f_min = f_lo, as a Fraction, and
    |d f_min^2 / d lambda| there.  On the piece f_s = lambda v sigma + G e_z, sigma = -4 + 6 t in
    [-4, 2]; for lambda <= 1/4 the unconstrained minimiser -G v_z / (lambda |v|^2) lies beyond 2
    (asserted), so f_min^2 = 4 |v|^2 lambda^2 + 4 G v_z lambda + G^2, decreasing on (0, 1/4]."""
    pieces = Z._deficient_pieces()
    v = [p[1] for p in pieces[2][0]]  # the cubic is p2 + v t (1 - t)^2
    g, vv, vz = Fr(G), sum(x * x for x in v), v[2]
    quad = [g * g - fr(f_lo) ** 2, 4 * g * vz, 4 * vv]
    assert -g * vz / (Fr(1, 4) * vv) > 2 and -4 * g * vz / (8 * vv) > Fr(1, 4)
    lam = Z._bisect(quad, Fr(0), Fr(1, 4))
    return lam, abs(8 * vv * lam + 4 * g * vz)


def check_dilate_ballistic(be, what):
    """f_min = 0.75 G alone on the free-falling arc: thrust G (1 - 1 / s^2) e_z, so s* = 2.  s_lo is
    1 here: below s = sqrt(4/7) the norm passes 0.75 G again (the vehicle pushing downwards), so
    from s_lo = 0.5 the call rightly returns s_lo.  Row 0 holds the arc as its second piece and
    its cubic piece meets the limit later: the larger of the two crossings."""
    (so, T, C), W, ex = zoo_w()
    f_lo, out = 0.75 * G, {}
    b, _ = rows((so, T, C), W, [BALL])
    # f_min = G (1 - 1 / s^2): d f_min / d s = 2 G / s^3
    out[BALL] = _closed(be, what + " arc", *b, one_limit(f_lo=f_lo), 2.0, DR.THRUST_LOW,
                        s_tolerance(DR.THRUST_LOW, 2.0, f_lo, 2 * G / 8.0), s_lo=1.0)
    lam, dq = _cubic_crossing(f_lo)
    want = max(2.0, float(1 / lam) ** 0.5)
    assert want > 2.0  # the cubic's crossing is the later one
    # f_min^2 = q(lambda): d f_min / d s = (dq / (2 f_lo)) (2 / s^3)
    b, _ = rows((so, T, C), W, [DEF4])
    out[DEF4] = _closed(be, what + " row 0", *b, one_limit(f_lo=f_lo), want, DR.THRUST_LOW,
                        s_tolerance(DR.THRUST_LOW, want, f_lo, float(dq) / (2 * f_lo) * 2 / want ** 3), s_lo=1.0)
    return out


def arc_fz_min(T_out, C_out, seg):
    """min over the segment of the thrust's z component of an output row, on the long-double grid."""
    c = np.asarray(C_out[seg, 2], dtype=LD)
    dd = R._deriv(R._deriv(c))
    return float((R._polyval(dd, Z.GRID * LD(T_out[seg])) + LD(G)).min())


def check_free_fall_tilt(be, what):
    """A finite tilt_max alone on the arc, s_lo = 0.5: at s = 1 the thrust vanishes and the tilt is
    undefined.  include/tgms.h: the result is finite, carries no TGMS_FEAS_NONFINITE and is feasible
    with a vanishing thrust counted as upright: f_z >= -1e-9 g along the arc, that is s >= 1 - 1e-9
    (f_z = g (1 - 1 / s^2) >= -1e-9 g gives 1 / s^2 <= 1 + 1e-9, s >= 1 - 0.5e-9)."""
    (so, T, C), W, ex = zoo_w()
    out = {}
    for r, seg in ((BALL, 0), (DEF4, 1)):
        b, _ = rows((so, T, C), W, [r])
        s, act, fl, T_out, C_out = be.dilate(*b, one_limit(tilt=0.5), 0.5, S_HI, G)
        print("%s free fall row %d: s - 1 = %.3g, active %d, flags %#x" % (what, r, s[0] - 1.0, act[0], fl[0]))
        assert np.isfinite(s[0]) and not fl[0] & DR.NONFINITE, (r, s, fl)
        assert s[0] >= 1.0 - TOL, (r, s[0])
        fz = arc_fz_min(T_out, C_out, seg)
        note("%s free fall row %d, -f_z / g on the arc" % (what, r), max(-fz / G, 0.0), TOL)
        assert fz >= -TOL * G, (r, fz)
        assert act[0] == DR.TILT and fl[0] & DR.MASK == 0, (r, act, fl)
        out[r] = (s[0], int(act[0]), int(fl[0] & DR.MASK))
    return out


def grid_quantities(so, T_out, C_out, g=G):
    """dilate_ref.quantities from poly_zoo's long-double grid."""
    gb, gt = Z.grid_bounds(so, T_out, C_out), Z.grid_thrust(so, T_out, C_out, g)
    return np.c_[gb[:, 6:9], gt[:, 1], gt[:, 0], gt[:, 2]]


def contract_batch():
    """cheb, touch and deficient: (so, T, C)."""
    (so, T, C), W, ex = zoo_w()
    return Z.take((so, T, C), [CHEB, TOUCH, PARTNER, DEF4, LIN, BALL, CUBIC, HOLD])


def check_dilate_contract(be, what, grid=False, s_lo=0.75):
    """Feasible and tight of include/tgms.h with all six limits finite, by dilate_ref.check_contract
    (np.roots references of the output) and, with grid, once more by the long-double grid, against
    which the references are first held to poly_zoo.CAP in the contract's own units."""
    so, T, C = contract_batch()
    s, act, fl, T_out, C_out = be.dilate(so, T, C, LIM6, s_lo, S_HI, G)
    assert (fl & DR.MASK == 0).all()
    feas, tight, _ = DR.check_contract(so, T_out, C_out, s, act, fl, LIM6, s_lo, g=G, label=what + " zoo")
    note(what + " dilate contract feasible excess", max(feas, 0.0), TOL)
    note(what + " dilate contract tight deviation", tight, TOL)
    assert (act != DR.NONE).any()
    if grid:
        q, qg = DR.quantities(so, T_out, C_out, G), grid_quantities(so, T_out, C_out, G)
        F = q[:, 3]
        cap = np.c_[np.abs(q[:, 0:3] - qg[:, 0:3]) / np.where(q[:, 0:3] == 0, 1.0, q[:, 0:3]),
                    np.abs(q[:, 3:5] ** 2 - qg[:, 3:5] ** 2) / (F * F)[:, None],
                    np.abs(q[:, 5] - qg[:, 5]) * q[:, 4] / F]
        print("reference cap, dilate output: references vs 65,537-point grid %.3g" % cap.max())
        assert (cap <= Z.CAP).all(), cap
        e = DR.excesses(qg, LIM6)
        assert e.max() <= TOL, e
        col = {DR.SPEED: 0, DR.ACCEL: 1, DR.JERK: 2, DR.THRUST_HIGH: 3, DR.THRUST_LOW: 4, DR.TILT: 5}
        for b in np.flatnonzero(act != DR.NONE):
            d = e[b].copy()
            d[4] = (LIM6[3] - qg[b, 4]) / LIM6[3]
            assert abs(d[col[int(act[b])]]) <= TOL, (b, act[b], d)
    return s, act, fl & DR.MASK


def check_dilate_translation(be):
    """Position enters no limit: scale, active, flags (evaluation count included) and every
    coefficient but c_0 are bit-equal, c_0 is the translated c_0 (c_0 r^0 = c_0 * 1)."""
    (so, T, C), W, ex = zoo_w()
    C2 = Z.translate(C)
    a = be.dilate(so, T, C, LIM6, 0.75, S_HI, G)
    b = be.dilate(so, T, C2, LIM6, 0.75, S_HI, G)
    assert bit_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and bit_equal(a[3], b[3])
    assert bit_equal(a[4][..., 1:], b[4][..., 1:]) and bit_equal(b[4][..., 0], C2[..., 0])


def scaled_limits(lim, k):
    v, a, j, f_lo, f_hi, tilt = lim
    return (np.ldexp(v, -k), np.ldexp(a, -2 * k), np.ldexp(j, -3 * k), np.ldexp(f_lo, -2 * k), np.ldexp(f_hi, -2 * k), tilt)


def check_dilate_rescale(be, k):
    """The same curve flown 2^k times slower with g and the limits scaled to match (all exact: G is
    dyadic).  Kinematic runs: scale bit-equal and seg_times_out the unscaled ones times 2^k.  Thrust
    runs: each run returns the feasible end of a bracket of relative width 2^-41 in lambda (2^-42 in
    s) about a crossing, and each crossing is within the tight clause of s*: |s_k - s_0| <= (2 *
    2^-41 + the closed form's tolerance) s."""
    (so, T, C), W, ex = zoo_w()
    T2, C2 = Z.rescale_time(T, C, k)
    g2 = float(np.ldexp(G, -2 * k))
    for lim in (one_limit(v=1.0), one_limit(a=2.0), one_limit(j=4.0)):
        a = be.dilate(so, T, C, lim, 0.5, S_HI, G)
        b = be.dilate(so, T2, C2, scaled_limits(lim, k), 0.5, S_HI, g2)
        assert bit_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] != DR.NONE).any()
        assert bit_equal(np.ldexp(a[3], k), b[3])
        assert bit_equal(np.ldexp(a[4], -k * np.arange(8)), b[4])
    for r, lim, code, s_lo in ((KP2, one_limit(f_hi=10.0), DR.THRUST_HIGH, 0.5), (KP3, one_limit(tilt=0.25), DR.TILT, 0.5),
                               (BALL, one_limit(f_lo=0.75 * G), DR.THRUST_LOW, 1.0)):
        b0 = Z.take((so, T, C), [r])
        b1 = Z.take((so, T2, C2), [r])
        s0, a0 = be.dilate(*b0, lim, s_lo, S_HI, G)[:2]
        s1, a1 = be.dilate(*b1, scaled_limits(lim, k), s_lo, S_HI, g2)[:2]
        tol = 2 * 2.0 ** -41 + (s_tolerance(code, None, lim[4] if code == DR.THRUST_HIGH else lim[5])
                                if code != DR.THRUST_LOW else s_tolerance(code, 2.0, lim[3], 2 * G / 8.0))
        note("dilate rescale 2^%d row %d, |s_k / s_0 - 1|" % (k, r), abs(s1[0] / s0[0] - 1), tol)
        assert a0[0] == a1[0] == code and abs(s1[0] - s0[0]) <= tol * s0[0]


def _cond(T, C, order):
    """max over a batch's segments and axes of the Horner condition sum of the derivative of that
    order over [0, T]: sum_j j! / (j - order)! |c_j| T^(j - order)."""
    j = np.arange(8)
    fall = np.array([np.prod(np.arange(x - order + 1, x + 1)) if x >= order else 0.0 for x in j])
    p = np.where(j >= order, j - order, 0)
    return (np.abs(C) * fall * np.asarray(T)[:, None, None] ** p).sum(axis=2).max()


def check_dilate_idempotence(be, what):
    """The output fed back under the same single kinematic limit.  The first call leaves the peak
    within 1e-9 relative of the limit, the second one again: s_2^n within (1 +- 1e-9)^2 of 1, so |s_2
    - 1| <= 2e-9 / n <= 2e-9; to that comes the rounding of c_k r^k in the first output (k + 1 <= 8
    roundings of 2^-53 per coefficient), which moves a derivative value by at most 8 * 2^-53 of its
    condition sum: relative to the peak, 8 * 2^-53 cond / peak."""
    (so, T, C), W, ex = zoo_w()
    for n, (name, code) in enumerate((("v", DR.SPEED), ("a", DR.ACCEL), ("j", DR.JERK))):
        for r in (CHEB, KP2, KP3, TOUCH, CUBIC):
            b = Z.take((so, T, C), [r])
            peak = zoo_reference()["bounds"][r, 6 + n]
            lim = one_limit(**{name: peak / 2.0})
            s1, a1, f1, T1, C1 = be.dilate(*b, lim, 0.5, S_HI, G)
            assert a1[0] == code
            tol = 2e-9 + 8 * 2.0 ** -53 * _cond(T1, C1, n + 1) / (peak / 2.0)
            s2, a2, f2, _, _ = be.dilate(b[0], T1, C1, lim, 0.5, S_HI, G)
            note("%s dilate idempotence %s row %d, |s_2 - 1|" % (what, name, r), abs(s2[0] - 1), tol)
            assert a2[0] == code and abs(s2[0] - 1.0) <= tol, (r, name, s2, a2)
            s3, a3, _, _, _ = be.dilate(b[0], T1, C1, lim, 1.0, S_HI, G)
            assert 1.0 <= s3[0] <= 1.0 + tol, (r, name, s3)


def check_dilate_round_trip(be, what):
    """bounds and thrust records of the dilate call's own output: feasible and tight of the header
    with 2e-9 in place of 1e-9 (each call contributes 1e-9)."""
    so, T, C = contract_batch()
    (s, act, fl, T_out, C_out), ext, th = be.dilate_records(so, T, C, LIM6, 0.75, G)
    assert (fl & DR.MASK == 0).all()
    q = np.c_[ext[:, 6:9], th[:, 2], th[:, 0], th[:, 4]]
    e = DR.excesses(q, LIM6)
    note(what + " dilate round trip, feasible excess", max(e.max(), 0.0), 2e-9)
    assert e.max() <= 2e-9, e
    col = {DR.SPEED: 0, DR.ACCEL: 1, DR.JERK: 2, DR.THRUST_HIGH: 3, DR.THRUST_LOW: 4, DR.TILT: 5}
    for b in np.flatnonzero(act != DR.NONE):
        d = e[b].copy()
        d[4] = (LIM6[3] - q[b, 4]) / LIM6[3]
        assert abs(d[col[int(act[b])]]) <= 2e-9, (b, act[b], d)


# =====================================================================================
# B. cut
# =====================================================================================

def cut_times():
    """Per zoo row the list of cut times: 0, every interior knot with its two neighbours, the
    exact extremum times, D and +inf."""
    (so, T, C), W, ex = zoo_w()
    out = []
    for b in range(len(so) - 1):
        k = [float(x) for x in CR.knots(T[so[b]:so[b + 1]])]
        t = [0.0]
        for x in k[1:-1]:
            t += [np.nextafter(x, -INF), x, np.nextafter(x, INF)]
        t += {CHEB: [ex["cheb"]["x_hi_u"] * 2.0], KP2: [ex["kp2"]["t_knot"]], KP3: [ex["kp3"]["t_knot"]],
              TOUCH: [ex["touch"]["t_touch"], 0.5], PARTNER: [ex["touch"]["t_touch"], 0.5]}.get(b, [])
        out.append(t + [k[-1], INF])
    return out


def check_cut_against_ref(be, what, batch=None, W=None, times=None):
    """Every zoo row at every special time against cut_ref.cut (Fraction)."""
    if batch is None:
        batch, W, _ = zoo_w()
    so, T, C = batch
    times = cut_times() if times is None else times
    worst = 0.0
    for n in range(max(len(t) for t in times)):
        tc = np.array([t[n % len(t)] for t in times])
        out = be.cut(so, W, T, C, tc, 0.0)
        ref = CR.cut(so, W, T, C, tc, 0.0)
        CR.compare(out, ref)
        ev = ref["C_tol"] > 0
        if ev.any():
            worst = max(worst, (np.abs(out[4][ev] - ref["C"][ev]) / ref["C_tol"][ev]).max())
    note(what + " cut, shifted coefficients in units of the condition bound", worst, 1.0)


def check_cut_reference_against_longdouble():
    """cut_ref's Fraction values against a long-double Horner evaluation of the same state, to
    poly_zoo.CAP of the condition sum."""
    (so, T, C), W, ex = zoo_w()
    for b, t in ((CHEB, 0.7), (TOUCH, 0.5), (KP2, 1.25), (CUBIC, 0.375)):
        c = C[so[b]]
        for ax in range(3):
            val, cond = CR.shifted(c[ax], t)
            p = np.asarray(c[ax], dtype=LD)
            for k in range(4):
                got = R._polyval(p, LD(t)) / LD(np.prod(np.arange(1, k + 1)))
                assert abs(float(got - LD(float(val[k])))) <= Z.CAP * cond[k] + 1e-300, (b, ax, k)
                p = R._deriv(p)


def check_cut_knot_peak(be):
    """A cut exactly on the knot that is also the extremum: it belongs to the later segment at local
    time 0, nothing is evaluated."""
    (so, T, C), W, ex = zoo_w()
    for r, key in ((KP2, "kp2"), (KP3, "kp3")):
        b, Wb = rows((so, T, C), W, [r])
        seg = ex[key]["seg"] + 1  # the mirrored segment
        so2, W2, T2, ED2, C2, parent, t0, fl = be.cut(b[0], Wb, b[1], b[2], np.array([ex[key]["t_knot"]]), 0.0)
        assert fl[0] == CR.DONE and list(so2) == [0, 1] and parent[0] == seg
        assert t0[0] == ex[key]["t_knot"] and bit_equal(T2, b[1][seg:])  # t_loc == 0: the time is copied
        assert bit_equal(W2[0], Wb[seg]) and bit_equal(W2[1], Wb[seg + 1])
        ed = ED2.reshape(-1)
        assert (ed[0:3] == 0.0).all() and ed[3] == -ACC and (ed[4:6] == 0.0).all()  # v = 0, a = (acc, 0, 0) exactly
        assert (ed[9:18] == 0.0).all()
        assert bit_equal(C2[0], b[2][seg])


def check_cut_deficient(be):
    """Cuts inside every piece of the deficient rows: a shifted coefficient above the piece's true
    degree is exactly 0.0 (its condition sum is 0), the hold piece returns its constant bit for
    bit."""
    (so, T, C), W, ex = zoo_w()
    deg = {0: 1, 1: 2, 2: 3, 3: 0}
    for r, pieces in ((DEF4, (0, 1, 2, 3)), (LIN, (0,)), (BALL, (1,)), (CUBIC, (2,)), (HOLD, (3,))):
        b, Wb = rows((so, T, C), W, [r])
        k = CR.knots(b[1])
        for i, piece in enumerate(pieces):
            tc = np.array([float(k[i]) + 0.375 * b[1][i]])
            out = be.cut(b[0], Wb, b[1], b[2], tc, 0.0)
            CR.compare(out, CR.cut(b[0], Wb, b[1], b[2], tc, 0.0))
            c = out[4][0]
            assert (c[:, deg[piece] + 1:] == 0.0).all() and not np.signbit(c[:, deg[piece] + 1:]).any(), (r, piece, c)
            if piece == 3:
                assert bit_equal(c, b[2][i]) and bit_equal(out[1][0], Wb[i])


def compose_times():
    """(t1, t2) per zoo row, t1 < t2 in one segment (the first), and in the first and the last
    (M = 1: the one segment again).  Multiples of 2^-10: every knot sum and difference is exact."""
    (so, T, C), W, ex = zoo_w()
    same, two = [], []
    for b in range(len(so) - 1):
        Tb = T[so[b]:so[b + 1]]
        k = [float(x) for x in CR.knots(Tb)]
        same.append((Tb[0] / 4, Tb[0] / 2))
        two.append((Tb[0] / 4, k[-2] + Tb[-1] / 2))
    return np.array(same), np.array(two)


def check_cut_composition(be, what):
    """cut(t1) then cut(t2 - t0_out) against cut(t2).  The second call shifts coefficients that
    carry the first call's error e_j <= 1e-9 cond1_j; a shift by t' maps it to sum_j C(j, k) e_j
    t'^(j - k), and adds its own 1e-9 cond2_k: the sum of the two calls' condition bounds."""
    (so, T, C), W, ex = zoo_w()
    for times in compose_times():
        t1, t2 = times[:, 0], times[:, 1]
        a = be.cut(so, W, T, C, t1, 0.0)
        ra = CR.cut(so, W, T, C, t1, 0.0)
        CR.compare(a, ra)
        t_rel = t2 - a[6]
        assert (t_rel + a[6] == t2).all()  # exact
        bb = be.cut(a[0], a[1], a[2], a[4], t_rel, 0.0, a[3])
        rb = CR.cut(a[0], a[1], a[2], a[4], t_rel, 0.0, a[3])
        rd = CR.cut(so, W, T, C, t2, 0.0)
        assert np.array_equal(bb[0], rd["so"]) and np.array_equal(a[5][bb[5]], rd["parent"])
        assert np.array_equal(bb[7] & ~CR.SNAPPED, rd["flags"] & ~CR.SNAPPED)
        assert bit_equal(bb[2], rd["T"])
        D = np.array([float(CR.knots(T[so[b]:so[b + 1]])[-1]) for b in range(len(so) - 1)])
        assert (np.abs(a[6] + bb[6] - rd["t0"]) <= 2 * np.spacing(D)).all()
        copy = rd["C_tol"] == 0.0
        assert np.array_equal(CR.bits(bb[4])[copy], CR.bits(rd["C"])[copy])
        worst = 0.0
        for b in range(len(so) - 1):
            s2 = bb[0][b]  # the row's first output segment: the shifted one
            first = ra["so"][b]
            for ax in range(3):
                e1 = ra["C_tol"][first, ax] if rb["s"][b] == 0 else np.zeros(8)
                tl = float(rb["t_loc"][b])
                prop = np.array([sum(comb(j, k) * e1[j] * tl ** (j - k) for j in range(k, 8)) for k in range(8)])
                tol = prop + rb["C_tol"][s2, ax]
                err = np.abs(bb[4][s2, ax] - rd["C"][s2, ax])
                assert (err <= tol).all(), (b, ax, err, tol)
                worst = max(worst, (err[tol > 0] / tol[tol > 0]).max() if (tol > 0).any() else 0.0)
        note(what + " cut composition, in units of the two calls' bounds", worst, 1.0)


def check_cut_translation(be):
    """The translated zoo meets the reference; everything that holds no position is bit-equal to the
    untranslated call (the Horner chains of p', p'', p''' and of the higher shifted coefficients
    never read c_0)."""
    (so, T, C), W, ex = zoo_w()
    d = np.asarray(Z.SHIFT)
    C2, W2 = Z.translate(C, d), W + d
    times = cut_times()
    for n in (1, 2, 4):
        tc = np.array([t[n % len(t)] for t in times])
        a = be.cut(so, W, T, C, tc, 0.0)
        b = be.cut(so, W2, T, C2, tc, 0.0)
        ra, rb = CR.cut(so, W, T, C, tc, 0.0), CR.cut(so, W2, T, C2, tc, 0.0)
        CR.compare(b, rb)
        for i in (0, 2, 3, 5, 6, 7):
            assert np.array_equal(CR.bits(a[i]), CR.bits(b[i])), i
        assert bit_equal(a[4][..., 1:], b[4][..., 1:])
        assert (np.abs(b[4][..., 0] - (a[4][..., 0] + d)) <= ra["C_tol"][..., 0] + rb["C_tol"][..., 0]
                + np.spacing(np.abs(d))).all()
        assert (np.abs(b[1] - (a[1] + d)) <= ra["W_tol"] + rb["W_tol"] + np.spacing(np.abs(d))).all()


def check_cut_rescale(be, k):
    """A Horner chain scales exactly by powers of two (products and fused products alike), so every
    output of the rescaled call is ldexp of the unscaled one; no zoo value leaves the normal range."""
    (so, T, C), W, ex = zoo_w()
    T2, C2 = Z.rescale_time(T, C, k)
    nz = np.abs(C2[C2 != 0.0])
    assert nz.min() > 2.0 ** -900 and nz.max() < 2.0 ** 900
    times = cut_times()
    for n in (2, 4, 5):
        tc = np.array([t[n % len(t)] for t in times])
        a = be.cut(so, W, T, C, tc, 0.0)
        b = be.cut(so, W, T2, C2, np.ldexp(tc, k), 0.0)
        for i in (0, 1, 5, 7):
            assert np.array_equal(CR.bits(a[i]), CR.bits(b[i])), i
        assert bit_equal(np.ldexp(a[2], k), b[2]) and bit_equal(np.ldexp(a[6], k), b[6])
        assert bit_equal(np.ldexp(a[4], -k * np.arange(8)), b[4])
        ed = np.ldexp(a[3].reshape(-1, 2, 3, 3), -k * np.arange(1, 4)[None, None, :, None])
        assert bit_equal(ed, b[3].reshape(-1, 2, 3, 3))


def check_cut_round_trips(be, what):
    """The cut's output straight into the analysis call that a planner runs next."""
    (so, T, C), W, ex = zoo_w()
    ref = zoo_reference()
    # cheb before its maximum: pmax_x is still the exact one
    b, Wb = rows((so, T, C), W, [CHEB])
    t_hi = ex["cheb"]["x_hi_u"] * 2.0
    out, ext = be.cut_then(b[0], Wb, b[1], b[2], np.array([t_hi / 2]), "bounds")
    pm = np.abs(ref["bounds"][CHEB, 0:6]).max()
    e = abs(ext[0, 3] - ex["cheb"]["pmax"][0]) / pm
    note(what + " cut -> bounds, cheb before the maximum, x max|p|", e, TOL)
    assert e <= TOL
    # after it: the grid maximum of the tail, strictly below
    t_c = (t_hi + 2.0) / 2
    a = Z._axis_u(C[so[CHEB], 0], 2.0)
    tail = float(Z.grid_max(lambda u: R._polyval(a, u), LD(t_c) / 2, LD(1)))
    assert tail < ex["cheb"]["pmax"][0] - 1e-3
    out, ext = be.cut_then(b[0], Wb, b[1], b[2], np.array([t_c]), "bounds")
    e = abs(ext[0, 3] - tail) / pm
    note(what + " cut -> bounds, cheb after the maximum, x max|p|", e, TOL)
    assert e <= TOL
    # knot_peak(3) cut inside its hold: the knot's thrust extremes survive
    b, Wb = rows((so, T, C), W, [KP3])
    out, th = be.cut_then(b[0], Wb, b[1], b[2], np.array([0.375]), "thrust")
    F, m = ex["kp3"]["f_max"], G
    assert abs(th[0, 2] ** 2 - F * F) <= TOL * F * F and abs(th[0, 4] - ex["kp3"]["tilt_max"]) <= TOL * F / m
    assert th[0, 3] == ex["kp3"]["t_knot"] - out[6][0] and th[0, 5] == th[0, 3]  # on the new clock, still the knot
    # the touch pair, both cut at 0.5: d^2 = (t - 1)^4 / 64 on the old clock
    b, Wb = rows((so, T, C), W, [TOUCH, PARTNER])
    pairs = np.array([[0, 1]], np.int32)
    L = np.abs(ref["bounds"][[TOUCH, PARTNER], 0:6]).max()
    out, sep = be.cut_then(b[0], Wb, b[1], b[2], np.array([0.5, 0.5]), "separation", pairs=pairs)
    assert (out[6] == 0.5).all()
    note(what + " cut -> separation, the touch, d_min^2 / L^2", sep[0, 0] ** 2 / L ** 2, TOL)
    assert sep[0, 0] ** 2 <= TOL * L * L
    # dist(t_min)^2 within 1e-9 L^2 of d_min^2 <= 1e-9 L^2: (t - 1)^4 / 64 <= 2e-9 L^2
    assert abs(sep[0, 1] - 1.0) <= (64 * 2 * TOL * L * L) ** 0.25, sep
    # both cut at 1.5, after the touch: d grows from there on, the minimum is d(1.5) = 1 / 32
    trajs = __import__("separation_ref").batch_trajs(b[0], b[1], b[2])
    dist = lambda t: np.sqrt(((trajs[0].pos(t) - trajs[1].pos(t)) ** 2).sum(axis=1))  # noqa: E731
    d2 = float(Z.grid_min(lambda t: dist(t) ** 2, LD(1.5), LD(2.0)))
    assert d2 ** 0.5 > 1e-3 and abs(d2 - 2.0 ** -10) <= Z.CAP
    out, sep = be.cut_then(b[0], Wb, b[1], b[2], np.array([1.5, 1.5]), "separation", pairs=pairs)
    e = abs(sep[0, 0] ** 2 - d2) / L ** 2
    note(what + " cut -> separation, after the touch, x L^2", e, TOL)
    assert e <= TOL and 1.5 <= sep[0, 1] <= 2.0


# =====================================================================================
# C. split
# =====================================================================================

FAR = 128.0


def box_faces(d):
    """Six faces: x <= d and five far ones."""
    return np.array([[1.0, 0.0, 0.0, d], [-1.0, 0.0, 0.0, FAR], [0.0, 1.0, 0.0, FAR], [0.0, -1.0, 0.0, FAR],
                     [0.0, 0.0, 1.0, FAR], [0.0, 0.0, -1.0, FAR]])


def per_segment(faces, S):
    return np.tile(faces, (S, 1)), len(faces) * np.arange(S + 1, dtype=np.int64)


def _run_split(be, so, W, T, C, faces, fo, r, mode, min_frac=0.1, seg=None):
    from test_split_host import compare
    if seg is None:
        seg = be.corridor(so, T, C, faces, fo, r)[2:4]
    out = be.split(so, W, T, C, faces, fo, seg[0], seg[1], r, mode, min_frac)
    ref = SR.split(so, W, T, C, faces, fo, seg[0], seg[1], r, mode, min_frac)
    compare(out, ref)  # the bit rules, and inserted waypoints to 1e-9 L of the long-double value
    return out, ref, seg


def time_tolerance(Lh, d2, d3):
    """How far the time of a smooth maximum may lie from the exact one when the stored margin is
    within 1e-9 L_h of the true maximum: m(t* + dt) = m* - |m''| dt^2 / 2 + m''' dt^3 / 6, so dt <=
    sqrt(2e-9 L_h / |m''|) to second order; the factor 1.5 covers the cubic term, which the assert
    holds below a third of the quadratic one."""
    dt = (2 * TOL * Lh / abs(d2)) ** 0.5
    assert abs(d3) * (1.5 * dt) / 3 <= abs(d2) / 3
    return 1.5 * dt


def check_split_cheb(be, what, mode):
    """The worst excursion inside a degree-7 segment at a time known exactly."""
    (so, T, C), W, ex = zoo_w()
    b, Wb = rows((so, T, C), W, [CHEB])
    X = ex["cheb"]["pmax"][0]
    d = np.floor((X - 2.0 ** -6) * 64) / 64  # a dyadic step below the maximum
    faces, fo = per_segment(box_faces(d), 1)
    out, ref, seg = _run_split(be, *b[:1], Wb, b[1], b[2], faces, fo, 0.0, mode)
    so2, W2, T2, f2, fo2, parent, fl = out
    assert list(so2) == [0, 2] and list(parent) == [0, 0] and fl[0] == SR.DONE and seg[1][0] == 0
    px = [fr(x) for x in b[2][0, 0]]
    t_x = ex["cheb"]["x_hi_u"] * 2.0
    d2, d3 = (float(Z._val(Z._der(Z._der(px)), fr(t_x))), float(Z._val(Z._der(Z._der(Z._der(px))), fr(t_x))))
    Lh = np.abs(ref["L"][0]) + abs(d)
    tol = time_tolerance(Lh, d2, d3)
    note("%s split cheb mode %d, |T_left - t_x|" % (what, mode), abs(T2[0] - t_x), tol)
    assert abs(T2[0] - t_x) <= tol and T2[0] == seg[0][0, 1]
    assert abs((T2[0] + T2[1]) - 2.0) <= np.spacing(2.0)
    p = np.array([float(Z._val([fr(x) for x in b[2][0, ax]], fr(T2[0]))) for ax in range(3)])
    if mode == SR.PULL:
        assert p[0] > d
        p[0] = d  # pulled back along -e_x to the face
        assert abs(W2[1, 0] - d) <= TOL * Lh  # test_split_host.check_pull_lands_on_the_face's bound
    else:
        p = Wb[0] + (T2[0] / 2.0) * (Wb[1] - Wb[0])
    e = np.abs(W2[1] - p).max() / ref["L"][0]
    note("%s split cheb mode %d, inserted waypoint x L" % (what, mode), e, TOL)
    assert e <= TOL
    return out


def check_split_knot_peak(be, what):
    """The worst excursion exactly on an interior knot, u = 1 of one segment and u = 0 of the
    next: neither is split, whatever the depth of the face.  (The worst excursion of these rows is
    on the knot for every face x <= d, so no face moves it inside; the second half feeds the split
    a corridor row whose time lies 0.3 T inside the segment, which is then split at the reference's
    place.)"""
    (so, T, C), W, ex = zoo_w()
    for r, key in ((KP2, "kp2"), (KP3, "kp3")):
        b, Wb = rows((so, T, C), W, [r])
        M = int(b[0][1])
        for depth in (2.0 ** -6, 0.75):
            faces, fo = per_segment(box_faces(ex[key]["pmax_x"] - depth), M)
            out, ref, seg = _run_split(be, b[0], Wb, b[1], b[2], faces, fo, 0.0, SR.PULL)
            assert out[6][0] == SR.AT_END and np.array_equal(out[0], b[0]) and bit_equal(out[1], Wb)
            assert bit_equal(out[2], b[1]) and np.array_equal(out[4], fo) and np.array_equal(out[5], np.arange(M))
            s = ex[key]["seg"]
            assert (seg[0][[s, s + 1], 0] > 0).all() and seg[0][s, 1] == ex[key]["t_knot"] == seg[0][s + 1, 1]
        rec = seg[0].copy()
        rec[s, 1] = ex[key]["t_knot"] - 0.3 * b[1][s]
        out, ref, _ = _run_split(be, b[0], Wb, b[1], b[2], faces, fo, 0.0, SR.PULL, seg=(rec, seg[1]))
        assert out[6][0] == SR.DONE | SR.AT_END and list(out[5]) == sorted(list(range(M)) + [s])
        assert out[2][s] == np.float64(rec[s, 1]) - np.float64(ex[key]["t_knot"] - b[1][s])


def check_split_deficient(be, what, mode):
    """Row 0 against x <= 1/4: the constant-velocity piece and the arc cross it with the worst
    point at their ends, the hold is constant (its worst time is its start): none of the three is
    split.  The cubic x = 5/4 + t (1 - t)^2 has its stationary maximum at t = 1/3 exactly."""
    (so, T, C), W, ex = zoo_w()
    b, Wb = rows((so, T, C), W, [DEF4])
    faces, fo = per_segment(box_faces(0.25), 4)
    out, ref, seg = _run_split(be, b[0], Wb, b[1], b[2], faces, fo, 0.0, mode)
    so2, W2, T2, f2, fo2, parent, fl = out
    assert fl[0] == SR.DONE | SR.AT_END and list(parent) == [0, 1, 2, 2, 3] and (seg[0][:, 0] > 0).all()
    Lh = ref["L"][2] + 0.25
    tol = time_tolerance(Lh, -2.0, 6.0)  # x'' = -4 + 6 t = -2 at 1/3, x''' = 6
    note("%s split deficient mode %d, |T_left - 1/3|" % (what, mode), abs(T2[2] - 1.0 / 3.0), tol)
    assert abs(T2[2] - 1.0 / 3.0) <= tol
    p = np.array([float(Z._val([fr(x) for x in b[2][2, ax]], fr(T2[2]))) for ax in range(3)])
    if mode == SR.PULL:
        p[0] = 0.25
    else:
        p = Wb[2] + (T2[2] / b[1][2]) * (Wb[3] - Wb[2])
    assert np.abs(W2[3] - p).max() <= TOL * ref["L"][2]
    return out


def check_split_round_trip(be, what, mode):
    """Split, solve, corridor on the split's own faces and offsets: the new trajectory passes through
    the inserted waypoint (test_split_host.check_round_trip's bounds: 1e-9 scale at a segment's
    start, 8e-9 scale at its end), and in PULL mode its excursion at the inserted knot is at most
    the pulled point's bound plus that of the solve."""
    from trajectory_generator_ros2_amd import FEAS_NONFINITE
    for check, row_seg in ((check_split_cheb, 0), (check_split_deficient, 2)):
        so2, W2, T2, f2, fo2, parent, fl = check(be, what, mode)
        C2, st, worst = be.solve(so2, W2, T2, None)
        assert worst == 0 and not st.any()
        rws = np.arange(len(T2))
        end = (C2 * T2[:, None, None] ** np.arange(8)).sum(axis=2)
        scale = max(np.abs(W2).max(), 1.0)
        assert np.abs(C2[:, :, 0] - W2[rws]).max() <= 1e-9 * scale and np.abs(end - W2[rws + 1]).max() <= 8e-9 * scale
        rec, where, seg_rec, seg_face, cfl = be.corridor(so2, T2, C2, f2, fo2, 0.0)
        assert not (cfl & FEAS_NONFINITE).any()
        if mode == SR.PULL:
            child = row_seg + 1  # the right child starts at the inserted waypoint
            f = f2[fo2[child]]
            m = f[:3] @ C2[child, :, 0] - f[3]
            Lh = np.abs(f[:3]).sum() * scale + abs(f[3])
            note("%s split round trip, excursion at the inserted knot / L_h" % what, max(m, 0.0) / Lh, 2e-9)
            assert m <= 1e-9 * Lh + 1e-9 * scale
