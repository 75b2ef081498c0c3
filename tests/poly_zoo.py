"""Constructed polynomials for the continuous-analysis calls (tgms_bounds_*, tgms_thrust_*,
tgms_rate_*, tgms_corridor_*, tgms_separation_*, tgms_neighbors_*, tgms_clearance_*), shared by
test_poly_zoo_host.py and test_gpu_poly_zoo.py.  The contract tests of those calls feed them
min-snap solutions, which are generic polynomials; the builders here make the input a planner
also produces and a generic solve never does:
    cheb        every interval of a ladder level holds a root, extents attained four times
    deficient   hold, constant velocity, ballistic arc, cubic: trailing zero coefficients
    knot_peak   the extremum exactly on an interior knot (u = 1 of one segment, u = 0 of the next)
    touch       a double root of the derivative (no sign change) beside a true minimum
and the transforms a planner applies: a translation large against the motion, a time rescale by
a power of two, start times on a wall clock.
Every coefficient is built in fractions.Fraction and asserted to be exactly representable, so
the fp64 input IS the polynomial the exact answers belong to.  A builder returns
(so, T, C, exact); `exact` maps a name to the exact answer rounded once to fp64.

The second half is the grid every *_ref.py reference is held against before a case may use it
(grid_*): 65,537 uniform points per piece in np.longdouble.  The grid's own value is short of a
smooth extremum by up to Q'' h^2 / 8 (1e-7 for a degree-7 Chebyshev polynomial), so each local
extremum of the grid is refined by a golden-section search on its bracket, again on the quantity
itself and in np.longdouble: no derivative, no root-finder, no np.roots."""
import math
from fractions import Fraction as Fr

import numpy as np

import bounds_ref as R
import thrust_ref as TR

LD = np.longdouble
G = 9.8125  # m/s^2, dyadic: g T^2 and g 2^(-2k) stay exact
SHIFT = (2.0 ** 14, -(2.0 ** 15), 2.0 ** 12)
RESCALES = (-10, -4, 4, 10)
CLOCKS = (2.0 ** 20, 1700000000.0)
CAP = 1e-10  # a reference may differ from the grid by this much, in the contract's own unit


# ---- exact polynomial arithmetic (ascending lists of Fraction) ----

def _mul(p, q):
    out = [Fr(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def _add(p, q):
    n = max(len(p), len(q))
    return [(p[i] if i < len(p) else 0) + (q[i] if i < len(q) else 0) for i in range(n)]


def _scale(p, k):
    return [Fr(k) * a for a in p]


def _der(p):
    return [j * p[j] for j in range(1, len(p))]


def _integrate(p, c0):
    return [Fr(c0)] + [p[j] / (j + 1) for j in range(len(p))]


def _val(p, u):
    s = Fr(0)
    for a in reversed(p):
        s = s * u + a
    return s


def _compose_mirror(p):
    """p(1 - u)."""
    out, w = [Fr(0)], [Fr(1)]
    for a in p:
        out = _add(out, _scale(w, a))
        w = _mul(w, [Fr(1), Fr(-1)])
    return out


def cheb_shifted(n):
    """T_n*(u) = T_n(2 u - 1): integer coefficients, n + 1 extrema of +-1 on [0, 1]."""
    x = [Fr(-1), Fr(2)]
    a, b = [Fr(1)], x
    for _ in range(n - 1):
        a, b = b, _add(_scale(_mul(x, b), 2), _scale(a, -1))
    return b if n else a


def _bisect(p, lo, hi, steps=110):
    """The root of p in [lo, hi] (a sign change) to 2^-steps, as a Fraction."""
    flo = _val(p, lo)
    assert flo * _val(p, hi) < 0
    for _ in range(steps):
        m = (lo + hi) / 2
        if (_val(p, m) < 0) == (flo < 0):
            lo = m
        else:
            hi = m
    return (lo + hi) / 2


def _row(axes_u, T):
    """One segment [3, 8] from three polynomials in u = t / T: c_j = a_j / T^j, asserted exact."""
    c = np.zeros((3, 8))
    for ax, p in enumerate(axes_u):
        assert len(p) <= 8
        for j, a in enumerate(p):
            cj = a / Fr(T) ** j
            c[ax, j] = float(cj)
            assert Fr(c[ax, j]) == cj, (ax, j, cj)  # exactly representable
    return c


def _in_t(c_row):
    """A segment row back as three Fraction polynomials in t."""
    return [[Fr(float(x)) for x in c_row[ax]] for ax in range(3)]


def _csr(rows):
    """(so, T, C) of a list of trajectories, each a list of (c [3,8], T)."""
    so = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    T = np.array([float(s[1]) for r in rows for s in r])
    C = np.stack([s[0] for r in rows for s in r])
    assert (T * 256 == np.round(T * 256)).all()  # multiples of 2^-8: every knot sum is exact
    return so, T, C


def concat(*batches):
    """CSR concatenation of (so, T, C) batches."""
    so = [np.zeros(1, np.int32)]
    for b in batches:
        so.append(so[-1][-1] + np.asarray(b[0][1:], np.int32))
    return (np.concatenate(so).astype(np.int32), np.concatenate([np.asarray(b[1]).reshape(-1) for b in batches]),
            np.concatenate([np.asarray(b[2]).reshape(-1, 3, 8) for b in batches]))


def take(batch, rows):
    """The trajectories `rows` of a CSR batch, in that order."""
    so, T, C = batch
    segs = np.concatenate([np.arange(so[b], so[b + 1]) for b in rows])
    so2 = np.concatenate([[0], np.cumsum(np.diff(so)[list(rows)])]).astype(np.int32)
    return so2, np.asarray(T)[segs], np.asarray(C)[segs]


# ---- 1. cheb ----

def cheb():
    """M = 1, T = 2.  x'(u) = (105/8) T6*(u), integrated from x(0) = 1: six stationary points in
    (0, 1), alternating, so every interval of every level of the degree-6 ladder holds a root.
    y = T7*(u): extents exactly -1 and +1, each attained four times.  z = 2 + T5*(u) / 4.
    exact: pmin, pmax (x from the roots of T6* bracketed to 2^-110 in Fraction; y and z known),
    x_hi_u (where x is largest)."""
    T = 2
    dx = _scale(cheb_shifted(6), Fr(105, 8))
    x = _integrate(dx, 1)
    y = cheb_shifted(7)
    z = _add([Fr(2)], _scale(cheb_shifted(5), Fr(1, 4)))
    roots = [(1 + Fr(math.cos((2 * i - 1) * math.pi / 12))) / 2 for i in range(6, 0, -1)]  # approximate, ascending
    cuts = [Fr(0)] + [(roots[i] + roots[i + 1]) / 2 for i in range(5)] + [Fr(1)]
    st = [_bisect(dx, cuts[i], cuts[i + 1]) for i in range(6)]
    signs = [_val(dx, c) > 0 for c in cuts]
    assert all(signs[i] != signs[i + 1] for i in range(6))  # they alternate: six simple roots inside
    cand = [Fr(0), Fr(1)] + st
    xv = [_val(x, u) for u in cand]
    hi = max(range(8), key=lambda i: xv[i])
    assert hi >= 2 and min(xv) < min(xv[0], xv[1])  # both x extents are interior stationary points
    exact = dict(pmin=np.array([float(min(xv)), -1.0, 1.75]), pmax=np.array([float(max(xv)), 1.0, 2.25]),
                 x_hi_u=float(cand[hi]))
    return _csr([[(_row([x, y, z], T), T)]]) + (exact,)


# ---- 2. deficient ----

def _deficient_pieces():
    """[(axes in t, T)]: constant velocity, ballistic, cubic to rest, hold; C1 at the knots."""
    v0 = [Fr(1), Fr(1, 2), Fr(2)]
    p0 = [Fr(0), Fr(0), Fr(2)]
    g = Fr(G)
    out = []
    Ta = Fr(1, 2)
    out.append(([[p0[a], v0[a]] for a in range(3)], Ta))
    p1 = [p0[a] + v0[a] * Ta for a in range(3)]
    Tb = Fr(3, 4)
    acc = [Fr(0), Fr(0), -g]
    out.append(([[p1[a], v0[a], acc[a] / 2] for a in range(3)], Tb))
    p2 = [p1[a] + v0[a] * Tb + acc[a] * Tb * Tb / 2 for a in range(3)]
    v2 = [v0[a] + acc[a] * Tb for a in range(3)]
    Tc = Fr(1)
    out.append(([[p2[a], v2[a], -2 * v2[a], v2[a]] for a in range(3)], Tc))  # p2 + v t (1 - t)^2: p'(1) = 0
    p3 = [_val(out[-1][0][a], Tc) for a in range(3)]
    out.append(([[p3[a]] for a in range(3)], Fr(1, 4)))
    return out


def _piece_exact(axes, T):
    """Exact (lo[3], hi[3], v2, a2, j2, fmin2, fmax2) of one piece of degree <= 3 on [0, T]: the
    extents from the rational stationary points, the squared peaks and squared thrusts from the
    rational stationary points of quadratics in t."""
    g = Fr(G)
    lo, hi = [], []
    for p in axes:
        cand = [Fr(0), T]
        d = _der(p) + [Fr(0)] * 3
        a, b, c = d[2], d[1], d[0]  # p' = a t^2 + b t + c
        if a != 0:
            disc = b * b - 4 * a * c
            r = Fr(math.isqrt(disc.numerator), math.isqrt(disc.denominator))
            assert r * r == disc  # the builder's cubics have rational stationary points
            cand += [(-b + r) / (2 * a), (-b - r) / (2 * a)]
        elif b != 0:
            cand.append(-c / b)
        vals = [_val(p, t) for t in cand if 0 <= t <= T]
        lo.append(min(vals))
        hi.append(max(vals))

    def peak2(polys):
        """max over [0, T] of sum_a polys[a](t)^2, every polys[a] of degree <= 2.  Candidates: the
        ends and the axes' own stationary points (a sum of squares of k_a w(t) is stationary
        where w is; where the axes are linear the sum is convex and an end wins).  Held against a
        rational mesh of 513 points so that a missed stationary point cannot pass."""
        sq = [Fr(0)]
        for p in polys:
            sq = _add(sq, _mul(p, p))
        cand = [Fr(0), T]
        for p in polys:
            dp = _der(p) + [Fr(0)] * 2
            if dp[1] != 0:
                cand.append(-dp[0] / dp[1])
        best = max(_val(sq, t) for t in cand if 0 <= t <= T)
        assert best >= max(_val(sq, T * Fr(i, 512)) for i in range(513))
        return best

    d1 = [_der(p) or [Fr(0)] for p in axes]
    d2 = [_der(p) or [Fr(0)] for p in d1]
    d3 = [_der(p) or [Fr(0)] for p in d2]
    f = [list(p) for p in d2]
    f[2] = _add(f[2], [g])
    return lo, hi, peak2(d1), peak2(d2), peak2(d3), f


def deficient():
    """Row 0: M = 4, true degrees 1, 2, 3, 0 (constant velocity, a ballistic arc with a = (0, 0,
    -G), a cubic that comes to rest, a hold), C1 at the knots.  Rows 1..4: the same pieces as four
    M = 1 trajectories.  exact: ext [5, 9] (the bounds record), fmin2 / fmax2 [5] (the squared
    thrust extremes; on the cubic f = v s + G e_z with s = -4 + 6 t, a quadratic in s)."""
    pieces = _deficient_pieces()
    rows = [[(_row(axes, 1), T) for axes, T in pieces]] + [[(_row(axes, 1), T)] for axes, T in pieces]
    g = Fr(G)
    per = []
    for axes, T in pieces:
        lo, hi, v2, a2, j2, f = _piece_exact(axes, T)
        # |f|^2 along the piece: constant (degree <= 2) or a quadratic in s = -4 + 6 t on [-4, 2]
        if all(len([a for a in p[1:] if a != 0]) == 0 for p in f):
            fmin2 = fmax2 = sum(p[0] * p[0] for p in f)
        else:
            v = [p[1] / 6 for p in f]  # f_a = -4 v_a + [a == z] g + 6 v_a t
            vv, vz = sum(x * x for x in v), v[2]
            q = lambda s: vv * s * s + 2 * g * vz * s + g * g  # noqa: E731
            s_star = -g * vz / vv
            assert -4 < s_star < 2
            fmin2, fmax2 = q(s_star), max(q(Fr(-4)), q(Fr(2)))
        per.append((lo, hi, v2, a2, j2, fmin2, fmax2))

    def rec(ps):
        lo = [min(p[0][a] for p in ps) for a in range(3)]
        hi = [max(p[1][a] for p in ps) for a in range(3)]
        ext = [float(x) for x in lo + hi] + [math.sqrt(max(p[k] for p in ps)) for k in (2, 3, 4)]
        return ext, math.sqrt(min(p[5] for p in ps)), math.sqrt(max(p[6] for p in ps))

    recs = [rec(per)] + [rec([p]) for p in per]
    exact = dict(ext=np.array([r[0] for r in recs]), f_min=np.array([r[1] for r in recs]),
                 f_max=np.array([r[2] for r in recs]), low_degree=np.array([1, 2, 4]),  # M = 1 rows of degree <= 2
                 ballistic=2, low_segments=np.array([0, 1, 3, 4, 5, 7]))
    return _csr(rows) + (exact,)


# ---- 3. knot_peak ----

def knot_peak(M):
    """M = 2: q then q mirrored, T = 2 each.  M = 3: a hold of 0.75 s at q(0) first.  q'(u) =
    (105/256) (1 - u) (1 + u)^5 > 0 on [0, 1): x rises to its strict maximum q(1) exactly on the
    knot, u = 1 of one segment and u = 0 of the next.  q''(u) ~ (1 + u)^4 (4 - 6 u): |q''| is
    largest, 32 k, at the knot as well, so with y and z constant f_max and tilt_max sit there too.
    exact: pmax_x, seg (the lowest segment attaining it), t_knot (its prefix sum), f_max, tilt_max."""
    assert M in (2, 3)
    T, k = 2, Fr(105, 256)
    w = [Fr(1)]
    for _ in range(5):
        w = _mul(w, [Fr(1), Fr(1)])
    dq = _scale(_mul([Fr(1), Fr(-1)], w), k)
    q = _integrate(dq, Fr(-1, 2))
    qm = _compose_mirror(q)
    y, z = [Fr(3, 4)], [Fr(3, 2)]
    segs = [(_row([q, y, z], T), T), (_row([qm, y, z], T), T)]
    if M == 3:
        segs.insert(0, (_row([[q[0]], y, z], 1), Fr(3, 4)))
    top = _val(q, Fr(1))
    assert qm[0] == top and all(_val(q, Fr(i, 64)) < top for i in range(64))
    acc = _val(_der(dq), Fr(1)) / (T * T)  # q''(1) / T^2 = -32 k / 4
    exact = dict(pmax_x=float(top), seg=M - 2, t_knot=float(Fr(3, 4) * (M - 2) + T),
                 f_max=math.sqrt(float(acc * acc + Fr(G) ** 2)), tilt_max=math.atan2(abs(float(acc)), G))
    return _csr([segs]) + (exact,)


# ---- 4. touch ----

def touch():
    """Row 0: M = 1, T = 2, x'(u) = 12 (u - 1/2)^2 (u - 1/4): a true minimum at 1/4, an inflection
    (a touch of the derivative without a sign change) at 1/2; y = u / 2, z = 1.  Row 1: the
    partner for the separation call, row 0 with y + (u - 1/2)^2 / 2: d^2 = (u - 1/2)^4 / 4, one
    touch at a quadruple root.  exact: pmin_x, pmax_x, t_touch."""
    T = 2
    h = [Fr(-1, 2), Fr(1)]
    dx = _scale(_mul(_mul(h, h), [Fr(-1, 4), Fr(1)]), 12)
    x = _integrate(dx, Fr(1, 4))
    y, z = [Fr(0), Fr(1, 2)], [Fr(1)]
    y2 = _add(y, _scale(_mul(h, h), Fr(1, 2)))
    exact = dict(pmin_x=float(_val(x, Fr(1, 4))), pmax_x=float(max(_val(x, Fr(0)), _val(x, Fr(1)))), t_touch=1.0)
    assert _val(x, Fr(1, 4)) < min(_val(x, Fr(0)), _val(x, Fr(1)))
    return _csr([[(_row([x, y, z], T), T)], [(_row([x, y2, z], T), T)]]) + (exact,)


# ---- 5. transforms ----

def translate(C, d=SHIFT):
    out = np.array(C, dtype=np.float64).reshape(-1, 3, 8).copy()
    out[:, :, 0] += np.asarray(d)
    return out


def rescale_time(T, C, k):
    """(T 2^k, c_j 2^(-j k)): the same curve flown 2^k times slower.  Exact."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    return np.ldexp(T, k), np.ldexp(C, -k * np.arange(8))


def shift_clock(t0, s):
    out = np.asarray(t0, dtype=np.float64) + s
    assert (out - s == t0).all()  # exact: the start times are multiples of 2^-8
    return out


def ragged48_times():
    """bounds_ref.ragged48 with every time rounded to a multiple of 2^-8: (so, W, T)."""
    so, W, T = R.ragged48()
    return so, W, np.round(T * 256.0) / 256.0


def start_times(B, seed=5):
    """Seeded start times in [0, 5], multiples of 2^-8."""
    return np.round(np.random.default_rng(seed).uniform(0.0, 5.0, B) * 256.0) / 256.0


# ---- the grid the references are held against ----

GRID = np.linspace(0.0, 1.0, 65537).astype(LD)
_PHI = (np.sqrt(LD(5)) - 1) / 2


def grid_max(fn, lo=LD(0), hi=LD(1)):
    """max of fn over [lo, hi] (fn: longdouble array -> longdouble array): the 65,537-point grid,
    then 90 golden-section steps on the bracket of every local maximum of the grid."""
    u = lo + (hi - lo) * GRID
    v = fn(u)
    inner = np.flatnonzero((v[1:-1] >= v[:-2]) & (v[1:-1] >= v[2:])) + 1
    best = v.max()
    if len(inner) > 64:  # a plateau: its value is on the grid already
        inner = inner[np.argsort(v[inner])[-64:]]
    if len(inner):
        a, b = u[inner - 1].copy(), u[inner + 1].copy()
        n = len(a)
        for _ in range(90):
            c, d = b - _PHI * (b - a), a + _PHI * (b - a)
            f = fn(np.concatenate([c, d]))
            left = f[:n] > f[n:]
            b, a = np.where(left, d, b), np.where(left, a, c)
        best = max(best, fn((a + b) / 2).max())
    return best


def grid_min(fn, lo=LD(0), hi=LD(1)):
    return -grid_max(lambda u: -fn(u), lo, hi)


def _axis_u(c, T):
    return np.asarray(c, dtype=LD) * LD(T) ** np.arange(8, dtype=LD)


def grid_bounds(so, T, C):
    """[B, 9] as bounds_ref.records, from the grid."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    out = np.empty((len(so) - 1, 9))
    for b in range(len(so) - 1):
        lo, hi, n2 = [np.inf] * 3, [-np.inf] * 3, [0.0] * 3
        for s in range(int(so[b]), int(so[b + 1])):
            a = _axis_u(C[s], T[s])
            for ax in range(3):
                lo[ax] = min(lo[ax], float(grid_min(lambda u: R._polyval(a[ax], u))))
                hi[ax] = max(hi[ax], float(grid_max(lambda u: R._polyval(a[ax], u))))
            e = a
            for q in range(3):
                e = np.stack([R._deriv(e[ax]) for ax in range(3)])
                m = grid_max(lambda u: sum(R._polyval(e[ax], u) ** 2 for ax in range(3)))
                n2[q] = max(n2[q], float(m / LD(T[s]) ** (2 * (q + 1))))
        out[b] = lo + hi + list(np.sqrt(n2))
    return out


def grid_thrust(so, T, C, g):
    """[B, 3] as thrust_ref.records, from the grid."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    out = np.empty((len(so) - 1, 3))
    for b in range(len(so) - 1):
        r = [np.inf, 0.0, 0.0]
        for s in range(int(so[b]), int(so[b + 1])):
            e = TR._force_polys(C[s], T[s], g)
            r[0] = min(r[0], float(grid_min(lambda u: TR._values(e, T[s], u)[0])))
            r[1] = max(r[1], float(grid_max(lambda u: TR._values(e, T[s], u)[0])))
            r[2] = max(r[2], float(grid_max(lambda u: TR._values(e, T[s], u)[1])))
        out[b] = r
    return out


def grid_rate(so, T, C, g):
    """omega per segment [S], from the grid."""
    import rate_ref as RR
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    return np.array([float(np.sqrt(grid_max(lambda u: RR._omega2(TR._force_polys(C[s], T[s], g), T[s], u))))
                     for s in range(int(so[-1]))])


def grid_corridor(T, C, s, face):
    """The largest n . p - d of segment s against one face, from the grid."""
    a = _axis_u(np.asarray(C).reshape(-1, 3, 8)[s], np.asarray(T).reshape(-1)[s])
    n = np.asarray(face[:3], dtype=LD)
    return float(grid_max(lambda u: sum(n[ax] * R._polyval(a[ax], u) for ax in range(3)) - LD(face[3])))


def grid_pair(ti, tj, dist):
    """min over the window of dist(t)^2 of one pair of separation_ref.Traj, interval by interval
    of the merged knots, from the grid."""
    knots = np.unique(np.concatenate([ti.k, tj.k]))
    return float(min(grid_min(lambda t: dist(t) ** 2, a, b) for a, b in zip(knots[:-1], knots[1:])))


def grid_clearance(traj, ob, scale=None):
    """min over the trajectory of the squared clamped distance to one box, from the grid."""
    import clearance_ref as CL
    s = CL._scale(scale)
    return float(min(grid_min(lambda t: CL.clamp_d2(traj.pos(t), ob, s), traj.k[m], traj.k[m + 1])
                     for m in range(len(traj.T))))
