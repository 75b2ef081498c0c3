"""Reference for the continuous swarm separation (tgms_separation_batch*), shared by
test_separation_host.py and test_gpu_separation.py.  NumPy only and independent of the
library's derivative ladder, in the manner of bounds_ref.py:
  - per pair the merged knots of the two trajectories in np.longdouble (knot m of trajectory b
    is start_times[b] + the fp64 left-to-right prefix sum of its first m times, include/tgms.h);
  - per interval [a, b] of them the two sides' axis polynomials in u = (t - a) / (b - a) by
    longdouble composition (binomial expansion of p(la + h u)); a held side is its constant;
  - candidates: u = 0, 1 and the real roots of the derivative of sum_a e_a^2 from np.roots,
    polished by Newton steps in longdouble (bounds_ref._candidates), backed by a uniform floor
    of 1,025 points per interval;
  - every candidate is evaluated by dist(), which reads the ORIGINAL segment polynomials at the
    global time, not the composed ones.
pair_ref returns d2_ref (the minimum of the squared scaled distance), L (the largest scaled
coordinate magnitude either trajectory reaches) and the callable dist(t)."""
import functools
from math import comb

import numpy as np

import bounds_ref as R
from extrema_ref import ORACLE_TOL

LD = np.longdouble
GRID = np.linspace(0.0, 1.0, 1025).astype(LD)


class Traj:
    """One trajectory on its global interval: knots k [M + 1] (longdouble), times T, coeffs c."""

    def __init__(self, c, T, t0):
        self.c = np.asarray(c, dtype=LD).reshape(-1, 3, 8)
        self.T = np.asarray(T, dtype=np.float64).reshape(-1)
        acc, pre = 0.0, [0.0]
        for t in self.T:
            acc += float(t)
            pre.append(acc)
        self.k = LD(t0) + np.asarray(pre, dtype=LD)
        self.end64 = float(np.float64(t0) + np.float64(acc))  # the window's end as fp64 forms it

    def locate(self, t):
        """(segment, local time) at the global times t; held ends outside [k[0], k[M]]."""
        t = np.asarray(t, dtype=LD)
        M = len(self.T)
        seg = np.clip(np.searchsorted(self.k, t, side="right") - 1, 0, M - 1)
        loc = t - self.k[seg]
        loc = np.where(t <= self.k[0], LD(0), loc)
        loc = np.where(t >= self.k[M], LD(self.T[M - 1]), loc)
        return seg, loc

    def pos(self, t):
        """[n, 3] positions at the global times t, in longdouble."""
        seg, loc = self.locate(np.atleast_1d(t))
        out = np.empty((len(seg), 3), dtype=LD)
        for s in np.unique(seg):
            m = seg == s
            for ax in range(3):
                out[m, ax] = R._polyval(self.c[s, ax], loc[m])
        return out

    def in_u(self, a, b):
        """[3, 8] coefficients in u of the position over the interval [a, b] (a < b), which
        holds no knot of this trajectory inside."""
        mid = (a + b) / 2
        M = len(self.T)
        if mid <= self.k[0] or mid >= self.k[M]:
            q = np.zeros((3, 8), dtype=LD)
            q[:, 0] = self.pos(mid)[0]
            return q
        s = int(np.searchsorted(self.k, mid, side="right") - 1)
        la, h = a - self.k[s], b - a
        q = np.zeros((3, 8), dtype=LD)
        for k in range(8):
            for m in range(k, 8):
                q[:, k] += self.c[s, :, m] * LD(comb(m, k)) * la ** (m - k)
            q[:, k] *= h ** k
        return q


def pair_ref(ti, tj, scale=(1.0, 1.0, 1.0)):
    """(d2_ref, L, dist) of one pair of Traj."""
    s = np.asarray(scale, dtype=LD)

    def dist(t):
        d = (ti.pos(t) - tj.pos(t)) * s
        return np.sqrt((d * d).sum(axis=1))

    knots = np.unique(np.concatenate([ti.k, tj.k]))
    d2, L = LD(np.inf), LD(0)
    for a, b in zip(knots[:-1], knots[1:]):
        e = (ti.in_u(a, b) - tj.in_u(a, b)) * s[:, None]
        sq = sum(np.convolve(e[ax], e[ax]) for ax in range(3))
        u = np.concatenate([GRID, R._candidates(sq)])
        t = a + (b - a) * u
        d2 = min(d2, (dist(t) ** 2).min())
        L = max(L, np.abs(ti.pos(t) * s).max(), np.abs(tj.pos(t) * s).max())
    return float(d2), float(L), dist


def window(ti, tj):
    return min(float(ti.k[0]), float(tj.k[0])), max(ti.end64, tj.end64)


def batch_trajs(so, T, C, t0=None):
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    return [Traj(C[so[b]:so[b + 1]], T[so[b]:so[b + 1]], 0.0 if t0 is None else t0[b]) for b in range(len(so) - 1)]


def references(trajs, pairs, scale=(1.0, 1.0, 1.0)):
    """[(d2_ref, L, dist)] of the listed pairs."""
    return [pair_ref(trajs[i], trajs[j], scale) for i, j in pairs]


def check_contract(sep, trajs, pairs, refs, tol=ORACLE_TOL, what="separation"):
    """include/tgms.h: (1) |d_min^2 - d_ref^2| <= tol L^2, (2) t_min inside the window, (3) the
    distance at t_min is the returned one: |dist(t_min)^2 - d_min^2| <= tol L^2.  t_min itself is
    not compared: a flat minimum makes it ill-conditioned.  Returns the two worst errors in L^2."""
    sep = np.asarray(sep)
    assert sep.shape == (len(pairs), 2) and np.isfinite(sep).all()
    e1, e3 = np.empty(len(pairs)), np.empty(len(pairs))
    for n, ((i, j), (d2_ref, L, dist)) in enumerate(zip(pairs, refs)):
        lo, hi = window(trajs[i], trajs[j])
        assert lo <= sep[n, 1] <= hi, (n, sep[n, 1], lo, hi)
        d2 = LD(sep[n, 0]) ** 2
        e1[n] = float(abs(d2 - LD(d2_ref))) / L ** 2
        e3[n] = float(abs(dist(LD(sep[n, 1]))[0] ** 2 - d2)) / L ** 2
    print("%s vs reference: d_min^2 off by %.3g x L^2, dist(t_min)^2 off by %.3g x L^2" % (what, e1.max(), e3.max()))
    assert (e1 <= tol).all(), (int(e1.argmax()), float(e1.max()))
    assert (e3 <= tol).all(), (int(e3.argmax()), float(e3.max()))
    return float(e1.max()), float(e3.max())


# ---- the batches both test files use ----

def line(p0, v, T):
    """M = 1 linear motion p0 + v t on [0, T]: coefficients [1, 3, 8]."""
    C = np.zeros((1, 3, 8))
    C[0, :, 0], C[0, :, 1] = p0, v
    return C, np.array([float(T)])


def batch(*trajs):
    """CSR batch (so, T, C) of (C [M,3,8], T [M]) trajectories."""
    so = np.concatenate([[0], np.cumsum([len(t[1]) for t in trajs])]).astype(np.int32)
    return so, np.concatenate([t[1] for t in trajs]), np.concatenate([t[0] for t in trajs])


def crossing(split=False):
    """i: (t, 0, 0), j: (2 - t, 0.5, 0), both on [0, 2]: d_min = 0.5 at t_min = 1, while both ends
    give sqrt(4.25) = 2.06.  split: j as M = 2, cut at 0.7, which is no knot of i."""
    i = line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 2.0)
    if not split:
        return batch(i, line([2.0, 0.5, 0.0], [-1.0, 0.0, 0.0], 2.0))
    j0, j1 = line([2.0, 0.5, 0.0], [-1.0, 0.0, 0.0], 0.7), line([1.3, 0.5, 0.0], [-1.0, 0.0, 0.0], 1.3)
    return batch(i, (np.concatenate([j0[0], j1[0]]), np.concatenate([j0[1], j1[1]])))


@functools.lru_cache(maxsize=None)
def contract_case(name):
    """The 48-trajectory batch of bounds_ref.ragged48 (every M in 1..16 three times), rest to
    rest ("rest") or with bounds_ref.end_derivs48 ("end_derivs"), solved by the host backend,
    with seeded start times in [0, 5] and a seeded sample of 96 pairs in which every trajectory,
    so every M in 1..16, appears on both sides; the reference of every pair, computed once per
    session and left unchanged."""
    from trajectory_generator_ros2_amd.solver import Solver
    so, W, T = R.ragged48()
    ED = None if name == "rest" else R.end_derivs48()
    with Solver(host=True) as s:
        C, _, worst = s.solve(so, W, T, ED)
    assert worst == 0
    rng = np.random.default_rng(96 if name == "rest" else 97)
    t0 = rng.uniform(0.0, 5.0, 48)
    pairs = np.stack([np.concatenate([rng.permutation(48), rng.permutation(48)]),
                      np.concatenate([rng.permutation(48), rng.permutation(48)])], axis=1).astype(np.int32)
    Ms = np.diff(so)
    assert set(Ms[pairs[:, 0]]) == set(range(1, 17)) == set(Ms[pairs[:, 1]])
    trajs = batch_trajs(so, T, C, t0)
    refs = references(trajs, pairs)
    for a in (so, T, C, t0, pairs):
        a.setflags(write=False)
    return dict(so=so, T=T, C=C, t0=t0, pairs=pairs, trajs=trajs, refs=refs)
