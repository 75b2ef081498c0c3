"""Shared inputs, checks and reference of the distance-field clearance
(tgms_field_clearance_batch*), used by test_field_host.py and test_gpu_field.py.  Backend-agnostic
like clearance_ref.py: a backend is any object with
    field_clearance(so, T, C, origin, h, values, r_min, tol, lip=0.0, max_evals=1 << 20) -> near, evals, flags
(a Solver has it; the GPU file wraps the device entry point the same way).

The reference is NumPy and independent of the library's search:
  - phi: the trilinear interpolant at the clamped point, as include/tgms.h states it;
  - lipschitz: L from the largest edge difference per axis;
  - dense(): per segment V_s from the Bernstein control values of the velocity, uniform samples
    at a spacing dt with L V_s dt / 2 <= tol / 8, m_hi the least sample and m_lo = m_hi - tol / 8,
    which bracket the true minimum m* because no point is further than dt / 2 from a sample;
  - affine_min(): for a field that is affine inside the grid, m* from the real roots of the
    degree-6 derivative of n . p(t) - d per segment (np.roots) and the segment ends.
Every tolerance is eps = 1e-9 (F + L (P + h)) of include/tgms.h, F the largest |value|, P the
largest coordinate magnitude the row reaches (the knots and 64 points per segment)."""
import functools
from math import comb

import numpy as np

import bounds_ref as R
from trajectory_generator_ros2_amd import FLD_UNRESOLVED, SEP_CLOSE, SEP_NONFINITE

INF = float("inf")
BERN6 = np.array([[comb(i, k) / comb(6, k) if k <= i else 0.0 for k in range(7)] for i in range(7)])


# ---- the reference ----

def phi(origin, h, values, P):
    """The field at the points P [n, 3]; values [nz, ny, nx]."""
    v = np.asarray(values, dtype=np.float64)
    n = np.array(v.shape[::-1])
    q = np.clip((np.asarray(P, dtype=np.float64) - np.asarray(origin, dtype=np.float64)) / h, 0.0, n - 1.0)
    i = np.minimum(np.floor(q).astype(np.int64), n - 2)
    f = q - i
    out = np.zeros(len(q))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                out += w * v[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx]
    return out


def lipschitz(values, h):
    v = np.asarray(values, dtype=np.float64)
    g = [np.abs(np.diff(v, axis=a)).max() / h for a in (2, 1, 0)]
    return float(np.sqrt(sum(x * x for x in g)))


def positions(c, t):
    """p(t) [n, 3] of one segment c [3, 8] at the local times t [n]."""
    return np.stack([np.polyval(c[a, ::-1], t) for a in range(3)], axis=1)


def speed_bound(c, T):
    k = np.arange(1, 8)
    a = c[:, 1:] * k * T ** (k - 1.0)  # p' in u = t / T
    return float(np.sqrt((np.abs(a @ BERN6.T).max(axis=1) ** 2).sum()))


class Row:
    """One trajectory of a CSR batch: its segments, knots and what the checks need of it."""

    def __init__(self, so, T, C, b):
        self.T = np.asarray(T)[so[b]:so[b + 1]]
        self.c = np.asarray(C).reshape(-1, 3, 8)[so[b]:so[b + 1]]
        self.M = len(self.T)
        self.kn = np.concatenate([[0.0], np.cumsum(self.T)])
        self.D = self.kn[-1]

    def at(self, t):
        """p at the global time t: the segment whose left knot is the last one <= t."""
        m = int(np.clip(np.searchsorted(self.kn, t, side="right") - 1, 0, self.M - 1))
        return positions(self.c[m], np.array([min(max(t - self.kn[m], 0.0), self.T[m])]))

    def knots(self):
        return np.concatenate([self.c[:, :, 0], positions(self.c[-1], self.T[-1:])])

    def reach(self):
        return max(np.abs(positions(self.c[m], np.linspace(0.0, self.T[m], 65))).max() for m in range(self.M))


def eps_of(row, h, values, L):
    return 1e-9 * (float(np.abs(values).max()) + L * (row.reach() + h))


def dense(row, origin, h, values, L, tol):
    """(m_lo, m_hi) of one row by uniform sampling at the spacing the tolerance asks for."""
    m_hi = INF
    for m in range(row.M):
        LV = L * speed_bound(row.c[m], row.T[m])
        n = 2 if LV == 0.0 else int(np.ceil(row.T[m] * 4.0 * LV / tol)) + 1
        assert n <= 4_000_000, "the case is too fine for the dense reference"
        m_hi = min(m_hi, phi(origin, h, values, positions(row.c[m], np.linspace(0.0, row.T[m], n))).min())
    return m_hi - tol / 8.0, m_hi


def affine_min(row, normal, d):
    """The exact minimum of normal . p(t) - d over the row."""
    best = INF
    for m in range(row.M):
        q = normal @ row.c[m]  # [8] in t
        dq = q[1:] * np.arange(1, 8)
        while len(dq) > 1 and dq[-1] == 0.0:
            dq = dq[:-1]
        r = np.roots(dq[::-1]) if len(dq) > 1 else np.zeros(0)
        r = r[np.abs(r.imag) <= 1e-9 * max(1.0, row.T[m])].real
        t = np.concatenate([[0.0, row.T[m]], r[(r > 0.0) & (r < row.T[m])]])
        best = min(best, (np.polyval(q[::-1], t) - d).min())
    return float(best)


def check_rows(out, so, T, C, origin, h, values, r_min, tol, L, brackets=None, what=""):
    """The assertions of every usable row; brackets: per row (m_lo, m_hi), None to skip those two.
    Returns the rows' eps."""
    near, evals, flags = out
    B = len(so) - 1
    eps = np.zeros(B)
    for b in range(B):
        row = Row(so, T, C, b)
        e = eps[b] = eps_of(row, h, values, L)
        d_min, t_min = near[b]
        assert flags[b] & ~(SEP_CLOSE | FLD_UNRESOLVED) == 0 and np.isfinite(near[b]).all(), (what, b, flags[b], near[b])
        assert 0.0 <= t_min <= row.D, (what, b, t_min, row.D)
        again = phi(origin, h, values, row.at(t_min))[0]
        assert abs(again - d_min) <= e, (what, b, again, d_min, e)  # (1): the value is attained at t_min
        assert d_min <= phi(origin, h, values, row.knots()).min() + e, (what, b)
        assert bool(flags[b] & SEP_CLOSE) == bool(d_min < r_min), (what, b, d_min, r_min, flags[b])
        assert evals[b] >= row.M + 1, (what, b, evals[b])
        if brackets is not None:
            m_lo, m_hi = brackets[b]
            assert d_min >= m_lo - e, (what, b, d_min, m_lo, e)  # (1)
            if not flags[b] & FLD_UNRESOLVED:
                assert min(d_min - tol, r_min) <= m_hi + e, (what, b, d_min, tol, r_min, m_hi, e)  # (2)
    return eps


def resolved(out, what=""):
    """The condition of every case that is not about the budget: no row spent it."""
    assert not (out[2] & FLD_UNRESOLVED).any(), (what, np.flatnonzero(out[2] & FLD_UNRESOLVED), out[1].max())


# ---- the batches ----

@functools.lru_cache(maxsize=None)
def solved(name):
    """bounds_ref.ragged48 solved by the host backend, rest to rest ("rest") or with
    bounds_ref.end_derivs48 ("end_derivs"); "ragged65": 65 rows with M = 1 .. 16 in turn, four
    and a bit lane groups' worth, so that lane groups and wavefronts are crossed."""
    from trajectory_generator_ros2_amd import synthetic as S
    from trajectory_generator_ros2_amd.solver import Solver
    ED = None
    if name == "ragged65":
        rng = np.random.default_rng(65)
        Ms = (np.arange(65) % 16 + 1).astype(np.int32)
        so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
        n_w = int(so[-1]) + 65
        W = np.c_[rng.uniform(-5, 5, n_w), rng.uniform(-5, 5, n_w), rng.uniform(0.5, 5, n_w)]
        rows = np.arange(int(so[-1])) + np.repeat(np.arange(65), Ms)
        T = np.clip(np.linalg.norm(W[rows + 1] - W[rows], axis=1) / S.V_NOMINAL, S.T_MIN, S.T_MAX)
    else:
        so, W, T = R.ragged48()
        ED = None if name == "rest" else R.end_derivs48()
    with Solver(host=True) as s:
        C, _, worst = s.solve(so, W, T, ED)
        assert worst == 0
        ext, _ = s.bounds(so, T, C)
    for a in (so, T, C, ext):
        a.setflags(write=False)
    return so, T, C, ext


def waypoint_rows(paths, speed=1.5):
    """Rest-to-rest trajectories through the given waypoint lists, solved by the host backend."""
    from trajectory_generator_ros2_amd.solver import Solver
    so = np.concatenate([[0], np.cumsum([len(p) - 1 for p in paths])]).astype(np.int32)
    W = np.concatenate([np.asarray(p, dtype=np.float64) for p in paths])
    T = np.concatenate([np.maximum(np.linalg.norm(np.diff(np.asarray(p, dtype=np.float64), axis=0), axis=1) / speed, 0.5)
                        for p in paths])
    with Solver(host=True) as s:
        C, _, worst = s.solve(so, W, T, None)
    assert worst == 0
    return so, T, C


# ---- case: the affine field ----

AFFINE_N, AFFINE_D = np.array([0.5, -0.25, 1.0]), 0.375
# [nz, ny, nx]: x, y in +-96, z in +-32; badly timed rows of the batches overshoot their room by far
AFFINE_ORIGIN, AFFINE_H, AFFINE_SHAPE = (-96.0, -96.0, -32.0), 16.0, (5, 13, 13)
AFFINE_TOLS = (1e-1, 1e-3, 1e-6)


@functools.lru_cache(maxsize=None)
def affine_field():
    """values = n . x - d at the nodes: dyadic, so exact in float32 and reproduced by the interpolant."""
    nz, ny, nx = AFFINE_SHAPE
    z, y, x = np.meshgrid(*(o + AFFINE_H * np.arange(m) for o, m in zip(AFFINE_ORIGIN[::-1], AFFINE_SHAPE)), indexing="ij")
    v = AFFINE_N[0] * x + AFFINE_N[1] * y + AFFINE_N[2] * z - AFFINE_D
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    return v32


@functools.lru_cache(maxsize=None)
def affine_reference(name):
    so, T, C, ext = solved(name)
    hi = np.array(AFFINE_ORIGIN) + AFFINE_H * (np.array(AFFINE_SHAPE[::-1]) - 1)
    assert (ext[:, 0:3] >= np.array(AFFINE_ORIGIN)).all() and (ext[:, 3:6] <= hi).all()  # the field is affine where they fly
    return np.array([affine_min(Row(so, T, C, b), AFFINE_N, AFFINE_D) for b in range(len(so) - 1)])


def check_affine(be, name, tol, lip=0.0):
    so, T, C, _ = solved(name)
    v = affine_field()
    m = affine_reference(name)
    L = lipschitz(v, AFFINE_H)
    assert abs(L - np.linalg.norm(AFFINE_N)) <= 1e-12
    out = near, evals, flags = be.field_clearance(so, T, C, AFFINE_ORIGIN, AFFINE_H, v, INF, tol, lip=lip)
    resolved(out, name)
    eps = check_rows(out, so, T, C, AFFINE_ORIGIN, AFFINE_H, v, INF, tol, L, what=name)
    off = near[:, 0] - m
    print("affine %s tol %g: d_min - m* in [%.3g, %.3g], evals mean %.1f max %d" % (name, tol, off.min(), off.max(),
                                                                                 evals.mean(), evals.max()))
    assert (off >= -eps).all() and (off <= tol + eps).all(), (off.min(), off.max(), tol)
    return out


# ---- case: the sphere ----

SPHERE_C, SPHERE_R = np.array([0.125, -0.0625, 0.25]), 1.0
SPHERE_ORIGIN, SPHERE_H, SPHERE_TOL = (-2.875, -2.875, -2.875), 0.25, 1e-3
SPHERE_PATHS = (
    [(-2.5, 0.0, 0.0), (2.5, 0.2, 0.4)],                                      # through
    [(-2.5, -2.0, 0.3), (0.1, 0.3, 0.2), (2.4, 2.2, -0.5)],                   # through, M = 2
    [(-2.5, 1.1, 0.25), (0.0, 1.03, 0.3), (2.5, 1.1, 0.25)],                  # grazing outside
    [(-2.0, 1.4, 1.0), (0.0, 1.0, 0.6), (1.0, 0.0, 1.2), (2.0, -1.5, 1.0)],   # grazing, M = 3
    [(-2.5, 2.5, 2.0), (2.5, 2.4, 2.5)],                                      # far
    [(-2.5, -2.5, -2.5), (-2.0, 2.5, -2.4), (2.5, 2.5, -2.0), (2.5, -2.5, -2.5), (-2.4, -2.4, -2.0)],  # far, M = 4
)


@functools.lru_cache(maxsize=None)
def sphere_case():
    """The exact signed distance to a sphere on a 24^3 grid; rows through it, grazing it and far
    from it; the dense reference of every row."""
    ax = [o + SPHERE_H * np.arange(24) for o in SPHERE_ORIGIN]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    v = (np.sqrt((x - SPHERE_C[0]) ** 2 + (y - SPHERE_C[1]) ** 2 + (z - SPHERE_C[2]) ** 2) - SPHERE_R).astype(np.float32)
    so, T, C = waypoint_rows(SPHERE_PATHS)
    L = lipschitz(v, SPHERE_H)
    ref = [dense(Row(so, T, C, b), SPHERE_ORIGIN, SPHERE_H, v, L, SPHERE_TOL) for b in range(len(so) - 1)]
    hi = np.array([r[1] for r in ref])
    assert (hi[:2] < -0.5).all() and (np.abs(hi[2:4]) < 0.2).all() and (hi[4:] > 0.6).all(), hi  # through, grazing, far
    return so, T, C, v, L, ref


def check_sphere(be, r_min, lip=0.0):
    so, T, C, v, L, ref = sphere_case()
    out = be.field_clearance(so, T, C, SPHERE_ORIGIN, SPHERE_H, v, r_min, SPHERE_TOL, lip=lip)
    print("sphere r_min %g: d_min %s evals %s flags %s" % (r_min, out[0][:, 0], out[1], out[2]))
    resolved(out, "sphere")
    check_rows(out, so, T, C, SPHERE_ORIGIN, SPHERE_H, v, r_min, SPHERE_TOL, L, ref, "sphere r_min %g" % r_min)
    return out


# ---- case: the rough field ----

ROUGH_ORIGIN, ROUGH_H, ROUGH_TOL = (-1.0, -1.5, 0.0), 0.5, 1e-2
ROUGH_PATHS = (
    [(-0.5, -1.0, 0.5), (2.0, 2.0, 4.0)],
    [(2.2, -1.2, 4.2), (1.0, 0.5, 2.0), (-0.8, 2.2, 0.3)],
    [(0.0, 0.0, 1.0), (0.5, 0.5, 1.5), (1.0, 0.0, 2.0), (0.5, -0.5, 2.5), (0.0, 0.0, 3.0), (1.5, 1.0, 3.5)],
)


@functools.lru_cache(maxsize=None)
def rough_case():
    """Uniform noise on an 8 x 9 x 10 grid (nx, ny, nz): L is that of the noise, far above a distance field's."""
    v = np.random.default_rng(8910).uniform(0.0, 1.0, (10, 9, 8)).astype(np.float32)
    so, T, C = waypoint_rows(ROUGH_PATHS)
    L = lipschitz(v, ROUGH_H)
    assert L > 3.0
    ref = [dense(Row(so, T, C, b), ROUGH_ORIGIN, ROUGH_H, v, L, ROUGH_TOL) for b in range(len(so) - 1)]
    return so, T, C, v, L, ref


def check_rough(be, given):
    so, T, C, v, L, ref = rough_case()
    out = be.field_clearance(so, T, C, ROUGH_ORIGIN, ROUGH_H, v, INF, ROUGH_TOL, lip=L if given else 0.0)
    print("rough lip %s: d_min %s evals %s" % ("given" if given else "reduced", out[0][:, 0], out[1]))
    resolved(out, "rough")
    check_rows(out, so, T, C, ROUGH_ORIGIN, ROUGH_H, v, INF, ROUGH_TOL, L, ref, "rough")
    return out


# ---- case: the constant field ----

def check_constant(be):
    so, T, C, _ = solved("ragged65")
    v = np.full((3, 4, 5), 0.7, dtype=np.float32)
    near, evals, flags = be.field_clearance(so, T, C, (-6.0, -6.0, 0.0), 3.0, v, 1.0, 1e-3, lip=0.0)
    assert (near[:, 0] == np.float64(np.float32(0.7))).all()  # to the bit
    assert np.array_equal(evals, np.diff(so) + 1) and (flags == SEP_CLOSE).all()


# ---- case: degenerate geometry ----

def hover(p, T=1.0, M=1):
    C = np.zeros((M, 3, 8))
    C[:, :, 0] = p
    return np.arange(0, M + 1, M, dtype=np.int32), np.full(M, T), C


def check_degenerate(be):
    # the 2 x 2 x 2 grid: one cell, values 0 .. 7 by node index, so phi = x + 2 y + 4 z inside it
    v2 = np.arange(8, dtype=np.float32).reshape(2, 2, 2)
    L2 = lipschitz(v2, 1.0)
    so, T, C = waypoint_rows([[(0.9, 0.8, 0.7), (0.2, 0.1, 0.3), (0.6, 0.9, 0.1)]])
    out = be.field_clearance(so, T, C, (0.0, 0.0, 0.0), 1.0, v2, INF, 1e-4)
    resolved(out, "2x2x2")
    ref = [dense(Row(so, T, C, 0), (0.0, 0.0, 0.0), 1.0, v2, L2, 1e-4)]
    check_rows(out, so, T, C, (0.0, 0.0, 0.0), 1.0, v2, INF, 1e-4, L2, ref, "2x2x2")
    # wholly outside the grid: the value at the clamped point, against the dense reference on clamped points
    so, T, C = waypoint_rows([[(3.0, -2.0, 0.5), (2.0, 0.5, 3.0), (5.0, 0.2, -1.0)]])
    out = be.field_clearance(so, T, C, (0.0, 0.0, 0.0), 1.0, v2, INF, 1e-3)
    resolved(out, "outside")
    ref = [dense(Row(so, T, C, 0), (0.0, 0.0, 0.0), 1.0, v2, L2, 1e-3)]
    check_rows(out, so, T, C, (0.0, 0.0, 0.0), 1.0, v2, INF, 1e-3, L2, ref, "outside")
    assert out[0][0, 0] >= 1.0  # x is clamped to 1 all the way
    # ends exactly on the upper corner of the sphere's grid
    _, _, _, v, L, _ = sphere_case()
    corner = tuple(o + SPHERE_H * 23 for o in SPHERE_ORIGIN)
    so, T, C = waypoint_rows([[(0.0, 2.0, 0.0), corner]])
    out = be.field_clearance(so, T, C, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL)
    resolved(out, "corner")
    ref = [dense(Row(so, T, C, 0), SPHERE_ORIGIN, SPHERE_H, v, L, SPHERE_TOL)]
    check_rows(out, so, T, C, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL, L, ref, "corner")
    # a constant position: V = 0, one evaluation per knot
    for M in (1, 3):
        so, T, C = hover((0.4, 0.3, 1.6), M=M)
        near, evals, flags = be.field_clearance(so, T, C, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL)
        want = phi(SPHERE_ORIGIN, SPHERE_H, v, np.array([[0.4, 0.3, 1.6]]))[0]
        assert evals[0] == M + 1 and flags[0] == SEP_CLOSE and abs(near[0, 0] - want) <= 1e-9, (evals, flags, near, want)
        assert 0.0 <= near[0, 1] <= M
    # B = 1 with M = 1, moving
    so, T, C = waypoint_rows([[(-2.0, 0.3, 0.2), (2.0, 0.1, 0.4)]])
    out = be.field_clearance(so, T, C, SPHERE_ORIGIN, SPHERE_H, v, 0.3, SPHERE_TOL)
    resolved(out, "B = 1")
    ref = [dense(Row(so, T, C, 0), SPHERE_ORIGIN, SPHERE_H, v, L, SPHERE_TOL)]
    check_rows(out, so, T, C, SPHERE_ORIGIN, SPHERE_H, v, 0.3, SPHERE_TOL, L, ref, "B = 1")
    assert out[2][0] == SEP_CLOSE


# ---- case: the budget ----

def check_budget(be):
    so, T, C, v, L, ref = sphere_case()
    b = 2  # grazing, M = 2
    so1, T1, C1 = np.array([0, 2], np.int32), T[so[b]:so[b + 1]], C[so[b]:so[b + 1]]
    full = be.field_clearance(so1, T1, C1, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL)
    resolved(full, "budget")
    assert full[1][0] > 3  # the condition: the row needs more than its knots
    out = near, evals, flags = be.field_clearance(so1, T1, C1, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL, max_evals=3)
    assert flags[0] & FLD_UNRESOLVED and evals[0] == 3, (flags, evals)
    check_rows(out, so1, T1, C1, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL, L, [ref[b]], "budget")  # (1) still holds
    # exactly the evaluations the full search took is enough; one fewer is not
    out = be.field_clearance(so1, T1, C1, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL, max_evals=int(full[1][0]))
    assert not out[2][0] & FLD_UNRESOLVED and np.array_equal(out[0], full[0])
    out = be.field_clearance(so1, T1, C1, SPHERE_ORIGIN, SPHERE_H, v, INF, SPHERE_TOL, max_evals=int(full[1][0]) - 1)
    assert out[2][0] & FLD_UNRESOLVED


# ---- case: unusable rows ----

UNUSABLE = (1, 4)  # a NaN coefficient in the last segment, a zero time


def check_unusable(be):
    so, T, C, v, L, ref = sphere_case()
    T2, C2 = T.copy(), C.copy()
    C2[so[UNUSABLE[0] + 1] - 1, 1, 5] = np.nan
    T2[so[UNUSABLE[1]]] = 0.0
    want = be.field_clearance(so, T, C, SPHERE_ORIGIN, SPHERE_H, v, 0.3, SPHERE_TOL)
    near, evals, flags = be.field_clearance(so, T2, C2, SPHERE_ORIGIN, SPHERE_H, v, 0.3, SPHERE_TOL)
    for b in range(len(so) - 1):
        if b in UNUSABLE:
            assert flags[b] == SEP_NONFINITE and np.isnan(near[b]).all() and evals[b] == 0, (b, flags[b], near[b], evals[b])
        else:  # the other rows are those of the batch without the spoiled ones
            assert np.array_equal(near[b], want[0][b]) and evals[b] == want[1][b] and flags[b] == want[2][b]
    # a NaN node on the way: the row that meets it is unusable
    vn = v.copy()
    vn[:, :, :] = np.nan
    near, evals, flags = be.field_clearance(so[:2], T[:so[1]], C[:so[1]], SPHERE_ORIGIN, SPHERE_H, vn, 0.3, SPHERE_TOL, lip=1.8)
    assert flags[0] == SEP_NONFINITE and np.isnan(near[0]).all() and evals[0] == 0


# ---- arguments: what both entry points refuse ----

def bad_arguments():
    """(label, keyword overrides of a valid call) for every TGMS_ERR_INVALID_ARG that can be
    reached through the backend interface."""
    nan = float("nan")
    v = np.zeros((3, 3, 3), np.float32)
    return [
        ("n_x < 2", dict(values=np.zeros((3, 3, 1), np.float32))),
        ("n_y < 2", dict(values=np.zeros((3, 1, 3), np.float32))),
        ("n_z < 2", dict(values=np.zeros((1, 3, 3), np.float32))),
        ("h nan", dict(values=v, h=nan)), ("h inf", dict(values=v, h=INF)), ("h zero", dict(values=v, h=0.0)),
        ("h negative", dict(values=v, h=-1.0)),
        ("origin nan", dict(values=v, origin=(0.0, nan, 0.0))), ("origin inf", dict(values=v, origin=(INF, 0.0, 0.0))),
        ("tol zero", dict(values=v, tol=0.0)), ("tol negative", dict(values=v, tol=-1.0)), ("tol nan", dict(values=v, tol=nan)),
        ("tol inf", dict(values=v, tol=INF)),
        ("r_min nan", dict(values=v, r_min=nan)), ("r_min zero", dict(values=v, r_min=0.0)),
        ("r_min negative", dict(values=v, r_min=-1.0)),
        ("lip negative", dict(values=v, lip=-1.0)), ("lip nan", dict(values=v, lip=nan)), ("lip inf", dict(values=v, lip=INF)),
        ("max_evals 0", dict(values=v, max_evals=0)), ("max_evals negative", dict(values=v, max_evals=-5)),
    ]


def check_arguments(be, TgmsError, ERR_INVALID_ARG):
    import pytest
    so, T, C = hover((0.5, 0.5, 0.5))
    base = dict(origin=(0.0, 0.0, 0.0), h=1.0, r_min=1.0, tol=1e-3, lip=0.0, max_evals=100)
    ok = be.field_clearance(so, T, C, values=np.zeros((3, 3, 3), np.float32), **base)
    assert ok[2][0] == SEP_CLOSE and ok[0][0, 0] == 0.0
    for label, kw in bad_arguments():
        a = dict(base)
        a.update(kw)
        with pytest.raises(TgmsError) as e:
            be.field_clearance(so, T, C, **a)
        assert e.value.status == ERR_INVALID_ARG, label
