"""Shared inputs, checks and reference of the obstacle clearance (tgms_clearance_batch*), used by
test_clearance_host.py and test_gpu_clearance.py.  Backend-agnostic like neighbors_ref.py: a
backend is any object with
    clearance(so, T, C, obstacles, r_min, scale=None) -> near, obs, count, tested, flags
(a Solver has it; the GPU file wraps the device entry point the same way).

The reference is NumPy longdouble and independent of the library's combination trick.  Per
(segment, obstacle):
  - the times an axis crosses a face: np.roots of p_a - lo_a and p_a - hi_a in u = t / T;
  - the interval [0, 1] cut there; per piece the active set of axis states at the midpoint and
    the piece's own polynomial sum_a (s_a e_a)^2;
  - candidates: the cuts, bounds_ref._candidates of the piece's polynomial (np.roots polished by
    Newton steps in longdouble), and a uniform floor of 1,025 points per segment;
  - every candidate evaluated as the true clamped distance from the ORIGINAL coefficients.
pair_ref returns d2_ref per scale, L per scale and dist(t, scale).  The contract reference (48
trajectories x 12 obstacles = 576 pairs, both scales in one pass) takes about 12 s per batch
on one CPU core (measured: 12.1 s and 13.4 s) and is computed once per session."""
import functools

import numpy as np

import bounds_ref as R
import separation_ref as SR
from trajectory_generator_ros2_amd import CLR_BAD_OBSTACLE, NEAR_NONE, SEP_CLOSE, SEP_NONFINITE

LD = np.longdouble
TOL = 1e-9  # the project's tolerance on d^2, in L^2 (include/tgms.h)
SCALES = {"unit": None, "third": (1.0, 1.0, 1.0 / 3.0)}
GRID = np.linspace(0.0, 1.0, 1025).astype(LD)


def _scale(scale):
    return np.ones(3, dtype=LD) if scale is None else np.asarray(scale, dtype=LD)


def clamp_d2(p, ob, s):
    """Squared scaled clamped distance of the points p [n, 3] (longdouble) to the box ob [6]."""
    ob = np.asarray(ob, dtype=LD)
    g = np.maximum(np.maximum(ob[0:3] - p, p - ob[3:6]), LD(0)) * s
    return (g * g).sum(axis=1)


def _crossings(a, ob, pg):
    """The u in (0, 1) at which an axis polynomial a [3][8] (in u) meets a face of ob.  pg: the
    segment on the uniform floor; a face further outside its range than 1 % of that range cannot
    be met (between two of 1,025 points a degree-7 polynomial leaves the range by far less)."""
    cuts = []
    for ax in range(3):
        lo, hi = float(pg[:, ax].min()), float(pg[:, ax].max())
        for bound in (ob[ax], ob[3 + ax]):
            if bound < lo - 0.01 * (hi - lo) or bound > hi + 0.01 * (hi - lo):
                continue
            q = np.asarray(a[ax], dtype=np.float64).copy()
            q[0] -= bound
            while len(q) and q[-1] == 0.0:
                q = q[:-1]
            if len(q) < 2:
                continue
            r = np.roots(q[::-1])
            r = r[np.abs(r.imag) <= 1e-6].real
            cuts.extend(r[(r > 0.0) & (r < 1.0)])
    return np.unique(np.concatenate([[0.0], cuts, [1.0]])).astype(LD)


@functools.lru_cache(maxsize=None)
def _segment_grid(traj, m):
    """Positions [1025, 3] of segment m of an SR.Traj on the uniform floor; the same for every obstacle."""
    t = GRID * LD(traj.T[m])
    return np.stack([R._polyval(traj.c[m, ax], t) for ax in range(3)], axis=1)


def pair_ref(traj, ob, scales):
    """([d2_ref per scale], [L per scale]) of one SR.Traj (start 0) against one box ob [6]."""
    ob64 = np.asarray(ob, dtype=np.float64)
    obl = ob64.astype(LD)
    ss = [_scale(s) for s in scales]
    d2 = [LD(np.inf)] * len(ss)
    L = [np.abs(obl.reshape(2, 3) * s).max() for s in ss]
    for m, T in enumerate(traj.T):
        c = traj.c[m]
        a = c * LD(T) ** np.arange(8, dtype=LD)  # in u
        pg = _segment_grid(traj, m)
        cuts = _crossings(a, ob64, pg)
        us = [[cuts] for _ in ss]
        for ua, ub in zip(cuts[:-1], cuts[1:]):
            mid = (ua + ub) / 2
            pm = np.array([R._polyval(a[ax], np.atleast_1d(mid))[0] for ax in range(3)])
            e = []
            for ax in range(3):
                q = np.zeros(8, dtype=LD)
                if pm[ax] < obl[ax]:
                    q = -a[ax].copy()
                    q[0] += obl[ax]
                elif pm[ax] > obl[3 + ax]:
                    q = a[ax].copy()
                    q[0] -= obl[3 + ax]
                e.append(q)
            for n, s in enumerate(ss):
                sq = sum(np.convolve(e[ax] * s[ax], e[ax] * s[ax]) for ax in range(3))
                if np.any(sq != 0):
                    us[n].append(R._candidates(sq))
        for n, s in enumerate(ss):
            u = np.concatenate(us[n])
            p = np.stack([R._polyval(c[ax], u * LD(T)) for ax in range(3)], axis=1)
            d2[n] = min(d2[n], clamp_d2(p, obl, s).min(), clamp_d2(pg, obl, s).min())
            L[n] = max(L[n], np.abs(p * s).max(), np.abs(pg * s).max())
    return [float(x) for x in d2], [float(x) for x in L]


def dist2_at(traj, ob, t, scale):
    """The true squared clamped distance at the global time t, in longdouble."""
    return clamp_d2(traj.pos(np.atleast_1d(LD(t))), ob, _scale(scale))[0]


def none_rows(out, rows, flag=0):
    near, obs, count, tested, flags = out
    for i in rows:
        assert near[i, 0] == np.inf and near[i, 1] == 0.0, (i, near[i])
        assert obs[i] == NEAR_NONE and count[i] == 0 and flags[i] == flag, (i, obs[i], count[i], flags[i])


# ---- case 1 / 2: the fly-by ----

def flyby(split=False):
    """p = (-2 + 2 t, 0, 0) on [0, 2]; split: as M = 2, cut at t = 0.7."""
    if not split:
        return SR.batch(SR.line([-2.0, 0.0, 0.0], [2.0, 0.0, 0.0], 2.0))
    a, b = SR.line([-2.0, 0.0, 0.0], [2.0, 0.0, 0.0], 0.7), SR.line([-2.0 + 2.0 * 0.7, 0.0, 0.0], [2.0, 0.0, 0.0], 1.3)
    return SR.batch((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])))


FACE = [-0.5, 0.75, -1.0, 0.5, 1.75, 1.0]
EDGE = [-0.5, 0.3, 0.4, 0.5, 1.0, 1.0]
POINT = [0.0, 0.5, 0.0, 0.0, 0.5, 0.0]
PENETRATED = [0.5, -0.25, -0.25, 1.0, 0.25, 0.25]
BYSTANDER = [-0.5, 1000.75, -1.0, 0.5, 1001.75, 1.0]  # the face box shifted by y = 1000
FLYBY_L = 2.0  # the trajectory reaches |x| = 2; no corner of the four near boxes lies further out


def check_flyby(be):
    for split in (False, True):
        so, T, C = flyby(split)

        def one(ob):
            out = near, obs, count, tested, flags = be.clearance(so, T, C, [ob], 1.0)
            print("split %s, obstacle %s: d_min %.17g t_min %.17g count %d tested %d" % (split, ob, near[0, 0], near[0, 1],
                                                                                       count[0], tested[0]))
            return out
        near, obs, count, tested, flags = one(FACE)
        assert (count[0], obs[0], tested[0], flags[0]) == (1, 0, 1, SEP_CLOSE)
        assert near[0, 0] == 0.75 and 0.75 <= near[0, 1] <= 1.25, near  # a flat minimum: attained anywhere in there
        near, obs, count, tested, flags = one(EDGE)
        assert (count[0], obs[0], tested[0]) == (1, 0, 1) and abs(near[0, 0] - 0.5) <= 1e-12, near
        near, obs, count, tested, flags = one(POINT)
        assert (count[0], obs[0], tested[0]) == (1, 0, 1)
        assert abs(near[0, 0] - 0.5) <= 1e-12 and abs(near[0, 1] - 1.0) <= 1e-9, near
        near, obs, count, tested, flags = one(PENETRATED)
        assert (count[0], obs[0], tested[0]) == (1, 0, 1)
        assert near[0, 0] ** 2 <= TOL * FLYBY_L ** 2 and 1.25 - 1e-6 <= near[0, 1] <= 1.5 + 1e-6, near
        out = one(BYSTANDER)
        none_rows(out, [0])
        assert out[3][0] == 0  # a straight line: any sound box bound culls it
        near, obs, count, tested, flags = be.clearance(so, T, C, [FACE, EDGE, POINT, PENETRATED, BYSTANDER], 1.0)
        assert (count[0], obs[0], tested[0], flags[0]) == (4, 3, 4, SEP_CLOSE), (count, obs, tested, flags)
        assert near[0, 0] ** 2 <= TOL * FLYBY_L ** 2


def check_strict(be):
    so, T, C = flyby()
    out = be.clearance(so, T, C, [EDGE], 0.5)
    print("edge at r_min 0.5:", out)
    assert out[2][0] == 0
    none_rows(out, [0])
    near, obs, count, tested, flags = be.clearance(so, T, C, [EDGE], float(np.nextafter(0.5, 1.0)))
    print("edge at r_min nextafter(0.5):", near, count)
    # a margin applied inward, or a slack on the wrong side, would lose the obstacle
    assert count[0] == 1 and obs[0] == 0 and near[0, 0] <= 0.5


# ---- case 3: chunk edges and the tie rule ----

LATTICE = tuple((n, n) for n in (1, 2, 63, 64, 65, 129)) + ((3, 129), (129, 3))


def lattice(B, K):
    """Vehicles hovering at x = i, rods [k + 0.25, k + 0.75] x {0} x {0}."""
    C = np.zeros((B, 3, 8))
    C[:, 0, 0] = np.arange(B)
    ob = np.zeros((K, 6))
    ob[:, 0], ob[:, 3] = np.arange(K) + 0.25, np.arange(K) + 0.75
    return np.arange(B + 1, dtype=np.int32), np.ones(B), C, ob


def lattice_want(B, K):
    i = np.arange(B)
    own, left = i < K, (i >= 1) & (i - 1 < K)
    count = own.astype(np.int32) + left.astype(np.int32)
    obs = np.where(left, i - 1, np.where(own, i, NEAR_NONE)).astype(np.int32)
    return count, obs


def check_lattice(be, B, K):
    so, T, C, ob = lattice(B, K)
    out = near, obs, count, tested, flags = be.clearance(so, T, C, ob, 1.0)
    want_count, want_obs = lattice_want(B, K)
    assert np.array_equal(count, want_count), (count, want_count)
    assert np.array_equal(obs, want_obs), (obs, want_obs)  # the lowest index on a stored tie
    assert np.array_equal(tested, count), (tested, count)  # the next rods are 1.25 away
    hit = count > 0
    assert (near[hit, 0] == 0.25).all() and ((near[hit, 1] >= 0.0) & (near[hit, 1] <= 1.0)).all()
    assert (flags[hit] == SEP_CLOSE).all()
    none_rows(out, np.flatnonzero(~hit))


# ---- case 4: the contract on solved trajectories ----

@functools.lru_cache(maxsize=None)
def contract_inputs(name):
    """bounds_ref.ragged48 (every M in 1..16 three times), rest to rest ("rest") or with
    bounds_ref.end_derivs48 ("end_derivs"), solved by the host backend as
    separation_ref.contract_case does, and K = 12 seeded boxes: centres uniform in the hull of
    the batch's continuous extents, sides 0.05 to 0.3 of the hull's side, the first three
    degenerate (a point, a rod along x, a plate normal to z)."""
    from trajectory_generator_ros2_amd.solver import Solver
    so, W, T = R.ragged48()
    ED = None if name == "rest" else R.end_derivs48()
    with Solver(host=True) as s:
        C, _, worst = s.solve(so, W, T, ED)
        assert worst == 0
        ext, _ = s.bounds(so, T, C)
    lo, hi = ext[:, 0:3].min(axis=0), ext[:, 3:6].max(axis=0)
    rng = np.random.default_rng(12 if name == "rest" else 13)
    K = 12
    centre = rng.uniform(lo, hi, (K, 3))
    side = rng.uniform(0.05, 0.3, (K, 3)) * (hi - lo)
    side[0, :] = 0.0
    side[1, 1:] = 0.0
    side[2, 2] = 0.0
    ob = np.concatenate([centre - side / 2, centre + side / 2], axis=1)
    for a in (so, T, C, ob, ext):
        a.setflags(write=False)
    return so, T, C, ob, ext, SR.batch_trajs(so, T, C)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{scale_name: (d2 [B, K], L [B, K])} over all 576 pairs, once per session."""
    so, T, C, ob, ext, trajs = contract_inputs(name)
    names = sorted(SCALES)
    B, K = len(trajs), len(ob)
    d2, L = np.empty((len(names), B, K)), np.empty((len(names), B, K))
    for b in range(B):
        for k in range(K):
            x, y = pair_ref(trajs[b], ob[k], [SCALES[n] for n in names])
            d2[:, b, k], L[:, b, k] = x, y
    d2.setflags(write=False)
    L.setflags(write=False)
    return {n: (d2[q], L[q]) for q, n in enumerate(names)}


def choose_r_min(d_ref, L2):
    """The midpoint of the gap in the sorted reference distances nearest the 20th percentile at
    which no pair has |d_ref^2 - r^2| <= TOL L^2."""
    ds = np.sort(d_ref.ravel())
    k0 = int(round(0.2 * (len(ds) - 1)))
    for k in sorted(range(len(ds) - 1), key=lambda k: abs(k - k0)):
        if ds[k + 1] == ds[k]:
            continue
        r = 0.5 * (ds[k] + ds[k + 1])
        if not (np.abs(d_ref ** 2 - r * r) <= TOL * L2).any():
            return float(r)
    raise AssertionError("no usable gap in the reference distances")


def check_contract(be, name, scale_name, what):
    so, T, C, ob, ext, trajs = contract_inputs(name)
    scale = SCALES[scale_name]
    d2_ref, L = reference(name)[scale_name]
    B, K = d2_ref.shape
    L2 = L * L
    d_ref = np.sqrt(d2_ref)
    r_min = choose_r_min(d_ref, L2)
    # the conditions, asserted on the reference alone
    assert not (np.abs(d2_ref - r_min ** 2) <= TOL * L2).any()
    count_ref = (d_ref < r_min).sum(axis=1)
    assert (count_ref > 0).any() and (count_ref == 0).any()
    near, obs, count, tested, flags = be.clearance(so, T, C, ob, r_min, scale)
    share = tested.sum() / (B * K)
    print("%s %s/%s: r_min %.6g, tested %d of %d pairs (%.3f), %d within r_min" % (what, name, scale_name, r_min,
                                                                                  tested.sum(), B * K, share, count.sum()))
    assert np.array_equal(count, count_ref), (count, count_ref)  # culling soundness
    assert np.array_equal(flags, np.where(count_ref > 0, SEP_CLOSE, 0))
    assert ((count <= tested) & (tested <= K)).all()
    worst1 = worst3 = 0.0
    for i in range(B):
        if count_ref[i] == 0:
            assert near[i, 0] == np.inf and near[i, 1] == 0.0 and obs[i] == NEAR_NONE
            continue
        k = int(obs[i])
        kmin = int(d2_ref[i].argmin())
        assert 0 <= k < K and d2_ref[i, k] - d2_ref[i, kmin] <= 2 * TOL * max(L2[i, k], L2[i, kmin]), (i, k, kmin)
        e1 = abs(near[i, 0] ** 2 - d2_ref[i, kmin]) / L2[i, kmin]
        assert 0.0 <= near[i, 1] <= ext[i, 9], (i, near[i, 1], ext[i, 9])
        e3 = float(abs(dist2_at(trajs[i], ob[k], near[i, 1], scale) - LD(near[i, 0]) ** 2)) / L2[i, k]
        worst1, worst3 = max(worst1, e1), max(worst3, e3)
    print("%s %s/%s: d_min^2 off by %.3g x L^2, dist(t_min)^2 off by %.3g x L^2" % (what, name, scale_name, worst1,
                                                                                   worst3))
    assert worst1 <= TOL and worst3 <= TOL, (worst1, worst3)
    return r_min, (near, obs, count, tested, flags)


# ---- case 5: unusable trajectories and obstacles ----

UNUSABLE = (3, 7, 10)  # a NaN coefficient in the last segment, a zero time, a NaN coefficient in the first segment
BAD_OBS = (2, 9)       # positions of the spoiled obstacles in the list of 14: a NaN entry, lo > hi


def unusable_case():
    so, T, C, ob, _, _ = contract_inputs("rest")
    B = 14
    so, T, C = so[:B + 1].copy(), T[:so[B]].copy(), C[:so[B]].copy()
    good = (T.copy(), C.copy())
    C[so[UNUSABLE[0] + 1] - 1, 1, 5] = np.nan
    T[so[UNUSABLE[1]]] = 0.0
    C[so[UNUSABLE[2]], 2, 0] = np.nan
    keep = np.array([b for b in range(B) if b not in UNUSABLE])
    segs = np.concatenate([np.arange(so[b], so[b + 1]) for b in keep])
    so2 = np.concatenate([[0], np.cumsum(np.diff(so)[keep])]).astype(np.int32)
    spoiled = [ob[0].copy(), ob[5].copy()]
    spoiled[0][4] = np.nan
    spoiled[1][[2, 5]] = spoiled[1][[5, 2]] + [1.0, 0.0]  # lo_z = hi_z + 1 > hi_z = lo_z
    ob14 = np.insert(np.asarray(ob), [BAD_OBS[0], BAD_OBS[1] - 1], spoiled, axis=0)
    okeep = np.array([k for k in range(14) if k not in BAD_OBS])
    assert np.array_equal(ob14[okeep], ob)
    return (so, T, C, ob14), (so2, good[0][segs], good[1][segs], np.asarray(ob)), keep, okeep


def check_unusable(be, r_min=1.0):
    (so, T, C, ob14), (so2, T2, C2, ob2), keep, okeep = unusable_case()
    near, obs, count, tested, flags = be.clearance(so, T, C, ob14, r_min)
    for b in UNUSABLE:
        assert flags[b] == SEP_NONFINITE and np.isnan(near[b]).all() and obs[b] == NEAR_NONE, (b, flags[b], near[b])
        assert count[b] == 0 and tested[b] == 0
    near2, obs2, count2, tested2, flags2 = be.clearance(so2, T2, C2, ob2, r_min)
    assert count2.sum() > 0 and (count2 == 0).any()  # the horizon finds something, so the comparison says something
    assert not (flags2 & CLR_BAD_OBSTACLE).any()
    assert np.array_equal(near[keep], near2)
    assert np.array_equal(obs[keep], np.where(obs2 >= 0, okeep[np.maximum(obs2, 0)], NEAR_NONE))
    assert np.array_equal(count[keep], count2) and np.array_equal(tested[keep], tested2)
    assert np.array_equal(flags[keep], flags2 | CLR_BAD_OBSTACLE)
