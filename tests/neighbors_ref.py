"""Shared inputs and checks of the swarm neighbour search (tgms_neighbors_batch*), used by
test_neighbors_host.py and test_gpu_neighbors.py.  The reference of every comparison is the
separation call over all ordered pairs (i, j), i != j, reduced here in NumPy with the lowest-j
tie-break; that call is pinned to separation_ref.py by its own tests.

A backend is any object with
    neighbors(so, T, C, r_min, start_times=None, scale=None) -> near, nbr, count, tested, flags
    separation(so, T, C, pairs, start_times=None, scale=None) -> sep [P, 2]
(a Solver has both; the GPU file wraps the device entry points the same way)."""
import functools

import numpy as np

import separation_ref as SR
from trajectory_generator_ros2_amd import NEAR_NONE, SEP_CLOSE, SEP_NONFINITE

TOL = 1e-9  # the project's tolerance on d^2, in L^2 (include/tgms.h)
SCALES = {"unit": None, "third": (1.0, 1.0, 1.0 / 3.0)}


def ordered_pairs(B):
    i, j = np.meshgrid(np.arange(B), np.arange(B), indexing="ij")
    m = i != j
    return np.stack([i[m], j[m]], axis=1).astype(np.int32)


def reduce_rows(B, pairs, sep, r_min):
    """(d [B], t [B], nbr [B], count [B]) of the all-pairs records: strict d < r_min on the
    stored value, the smallest d, ties to the lowest j; +inf, 0, NEAR_NONE, 0 for nobody."""
    d, t = np.full(B, np.inf), np.zeros(B)
    nbr, count = np.full(B, NEAR_NONE, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for (i, j), (dm, tm) in zip(pairs, sep):
        if dm < r_min:
            count[i] += 1
            if dm < d[i] or (dm == d[i] and j < nbr[i]):
                d[i], t[i], nbr[i] = dm, tm, j
    return d, t, nbr, count


def none_rows(out, rows):
    near, nbr, count, tested, flags = out
    for i in rows:
        assert near[i, 0] == np.inf and near[i, 1] == 0.0, (i, near[i])
        assert nbr[i] == NEAR_NONE and count[i] == 0 and flags[i] == 0, (i, nbr[i], count[i], flags[i])


# ---- case 1 / 2: the crossing and a bystander ----

def crossing3(split=False):
    so, T, C = SR.crossing(split)
    trajs = [(C[so[b]:so[b + 1]], T[so[b]:so[b + 1]]) for b in range(2)]
    return SR.batch(*trajs, SR.line([0.0, 1000.0, 0.0], [1.0, 0.0, 0.0], 2.0))


def check_crossing(be):
    for split in (False, True):
        so, T, C = crossing3(split)
        out = near, nbr, count, tested, flags = be.neighbors(so, T, C, 1.0)
        assert list(count) == [1, 1, 0] and list(nbr) == [1, 0, NEAR_NONE]
        assert list(tested) == [1, 1, 0], tested  # straight lines: any sound box bound culls the bystander
        assert list(flags) == [SEP_CLOSE, SEP_CLOSE, 0]
        assert np.allclose(near[:2, 0], 0.5, rtol=0, atol=1e-12) and np.allclose(near[:2, 1], 1.0, rtol=0, atol=1e-9)
        none_rows(out, [2])


def check_strict(be):
    so, T, C = crossing3()
    out = be.neighbors(so, T, C, 0.5)
    assert list(out[2]) == [0, 0, 0]
    none_rows(out, [0, 1, 2])
    near, nbr, count, tested, flags = be.neighbors(so, T, C, float(np.nextafter(0.5, 1.0)))
    # the box distance is exactly 0.5: a margin applied inward would lose the pair
    assert list(count) == [1, 1, 0] and near[0, 0] == 0.5 and near[1, 0] == 0.5
    assert list(nbr) == [1, 0, NEAR_NONE]


# ---- case 3: a lattice of hovering vehicles ----

LATTICE_B = (1, 2, 63, 64, 65, 129)


def lattice(B):
    C = np.zeros((B, 3, 8))
    C[:, 0, 0] = np.arange(B)
    return np.arange(B + 1, dtype=np.int32), np.ones(B), C


def check_lattice(be, B):
    so, T, C = lattice(B)
    out = near, nbr, count, tested, flags = be.neighbors(so, T, C, 1.5)
    if B == 1:
        none_rows(out, [0])
        assert tested[0] == 0
        return
    want = np.full(B, 2)
    want[0] = want[-1] = 1
    assert np.array_equal(count, want)
    assert np.array_equal(tested, count), (tested, count)  # the next vehicles are 2.0 away
    assert (near[:, 0] == 1.0).all()
    want_nbr = np.arange(B) - 1
    want_nbr[0] = 1
    assert np.array_equal(nbr, want_nbr)
    assert (flags == SEP_CLOSE).all()
    assert ((near[:, 1] >= 0.0) & (near[:, 1] <= 1.0)).all()


# ---- case 4: start times and held ends ----

def held_case(shift=0.0, stagger=0.0):
    """0 flies (0,0,0) -> (5,0,0) in 1 s and stays there; 1 flies x = 5.25 from y = -10 at 2 m/s
    for 10 s, starting at 3 + shift: it passes the landed vehicle at 0.25 m, 5 s after its
    start, whatever the shift.  2 and 3 fly at 1 m/s for 8 s through the same point (0, 0, 100)
    4 s after their starts, 2 along x from -4 and 3 along y from -4: at equal starts they meet
    (d = 0); their distance is stagger / sqrt(2) while both fly, and once the stagger exceeds
    the flight time the first has landed at (4, 0, 100), 4 m from the other's line.  (Two
    vehicles on the very same line can never be clear under the held-end rule: the later one
    waits on, or flies into, a point the other occupies.)  All numbers are exact in fp64."""
    b = SR.batch(SR.line([0.0, 0.0, 0.0], [5.0, 0.0, 0.0], 1.0), SR.line([5.25, -10.0, 0.0], [0.0, 2.0, 0.0], 10.0),
                 SR.line([-4.0, 0.0, 100.0], [1.0, 0.0, 0.0], 8.0), SR.line([0.0, -4.0, 100.0], [0.0, 1.0, 0.0], 8.0))
    return b + (np.array([0.0, 3.0 + shift, 0.0, stagger]),)


def check_held(be):
    r_min = 0.5
    for shift in (0.0, 100.0):
        so, T, C, t0 = held_case(shift=shift)
        near, nbr, count, tested, flags = be.neighbors(so, T, C, r_min, t0)
        assert list(nbr) == [1, 0, 3, 2] and list(count) == [1, 1, 1, 1]
        assert near[0, 0] == 0.25 and near[1, 0] == 0.25
        assert abs(near[0, 1] - (8.0 + shift)) <= 1e-9 * (8.0 + shift)
        assert near[2, 0] <= 1e-7 and near[3, 0] <= 1e-7 and abs(near[2, 1] - 4.0) <= 1e-6
    # staggered by more than the flight time (8 s) plus r_min / speed (0.5 s): clear
    so, T, C, t0 = held_case(stagger=8.75)
    out = be.neighbors(so, T, C, r_min, t0)
    assert list(out[1]) == [1, 0, NEAR_NONE, NEAR_NONE] and list(out[2]) == [1, 1, 0, 0]
    none_rows(out, [2, 3])
    # staggered by less than r_min / speed * sqrt(2): still in conflict, at stagger / sqrt(2)
    so, T, C, t0 = held_case(stagger=0.5)
    near, nbr, count, tested, flags = be.neighbors(so, T, C, r_min, t0)
    assert list(nbr) == [1, 0, 3, 2] and abs(near[2, 0] - 0.5 / np.sqrt(2.0)) <= 1e-12


# ---- case 5: the contract on solved trajectories ----

@functools.lru_cache(maxsize=None)
def contract_inputs(name):
    c = SR.contract_case(name)
    return c["so"], c["T"], c["C"], c["t0"], c["trajs"]


def pair_L(be_bounds, so, T, C, scale):
    """L of every vehicle: the largest scaled coordinate magnitude it reaches (continuous extents)."""
    ext, _ = be_bounds(so, T, C)
    s = np.ones(3) if scale is None else np.asarray(scale)
    return np.maximum(np.abs(ext[:, 0:3]) * s, np.abs(ext[:, 3:6]) * s).max(axis=1)


def choose_r_min(B, pairs, d_ref, L2):
    """The midpoint of the two consecutive sorted reference values nearest the 20th percentile
    such that, on the reference alone, no pair has |d^2 - r^2| <= TOL L^2 and no row's best two
    neighbours within r are closer than TOL L^2 to each other on d^2; else the next gap."""
    order = np.argsort(d_ref, kind="stable")
    ds = d_ref[order]
    k0 = int(round(0.2 * (len(ds) - 1)))
    for k in range(k0, len(ds) - 1):
        if ds[k + 1] == ds[k]:
            continue
        r = 0.5 * (ds[k] + ds[k + 1])
        if (np.abs(d_ref ** 2 - r * r) <= TOL * L2).any():
            continue
        ok = True
        for i in range(B):
            m = (pairs[:, 0] == i) & (d_ref < r)
            d2 = np.sort(d_ref[m] ** 2)
            if len(d2) >= 2 and d2[1] - d2[0] <= TOL * L2[m].max():
                ok = False
        if ok:
            return r
    raise AssertionError("no usable gap in the reference distances")


def check_contract(be, ref_sep, bounds, name, scale_name, what):
    so, T, C, t0, trajs = contract_inputs(name)
    scale = SCALES[scale_name]
    B = len(so) - 1
    pairs = ordered_pairs(B)
    sep = ref_sep(name, scale_name)
    assert sep.shape == (B * (B - 1), 2) and np.isfinite(sep).all()
    Lb = pair_L(bounds, so, T, C, scale)
    L2 = np.maximum(Lb[pairs[:, 0]], Lb[pairs[:, 1]]) ** 2
    r_min = choose_r_min(B, pairs, sep[:, 0], L2)
    # the condition, asserted on the reference alone
    assert not (np.abs(sep[:, 0] ** 2 - r_min ** 2) <= TOL * L2).any()
    d, t, nbr_ref, count_ref = reduce_rows(B, pairs, sep, r_min)
    near, nbr, count, tested, flags = be.neighbors(so, T, C, r_min, t0, scale)
    assert np.array_equal(count, count_ref)
    assert np.array_equal(nbr, nbr_ref)
    assert np.array_equal(flags, np.where(count_ref > 0, SEP_CLOSE, 0))
    assert ((count <= tested) & (tested <= B - 1)).all()
    s = np.ones(3, dtype=SR.LD) if scale is None else np.asarray(scale, dtype=SR.LD)
    worst1 = worst3 = 0.0
    for i in range(B):
        if nbr_ref[i] == NEAR_NONE:
            assert near[i, 0] == np.inf and near[i, 1] == 0.0
            continue
        j = int(nbr[i])
        l2 = max(Lb[i], Lb[j]) ** 2
        e1 = abs(near[i, 0] ** 2 - d[i] ** 2) / l2
        lo, hi = SR.window(trajs[i], trajs[j])
        assert lo <= near[i, 1] <= hi, (i, j, near[i, 1], lo, hi)
        tt = np.atleast_1d(SR.LD(near[i, 1]))
        dd = (trajs[i].pos(tt) - trajs[j].pos(tt)) * s
        e3 = float(abs((dd * dd).sum() - SR.LD(near[i, 0]) ** 2)) / l2
        worst1, worst3 = max(worst1, e1), max(worst3, e3)
    share = tested.sum() / (B * (B - 1))
    print("%s %s/%s: r_min %.6g, d_min^2 off by %.3g x L^2, dist(t_min)^2 off by %.3g x L^2, tested %d of %d "
          "ordered pairs (%.3f), %d within r_min" % (what, name, scale_name, r_min, worst1, worst3, tested.sum(),
                                                     B * (B - 1), share, count.sum()))
    assert worst1 <= TOL and worst3 <= TOL, (worst1, worst3)
    return near, nbr, count, tested, flags


# ---- case 6: unusable vehicles ----

UNUSABLE = (3, 7, 10)  # a NaN coefficient in the last segment, a zero time, a NaN start time


def unusable_case():
    so, T, C, t0, _ = contract_inputs("rest")
    B = 14
    so, T, C, t0 = so[:B + 1].copy(), T[:so[B]].copy(), C[:so[B]].copy(), t0[:B].copy()
    good = (so, T.copy(), C.copy(), t0.copy())
    C[so[UNUSABLE[0] + 1] - 1, 1, 5] = np.nan
    T[so[UNUSABLE[1]]] = 0.0
    t0[UNUSABLE[2]] = np.nan
    keep = np.array([b for b in range(B) if b not in UNUSABLE])
    segs = np.concatenate([np.arange(so[b], so[b + 1]) for b in keep])
    so2 = np.concatenate([[0], np.cumsum(np.diff(so)[keep])]).astype(np.int32)
    return (so, T, C, t0), (so2, good[1][segs], good[2][segs], good[3][keep]), keep


def check_unusable(be, r_min=3.0):
    (so, T, C, t0), (so2, T2, C2, t02), keep = unusable_case()
    near, nbr, count, tested, flags = be.neighbors(so, T, C, r_min, t0)
    for b in UNUSABLE:
        assert flags[b] == SEP_NONFINITE and np.isnan(near[b]).all() and nbr[b] == NEAR_NONE and count[b] == 0
    near2, nbr2, count2, tested2, flags2 = be.neighbors(so2, T2, C2, r_min, t02)
    assert count2.sum() > 0  # the horizon finds something, so the comparison says something
    assert np.array_equal(near[keep], near2)
    assert np.array_equal(nbr[keep], np.where(nbr2 >= 0, keep[np.maximum(nbr2, 0)], NEAR_NONE))
    assert np.array_equal(count[keep], count2) and np.array_equal(tested[keep], tested2)
    assert np.array_equal(flags[keep], flags2)
