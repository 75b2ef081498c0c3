"""Shared inputs, checks and reference of the corridor subdivision (tgms_corridor_subdivide_batch*),
used by test_subdivide_host.py and test_gpu_subdivide.py.  A backend is any object with
    corridor_subdivide(so, W, origin, h, values, r_free, max_depth, seg_times=None)
        -> seg_offsets', waypoints', seg_times' (or None), parent, seg_flags, flags
(a Solver has it; the GPU file wraps the device entry point the same way).

The reference follows include/tgms.h literally and shares nothing with the library's core: the
points P(i) in plain Python floats (one rounding per operation), the seed per axis, the non-free
nodes of a seed counted by slicing values < float32(r_free) (NaN counts as non-free; no table),
need() and the leaves by recursion on the pieces, the depth tried from max_depth downwards."""
import functools

import numpy as np

from trajectory_generator_ros2_amd import (FEAS_NONFINITE, INF_BLOCKED, INF_OUTSIDE, SUB_BLOCKED, SUB_DONE, SUB_FULL,
                                           SUB_OUTSIDE)
from trajectory_generator_ros2_amd import synthetic as S

MAX_SEGMENTS = 16  # TGMS_MAX_SEGMENTS

NAMES = ("seg_offsets", "waypoints", "seg_times", "parent", "seg_flags", "flags")


# ---- the reference ----

def point(w0, w1, i):
    if i == 0:
        return float(w0)
    if i == 16:
        return float(w1)
    d = float(w1) + (-float(w0))
    p = (i / 16.0) * d
    return float(w0) + p


def seed_axis(o, h, a, b):
    mn, mx = (b if b < a else a), (b if b > a else a)
    lo = float(np.floor((mn - o) / h))
    if o + h * lo > mn:
        lo -= 1.0
    hi = float(np.ceil((mx - o) / h))
    if o + h * hi < mx:
        hi += 1.0
    return lo, hi


class Leg:
    def __init__(self, origin, h, notfree, w0, w1):
        self.o, self.h, self.nf = [float(x) for x in origin], float(h), notfree
        self.w0, self.w1 = [float(x) for x in w0], [float(x) for x in w1]
        d = [b + (-a) for a, b in zip(self.w0, self.w1)]
        self.status = 0
        if not np.isfinite(self.w0 + self.w1 + d).all():
            self.status = FEAS_NONFINITE
        elif self.box(0, 16) is None:
            self.status = SUB_OUTSIDE

    def box(self, i0, i1):
        """The seed of P(i0), P(i1) as slices (z, y, x), or None where it leaves the grid."""
        sl = []
        for a in range(3):
            lo, hi = seed_axis(self.o[a], self.h, point(self.w0[a], self.w1[a], i0), point(self.w0[a], self.w1[a], i1))
            if not (lo >= 0.0 and hi <= self.nf.shape[2 - a] - 1):
                return None
            sl.append(slice(int(lo), int(hi) + 1))
        return tuple(sl[::-1])

    @functools.lru_cache(maxsize=None)
    def clear(self, k, j):
        step = 16 >> k
        b = self.box(j * step, (j + 1) * step)
        return b is not None and int(self.nf[b].sum()) == 0

    def need(self, D, k=0, j=0):
        if self.status or self.clear(k, j) or k == D:
            return 1
        return self.need(D, k + 1, 2 * j) + self.need(D, k + 1, 2 * j + 1)

    def leaves(self, D, k=0, j=0):
        """[(i0, i1, flag)] left to right."""
        step = 16 >> k
        if self.status:
            return [(0, 16, self.status)]
        if self.clear(k, j):
            return [(j * step, (j + 1) * step, 0)]
        if k == D:
            return [(j * step, (j + 1) * step, SUB_BLOCKED)]
        return self.leaves(D, k + 1, 2 * j) + self.leaves(D, k + 1, 2 * j + 1)


def reference(so, W, T, origin, h, values, r_free, max_depth, counts=None):
    """The six outputs; counts (a list) receives per trajectory [sum_s need(s, D) for D = 0..4]."""
    so = np.asarray(so, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(values, dtype=np.float32)
    notfree = ~(v >= np.float32(r_free))
    so2, W2, T2, parent, seg_flags, flags = [0], [], [], [], [], []
    for b in range(len(so) - 1):
        legs = [Leg(origin, h, notfree, W[s + b], W[s + b + 1]) for s in range(so[b], so[b + 1])]
        sums = [sum(leg.need(D) for leg in legs) for D in range(5)]
        if counts is not None:
            counts.append(sums)
        D = next(D for D in range(max_depth, -1, -1) if sums[D] <= MAX_SEGMENTS)
        fl = SUB_FULL if D < max_depth else 0
        n0 = len(parent)
        for m, leg in enumerate(legs):
            s = int(so[b]) + m
            for i0, i1, f in leg.leaves(D):
                W2.append([point(leg.w0[a], leg.w1[a], i0) if i0 else W[s + b, a] for a in range(3)])
                if T is not None:
                    T2.append(T[s] if i1 - i0 == 16 else T[s] * ((i1 - i0) / 16.0))
                parent.append(s)
                seg_flags.append(f)
                fl |= f
        W2.append(W[so[b + 1] + b])
        if len(parent) - n0 > len(legs):
            fl |= SUB_DONE
        flags.append(fl)
        so2.append(len(parent))
    return (np.array(so2, np.int32), np.array(W2, np.float64).reshape(-1, 3),
            None if T is None else np.array(T2, np.float64), np.array(parent, np.int32).reshape(-1),
            np.array(seg_flags, np.int32).reshape(-1), np.array(flags, np.int32).reshape(-1))


# ---- comparisons: everything to the bit ----

def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if w is None or g is None:
            assert g is None and w is None, (what, name)
            continue
        assert same_bits(g, w), (what, name, g, w)


def check_equal(be, so, W, T, origin, h, values, r_free, max_depth, what=""):
    got = be.corridor_subdivide(so, W, origin, h, values, r_free, max_depth, T)
    want = reference(so, W, T, origin, h, values, r_free, max_depth)
    assert_same(got, want, what)
    return got


# ---- constructed cases ----

G_N, G_ORIGIN, G_H = (17, 17, 17), (0.0, 0.0, 0.0), 1.0


def g_values(nodes=(), fill=1.0, bad=0.0):
    v = np.full(G_N[::-1], fill, np.float32)
    for i, j, k in nodes:
        v[k, j, i] = bad
    return v


def path(points):
    """One trajectory through `points`: (so, W, T) with times 1, 2, 3, ..."""
    W = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    M = len(W) - 1
    return np.array([0, M], np.int32), W, 1.0 + np.arange(M, dtype=np.float64)


def batch(paths):
    so, W, T = [0], [], []
    for p in paths:
        _, w, t = path(p)
        so.append(so[-1] + len(t))
        W.append(w)
        T.append(t * (1.0 + 0.25 * len(so)))
    return np.array(so, np.int32), np.concatenate(W), np.concatenate(T)


def ragged_in_grid(B, m_hi=16, seed=7):
    """A ragged batch inside the 17^3 grid, M mixed 1..m_hi."""
    rng = np.random.default_rng(seed)
    Ms = rng.integers(1, m_hi + 1, size=B)
    so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    W = rng.uniform(0.25, 15.75, size=(int(so[-1]) + B, 3))
    T = rng.uniform(0.5, 4.0, size=int(so[-1]))
    return so, W, T


def random_nodes(count, seed=11):
    rng = np.random.default_rng(seed)
    return [tuple(int(x) for x in rng.integers(0, 17, size=3)) for _ in range(count)]


def check_empty_map(be):
    so, W, T = ragged_in_grid(9)
    for depth in (0, 4):
        got = be.corridor_subdivide(so, W, G_ORIGIN, G_H, g_values(), 0.3, depth, T)
        assert_same(got, (so, W, T, np.arange(so[-1], dtype=np.int32), np.zeros(so[-1], np.int32),
                          np.zeros(len(so) - 1, np.int32)), "empty map")


def check_hand(be):
    """One leg (0.5, 0.5, 0.5) -> (8.5, 8.5, 0.5), the node (8, 1, 0) not free: the leg's seed x, y in
    0..9 holds it, the halves' seeds 0..5 and 4..9 do not."""
    so, W, T = path([(0.5, 0.5, 0.5), (8.5, 8.5, 0.5)])
    T[0] = 3.0
    v = g_values([(8, 1, 0)])
    so2, W2, T2, parent, seg_flags, flags = be.corridor_subdivide(so, W, G_ORIGIN, G_H, v, 0.3, 4, T)
    assert list(so2) == [0, 2] and list(parent) == [0, 0] and list(seg_flags) == [0, 0] and list(flags) == [SUB_DONE]
    assert same_bits(W2, np.array([[0.5, 0.5, 0.5], [4.5, 4.5, 0.5], [8.5, 8.5, 0.5]]))
    assert same_bits(T2, np.array([1.5, 1.5]))
    got = check_equal(be, so, W, T, G_ORIGIN, G_H, v, 0.3, 0, "hand, depth 0")
    assert list(got[0]) == [0, 1] and list(got[4]) == [SUB_BLOCKED] and list(got[5]) == [SUB_BLOCKED]
    assert same_bits(got[1], W) and same_bits(got[2], T)


def check_on_chord(be):
    """Non-free nodes on the chord itself: some leaf of depth max_depth stays blocked, and a clear
    sibling is not split further."""
    so, W, T = path([(0.5, 0.5, 0.5), (15.5, 15.5, 0.5), (0.5, 15.5, 8.5)])
    v = g_values([(5, 5, 0), (5, 5, 1), (12, 4, 2)], bad=np.nan)
    for depth in range(5):
        so2, W2, T2, parent, seg_flags, flags = check_equal(be, so, W, T, G_ORIGIN, G_H, v, 0.3, depth, "on chord")
        k = np.round(np.log2(T[parent] / T2)).astype(int)
        assert (seg_flags[parent == 0] == SUB_BLOCKED).any() and (k[seg_flags == SUB_BLOCKED] == depth).all()
        assert flags[0] & SUB_BLOCKED and not flags[0] & SUB_FULL
        if depth >= 2:
            assert (k[(parent == 0) & (seg_flags == 0)] < depth).any()


def zigzag(legs, z=1.5):
    """Legs between (1.5, 1.5, z) and (9.5, 9.5, z): with the node (5, 2, k) not free a leg is blocked
    by its box at depth 0, its first half (lattice 1..6) at depth 1, and no quarter (1..4, 3..6) is:
    need = 1, 2, 3, 3, 3."""
    return [(1.5, 1.5, z) if i % 2 == 0 else (9.5, 9.5, z) for i in range(legs + 1)]


def check_budget(be):
    v = g_values([(5, 2, 1), (5, 2, 2)])
    so, W, T = batch([zigzag(10), zigzag(5), zigzag(6), zigzag(16), zigzag(16, z=8.5)])
    counts = []
    reference(so, W, T, G_ORIGIN, G_H, v, 0.3, 4, counts)
    assert counts[0] == [10, 20, 30, 30, 30] and counts[1] == [5, 10, 15, 15, 15] and counts[4] == [16] * 5
    so2, _, _, parent, seg_flags, flags = check_equal(be, so, W, T, G_ORIGIN, G_H, v, 0.3, 4, "budget")
    M2 = np.diff(so2)
    for b, sums in enumerate(counts):
        D = max(D for D in range(5) if sums[D] <= MAX_SEGMENTS)
        assert M2[b] == sums[D] <= MAX_SEGMENTS and (D == 4 or sums[D + 1] > MAX_SEGMENTS)
        assert bool(flags[b] & SUB_FULL) == (D < 4)
    assert list(M2) == [10, 15, 12, 16, 16]
    assert list(flags) == [SUB_FULL | SUB_BLOCKED, SUB_DONE, SUB_DONE | SUB_FULL | SUB_BLOCKED, SUB_FULL | SUB_BLOCKED, 0]
    # a lower max_depth than the budget allows: no FULL
    got = check_equal(be, so[1:3] - so[1], W[11:17], T[10:15], G_ORIGIN, G_H, v, 0.3, 1, "budget, depth 1")
    assert list(got[5]) == [SUB_DONE | SUB_BLOCKED]


def check_isolation(be):
    """A leg with a waypoint off the grid, a NaN waypoint, an infinite difference: kept whole and
    flagged, the other legs of the trajectory as without it."""
    v = g_values([(5, 2, 1)])
    clean = zigzag(4) + [(1.5, 9.5, 1.5)]
    ref = be.corridor_subdivide(*path(clean)[:2], G_ORIGIN, G_H, v, 0.3, 4, path(clean)[2])
    for bad, flag in (((20.5, 9.5, 1.5), SUB_OUTSIDE), ((np.nan, 9.5, 1.5), FEAS_NONFINITE),
                      ((1e308, 9.5, 1.5), FEAS_NONFINITE)):
        pts = list(clean)
        pts[5] = bad
        if bad[0] == 1e308:
            pts[4] = (-1e308, 9.5, 1.5)  # finite waypoints, an infinite difference
        so, W, T = path(pts)
        so2, W2, T2, parent, seg_flags, flags = check_equal(be, so, W, T, G_ORIGIN, G_H, v, 0.3, 4, "isolation")
        touched = 2 if bad[0] == 1e308 else 1  # legs 3 and 4, or leg 4 alone
        keep = parent < 5 - touched
        assert same_bits(W2[:keep.sum()], ref[1][:keep.sum()]) and same_bits(T2[keep], ref[2][:keep.sum()])
        assert np.array_equal(seg_flags[keep], ref[4][:keep.sum()])
        assert seg_flags[-1] == flag and parent[-1] == 4 and same_bits(T2[-1:], T[-1:])
        assert flags[0] == SUB_DONE | flag | (SUB_OUTSIDE if touched == 2 else 0)


def check_times(be):
    so, W, T = ragged_in_grid(6, seed=3)
    v = g_values(random_nodes(40))
    so2, W2, T2, parent, seg_flags, flags = check_equal(be, so, W, T, G_ORIGIN, G_H, v, 0.3, 4, "times")
    assert (flags & SUB_DONE).any()
    for s in range(int(so[-1])):
        t = T2[parent == s]
        assert all(T[s] / x in (1.0, 2.0, 4.0, 8.0, 16.0) for x in t) and sum(16.0 / (T[s] / x) for x in t) == 16.0
        if len(t) == 1:
            assert same_bits(t, T[s:s + 1])
    got = check_equal(be, so, W, None, G_ORIGIN, G_H, v, 0.3, 4, "no times")
    assert got[2] is None and same_bits(got[1], W2)


def check_random(be, depth, B=24, shift=0.0, seed=5):
    so, W, T = ragged_in_grid(B, seed=seed)
    W = W + shift
    return check_equal(be, so, W, T, G_ORIGIN, G_H, g_values(random_nodes(60), bad=0.25), 0.3, depth, "random")


# ---- the room: a round trip through the inflation call, and the certificate ----

R_N, R_ORIGIN, R_H, R_FREE = (32, 32, 32), (-6.0, -6.0, -0.5), 0.4, 0.3
R_BOXES = [[-3.0, -3.5, 0.0, -2.2, -2.6, 2.4], [1.5, 0.5, 1.0, 2.3, 1.4, 5.5], [-1.0, 2.5, 0.0, 0.2, 3.3, 3.0],
           [2.8, -3.8, 2.0, 3.6, -3.0, 5.0]]


@functools.lru_cache(maxsize=None)
def room():
    so, W, T = S.ragged_batch(64)
    return so, W, T, S.box_field(R_BOXES, R_ORIGIN, R_H, R_N)


@functools.lru_cache(maxsize=None)
def room_reference():
    so, W, T, v = room()
    return reference(so, W, T, R_ORIGIN, R_H, v, R_FREE, 4)


def check_round_trip(be, inflater=None):
    """corridor_inflate on the output: INF_BLOCKED exactly where SUB_BLOCKED is, INF_OUTSIDE exactly
    where SUB_OUTSIDE is."""
    so, W, T, v = room()
    got = be.corridor_subdivide(so, W, R_ORIGIN, R_H, v, R_FREE, 4, T)
    assert_same(got, room_reference(), "room")
    so2, W2, _, _, seg_flags, flags = got
    _, _, _, inf_seg, inf_fl = (inflater or be).corridor_inflate(so2, W2, R_ORIGIN, R_H, v, R_FREE, 2)
    assert np.array_equal((inf_seg & INF_BLOCKED) != 0, (seg_flags & SUB_BLOCKED) != 0)
    assert np.array_equal((inf_seg & INF_OUTSIDE) != 0, (seg_flags & SUB_OUTSIDE) != 0)
    assert np.array_equal((inf_fl & INF_BLOCKED) != 0, (flags & SUB_BLOCKED) != 0)
    assert (seg_flags & SUB_BLOCKED).any() and (flags & SUB_DONE).any()


def check_certificate(be):
    """phi at 33 points along every unflagged output chord is >= float32(r_free), to the field
    call's own rounding bound 1e-9 (F + L (P + h)); at least a quarter of the segments are unflagged."""
    import field_ref as FR
    so, W, T, v = room()
    ref = room_reference()
    assert (ref[4] == 0).sum() * 4 >= len(ref[4]), "the scene itself must leave a quarter unflagged"
    so2, W2, _, _, seg_flags, _ = be.corridor_subdivide(so, W, R_ORIGIN, R_H, v, R_FREE, 4, T)
    rows = np.arange(so2[-1]) + np.repeat(np.arange(len(so2) - 1), np.diff(so2))
    free = np.flatnonzero(seg_flags == 0)
    assert len(free) * 4 >= len(seg_flags)
    lam = np.linspace(0.0, 1.0, 33)[None, :, None]
    P = (W2[rows[free]][:, None, :] * (1.0 - lam) + W2[rows[free] + 1][:, None, :] * lam).reshape(-1, 3)
    eps = 1e-9 * (float(np.abs(v).max()) + FR.lipschitz(v, R_H) * (float(np.abs(P).max()) + R_H))
    assert FR.phi(R_ORIGIN, R_H, v, P).min() >= float(np.float32(R_FREE)) - eps


def check_arguments(be, TgmsError, ERR_INVALID_ARG):
    so, W, T = path([(0.5, 0.5, 0.5), (8.5, 8.5, 0.5)])
    v = g_values()
    for kw in (dict(max_depth=-1), dict(max_depth=5), dict(r_free=np.nan), dict(r_free=np.inf), dict(h=0.0),
               dict(h=np.nan), dict(origin=(0.0, np.inf, 0.0))):
        a = dict(origin=G_ORIGIN, h=G_H, r_free=0.3, max_depth=4)
        a.update(kw)
        try:
            be.corridor_subdivide(so, W, a["origin"], a["h"], v, a["r_free"], a["max_depth"], T)
        except TgmsError as e:
            assert e.status == ERR_INVALID_ARG, kw
        else:
            raise AssertionError(kw)
    try:
        be.corridor_subdivide(so, W, G_ORIGIN, G_H, v[:, :, :1], 0.3, 4, T)  # nx = 1
    except TgmsError as e:
        assert e.status == ERR_INVALID_ARG
    else:
        raise AssertionError("nx = 1")
    # B == 0
    got = be.corridor_subdivide(np.zeros(1, np.int32), np.zeros((0, 3)), G_ORIGIN, G_H, v, 0.3, 4, np.zeros(0))
    assert list(got[0]) == [0] and all(len(x) == 0 for x in got[1:])
