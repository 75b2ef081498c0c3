"""Shared inputs, checks and reference of the corridor inflation (tgms_corridor_inflate_batch*,
tgms_field_occupancy_device), used by test_inflate_host.py and test_gpu_inflate.py.
Backend-agnostic like field_ref.py: a backend is any object with
    corridor_inflate(so, W, origin, h, values, r_free, max_grow) -> box, faces, face_offsets, seg_flags, flags
(a Solver has it; the GPU file wraps the two device entry points the same way).

The reference is brute-force NumPy and shares no algorithm with the library: it has no table, a
slab is tested by slicing the boolean mask values >= float32(r_free).  include/tgms.h fixes the
result to the bit (integers, and doubles with stated rounding; NumPy's fp64 operations are each
rounded on their own, never fused), so every comparison here is for equality, the sign of a zero
included."""
import functools

import numpy as np

from trajectory_generator_ros2_amd import FEAS_NONFINITE, INF_BLOCKED, INF_CAPPED, INF_OUTSIDE, NEAR_NONE
from trajectory_generator_ros2_amd import synthetic as S

SPECIAL = INF_BLOCKED | INF_OUTSIDE | FEAS_NONFINITE


# ---- the reference ----

def rows_of(so):
    """Per segment its trajectory and its first waypoint row s + b."""
    so = np.asarray(so, dtype=np.int64)
    b = np.repeat(np.arange(len(so) - 1), np.diff(so))
    return b, np.arange(int(so[-1])) + b


def plane(origin, h, i):
    return origin + h * np.float64(i)  # two roundings


def seed(origin, h, w0, w1):
    """mn, mx, lo, hi of one segment as float64 [3] each (lo, hi hold integers)."""
    o = np.asarray(origin, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        mn, mx = np.where(w1 < w0, w1, w0), np.where(w1 > w0, w1, w0)
        lo = np.floor((mn - o) / h)
        lo = lo - (o + h * lo > mn)
        hi = np.ceil((mx - o) / h)
        hi = hi + (o + h * hi < mx)
    return mn, mx, lo, hi


def slab(lo, hi, d):
    """The box of the next layer in direction d (+x -x +y -y +z -z) of the box lo..hi."""
    a = d >> 1
    l2, h2 = lo.copy(), hi.copy()
    l2[a] = h2[a] = hi[a] + 1 if d % 2 == 0 else lo[a] - 1
    return l2, h2


def any_blocked(notfree, lo, hi):
    return bool(notfree[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].any())


def reference(so, W, origin, h, values, r_free, max_grow):
    v = np.asarray(values, dtype=np.float32)
    n = np.array(v.shape[::-1])
    notfree = ~(v >= np.float32(r_free))  # NaN is not free
    so = np.asarray(so, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float64)
    B, Sg = len(so) - 1, int(so[-1])
    box = np.full((Sg, 6), NEAR_NONE, dtype=np.int32)
    faces = np.zeros((Sg, 6, 4))
    seg_flags = np.zeros(Sg, dtype=np.int32)
    tb, row = rows_of(so)
    for s in range(Sg):
        w0, w1 = W[row[s]], W[row[s] + 1]
        if not (np.isfinite(w0).all() and np.isfinite(w1).all()):
            seg_flags[s] = FEAS_NONFINITE
            faces[s] = np.nan
            continue
        mn, mx, flo, fhi = seed(o, h, w0, w1)
        for a in range(3):
            faces[s, 2 * a, a], faces[s, 2 * a + 1, a] = 1.0, -1.0
        if (flo < 0).any() or (fhi > n - 1).any():
            seg_flags[s] = INF_OUTSIDE
            faces[s, 0::2, 3], faces[s, 1::2, 3] = mx, -mn
            continue
        lo, hi = flo.astype(np.int64), fhi.astype(np.int64)
        if any_blocked(notfree, lo, hi):
            seg_flags[s] = INF_BLOCKED
        else:
            is_open = [True] * 6
            for _ in range(max_grow):
                if not any(is_open):
                    break
                for d in range(6):
                    if not is_open[d]:
                        continue
                    l2, h2 = slab(lo, hi, d)
                    a = d >> 1
                    if l2[a] < 0 or h2[a] > n[a] - 1 or any_blocked(notfree, l2, h2):
                        is_open[d] = False
                    elif d % 2 == 0:
                        hi[a] += 1
                    else:
                        lo[a] -= 1
            if any(is_open):
                seg_flags[s] = INF_CAPPED
        box[s, :3], box[s, 3:] = lo, hi
        faces[s, 0::2, 3] = plane(o, h, hi)
        faces[s, 1::2, 3] = -plane(o, h, lo)
    flags = np.zeros(B, dtype=np.int32)
    np.bitwise_or.at(flags, tb, seg_flags)
    return box, faces.reshape(-1, 4), 6 * np.arange(Sg + 1, dtype=np.int64), seg_flags, flags


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))
                and np.array_equal(np.isnan(a), np.isnan(b)))


NAMES = ("box", "faces", "face_offsets", "seg_flags", "flags")


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert same_bits(g, w), (name, np.argwhere(np.asarray(g) != np.asarray(w))[:4], g[:2], w[:2])


def check_equal(be, so, W, origin, h, values, r_free, max_grow):
    got = be.corridor_inflate(so, W, origin, h, values, r_free, max_grow)
    assert_same(got, reference(so, W, origin, h, values, r_free, max_grow))
    return got


# ---- properties that hold whatever the algorithm, from the values alone ----

def check_properties(got, so, W, origin, h, values, r_free, max_grow):
    box, faces, fo, seg_flags, flags = got
    v = np.asarray(values, dtype=np.float32)
    n = np.array(v.shape[::-1])
    notfree = ~(v >= np.float32(r_free))
    W = np.asarray(W, dtype=np.float64).reshape(-1, 3)
    tb, row = rows_of(so)
    assert np.array_equal(fo, 6 * np.arange(len(seg_flags) + 1))
    want = np.zeros_like(flags)
    np.bitwise_or.at(want, tb, seg_flags)
    assert np.array_equal(flags, want)
    checked = 0
    for s in np.flatnonzero((seg_flags & SPECIAL) == 0):
        lo, hi = box[s, :3].astype(np.int64), box[s, 3:].astype(np.int64)
        assert (lo >= 0).all() and (hi <= n - 1).all() and (lo <= hi).all(), (s, box[s])
        assert not any_blocked(notfree, lo, hi), (s, box[s])  # every node of the box is free
        f = faces[6 * s:6 * s + 6]
        for w in (W[row[s]], W[row[s] + 1]):  # n . w <= d exactly: n is a signed unit vector
            assert ((f[:, :3] * w).sum(axis=1) <= f[:, 3]).all(), (s, w, f)
        _, _, flo, fhi = seed(origin, h, W[row[s]], W[row[s] + 1])
        grew = np.stack([hi - fhi, flo - lo], axis=1).reshape(6)  # layers per direction, in face order
        assert (grew >= 0).all() and (grew <= max_grow).all(), (s, grew)
        for d in range(6):
            l2, h2 = slab(lo, hi, d)
            a = d >> 1
            at_edge = l2[a] < 0 or h2[a] > n[a] - 1
            capped = grew[d] == max_grow and (seg_flags[s] & INF_CAPPED) != 0
            assert at_edge or capped or any_blocked(notfree, l2, h2), (s, d, box[s], seg_flags[s])
        checked += 1
    return checked


# ---- the random scene: 24 boxes on a 40 x 36 x 32 grid, the ragged 65-trajectory batch ----

SCENE_ORIGIN, SCENE_H, SCENE_N, SCENE_R = (-5.07, -4.61, 0.23), 0.26, (40, 36, 32), 0.3


@functools.lru_cache(maxsize=None)
def scene():
    rng = np.random.default_rng(S.SEED + 7)
    ext = SCENE_H * (np.array(SCENE_N) - 1)
    c = np.array(SCENE_ORIGIN) + rng.uniform(0.05, 0.95, size=(24, 3)) * ext
    half = rng.uniform(0.05, 0.25, size=(24, 3))
    v = S.box_field(np.concatenate([c - half, c + half], axis=1), SCENE_ORIGIN, SCENE_H, SCENE_N)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def ragged(shift=0.0):
    """ragged_batch(65, 2, 16) clipped into the grid; shift > 0 moves it along x afterwards, so that
    some waypoints leave the grid."""
    so, W, _ = S.ragged_batch(65, 2, 16)
    o = np.array(SCENE_ORIGIN)
    W = np.clip(W, o + 1e-3, o + SCENE_H * (np.array(SCENE_N) - 1) - 1e-3)
    W[:, 0] += shift
    W.setflags(write=False)
    return so, W


def check_random(be, max_grow, shift=0.0):
    so, W = ragged(shift)
    a = (so, W, SCENE_ORIGIN, SCENE_H, scene(), SCENE_R, max_grow)
    got = check_equal(be, *a)
    n_ok = check_properties(got, *a)
    sf = got[3]
    blocked, outside = int((sf & INF_BLOCKED != 0).sum()), int((sf & INF_OUTSIDE != 0).sum())
    # both paths are exercised: a fair share of the legs is blocked, a fair share grown
    assert blocked >= len(sf) // 10 and n_ok >= len(sf) // 10, (blocked, n_ok, len(sf))
    assert (outside > 0) == (shift > 0.0), outside
    return got


# ---- constructed scenes with known answers, on a 9 x 8 x 7 grid ----

G_ORIGIN, G_H, G_N = (-1.0, 0.5, 2.0), 0.5, (9, 8, 7)  # exact arithmetic: h a power of two
SEED_LO, SEED_HI = (3, 3, 2), (5, 4, 3)


def g_point(q):
    return np.array(G_ORIGIN) + G_H * np.asarray(q, dtype=np.float64)


def g_values(fill=1.0):
    return np.full(G_N[::-1], fill, dtype=np.float32)


def one_leg(q0=(3.2, 3.7, 2.4), q1=(4.6, 3.3, 2.9)):
    """One trajectory of one segment whose seed is SEED_LO .. SEED_HI."""
    return np.array([0, 1], dtype=np.int32), np.stack([g_point(q0), g_point(q1)])


def g_faces(lo, hi):
    f = np.zeros((6, 4))
    for a in range(3):
        f[2 * a, a], f[2 * a, 3] = 1.0, G_ORIGIN[a] + G_H * hi[a]
        f[2 * a + 1, a], f[2 * a + 1, 3] = -1.0, -(G_ORIGIN[a] + G_H * lo[a])
    return f


def expect_one(be, values, max_grow, lo, hi, flag, leg=None):
    so, W = leg if leg is not None else one_leg()
    got = check_equal(be, so, W, G_ORIGIN, G_H, values, 0.3, max_grow)
    assert list(got[0][0]) == list(lo) + list(hi), got[0]
    assert same_bits(got[1], g_faces(lo, hi)), got[1]
    assert list(got[2]) == [0, 6] and list(got[3]) == [flag] and list(got[4]) == [flag], got[2:]


def check_empty_map(be):
    top = tuple(n - 1 for n in G_N)
    expect_one(be, g_values(), 100, (0, 0, 0), top, 0)  # the whole grid, every direction closed at an edge
    expect_one(be, g_values(), 2, (1, 1, 0), (7, 6, 5), INF_CAPPED)  # seed +- 2
    expect_one(be, g_values(), 0, SEED_LO, SEED_HI, INF_CAPPED)  # nothing tested, all six open
    expect_one(be, g_values(0.3), 100, (0, 0, 0), top, 0)  # >= : a node at the threshold is free


def check_closed_direction_stays_closed(be, bad=0.0):
    """A node that is not free beside the seed on +x, at the seed's lowest y and z: +x closes in the
    first round, every other direction runs to the edge, and the wider box does not reopen +x."""
    v = g_values()
    v[2, 3, 6] = bad
    expect_one(be, v, 100, (0, 0, 0), (5, 7, 6), 0)
    # the same node one layer further: taken into account only when the box gets there
    v = g_values()
    v[2, 3, 7] = bad
    expect_one(be, v, 100, (0, 0, 0), (6, 7, 6), 0)
    # a node diagonal to the seed stops -y, which meets it first (+x has grown past it by then)
    v = g_values()
    v[2, 2, 6] = bad
    expect_one(be, v, 100, (0, 3, 0), (8, 7, 6), 0)


def check_blocked(be):
    v = g_values()
    v[2, 3, 4] = 0.29999  # inside the seed
    expect_one(be, v, 100, SEED_LO, SEED_HI, INF_BLOCKED)
    v = g_values()
    v[3, 4, 5] = np.nan  # the seed's far corner
    expect_one(be, v, 100, SEED_LO, SEED_HI, INF_BLOCKED)


def check_on_a_node(be):
    """A leg in the plane x = node 3: a seed of no thickness there; both waypoints equal and on a
    node: a single node; both equal inside a cell: that cell."""
    expect_one(be, g_values(), 0, (3, 3, 2), (3, 4, 3), INF_CAPPED, one_leg((3.0, 3.7, 2.4), (3.0, 3.3, 2.9)))
    expect_one(be, g_values(), 1, (2, 2, 1), (4, 5, 4), INF_CAPPED, one_leg((3.0, 3.7, 2.4), (3.0, 3.3, 2.9)))
    expect_one(be, g_values(), 0, (3, 4, 2), (3, 4, 2), INF_CAPPED, one_leg((3.0, 4.0, 2.0), (3.0, 4.0, 2.0)))
    expect_one(be, g_values(), 0, (3, 4, 2), (4, 5, 3), INF_CAPPED, one_leg((3.5, 4.25, 2.75), (3.5, 4.25, 2.75)))
    expect_one(be, g_values(), 0, (0, 0, 0), (8, 7, 6), INF_CAPPED, one_leg((0.0, 0.0, 0.0), (8.0, 7.0, 6.0)))


U_ORIGIN, U_H, U_N = (0.3, -0.2, 0.1), 0.1, (9, 8, 7)  # h and the origins are not dyadic: real rounding


def check_one_ulp(be):
    """A waypoint on every x node of a grid whose planes are rounded, and one ulp either side of it.
    The quotient (w - origin) / h is rounded, so floor and ceil may land one plane off; the
    correction step keeps containment exact: origin + h lo <= w <= origin + h hi as the faces state
    them, with lo and hi never further than one plane from the tightest pair, found here by
    looking at every plane."""
    o, n = np.array(U_ORIGIN), np.array(U_N)
    planes = [plane(o[a], U_H, np.arange(n[a])) for a in range(3)]
    legs = []
    for i in range(n[0]):
        for w in (np.nextafter(planes[0][i], -np.inf), planes[0][i], np.nextafter(planes[0][i], np.inf)):
            if planes[0][1] <= w <= planes[0][-2]:
                legs.append([w, planes[1][3], planes[2][2]])
    W = np.repeat(np.array(legs), 2, axis=0)  # each leg a trajectory of one segment, both waypoints equal
    so = np.arange(len(legs) + 1, dtype=np.int32)
    v = np.ones(U_N[::-1], dtype=np.float32)
    box, faces, _, seg_flags, _ = check_equal(be, so, W, U_ORIGIN, U_H, v, 0.3, 0)
    assert (seg_flags == INF_CAPPED).all()
    for s, leg in enumerate(legs):
        for a in range(3):
            lo, hi = box[s, a], box[s, 3 + a]
            assert planes[a][lo] <= leg[a] <= planes[a][hi], (s, a, leg, box[s])  # exact, on the planes themselves
            assert faces[6 * s + 2 * a, 3] == planes[a][hi] and faces[6 * s + 2 * a + 1, 3] == -planes[a][lo]
            tight_lo = int(np.flatnonzero(planes[a] <= leg[a]).max())
            tight_hi = int(np.flatnonzero(planes[a] >= leg[a]).min())
            assert tight_lo - 1 <= lo <= tight_lo and tight_hi <= hi <= tight_hi + 1, (s, a, leg, box[s])
    assert (box[:, 3] - box[:, 0]).min() == 0  # a waypoint on a node: no thickness there


def check_row_lengths(be):
    """M = 1 and M = 16 side by side, on the random scene."""
    _, W = ragged()
    so = np.array([0, 1, 17, 18], dtype=np.int32)
    a = (so, W[:so[-1] + 3], SCENE_ORIGIN, SCENE_H, scene(), SCENE_R, 8)
    check_properties(check_equal(be, *a), *a)


def check_nan_waypoint(be):
    """A NaN coordinate in the second waypoint of the middle trajectory: its two segments carry
    FEAS_NONFINITE alone, NaN faces and no box; everything else is the batch without the NaN."""
    _, W = ragged()
    so = np.array([0, 3, 7, 9], dtype=np.int32)
    W = W[:12].copy()
    a = (SCENE_ORIGIN, SCENE_H, scene(), SCENE_R, 8)
    clean = be.corridor_inflate(so, W, *a)
    W[5, 1] = np.nan  # trajectory 1 owns rows 4..8; row 5 ends segment 3 and starts segment 4
    box, faces, fo, seg_flags, flags = check_equal(be, so, W, *a)
    assert list(seg_flags[3:5]) == [FEAS_NONFINITE] * 2 and (box[3:5] == NEAR_NONE).all() and np.isnan(faces[18:30]).all()
    assert flags[1] & FEAS_NONFINITE and not (flags[[0, 2]] & FEAS_NONFINITE).any()
    keep = np.array([0, 1, 2, 5, 6, 7, 8])
    assert np.array_equal(box[keep], clean[0][keep]) and np.array_equal(seg_flags[keep], clean[3][keep])
    fk = (6 * keep[:, None] + np.arange(6)).reshape(-1)
    assert same_bits(faces[fk], clean[1][fk]) and np.array_equal(fo, clean[2])
    W[5, 1] = np.inf
    check_equal(be, so, W, *a)


def check_far_waypoints(be):
    """Coordinates far beyond the grid, up to the largest double: INF_OUTSIDE, faces the
    waypoints' own bounding box, no integer overflow on the way."""
    so = np.array([0, 3], dtype=np.int32)
    W = np.array([g_point((3.2, 3.7, 2.4)), [1e300, 1.0, 3.0], [-1.7e308, 1.7e308, 3.0], g_point((4.6, 3.3, 2.9))])
    box, faces, _, seg_flags, flags = check_equal(be, so, W, G_ORIGIN, G_H, g_values(), 0.3, 4)
    assert list(seg_flags) == [INF_OUTSIDE] * 3 and list(flags) == [INF_OUTSIDE] and (box == NEAR_NONE).all()
    assert faces[0, 3] == 1e300 and faces[6 + 1, 3] == 1.7e308


# ---- the table ----

TABLE_GRIDS = [(2, 2, 2), (9, 8, 7), (300, 3, 2), (3, 300, 2), (3, 2, 300)]


def table_values(n):
    nx, ny, nz = n
    rng = np.random.default_rng(S.SEED + nx + 7 * ny + 49 * nz)
    v = rng.uniform(0.0, 1.0, size=(nz, ny, nx)).astype(np.float32)
    v[rng.uniform(size=v.shape) < 0.05] = np.nan
    return v


def table_reference(values, r_free):
    m = ~(np.asarray(values, dtype=np.float32) >= np.float32(r_free))
    t = np.zeros(tuple(x + 1 for x in m.shape), dtype=np.int32)
    t[1:, 1:, 1:] = m.astype(np.int32).cumsum(axis=0).cumsum(axis=1).cumsum(axis=2)
    return t


def check_table(occupancy, n):
    """occupancy(origin, h, values, r_free) -> table [(nz+1),(ny+1),(nx+1)] int32."""
    v = table_values(n)
    for r_free in (0.5, 0.1):  # float32(0.1) != 0.1
        assert np.array_equal(occupancy((0.0, 0.0, 0.0), 1.0, v, r_free), table_reference(v, r_free)), (n, r_free)
    # values on either side of float32(r_free), the threshold a double that float32 rounds up
    r_free = 0.1
    t32 = np.float32(r_free)
    assert float(t32) > r_free
    v2 = v.copy()
    v2.reshape(-1)[0::3] = t32
    v2.reshape(-1)[1::3] = np.nextafter(t32, np.float32(0))  # below the fp32 threshold: the only nodes that are not free
    v2.reshape(-1)[2::3] = np.nextafter(t32, np.float32(1))
    got = occupancy((0.0, 0.0, 0.0), 1.0, v2, r_free)
    assert np.array_equal(got, table_reference(v2, r_free)), n
    assert got[-1, -1, -1] == len(v2.reshape(-1)[1::3])


# ---- arguments, through the Python interface ----

def check_arguments(be, TgmsError, ERR_INVALID_ARG):
    so, W = one_leg()
    good = dict(origin=G_ORIGIN, h=G_H, values=g_values(), r_free=0.3, max_grow=4)
    bad = [dict(values=np.ones((7, 8, 1), np.float32)), dict(values=np.ones((7, 1, 9), np.float32)),
           dict(values=np.ones((1, 8, 9), np.float32)), dict(h=0.0), dict(h=-0.5), dict(h=float("nan")),
           dict(h=float("inf")), dict(origin=(0.0, float("inf"), 0.0)), dict(origin=(float("nan"), 0.0, 0.0)),
           dict(r_free=float("nan")), dict(r_free=float("inf")), dict(r_free=-float("inf")), dict(max_grow=-1)]
    for change in bad:
        a = {**good, **change}
        try:
            be.corridor_inflate(so, W, a["origin"], a["h"], a["values"], a["r_free"], a["max_grow"])
        except TgmsError as e:
            assert e.status == ERR_INVALID_ARG, (change, e)
        else:
            raise AssertionError(f"accepted {change}")
    be.corridor_inflate(so, W, **good)  # and the unchanged call is fine
