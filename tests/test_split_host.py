"""CPU: the corridor split on the explicit host backend (tgms_corridor_split_batch on a
tgms_create_host handle; csrc/tgms_host.cpp corridor_split(), the decisions of
csrc/tgms_corridor_split_core.h) against the reference of split_ref.py.  The identical seg_rec /
seg_face arrays of one corridor call go to the reference and to the backend, so every integer
and every time is compared to the bit, no row excluded; inserted waypoints to 1e-9 of max |p|
over the segment.  tests/test_gpu_split.py repeats the checks on the device.

A backend is a pair of calls:
    cor(so, T, C, faces, fo, r)  -> (rec, where, seg_rec, seg_face, flags)
    split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac)
                                 -> (so', W', T', faces', fo', parent, flags)"""
import os

import numpy as np
import pytest

import bounds_ref as R
import split_ref as SR
from test_corridor_host import parabola
from test_split_ref import cubic

WIDTH, RADIUS = 2.5, 0.5  # the ragged fixture's corridor (test_corridor_host.py): split, unsplit and FULL rows (asserted)
TOL = 1e-9                # inserted waypoints against the reference, of L = max |p| over the segment
MODES = [SR.PULL, SR.CHORD]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.build import LIB_TGMS, build_tgms
    from trajectory_generator_ros2_amd.solver import Solver
    if not os.path.exists(LIB_TGMS):
        build_tgms()
    s = Solver(host=True)
    yield s
    s.close()


def backend(s):
    return (lambda so, T, C, faces, fo, r: s.corridor(so, T, C, faces, fo, r)), s.corridor_split


# ---- checks shared with test_gpu_split.py ----

def compare(out, ref, tol=TOL):
    """A result against a reference: integers, times, copied waypoints and faces to the bit,
    inserted waypoints to tol L."""
    so, W, T, faces, fo, parent, flags = out
    assert np.array_equal(so, ref["so"]) and so.dtype == np.int32
    assert np.array_equal(parent, ref["parent"]) and np.array_equal(flags, ref["flags"])
    assert np.array_equal(_bits(T), _bits(ref["T"]))
    assert (fo is None) == (ref["fo"] is None)
    if fo is not None:
        assert np.array_equal(fo, ref["fo"]) and fo.dtype == np.int64
        assert np.array_equal(_bits(faces), _bits(ref["faces"]))
    B = len(so) - 1
    rows = np.arange(len(T)) + np.repeat(np.arange(B), np.diff(so)) + 1  # a segment's end waypoint
    ins = np.zeros(len(W), bool)
    ins[rows[ref["inserted"]]] = True
    assert W.shape == ref["W"].shape and np.array_equal(_bits(W[~ins]), _bits(ref["W"][~ins]))
    with np.errstate(invalid="ignore"):  # an unusable row may hold inf on both sides
        err = np.abs(W[rows] - ref["W"][rows]).max(axis=1)
    assert (err[ref["inserted"]] <= tol * ref["L"][ref["inserted"]]).all(), (err / ref["L"]).max()


def run(be, so, W, T, C, faces, fo, r, mode, min_frac=0.1, seg=None):
    """A corridor call, then the split and the reference on its rows.  seg: (seg_rec, seg_face)
    to use instead."""
    cor, split = be
    if seg is None:
        seg = cor(so, T, C, faces, fo, r)[2:4]
    out = split(so, W, T, C, faces, fo, seg[0], seg[1], r, mode, min_frac)
    ref = SR.split(so, W, T, C, faces, fo, seg[0], seg[1], r, mode, min_frac)
    compare(out, ref)
    return out, ref


def check_parabola(be, mode):
    Tm, d, r, k = 2.0, 0.1, 0.25, 0.7
    so, T, C = parabola(k, Tm)
    W = np.array([[0.3, 0.0, 2.0], [0.3, 0.0, 2.0]])
    faces = np.array([[0.0, 1.0, 0.0, d]])
    out, _ = run(be, so, W, T, C, faces, np.array([0, 1], np.int64), r, mode)
    so2, W2, T2, faces2, fo2, parent, fl = out
    assert list(so2) == [0, 2] and list(parent) == [0, 0] and fl[0] == SR.DONE
    assert abs(T2[0] - Tm / 2) <= 1e-9 * Tm
    assert np.abs(W2[1] - [0.3, d - r if mode == SR.PULL else 0.0, 2.0]).max() <= 1e-9 * k * Tm * Tm
    assert list(fo2) == [0, 1, 2] and np.array_equal(faces2, np.repeat(faces, 2, axis=0))


def check_at_end(be):
    L, Tm = 3.0, 2.0
    so, T, C, _ = R.rest_to_rest(np.zeros(3), L, Tm, axis=0)
    W = np.array([[0.0, 0.0, 0.0], [L, 0.0, 0.0]])
    faces = np.array([[1.0, 0.0, 0.0, L / 2]])
    fo = np.array([0, 1], np.int64)
    out, _ = run(be, so, W, T, C, faces, fo, 0.0, SR.PULL)
    assert out[6][0] == SR.AT_END and np.array_equal(out[0], so) and np.array_equal(_bits(out[1]), _bits(W))
    assert np.array_equal(_bits(out[2]), _bits(T)) and np.array_equal(out[3], faces) and np.array_equal(out[4], fo)


def check_min_frac(be, Tm):
    so, W, T, C = cubic(Tm)
    out, _ = run(be, so, W, T, C, np.array([[0.0, 1.0, 0.0, 0.0]]), None, 0.0, SR.PULL)
    assert out[2][0] == np.float64(0.1) * np.float64(Tm) and out[6][0] == SR.DONE and out[4] is None


def ragged_case(solve, be, ed):
    """bounds_ref.ragged48 solved by `solve` in synthetic.box_corridor(WIDTH), with the corridor
    rows of `be` at RADIUS: computed once, never modified."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = R.ragged48()
    ED = R.end_derivs48() if ed else None
    C, _, worst = solve(so, W, T, ED)
    assert worst == 0
    faces, fo = S.box_corridor(so, W, WIDTH)
    seg = be[0](so, T, C, faces, fo, RADIUS)[2:4]
    c = dict(so=so, W=W, T=T, C=C, faces=faces, fo=fo, seg=seg, ED=ED)
    for a in (W, T, C, faces, fo) + tuple(seg):
        a.setflags(write=False)
    return c


def check_ragged(case, be, mode):
    """The fixture against the reference, and what the inserted waypoints promise."""
    c = case
    out, ref = run(be, c["so"], c["W"], c["T"], c["C"], c["faces"], c["fo"], RADIUS, mode, seg=c["seg"])
    so2, W2, T2, faces2, fo2, parent, fl = out
    M = np.diff(c["so"])
    assert (fl & SR.DONE).any() and (fl == 0).any() and (fl & SR.FULL).any(), "split, unsplit and FULL rows"
    assert np.array_equal(np.diff(so2) - M, [bin(int(x)).count("1") for x in _masks(c, ref)])
    assert (np.diff(so2) <= 16).all() and int(fo2[-1]) == len(faces2) == int(ref["fo"][-1])
    rows = np.arange(len(T2)) + np.repeat(np.arange(48), np.diff(so2))
    for s in np.flatnonzero(ref["inserted"]):
        w, p = W2[rows[s] + 1], int(parent[s])
        span = c["faces"][c["fo"][p]:c["fo"][p + 1]]
        Lh = np.abs(span[:, :3]).sum(axis=1) * ref["L"][s] + np.abs(span[:, 3])
        if mode == SR.PULL:
            f = c["faces"][c["seg"][1][p]]
            q = f[:3] @ w - f[3]
            assert q <= -RADIUS + 1e-9 * Lh.max()  # moved points sit at -r, the others are below it
        else:
            ends = np.maximum(span[:, :3] @ W2[rows[s]] - span[:, 3], span[:, :3] @ W2[rows[s] + 2] - span[:, 3])
            assert ((span[:, :3] @ w - span[:, 3]) <= ends + 1e-9 * Lh).all()
    return out


def _masks(c, ref):
    so, par = c["so"], ref["parent"]
    dup = np.bincount(par, minlength=int(so[-1])) - 1
    return [int(sum(int(dup[so[b] + i]) << i for i in range(so[b + 1] - so[b]))) for b in range(48)]


def check_pull_lands_on_the_face(case, be):
    """PULL: a point that was moved has |n . w - d + r| <= 1e-9 L_h."""
    c = case
    out, ref = run(be, c["so"], c["W"], c["T"], c["C"], c["faces"], c["fo"], RADIUS, SR.PULL, seg=c["seg"])
    so2, W2, T2, _, _, parent, _ = out
    rows = np.arange(len(T2)) + np.repeat(np.arange(48), np.diff(so2))
    moved = 0
    for s in np.flatnonzero(ref["inserted"]):
        p = int(parent[s])
        f = c["faces"][c["seg"][1][p]]
        x = SR.pull_point(c["C"][p], T2[s], np.r_[f[:3], np.inf], 0.0)  # d = inf: never moved, p(T_left) itself
        if f[:3] @ x - f[3] > -RADIUS:
            moved += 1
            Lh = np.abs(f[:3]).sum() * ref["L"][s] + abs(f[3])
            assert abs(f[:3] @ W2[rows[s] + 1] - f[3] + RADIUS) <= 1e-9 * Lh
    assert moved >= 8


def _one_row(M, m_of, Tm=1.0):
    """One trajectory of M parabolas along y, segment i peaking at m_of[i] above y = 0 (None: a
    flat segment at y = -1), one face y <= 0 per segment."""
    C = np.zeros((M, 3, 8))
    for i in range(M):
        if m_of.get(i) is None:
            C[i, 1, 0] = -1.0
        else:
            k = 4.0 * m_of[i] / Tm ** 2
            C[i, 1, 1], C[i, 1, 2] = k * Tm, -k
    W = np.zeros((M + 1, 3))
    W[:, 0] = np.arange(M + 1)
    faces = np.tile([[0.0, 1.0, 0.0, 0.0]], (M, 1))
    return np.array([0, M], np.int32), W, np.full(M, Tm), C, faces, np.arange(M + 1, dtype=np.int64)


def check_cap(be):
    out, _ = run(be, *_one_row(16, {i: 1.0 + i for i in range(16)}), 0.0, SR.CHORD)
    assert out[6][0] == SR.FULL and list(out[0]) == [0, 16] and list(out[5]) == list(range(16))
    out, _ = run(be, *_one_row(15, {3: 0.5, 9: 0.75}), 0.0, SR.CHORD)
    assert out[6][0] == SR.DONE | SR.FULL and list(np.flatnonzero(np.diff(out[5]) == 0)) == [9]
    out, _ = run(be, *_one_row(15, {3: 0.75, 9: 0.75}), 0.0, SR.CHORD)
    assert out[6][0] == SR.DONE | SR.FULL and list(np.flatnonzero(np.diff(out[5]) == 0)) == [3]
    out, _ = run(be, *_one_row(14, {3: 0.75, 9: 0.75}), 0.0, SR.CHORD)
    assert out[6][0] == SR.DONE and list(out[0]) == [0, 16]


def check_face_counts(solve, be):
    """0, 1 and TGMS_COR_MAX_FACES faces inside one trajectory, a second one behind it."""
    from trajectory_generator_ros2_amd import synthetic as S
    from test_corridor_host import ragged_faces
    so, W, T = S.ragged_batch(2, 4, 4, seed=12)
    C, _, worst = solve(so, W, T, None)
    assert worst == 0
    faces, fo = ragged_faces(np.random.default_rng(11), [7, 0, 256, 1, 0, 1, 7, 0])
    out, ref = run(be, so, W, T, C, faces, fo, 10.0, SR.PULL)  # r = 10: every segment with a face is wanted
    dup = np.bincount(out[5], minlength=8)
    assert dup[2] == 2 and (dup[3] == 2 or dup[5] == 2), "the 256-face and a 1-face segment are split"
    assert (dup[[1, 4, 7]] == 1).all(), "a segment without faces is never wanted"
    assert int(out[4][-1]) == int((np.diff(fo) * dup).sum()) == len(out[3])


def check_shared(case, be):
    c = case
    faces = np.array([[0.0, 0.0, 1.0, 3.0], [0.0, 0.0, -1.0, -1.0], [1.0, 0.0, 0.0, 4.0]])
    out, ref = run(be, c["so"], c["W"], c["T"], c["C"], faces, None, 0.25, SR.PULL)
    assert out[4] is None and np.array_equal(out[3], faces) and (out[6] & SR.DONE).any()


def spoiled(case, be):
    """The fixture with four unusable rows, each in the middle of the batch: a NaN seg_rec row (5),
    a seg_face outside its span (18), a non-finite waypoint (29), T = 0 (40)."""
    c = case
    so = c["so"]
    W, T = c["W"].copy(), c["T"].copy()
    seg_rec, seg_face = c["seg"][0].copy(), c["seg"][1].copy()
    seg_rec[so[5], 1] = np.nan
    s = so[18] + int(np.argmax(seg_rec[so[18]:so[19], 0]))
    seg_rec[s, 0] = 1.0  # wanted, whatever it was
    seg_face[s] = c["fo"][s + 1]
    W[so[29] + 29 + 1, 2] = np.inf
    T[so[41] - 1] = 0.0
    return W, T, seg_rec, seg_face


BAD = [5, 18, 29, 40]


def check_unusable(case, be, mode):
    c = case
    so = c["so"]
    W, T, seg_rec, seg_face = spoiled(c, be)
    out, ref = run(be, so, W, T, c["C"], c["faces"], c["fo"], RADIUS, mode, seg=(seg_rec, seg_face))
    clean, _ = run(be, so, c["W"], c["T"], c["C"], c["faces"], c["fo"], RADIUS, mode, seg=c["seg"])
    assert (out[6][BAD] == SR.NONFINITE).all()
    for b in range(48):
        a0, a1, b0, b1 = out[0][b], out[0][b + 1], clean[0][b], clean[0][b + 1]
        if b in BAD:  # copied through unchanged
            assert a1 - a0 == so[b + 1] - so[b]
            assert np.array_equal(_bits(out[2][a0:a1]), _bits(T[so[b]:so[b + 1]]))
            assert np.array_equal(_bits(out[1][a0 + b:a1 + b + 1]), _bits(W[so[b] + b:so[b + 1] + b + 1]))
            assert np.array_equal(out[5][a0:a1], np.arange(so[b], so[b + 1]))
            assert np.array_equal(np.diff(out[4][a0:a1 + 1]), np.diff(c["fo"][so[b]:so[b + 1] + 1]))
        else:  # bit-equal to the clean batch's row
            assert a1 - a0 == b1 - b0 and out[6][b] == clean[6][b]
            assert np.array_equal(_bits(out[2][a0:a1]), _bits(clean[2][b0:b1]))
            assert np.array_equal(_bits(out[1][a0 + b:a1 + b + 1]), _bits(clean[1][b0 + b:b1 + b + 1]))
            assert np.array_equal(out[5][a0:a1], clean[5][b0:b1])
            assert np.array_equal(_bits(out[3][out[4][a0]:out[4][a1]]), _bits(clean[3][clean[4][b0]:clean[4][b1]]))


def check_round_trip(case, solve, be, mode):
    """The split batch solves, its coefficients pass through the inserted waypoints, and the
    corridor call accepts the new faces."""
    from trajectory_generator_ros2_amd import FEAS_NONFINITE
    c = case
    out, ref = run(be, c["so"], c["W"], c["T"], c["C"], c["faces"], c["fo"], RADIUS, mode, seg=c["seg"])
    so2, W2, T2, faces2, fo2, _, _ = out
    C2, st, worst = solve(so2, W2, T2, c["ED"])
    assert worst == 0 and not st.any()
    rows = np.arange(len(T2)) + np.repeat(np.arange(48), np.diff(so2))
    end = (C2 * T2[:, None, None] ** np.arange(8)).sum(axis=2)
    scale = np.maximum(np.abs(W2).max(), 1.0)
    assert np.abs(C2[:, :, 0] - W2[rows]).max() <= 1e-9 * scale and np.abs(end - W2[rows + 1]).max() <= 1e-9 * scale * 8
    fl = be[0](so2, T2, C2, faces2, fo2, RADIUS)[4]
    assert not (fl & FEAS_NONFINITE).any()


# ---- the host backend ----

@pytest.fixture(scope="module", params=["rest", "end_derivs"])
def case(request, host):
    return ragged_case(host.solve, backend(host), request.param == "end_derivs")


@pytest.mark.parametrize("mode", MODES)
def test_parabola(host, mode):
    check_parabola(backend(host), mode)


def test_an_excursion_at_a_waypoint_is_not_split(host):
    check_at_end(backend(host))


@pytest.mark.parametrize("T", [0.3, 1.0, 7.0])
def test_min_frac_clamp(host, T):
    check_min_frac(backend(host), T)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_batch_equals_the_reference(host, case, mode):
    check_ragged(case, backend(host), mode)


def test_pulled_points_land_on_the_worst_face(host, case):
    check_pull_lands_on_the_face(case, backend(host))


def test_segment_cap(host):
    check_cap(backend(host))


def test_face_counts_0_1_and_256_in_one_trajectory(host):
    check_face_counts(host.solve, backend(host))


def test_shared_mode(host, case):
    check_shared(case, backend(host))


@pytest.mark.parametrize("mode", MODES)
def test_unusable_rows_leave_their_neighbours_alone(host, case, mode):
    check_unusable(case, backend(host), mode)


@pytest.mark.parametrize("mode", MODES)
def test_round_trip(host, case, mode):
    check_round_trip(case, host.solve, backend(host), mode)


def test_bad_arguments(host, case):
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError
    c = case
    args = (c["so"], c["W"], c["T"], c["C"], c["faces"], c["fo"], c["seg"][0], c["seg"][1])
    for kw in (dict(min_frac=0.0), dict(min_frac=0.6), dict(min_frac=float("nan")), dict(mode=2), dict(r=float("nan"))):
        with pytest.raises(TgmsError) as e:
            host.corridor_split(*args, **dict(dict(r=RADIUS, mode=SR.PULL, min_frac=0.1), **kw))
        assert e.value.status == ERR_INVALID_ARG, kw
    # face outputs given in shared mode
    L, S, B = host._L, int(c["so"][-1]), 48
    so2, W2, T2 = np.full(B + 1, -7, np.int32), np.full((2 * S + B, 3), -7.0), np.full(2 * S, -7.0)
    f2, fo2, tot = np.full((12, 4), -7.0), np.full(2 * S + 1, -7, np.int64), np.full(2, -7, np.int64)
    st = L.tgms_corridor_split_batch(host._h, B, c["so"].ctypes.data, c["W"].ctypes.data, c["T"].ctypes.data,
                                     c["C"].ctypes.data, 6, c["faces"].ctypes.data, None, c["seg"][0].ctypes.data,
                                     c["seg"][1].ctypes.data, RADIUS, 0, 0.1, so2.ctypes.data, W2.ctypes.data,
                                     T2.ctypes.data, f2.ctypes.data, fo2.ctypes.data, None, tot.ctypes.data, None)
    assert st == ERR_INVALID_ARG and all((a == -7).all() for a in (so2, W2, T2, f2, fo2, tot))
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.corridor_split_device(B, c["so"], c["W"], c["T"], c["C"], len(c["faces"]), c["faces"], c["fo"],
                                   c["seg"][0], c["seg"][1], RADIUS, 0, 0.1, so2, W2, T2, d_totals=tot)
    assert e.value.status == ERR_UNSUPPORTED
    out = host.corridor_split(np.zeros(1, np.int32), np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3, 8)),
                              np.zeros((0, 4)), np.zeros(1, np.int64), np.zeros((0, 2)), np.zeros(0, np.int32))
    assert list(out[0]) == [0] and len(out[2]) == 0  # B == 0


def test_exports_and_constants(host):
    import trajectory_generator_ros2_amd as P
    from trajectory_generator_ros2_amd import _lib
    for name in ("tgms_corridor_split_batch", "tgms_corridor_split_batch_device"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert (P.SPLIT_PULL, P.SPLIT_CHORD, P.SPLIT_DONE, P.SPLIT_FULL, P.SPLIT_AT_END) == (0, 1, 1, 2, 4)
    assert _lib.load().tgms_abi_version() == 2


def test_corridor_loop(host):
    """Six rounds on the fixture: every round's batch is a valid CSR with M <= 16 that still holds
    the original waypoints, in order.  The flagged counts are not asserted (DESIGN.md has them)."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = R.ragged48()
    faces, fo = S.box_corridor(so, W, WIDTH)
    for mode in MODES:
        for rounds in range(7):
            (so2, W2, T2, f2, fo2), C2, flagged = host.corridor_loop(so, W, T, faces, fo, RADIUS, rounds, mode, 0.1)
            M2 = np.diff(so2)
            assert so2[0] == 0 and (M2 >= 1).all() and (M2 <= 16).all() and len(T2) == so2[-1] == len(C2)
            assert len(W2) == so2[-1] + 48 and len(fo2) == so2[-1] + 1 and fo2[0] == 0 and fo2[-1] == len(f2)
            assert (np.diff(fo2) == 6).all() and (T2 > 0).all() and len(flagged) <= rounds + 1
            assert np.abs(np.add.reduceat(T2, so2[:-1]) - np.add.reduceat(T, so[:-1])).max() <= 1e-12 * T.sum()
            for b in range(48):  # the original waypoints, in order, the first and last in place
                mine, orig = W2[so2[b] + b:so2[b + 1] + b + 1], W[so[b] + b:so[b + 1] + b + 1]
                at = [int(np.flatnonzero((mine == w).all(axis=1))[0]) for w in orig]
                assert at == sorted(at) and at[0] == 0 and at[-1] == len(mine) - 1
            if flagged[-1] == 0:
                break
