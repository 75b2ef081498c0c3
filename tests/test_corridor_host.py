"""CPU: corridor containment on the explicit host backend (tgms_corridor_batch on a
tgms_create_host handle; csrc/tgms_host.cpp corridor(), the algorithm of
csrc/tgms_corridor_core.h).  Closed forms first, then the 1e-9 L_h contract of include/tgms.h
against the independent reference of corridor_ref.py on 48 + 48 solved ragged trajectories in
box corridors, the reported times, faces and flags, ragged face counts, ties, unusable rows and
faces, and argument errors.  tests/test_gpu_corridor.py repeats the cases on the device."""
import os
from fractions import Fraction

import numpy as np
import pytest

import bounds_ref as R
import corridor_ref as CR

P0 = np.array([0.0, -1.0, 2.0])
WIDTH, RADIUS = 2.5, 0.5  # the ragged fixture's corridor: some rows inside, some outside (asserted)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.build import LIB_TGMS, build_tgms
    from trajectory_generator_ros2_amd.solver import Solver
    if not os.path.exists(LIB_TGMS):
        build_tgms()
    s = Solver(host=True)
    yield s
    s.close()


def ragged_case(solve, call, ed):
    """bounds_ref.ragged48 (every M in 1..16 three times) solved by `solve`, rest to rest or
    with end_derivs48, in synthetic.box_corridor(WIDTH); the records of `call` at RADIUS and the
    reference, computed once."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = R.ragged48()
    C, _, worst = solve(so, W, T, R.end_derivs48() if ed else None)
    assert worst == 0
    faces, fo = S.box_corridor(so, W, WIDTH)
    out = call(so, T, C, faces, fo, RADIUS)
    case = dict(so=so, W=W, T=T, C=C, faces=faces, fo=fo, out=out, ref=CR.records(so, T, C, faces, fo))
    for a in (C, faces, fo) + tuple(out):
        a.setflags(write=False)
    return case


@pytest.fixture(scope="module", params=["rest", "end_derivs"])
def case(request, host):
    return ragged_case(host.solve, host.corridor, request.param == "end_derivs")


# ---- checks shared with test_gpu_corridor.py: each takes the call under test, ----
# ---- call(so, T, C, faces, face_offsets=None, r=0.0) -> (rec, where, seg_rec, seg_face, flags) ----

def parabola(k, T):
    """M = 1: p_y = k t (T - t), x and z constant."""
    C = np.zeros((1, 3, 8))
    C[0, 0, 0], C[0, 2, 0] = 0.3, 2.0
    C[0, 1, 1], C[0, 1, 2] = k * T, -k
    return np.array([0, 1], np.int32), np.array([T]), C


def check_rest_to_rest(call):
    """x from 0 to L: against (1,0,0 | L/2) the margin is L/2 at t = T, against (-1,0,0 | 0) it
    is 0 at t = 0, exactly (the Horner chain returns c_0 at u = 0)."""
    from trajectory_generator_ros2_amd import COR_OUTSIDE
    L, T = 3.0, 2.0
    so, Ts, C, _ = R.rest_to_rest(P0, L, T, axis=0)
    faces = np.array([[-1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, L / 2]])
    rec, where, seg_rec, seg_face, fl = call(so, Ts, C, faces, np.array([0, 2]))
    assert abs(rec[0, 0] - L / 2) <= 1e-12 * L and rec[0, 1] == T and list(where[0]) == [0, 1]
    assert fl[0] == COR_OUTSIDE and np.array_equal(_bits(seg_rec), _bits(rec)) and seg_face[0] == 1
    rec, where, _, _, fl = call(so, Ts, C, faces[:1], np.array([0, 1]))
    assert rec[0, 0] == 0.0 and rec[0, 1] == 0.0 and list(where[0]) == [0, 0]
    assert fl[0] == 0  # m_max > -r is strict: a waypoint on the face is not outside at r = 0
    assert call(so, Ts, C, faces[:1], np.array([0, 1]), 1e-300)[4][0] == COR_OUTSIDE


def check_parabola(call, T):
    k = 0.7
    so, Ts, C = parabola(k, T)
    rec, where, _, _, _ = call(so, Ts, C, np.array([[0.0, 1.0, 0.0, 0.0]]), np.array([0, 1]))
    assert abs(rec[0, 0] - k * T * T / 4) <= 1e-12 * k * T * T
    assert abs(rec[0, 1] - T / 2) <= 1e-9 * T  # the ladder's bracket is 2^-40 in u
    assert list(where[0]) == [0, 0]


def check_slanted(call):
    """corridor_ref's hand projection: x = 0.3 + 0.5 t, y = k t (T - t), n = (3, 4, 0) / 5."""
    k, T = 0.7, 2.0
    so, Ts, C = parabola(k, T)
    C[0, 0, 1] = 0.5
    ts = T / 2 + 0.3 / (1.6 * k)
    want = 0.6 * (0.3 + 0.5 * ts) + 0.8 * k * ts * (T - ts) - 1.0
    rec, _, _, _, _ = call(so, Ts, C, np.array([[0.6, 0.8, 0.0, 1.0]]))  # shared mode, F = 1
    assert abs(rec[0, 0] - want) <= 1e-12 * 3.0 and abs(rec[0, 1] - ts) <= 1e-9 * T


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding


def check_constant(call):
    """n . p0 - d with the rounding include/tgms.h names, at the first candidate of the first
    segment."""
    so = np.array([0, 3], np.int32)
    p = [0.1, -2.7, 3.3]
    C = np.zeros((3, 3, 8))
    C[:, :, 0] = p
    n, d = [0.5, -0.3, 2.1], 0.7
    want = _fma(n[2], p[2], _fma(n[1], p[1], _fma(n[0], p[0], -d)))
    rec, where, seg_rec, seg_face, fl = call(so, np.array([0.5, 2.0, 7.0]), C, np.array([n + [d]]))
    assert rec[0, 0] == want and rec[0, 1] == 0.0 and list(where[0]) == [0, 0]
    assert (seg_rec[:, 0] == want).all() and list(seg_rec[:, 1]) == [0.0, 0.5, 2.5] and not seg_face.any()


def check_ragged_contract(case, out=None):
    """The contract, the times and the flags of the ragged fixture; every row is compared: on
    the reference no row lies within the tolerance of the threshold."""
    from trajectory_generator_ros2_amd import COR_OUTSIDE
    c, ref = case, case["ref"]
    rec, where, seg_rec, seg_face, fl = case["out"] if out is None else out
    CR.check_contract(rec, ref, seg_rec=seg_rec)
    CR.check_times(c["so"], c["T"], c["C"], c["faces"], rec, where, ref, seg_rec, seg_face)
    assert (np.abs(ref["m"] + RADIUS) > 1e-9 * ref["L"]).all()
    want = np.where(ref["m"] > -RADIUS, COR_OUTSIDE, 0)
    assert 8 <= want.astype(bool).sum() <= 40, "the fixture holds rows inside and outside"
    assert np.array_equal(fl, want)
    assert np.array_equal(where[:, 0], ref["seg"])  # solved batches have no two segments tied at the top


def ragged_faces(rng, counts):
    """One trajectory's worth of random faces, counts[i] for segment i: unit normals, d such that
    the room's origin is inside by 0.5 .. 3."""
    n = rng.normal(size=(int(sum(counts)), 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.c_[n, rng.uniform(0.5, 3.0, len(n))], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def check_ragged_face_counts(solve, call):
    """0, 1, 7 and TGMS_COR_MAX_FACES faces mixed within one trajectory, a second one behind it."""
    from trajectory_generator_ros2_amd import COR_MAX_FACES, synthetic as S
    rng = np.random.default_rng(11)
    so, W, T = S.ragged_batch(2, 4, 4, seed=12)
    C, _, worst = solve(so, W, T, None)
    assert worst == 0
    faces, fo = ragged_faces(rng, [7, 0, COR_MAX_FACES, 1, 0, 1, 7, 0])
    rec, where, seg_rec, seg_face, fl = call(so, T, C, faces, fo)
    ref = CR.records(so, T, C, faces, fo)
    CR.check_contract(rec, ref, seg_rec=seg_rec)
    CR.check_times(so, T, C, faces, rec, where, ref, seg_rec, seg_face)
    assert list(seg_face[[1, 4, 7]]) == [-1] * 3 and np.isneginf(seg_rec[[1, 4, 7], 0]).all()
    assert seg_face[3] == 7 + COR_MAX_FACES and seg_face[5] == fo[5]
    assert ((seg_face == -1) | ((seg_face >= fo[:-1]) & (seg_face < fo[1:]))).all()


def check_shared_equals_repeated(case, call):
    """All F faces for every segment: bit-equal to the CSR call that repeats them, the face
    reported as the index into the F."""
    rng = np.random.default_rng(13)
    so, T, C = case["so"], case["T"], case["C"]
    S = int(so[-1])
    faces, _ = ragged_faces(rng, [7])
    faces[:, 3] += 6.0
    a = call(so, T, C, faces, None, RADIUS)
    b = call(so, T, C, np.tile(faces, (S, 1)), 7 * np.arange(S + 1, dtype=np.int64), RADIUS)
    seg_of = so[:-1] + a[1][:, 0]  # the winning segment's row in the batch
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert np.array_equal(a[1][:, 0], b[1][:, 0]) and np.array_equal(a[1][:, 1] + 7 * seg_of, b[1][:, 1])
    assert np.array_equal(a[3] + 7 * np.arange(S), b[3]) and np.array_equal(a[4], b[4])
    assert (a[3] >= 0).all() and (a[3] < 7).all() and len(set(a[4])) == 2
    ref = CR.records(so, T, C, faces)
    CR.check_contract(a[0], ref, seg_rec=a[2])
    CR.check_times(so, T, C, faces, a[0], a[1], ref, a[2], a[3])


def check_ties(call):
    """A duplicated face reports the lower index; two segments with equal margins report the
    lower segment, and a later, larger one still wins."""
    so, Ts, C = parabola(0.7, 1.0)
    f = np.array([[0.0, 1.0, 0.0, 0.0]])
    rec, where, _, seg_face, _ = call(so, Ts, C, np.repeat(f, 3, axis=0), np.array([0, 3]))
    assert list(where[0]) == [0, 0] and seg_face[0] == 0
    so3 = np.array([0, 3], np.int32)
    C3, T3 = np.repeat(C, 3, axis=0), np.repeat(Ts, 3)
    rec, where, seg_rec, seg_face, _ = call(so3, T3, C3, np.repeat(f, 4, axis=0), np.array([0, 0, 2, 4]))
    assert list(where[0]) == [1, 0] and list(seg_face) == [-1, 0, 2]
    assert seg_rec[1, 0] == seg_rec[2, 0] == rec[0, 0] and abs(rec[0, 1] - 1.5) <= 1e-9
    C3[2, 1, 0] = 2.0 ** -30  # the third segment a little higher
    rec, where, _, _, _ = call(so3, T3, C3, np.repeat(f, 4, axis=0), np.array([0, 0, 2, 4]))
    assert list(where[0]) == [2, 2]


def check_no_faces(call):
    """No face anywhere: (-inf, 0.0), (-1, -1), no flag, whatever r; with faces elsewhere in the
    batch, a trajectory that owns none is the same."""
    so, Ts, C = parabola(0.7, 1.0)
    for r in (0.0, 1e300, -1e300):
        rec, where, seg_rec, seg_face, fl = call(so, Ts, C, np.zeros((0, 4)), np.zeros(2, np.int64), r)
        assert np.isneginf(rec[0, 0]) and rec[0, 1] == 0.0 and list(where[0]) == [-1, -1] and fl[0] == 0
        assert np.isneginf(seg_rec[0, 0]) and seg_rec[0, 1] == 0.0 and seg_face[0] == -1
    rec, where, _, _, fl = call(so, Ts, C, np.zeros((0, 4)), None)  # shared mode with F == 0
    assert np.isneginf(rec[0, 0]) and list(where[0]) == [-1, -1] and fl[0] == 0
    so2, T2, C2 = np.array([0, 1, 2], np.int32), np.repeat(Ts, 2), np.repeat(C, 2, axis=0)
    rec, where, _, _, fl = call(so2, T2, C2, np.array([[0.0, 1.0, 0.0, 0.0]]), np.array([0, 0, 1]))
    assert np.isneginf(rec[0, 0]) and list(where[0]) == [-1, -1] and fl[0] == 0 and list(where[1]) == [0, 0]


BAD_ROWS = [3, 21, 30, 41, 47]


def spoil_rows(case):
    """The ragged fixture with five unusable rows: a NaN coefficient (3), a face span that
    decreases (21), one above the cap (30), T = 0 (41) and a span that ends above F (47)."""
    from trajectory_generator_ros2_amd import COR_MAX_FACES
    so = case["so"]
    assert (np.diff(so)[[21, 30]] >= 2).all()
    C, T, fo = case["C"].copy(), case["T"].copy(), case["fo"].copy()
    C[so[3], 1, 4] = np.nan
    fo[so[21] + 1] = fo[so[21]] - 1
    fo[so[30] + 1] = fo[so[30]] + COR_MAX_FACES + 1
    T[so[42] - 1] = 0.0
    fo[so[48]] = len(case["faces"]) + 1
    return C, T, fo


def check_bad_rows(case, call):
    """Each unusable row has NONFINITE alone, NaN records, -1 indices and NaN / -1 segment rows;
    every other row is bit-equal to the clean batch's."""
    from trajectory_generator_ros2_amd import FEAS_NONFINITE
    so = case["so"]
    C, T, fo = spoil_rows(case)
    rec, where, seg_rec, seg_face, fl = call(so, T, C, case["faces"], fo, RADIUS)
    keep = np.ones(48, bool)
    keep[BAD_ROWS] = False
    skeep = np.repeat(keep, np.diff(so))
    rec0, where0, seg_rec0, seg_face0, fl0 = case["out"]
    assert (fl[BAD_ROWS] == FEAS_NONFINITE).all() and np.isnan(rec[BAD_ROWS]).all() and (where[BAD_ROWS] == -1).all()
    assert np.isnan(seg_rec[~skeep]).all() and (seg_face[~skeep] == -1).all()
    assert np.array_equal(fl[keep], fl0[keep]) and np.array_equal(_bits(rec[keep]), _bits(rec0[keep]))
    assert np.array_equal(where[keep], where0[keep]) and np.array_equal(seg_face[skeep], seg_face0[skeep])
    assert np.array_equal(_bits(seg_rec[skeep]), _bits(seg_rec0[skeep]))


def check_bad_faces(case, call):
    """NaN in n, NaN in d and a zero normal, in rows 5, 17 and 29: COR_BAD_FACE on the owners
    only, the rest of every row that of the call without those faces."""
    from trajectory_generator_ros2_amd import COR_BAD_FACE
    so, T, C, fo = case["so"], case["T"], case["C"], case["fo"]
    ks = np.array([fo[so[5]] + 2, fo[so[17] + 1], fo[so[30]] - 1])  # first, any and last segment of a row
    faces = case["faces"].copy()
    faces[ks[0], 1], faces[ks[1], 3], faces[ks[2], :3] = np.nan, np.nan, 0.0
    rec, where, seg_rec, seg_face, fl = call(so, T, C, faces, fo, RADIUS)
    shift = lambda idx: idx - (ks[None, :] < np.asarray(idx)[..., None]).sum(axis=-1)
    rec0, where0, seg_rec0, seg_face0, fl0 = call(so, T, C, np.delete(faces, ks, axis=0), shift(fo), RADIUS)
    own = np.zeros(48, np.int32)
    own[[5, 17, 29]] = COR_BAD_FACE
    assert np.array_equal(fl, fl0 | own) and not (fl0 & COR_BAD_FACE).any()
    assert np.array_equal(_bits(rec), _bits(rec0)) and np.array_equal(_bits(seg_rec), _bits(seg_rec0))
    assert np.array_equal(where[:, 0], where0[:, 0]) and np.array_equal(shift(where[:, 1]), where0[:, 1])
    assert np.array_equal(shift(seg_face), seg_face0) and not np.isin(seg_face, ks).any()


def _host_call(host):
    return lambda so, T, C, faces, fo=None, r=0.0: host.corridor(so, T, C, faces, fo, r)


def test_rest_to_rest(host):
    check_rest_to_rest(_host_call(host))


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_parabola(host, T):
    check_parabola(_host_call(host), T)


def test_slanted_face(host):
    check_slanted(_host_call(host))


def test_constant_trajectory_gives_the_exact_value(host):
    check_constant(_host_call(host))


def test_ragged_batch_meets_the_contract(case):
    check_ragged_contract(case)


def test_ragged_face_counts(host):
    check_ragged_face_counts(host.solve, _host_call(host))


def test_shared_mode_equals_the_repeated_csr(host, case):
    check_shared_equals_repeated(case, _host_call(host))


def test_ties_go_to_the_lowest_segment_then_face(host):
    check_ties(_host_call(host))


def test_no_faces(host):
    check_no_faces(_host_call(host))


def test_unusable_rows_leave_their_neighbours_alone(host, case):
    check_bad_rows(case, _host_call(host))


def test_unusable_faces_are_left_out(host, case):
    check_bad_faces(case, _host_call(host))


def test_flag_is_strict_on_the_stored_value(host, case):
    from trajectory_generator_ros2_amd import COR_OUTSIDE
    c = case
    m = c["out"][0][:, 0]
    k = int(np.argsort(m)[24])
    fl = host.corridor(c["so"], c["T"], c["C"], c["faces"], c["fo"], -m[k])[4]
    assert fl[k] == 0 and np.array_equal(fl, np.where(m > m[k], COR_OUTSIDE, 0))
    fl = host.corridor(c["so"], c["T"], c["C"], c["faces"], c["fo"], -np.nextafter(m[k], -np.inf))[4]
    assert fl[k] == COR_OUTSIDE and np.array_equal(fl, np.where(m >= m[k], COR_OUTSIDE, 0))


def raw_args(c, L, h, **kw):
    """The positional arguments of tgms_corridor_batch for the fixture, fresh outputs last five."""
    B, S = 48, int(c["so"][-1])
    out = [np.full((B, 2), -7.0), np.full((B, 2), -7, np.int32), np.full((S, 2), -7.0), np.full(S, -7, np.int32),
           np.full(B, -7, np.int32)]
    a = dict(B=B, so=c["so"].ctypes.data, T=c["T"].ctypes.data, C=c["C"].ctypes.data, F=len(c["faces"]),
             faces=c["faces"].ctypes.data, fo=c["fo"].ctypes.data, r=0.0, out=[o.ctypes.data for o in out])
    a.update(kw)
    return (h, a["B"], a["so"], a["T"], a["C"], a["F"], a["faces"], a["fo"], a["r"], *a["out"]), out


def test_bad_arguments(host, case):
    from trajectory_generator_ros2_amd import (COR_MAX_FACES, ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError, _lib)
    c = case
    L = _lib.load()
    for kw in (dict(r=float("nan")), dict(r=float("inf")), dict(out=[None] * 5), dict(faces=None), dict(F=-1)):
        args, out = raw_args(c, L, host._h, **kw)
        assert L.tgms_corridor_batch(*args) == ERR_INVALID_ARG, kw
        assert all((o == -7).all() for o in out)
    with pytest.raises(TgmsError) as e:  # shared mode with F above the cap
        host.corridor(c["so"], c["T"], c["C"], c["faces"][:COR_MAX_FACES + 1])
    assert e.value.status == ERR_INVALID_ARG
    host.corridor(c["so"], c["T"], c["C"], c["faces"][:COR_MAX_FACES])  # the cap itself is allowed
    for k in range(5):  # one output alone is enough, and it is the full call's
        args, out = raw_args(c, L, host._h, r=RADIUS, out=[None] * 5)
        args = list(args)
        args[9 + k] = out[k].ctypes.data
        assert L.tgms_corridor_batch(*args) == 0
        assert np.array_equal(out[k], c["out"][k], equal_nan=True)
    so0 = np.zeros(1, np.int32)
    args, out = raw_args(c, L, host._h, B=0, so=so0.ctypes.data, T=None, C=None)
    assert L.tgms_corridor_batch(*args) == 0 and all((o == -7).all() for o in out)  # B == 0: nothing touched
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.corridor_device(48, c["so"], c["T"], c["C"], len(c["faces"]), c["faces"], c["fo"],
                             d_rec=np.zeros((48, 2)))
    assert e.value.status == ERR_UNSUPPORTED


def test_exports_hold_the_two_new_entry_points(host):
    from trajectory_generator_ros2_amd import _lib
    for name in ("tgms_corridor_batch", "tgms_corridor_batch_device"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().tgms_abi_version() == 2


def test_box_corridor_holds_the_waypoints():
    """Six faces per segment, and both waypoints of a segment inside every one by `width`."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, _ = R.ragged48()
    faces, fo = S.box_corridor(so, W, 0.25)
    assert faces.shape == (6 * so[-1], 4) and np.array_equal(fo, 6 * np.arange(so[-1] + 1)) and fo.dtype == np.int64
    rows = np.arange(so[-1]) + np.repeat(np.arange(48), np.diff(so))
    for w in (W[rows], W[rows + 1]):
        m = (faces[:, :3].reshape(-1, 6, 3) * w[:, None, :]).sum(-1) - faces[:, 3].reshape(-1, 6)
        assert (m <= -0.25 + 1e-12).all() and (m.max(axis=1) >= -0.25 - 1e-12).all()
