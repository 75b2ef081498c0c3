"""The host-pointer entry points' staging (workspace layout, uploads, downloads, status
fold), through the C ABI with ctypes so that optional arguments can be NULL: the Python
wrappers always pass every output, so nothing else runs the "records only" / "flags only"
downloads of the checks, the omitted outputs of the multi-output calls or the status == NULL
path of the solves.

Every comparison is bit for bit: the same kernel on the same inputs, whichever outputs the
caller asked for.  The shared batch is ragged with S = 19 segments (odd: every fp64 region
behind the first would lose its 16-byte alignment with its 256-byte rounding) and B = 5
(the (B + 1) * 4-byte offsets region is no multiple of 16)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS = (1, 3, 10, 2, 3)
B = len(MS)
S19 = sum(MS)
DT = 0.05
G = 9.80665


def _p(a):
    return None if a is None else a.ctypes.data


@pytest.fixture(scope="module")
def batch(solver):
    """so, W, T, ED and the solved coefficients (without / with end derivatives); read-only."""
    from trajectory_generator_ros2_amd import METHOD_REDUCED
    from trajectory_generator_ros2_amd import synthetic as S
    parts = [S.uniform_batch(1, m, seed=9100 + i) for i, m in enumerate(MS)]
    so = np.concatenate([[0], np.cumsum(MS)]).astype(np.int32)
    W = np.ascontiguousarray(np.concatenate([p[1].reshape(-1, 3) for p in parts]))
    T = np.ascontiguousarray(np.concatenate([p[2].reshape(-1) for p in parts]))
    ED = np.random.default_rng(9100).normal(size=(B, 18))
    assert so[-1] == 19
    solver.set_method(METHOD_REDUCED)
    C = {}
    for ed in (False, True):
        C[ed], st, worst = solver.solve(so, W, T, ED if ed else None)
        assert worst == 0 and (st == 0).all()
    for a in (so, W, T, ED, C[False], C[True]):
        a.setflags(write=False)
    return so, W, T, ED, C


def _limits():
    from trajectory_generator_ros2_amd._lib import Limits
    return Limits(pmin=[-1.0, -1.0, -1.0], pmax=[1.0, 1.0, 1.0], v_max=1.0, a_max=1.0)


def _pair_calls(call, n, stride):
    """call(records or None, flags or None) -> status, asked for both outputs, the records
    alone and the flags alone: the lone outputs equal the halves of the pair."""
    rec = np.full((n, stride), np.nan)
    fl = np.full(n, -1, np.int32)
    assert call(rec, fl) == 0
    assert not np.isnan(rec).all() and (fl != -1).all()
    rec1 = np.full((n, stride), np.nan)
    assert call(rec1, None) == 0
    fl1 = np.full(n, -1, np.int32)
    assert call(None, fl1) == 0
    assert np.array_equal(rec1, rec, equal_nan=True)
    assert np.array_equal(fl1, fl)
    return rec, fl


def _extrema_call(solver, batch, ed):
    so, W, T, ED, C = batch
    lim = _limits()
    return lambda rec, fl: solver._L.tgms_extrema_batch(
        solver._h, B, _p(so), _p(W), _p(T), _p(ED) if ed else None, _p(C[ed]), DT, ctypes.byref(lim), _p(rec), _p(fl))


@pytest.mark.parametrize("ed", [True, False], ids=["end_derivs", "rest"])
def test_pair_download_extrema(solver, batch, ed):
    from trajectory_generator_ros2_amd._lib import EXTREMA_STRIDE
    _pair_calls(_extrema_call(solver, batch, ed), B, EXTREMA_STRIDE)


def test_pair_download_bounds(solver, batch):
    from trajectory_generator_ros2_amd._lib import EXTREMA_STRIDE
    so, W, T, ED, C = batch
    lim = _limits()
    _pair_calls(lambda rec, fl: solver._L.tgms_bounds_batch(solver._h, B, _p(so), _p(T), _p(C[True]),
                                                            ctypes.byref(lim), _p(rec), _p(fl)), B, EXTREMA_STRIDE)


@pytest.mark.parametrize("starts", [True, False], ids=["start_times", "no_start_times"])
@pytest.mark.parametrize("explicit", [True, False], ids=["pairs", "all_pairs"])
def test_pair_download_separation(solver, batch, explicit, starts):
    """Explicit pairs over the five trajectories (one of them (i, i)), and pairs == NULL over
    the first three (every unordered pair): P = 3 both ways."""
    from trajectory_generator_ros2_amd._lib import SEP_STRIDE
    so, W, T, ED, C = batch
    nb = B if explicit else 3
    pairs = np.array([[0, 2], [3, 3], [4, 1]], np.int32) if explicit else None
    t0 = 0.25 * np.arange(nb) if starts else None
    so_n, S = so[:nb + 1], int(so[nb])
    T_n, C_n = np.ascontiguousarray(T[:S]), np.ascontiguousarray(C[False][:S])
    _pair_calls(lambda sep, fl: solver._L.tgms_separation_batch(solver._h, nb, _p(so_n), _p(T_n), _p(C_n), _p(t0), 3,
                                                                _p(pairs), None, 1.0, _p(sep), _p(fl)), 3, SEP_STRIDE)


@pytest.mark.parametrize("ed", [True, False], ids=["end_derivs", "rest"])
def test_refine_outputs_optional(solver, batch, ed):
    so, W, T, ED, C = batch

    def refine(T_io, coeffs, cost, st):
        return solver._L.tgms_refine_batch(solver._h, B, _p(so), _p(W), _p(T_io), _p(ED) if ed else None, 1.0, 0.1, 2,
                                           _p(coeffs), _p(cost), _p(st))

    T1, T2 = T.copy(), T.copy()
    r1 = refine(T1, np.zeros((19, 3, 8)), np.zeros(B), np.zeros(B, np.int32))
    r2 = refine(T2, None, None, None)
    assert r1 == r2 == 0
    assert not np.array_equal(T1, T)
    assert np.array_equal(T2, T1)


def _failing_solve_input(kind):
    from trajectory_generator_ros2_amd import synthetic as S
    if kind == "overflow":  # test_gpu_edges.test_overflow_reports_nonfinite_and_writes_zeros, M = 3
        so, W, T = S.uniform_batch(5, 3, seed=81)
        W, T = W.reshape(-1, 3).copy(), T.reshape(-1).copy()
        W[8:12] *= 1e306
        T[6:9] = 0.01
        return so, W, T, 2
    so, W, T = S.uniform_batch(3, 2, seed=77)  # test_gpu_edges.test_breakdown_writes_exact_zeros
    W, T = W.reshape(-1, 3).copy(), T.reshape(-1).copy()
    T[3] = kind
    return so, W, T, 1


@pytest.mark.parametrize("kind", [1e-100, 1e-200, "overflow"])
def test_status_optional_message_kept(solver, kind):
    """tgms_solve_batch with status == NULL: the same return value, the same message (the
    first trajectory with the worst status), the same coefficients."""
    from trajectory_generator_ros2_amd._lib import OK, status_string
    so, W, T, bad = _failing_solve_input(kind)
    nb, S = len(so) - 1, int(so[-1])

    def solve(st):
        C = np.full((S, 3, 8), np.nan)
        r = solver._L.tgms_solve_batch(solver._h, nb, _p(so), _p(W), _p(T), None, _p(C), _p(st))
        return r, C, solver.last_error()

    st = np.full(nb, -1, np.int32)
    r1, C1, msg1 = solve(st)
    print("status", st, "returned", r1, "message", repr(msg1))
    assert r1 == st.max() and (st[[b for b in range(nb) if b != bad]] == OK).all()
    if kind == "overflow":
        assert r1 != OK
    want = "" if r1 == OK else "trajectory %d: %s" % (int(np.flatnonzero(st == r1)[0]), status_string(r1))
    assert msg1 == want
    r2, C2, msg2 = solve(None)
    assert r2 == r1 and msg2 == want
    M = S // nb
    healthy = np.concatenate([np.arange(b * M, (b + 1) * M) for b in range(nb) if b != bad])
    assert np.isfinite(C1[healthy]).all()
    assert np.array_equal(C2[healthy], C1[healthy])
    assert np.array_equal(C2, C1, equal_nan=True)


def test_refine_failure_leaves_no_message(solver, batch):
    """tgms_refine_batch returns the worst status and leaves last_error empty (a message an
    earlier call left is cleared), with a status array and without."""
    from trajectory_generator_ros2_amd._lib import ERR_INVALID_ARG, OK
    so, W, T, ED, C = batch
    ED_bad = ED.copy()
    ED_bad[2, 7] = np.nan  # a non-finite end derivative: the trajectory is invalid (include/tgms.h)
    for with_status in (True, False):
        bso, bW, bT, _ = _failing_solve_input("overflow")
        bC = np.zeros((15, 3, 8))
        r = solver._L.tgms_solve_batch(solver._h, 5, _p(bso), _p(bW), _p(bT), None, _p(bC), None)
        assert r != OK and solver.last_error() != ""
        st = np.full(B, -1, np.int32) if with_status else None
        T_io = T.copy()
        r = solver._L.tgms_refine_batch(solver._h, B, _p(so), _p(W), _p(T_io), _p(ED_bad), 1.0, 0.1, 2, None, None,
                                        _p(st))
        assert r == ERR_INVALID_ARG
        assert solver.last_error() == ""
        if with_status:
            assert st[2] == ERR_INVALID_ARG and (np.delete(st, 2) == OK).all()


def test_workspace_regrowth(batch):
    """A larger call in between regrows the workspace: the small call's layout and results
    do not depend on the capacity it finds."""
    from trajectory_generator_ros2_amd import synthetic as S
    from trajectory_generator_ros2_amd._lib import EXTREMA_STRIDE
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(0) as s:
        call = _extrema_call(s, batch, True)

        def small():
            rec, fl = np.full((B, EXTREMA_STRIDE), np.nan), np.full(B, -1, np.int32)
            assert call(rec, fl) == 0
            return rec, fl

        rec1, fl1 = small()
        so, W, T = S.uniform_batch(300, 3, seed=9200)
        _, _, worst = s.solve(so, W.reshape(-1, 3), T.reshape(-1))
        assert worst == 0
        rec2, fl2 = small()
    assert np.isfinite(rec1).all() and (fl1 != -1).all()
    assert np.array_equal(rec2, rec1) and np.array_equal(fl2, fl1)


@pytest.mark.parametrize("ed", [True, False], ids=["end_derivs", "rest"])
def test_sampler_staging(solver, batch, ed):
    """tgms_sample_batch (the one host-pointer path with an int64 region) against
    tgms_sample_batch_device on the same arrays as device tensors."""
    import torch
    from trajectory_generator_ros2_amd._lib import GOAL_STRIDE
    so, W, T, ED, C = batch
    offs, out = solver.sample(so, W, T, ED if ed else None, C[ed], DT)
    assert out.shape[0] == offs[-1] > B and np.isfinite(out).all()
    dev = [torch.tensor(a, device="cuda") for a in (so, W, T, C[ed], offs, ED)]
    d_out = torch.full((int(offs[-1]), GOAL_STRIDE), float("nan"), dtype=torch.float64, device="cuda")
    solver.sample_device(B, dev[0], dev[1], dev[2], dev[3], DT, dev[4], d_out, d_end_derivs=dev[5] if ed else None)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), out, equal_nan=True)


def test_pair_download_thrust(solver, batch):
    from trajectory_generator_ros2_amd._lib import THRUST_STRIDE, ThrustLimits
    so, W, T, ED, C = batch
    lim = ThrustLimits(9.0, 10.5, 0.1)
    _pair_calls(lambda rec, fl: solver._L.tgms_thrust_batch(solver._h, B, _p(so), _p(T), _p(C[False]), G,
                                                            ctypes.byref(lim), _p(rec), _p(fl)), B, THRUST_STRIDE)


# ---- the calls with more than two outputs: any of them may be NULL ----


def _fresh(spec, names):
    """The outputs `names` of spec (name -> (shape, dtype), in argument order) filled with a
    sentinel (NaN / -7), None for the others."""
    return {k: np.full(sh, np.nan if dt == np.float64 else -7, dt) if k in names else None for k, (sh, dt) in spec.items()}


def _untouched(a):
    return np.isnan(a).all() if a.dtype == np.float64 else (a == -7).all()


def _subset_calls(call, spec, subsets, rows=None):
    """call(outputs: name -> array or None) -> status, asked for every output and then for each
    of `subsets`: an array asked for equals the full call's bit for bit.  rows(full) -> name ->
    count gives the rows a trimmed call writes: those are compared, and every row behind them
    still holds its sentinel."""
    full = _fresh(spec, spec)
    assert call(full) == 0
    n = rows(full) if rows else {k: len(v) for k, v in full.items()}
    for k, v in full.items():
        assert not _untouched(v[:n[k]]) and _untouched(v[n[k]:]), k
    for names in subsets:
        part = _fresh(spec, names)
        assert call(part) == 0, names
        for k in names:
            assert np.array_equal(part[k][:n[k]], full[k][:n[k]], equal_nan=True), (names, k)
            assert _untouched(part[k][n[k]:]), (names, k)
    return full


def _alone_and_omitted(spec, omitted=True):
    names = list(spec)
    return [(k,) for k in names] + ([tuple(x for x in names if x != k) for k in names] if omitted else [])


DILATE = dict(scale=((B,), np.float64), active=((B,), np.int32), flags=((B,), np.int32),
              seg_times_out=((S19,), np.float64), coeffs_out=((S19, 3, 8), np.float64))


def _dilate_call(solver, batch):
    from trajectory_generator_ros2_amd._lib import ThrustLimits
    so, W, T, ED, C = batch
    lim = ThrustLimits(9.0, 10.5, 0.1)  # close around hover: every row is stretched
    return lambda o: solver._L.tgms_dilate_batch(solver._h, B, _p(so), _p(T), _p(C[False]), G, None, ctypes.byref(lim),
                                                 0.25, 100.0, *(_p(o[k]) for k in DILATE))


def test_dilate_outputs_optional(solver, batch):
    from trajectory_generator_ros2_amd._lib import DIL_FLAG_MASK, DIL_NONE
    full = _subset_calls(_dilate_call(solver, batch), DILATE, _alone_and_omitted(DILATE, omitted=False))
    assert (full["active"] != DIL_NONE).all() and (full["scale"] > 0.25).all() and not (full["flags"] & DIL_FLAG_MASK).any()
    assert not np.array_equal(full["seg_times_out"], batch[2])


def test_dilate_staging_equals_the_device_call(solver, batch):
    import torch
    from trajectory_generator_ros2_amd._lib import ThrustLimits
    so, W, T, ED, C = batch
    full = _fresh(DILATE, DILATE)
    assert _dilate_call(solver, batch)(full) == 0
    dev = {k: torch.tensor(v, device="cuda") for k, v in _fresh(DILATE, DILATE).items()}
    solver.dilate_device(B, *(torch.tensor(a, device="cuda") for a in (so, T, C[False])), G, None,
                         ThrustLimits(9.0, 10.5, 0.1), 0.25, 100.0, dev["scale"], dev["active"], dev["flags"],
                         dev["seg_times_out"], dev["coeffs_out"])
    torch.cuda.synchronize()
    for k in DILATE:
        assert np.array_equal(dev[k].cpu().numpy(), full[k], equal_nan=True), k


CORRIDOR = dict(rec=((B, 2), np.float64), where=((B, 2), np.int32), seg_rec=((S19, 2), np.float64),
                seg_face=((S19,), np.int32), flags=((B,), np.int32))
WIDTH = 0.3  # of the split's box corridor: 10 of the 19 segments leave it, by 0.05 at the least


def _corridor_call(solver, batch, faces, fo):
    so, W, T, ED, C = batch
    return lambda o: solver._L.tgms_corridor_batch(solver._h, B, _p(so), _p(T), _p(C[False]), len(faces), _p(faces), _p(fo),
                                                   0.0, *(_p(o[k]) for k in CORRIDOR))


def test_corridor_outputs_optional(solver, batch):
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T, ED, C = batch
    faces, fo = S.box_corridor(so, W, WIDTH)
    full = _subset_calls(_corridor_call(solver, batch, faces, fo), CORRIDOR, _alone_and_omitted(CORRIDOR))
    assert np.isfinite(full["rec"]).all() and (full["seg_face"] >= fo[:-1]).all() and (full["seg_face"] < fo[1:]).all()


NEAR = dict(near=((B, 2), np.float64), index=((B,), np.int32), count=((B,), np.int32), tested=((B,), np.int32),
            flags=((B,), np.int32))
R_MIN = 1e3  # above every distance: nothing is culled
NEAR_SUBSETS = [("near",), ("index",), ("count",), ("flags",), ("tested", "flags")]


def _tested_alone_is_refused(solver, call):
    """`tested` alone is an argument error (include/tgms.h: one of the other four is needed)."""
    from trajectory_generator_ros2_amd._lib import ERR_INVALID_ARG
    part = _fresh(NEAR, ("tested",))
    assert call(part) == ERR_INVALID_ARG and _untouched(part["tested"])
    assert solver.last_error().endswith("all NULL")


def _neighbors_call(solver, batch):
    so, W, T, ED, C = batch
    t0 = 0.25 * np.arange(B)
    return lambda o: solver._L.tgms_neighbors_batch(solver._h, B, _p(so), _p(T), _p(C[False]), _p(t0), None, R_MIN,
                                                    *(_p(o[k]) for k in NEAR))


def test_neighbors_outputs_optional(solver, batch):
    call = _neighbors_call(solver, batch)
    full = _subset_calls(call, NEAR, NEAR_SUBSETS)
    assert (full["tested"] == B - 1).all() and (full["count"] == B - 1).all() and np.isfinite(full["near"]).all()
    _tested_alone_is_refused(solver, call)


def test_neighbors_staging_equals_the_device_call(solver, batch):
    import torch
    so, W, T, ED, C = batch
    full = _fresh(NEAR, NEAR)
    assert _neighbors_call(solver, batch)(full) == 0
    dev = {k: torch.tensor(v, device="cuda") for k, v in _fresh(NEAR, NEAR).items()}
    solver.neighbors_device(B, *(torch.tensor(a, device="cuda") for a in (so, T, C[False])), R_MIN,
                            torch.tensor(0.25 * np.arange(B), device="cuda"), None, dev["near"], dev["index"],
                            dev["count"], dev["tested"], dev["flags"])
    torch.cuda.synchronize()
    for k in NEAR:
        assert np.array_equal(dev[k].cpu().numpy(), full[k], equal_nan=True), k


def test_clearance_outputs_optional(solver, batch):
    so, W, T, ED, C = batch
    boxes = np.array([[0.0, 0.0, 2.5, 0.0, 0.0, 2.5], [3.0, 3.0, 0.0, 4.0, 4.0, 1.0]])  # K = 2: a point and a box
    call = lambda o: solver._L.tgms_clearance_batch(solver._h, B, _p(so), _p(T), _p(C[False]), len(boxes), _p(boxes), None,
                                                    R_MIN, *(_p(o[k]) for k in NEAR))
    full = _subset_calls(call, NEAR, NEAR_SUBSETS)
    assert (full["tested"] == len(boxes)).all() and (full["count"] == len(boxes)).all() and np.isfinite(full["near"]).all()
    _tested_alone_is_refused(solver, call)


SPLIT_ARGS = ("seg_offsets_out", "waypoints_out", "seg_times_out", "faces_out", "face_offsets_out", "parent", "totals",
              "flags")
SPLIT_PULL = 0


def _split_spec(F, shared):
    """The outputs at the header's capacities (2 S segments, 2 F faces); shared mode has no face
    outputs."""
    spec = dict(seg_offsets_out=((B + 1,), np.int32), waypoints_out=((2 * S19 + B, 3), np.float64),
                seg_times_out=((2 * S19,), np.float64), faces_out=((2 * F, 4), np.float64),
                face_offsets_out=((2 * S19 + 1,), np.int64), parent=((2 * S19,), np.int32), totals=((2,), np.int64),
                flags=((B,), np.int32))
    return {k: v for k, v in spec.items() if not (shared and k in ("faces_out", "face_offsets_out"))}


@pytest.mark.parametrize("shared", [False, True], ids=["per_segment", "shared"])
def test_split_outputs_optional_and_trimmed(solver, batch, shared):
    """Some but not all segments are split, so S < S' < 2 S: the rows behind S' (S' + B waypoints, F'
    faces) keep their sentinel.  Shared mode: one box 0.5 inside the waypoints' bounding box."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T, ED, C = batch
    if shared:
        lo, hi = W.min(axis=0) + 0.5, W.max(axis=0) - 0.5
        faces, fo = np.zeros((6, 4)), None
        for ax in range(3):
            faces[2 * ax, ax], faces[2 * ax, 3] = 1.0, hi[ax]
            faces[2 * ax + 1, ax], faces[2 * ax + 1, 3] = -1.0, -lo[ax]
    else:
        faces, fo = S.box_corridor(so, W, WIDTH)
    cor = _fresh(CORRIDOR, ("seg_rec", "seg_face"))
    assert _corridor_call(solver, batch, faces, fo)(cor) == 0
    spec = _split_spec(len(faces), shared)
    call = lambda o: solver._L.tgms_corridor_split_batch(
        solver._h, B, _p(so), _p(W), _p(T), _p(C[False]), len(faces), _p(faces), _p(fo), _p(cor["seg_rec"]),
        _p(cor["seg_face"]), 0.0, SPLIT_PULL, 0.1, *(_p(o.get(k)) for k in SPLIT_ARGS))

    def rows(full):
        S2, F2 = (int(x) for x in full["totals"])
        print("split: S' = %d, F' = %d" % (S2, F2))
        assert S19 < S2 < 2 * S19 and S2 == full["seg_offsets_out"][-1]
        return dict(seg_offsets_out=B + 1, waypoints_out=S2 + B, seg_times_out=S2, faces_out=F2, face_offsets_out=S2 + 1,
                    parent=S2, totals=2, flags=B)

    _subset_calls(call, spec, [tuple(k for k in spec if k not in omit) for omit in (("parent",), ("flags",), ("parent", "flags"))],
                  rows)


CUT = dict(seg_offsets_out=((B + 1,), np.int32), waypoints_out=((S19 + B, 3), np.float64),
           seg_times_out=((S19,), np.float64), end_derivs_out=((B, 18), np.float64), coeffs_out=((S19, 3, 8), np.float64),
           parent=((S19,), np.int32), t0_out=((B,), np.float64), totals=((1,), np.int64), flags=((B,), np.int32))
CUT_OPTIONAL = ("coeffs_out", "parent", "t0_out", "flags")


def test_cut_outputs_optional_and_trimmed(solver, batch):
    """t_cut at 40 % of every duration drops segments, so S' < S: the rows behind S' keep their
    sentinel."""
    so, W, T, ED, C = batch
    t_cut = 0.4 * np.add.reduceat(T, so[:-1])
    call = lambda o: solver._L.tgms_cut_batch(solver._h, B, _p(so), _p(W), _p(T), None, _p(C[False]), _p(t_cut), 0.1,
                                              *(_p(o[k]) for k in CUT))

    def rows(full):
        S2 = int(full["totals"][0])
        print("cut: S' = %d" % S2)
        assert 0 < S2 < S19 and S2 == full["seg_offsets_out"][-1]
        return dict(seg_offsets_out=B + 1, waypoints_out=S2 + B, seg_times_out=S2, end_derivs_out=B, coeffs_out=S2,
                    parent=S2, t0_out=B, totals=1, flags=B)

    subsets = [tuple(k for k in CUT if k != o) for o in CUT_OPTIONAL] + [tuple(k for k in CUT if k not in CUT_OPTIONAL)]
    _subset_calls(call, CUT, subsets, rows)
