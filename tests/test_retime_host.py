"""CPU: the segment re-timing on the explicit host backend (tgms_retime_batch on a tgms_create_host
handle; csrc/tgms_host.cpp retime(), the rule of csrc/tgms_retime_core.h on the peaks of
csrc/tgms_bounds_core.h).

The checks take a `call(so, T, C, lim, s_lo, s_hi, want=(1, 1, 1, 1), in_place=False)` that returns
(T_out, seg_rec, rec, flags) as numpy arrays (None for an output not asked for), so
test_gpu_retime.py runs the same ones through tgms_retime_batch_dev."""
import os

import numpy as np
import pytest

import bounds_ref as R
import poly_zoo as Z
import retime_ref as RR
from retime_ref import CAPPED, CHANGED, INF, NONFINITE, OVER, SEG_SHIFT

S_HI = 1.5  # of the contract runs: low enough for some segments of every batch to be capped
SEAMS = (1, 3, 4, 5, 9, 257)  # across the 4-trajectory tile


def _limits(lim):
    from trajectory_generator_ros2_amd import Limits
    return None if lim is None else Limits(v_max=lim[0], a_max=lim[1], j_max=lim[2])


def raw_call(solver, so, T, C, lim, s_lo, s_hi, want=(1, 1, 1, 1), in_place=False):
    """tgms_retime_batch itself, on outputs filled with NaN / -9; returns (status, outputs)."""
    from trajectory_generator_ros2_amd import _lib
    import ctypes
    so = np.ascontiguousarray(so, np.int32)
    T = np.array(T, np.float64).reshape(-1)  # copies: in place writes into them
    C = np.array(C, np.float64).reshape(-1, 3, 8)
    B, S = len(so) - 1, len(T)
    outs = [(T if in_place else np.full(S, np.nan)) if want[0] else None, np.full((S, 4), np.nan) if want[1] else None,
            np.full((B, 3), np.nan) if want[2] else None, np.full(B, -9, np.int32) if want[3] else None]
    L = _limits(lim)
    st = _lib.load().tgms_retime_batch(solver._h, B, so.ctypes.data, T.ctypes.data, C.ctypes.data,
                                       None if L is None else ctypes.byref(L), float(s_lo), float(s_hi),
                                       *[None if o is None else o.ctypes.data for o in outs])
    return st, tuple(outs)


def host_call(solver):
    def call(so, T, C, lim, s_lo, s_hi, want=(1, 1, 1, 1), in_place=False):
        st, outs = raw_call(solver, so, T, C, lim, s_lo, s_hi, want, in_place)
        assert st == 0, solver.last_error()
        return outs
    return call


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(x, y):
    return all((a is None and b is None) or np.array_equal(bits(a), bits(b)) for a, b in zip(x, y))


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.build import LIB_TGMS, build_tgms
    from trajectory_generator_ros2_amd.solver import Solver
    if not os.path.exists(LIB_TGMS):
        build_tgms()
    s = Solver(host=True)
    yield s
    s.close()


# ---- 1. against the reference ----

def check_reference(call, name, s_lo):
    """Peaks within 1e-9 relative (the bounds contract), r and T_out within 2e-9, D_in to the bit,
    r_max one of the row's r to the bit, flags equal on the rows the reference decides (>= 90 %)."""
    c = RR.cases()[name]
    so, T = c["so"], c["T"]
    T_ref, seg_ref, rec_ref, fl_ref = RR.rule(so, T, c["pk"], c["lim"], s_lo, S_HI)
    T_out, seg_rec, rec, flags = call(so, T, c["C"], c["lim"], s_lo, S_HI)
    assert np.isfinite(seg_rec).all() and np.isfinite(rec).all() and np.isfinite(T_out).all()

    def rel(x, ref):
        return np.where(ref == 0.0, np.abs(x), np.abs(x - ref) / np.where(ref == 0.0, 1.0, ref))
    e_pk, e_r, e_T = rel(seg_rec[:, :3], seg_ref[:, :3]).max(), rel(seg_rec[:, 3], seg_ref[:, 3]).max(), rel(T_out, T_ref).max()
    e_rec = rel(rec[:, [0, 2]], rec_ref[:, [0, 2]]).max()
    print("%s s_lo=%g: peaks %.3g, r %.3g, T_out %.3g, r_max/D_out %.3g relative" % (name, s_lo, e_pk, e_r, e_T, e_rec))
    assert e_pk <= 1e-9 and e_r <= 2e-9 and e_T <= 2e-9 and e_rec <= 2e-9
    assert np.array_equal(bits(rec[:, 1]), bits(rec_ref[:, 1]))  # the same left-to-right sum of the same times
    for b in range(len(so) - 1):
        rows = seg_rec[so[b]:so[b + 1], 3]
        seg = int(flags[b]) >> SEG_SHIFT
        assert rec[b, 0] == rows.max() == rows[seg] and (rows[:seg] < rows[seg]).all()
    dec, idx = RR.decided(so, seg_ref[:, 3], S_HI)
    low = OVER | CAPPED | CHANGED | NONFINITE
    assert dec.mean() >= 0.9, dec.mean()
    assert np.array_equal(flags[dec] & low, fl_ref[dec] & low)
    assert np.array_equal(flags[dec & idx], fl_ref[dec & idx])


def test_reference_decides_most_rows():
    """The reference alone: the batches and limits leave >= 90 % of the rows of each batch to
    compare flag bits on, and >= 90 % of all rows with the segment index as well (knot_peak's two
    pieces share their peak, so its rows tie on purpose)."""
    both = []
    for name in ("ragged48", "zoo"):
        c = RR.cases()[name]
        r = RR.rule(c["so"], c["T"], c["pk"], c["lim"], 1.0, S_HI)[1][:, 3]
        dec, idx = RR.decided(c["so"], r, S_HI)
        fl = RR.rule(c["so"], c["T"], c["pk"], c["lim"], 1.0, S_HI)[3]
        over, capped = ((fl & OVER) != 0).mean(), ((fl & CAPPED) != 0).mean()
        print("%s: decided %.2f, with the index %.2f, over %.2f, capped %.2f" % (name, dec.mean(), (dec & idx).mean(), over, capped))
        assert dec.mean() >= 0.9 and 0.25 <= over <= 0.75 and capped > 0.0, (name, dec.mean(), over, capped)
        both.append(dec & idx)
    assert np.concatenate(both).mean() >= 0.9


@pytest.mark.parametrize("s_lo", [1.0, 0.8])
@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_against_the_reference(host, name, s_lo):
    check_reference(host_call(host), name, s_lo)


# ---- 2. against the public calls of the same backend ----

def check_public_calls(call, solver, name):
    """Solver.bounds on the exploded batch (every segment its own trajectory) and seg_rec: both
    within 1e-9 of the truth, so within 2e-9 of each other.  Solver.dilate with the kinematic limits
    alone returns max(s_lo, s_kin), which is max(s_lo, r_max)."""
    c = RR.cases()[name]
    so, T, C, lim = c["so"], c["T"], c["C"], c["lim"]
    _, seg_rec, rec, _ = call(so, T, C, lim, 1.0, S_HI)
    ext, _ = solver.bounds(np.arange(len(T) + 1, dtype=np.int32), T, C)
    pk = ext[:, 6:9]
    err = np.abs(pk - seg_rec[:, :3]) / np.where(pk == 0.0, 1.0, pk)
    print("%s: seg_rec vs exploded bounds %.3g relative, bit-equal %s" % (name, err.max(), np.array_equal(bits(pk), bits(seg_rec[:, :3]))))
    assert err.max() <= 2e-9
    s_lo = 2.0 ** -10
    scale = solver.dilate(so, T, C, limits=_limits(lim), tlimits=None, s_lo=s_lo, s_hi=2.0 ** 10)[0]
    want = np.maximum(s_lo, rec[:, 0])
    print("%s: dilate scale vs max(s_lo, r_max) %.3g relative, bit-equal %s" % (name, np.abs(scale / want - 1.0).max(),
                                                                               np.array_equal(bits(scale), bits(want))))
    assert (np.abs(scale - want) <= 2e-9 * want).all()


@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_against_bounds_and_dilate(host, name):
    check_public_calls(host_call(host), host, name)


# ---- 3. exact cases ----

def check_straight(call):
    """p = w + V t with |V| = 5 (3, 4, 0) and v_max = 2.5: v == 5, a == j == 0, r == 2, T_out == 2 T."""
    so = np.array([0, 2], np.int32)
    T = np.array([0.75, 3.0])
    C = np.zeros((2, 3, 8))
    C[:, :, 0] = [[0.5, -1.0, 2.0], [2.75, 2.0, 2.0]]
    C[:, :, 1] = [3.0, 4.0, 0.0]
    T_out, seg_rec, rec, flags = call(so, T, C, (2.5, 1.0, INF), 1.0, 4.0)
    assert np.array_equal(seg_rec, [[5.0, 0.0, 0.0, 2.0]] * 2)
    assert np.array_equal(T_out, 2.0 * T) and np.array_equal(rec, [[2.0, 3.75, 7.5]])
    assert flags[0] == OVER | CHANGED  # the tie of the two segments goes to segment 0
    T_out, _, rec, flags = call(so, T, C, (2.5, 1.0, INF), 1.0, 1.5)
    assert np.array_equal(T_out, 1.5 * T) and flags[0] == OVER | CHANGED | CAPPED and rec[0, 0] == 2.0


def check_constant(call):
    so = np.array([0, 3], np.int32)
    T = np.array([0.5, 2.0, 7.0])
    C = np.zeros((3, 3, 8))
    C[:, :, 0] = [0.1, -2.7, 3.3]
    T_out, seg_rec, rec, flags = call(so, T, C, (1.0, 2.0, 3.0), 1.0, 4.0)
    assert not seg_rec.any() and np.array_equal(bits(T_out), bits(T)) and flags[0] == 0
    assert np.array_equal(rec, [[0.0, (0.5 + 2.0) + 7.0, (0.5 + 2.0) + 7.0]])
    T_out, seg_rec, rec, flags = call(so, T, C, (1.0, 2.0, 3.0), 0.25, 4.0)  # s == s_lo
    assert not seg_rec.any() and np.array_equal(T_out, 0.25 * T) and flags[0] == CHANGED and rec[0, 0] == 0.0


def check_translation(call, name):
    c = RR.cases()[name]
    a = call(c["so"], c["T"], c["C"], c["lim"], 0.8, S_HI)
    b = call(c["so"], c["T"], Z.translate(c["C"]), c["lim"], 0.8, S_HI)
    assert same(a, b)


def test_straight_segment(host):
    check_straight(host_call(host))


def test_constant_trajectory(host):
    check_constant(host_call(host))


@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_translation_changes_nothing(host, name):
    check_translation(host_call(host), name)


# ---- 4. independence ----

def check_permutation(call):
    c = RR.cases()["ragged48"]
    batch = (c["so"], c["T"], c["C"])
    perm = np.random.default_rng(7).permutation(len(c["so"]) - 1)
    so2, T2, C2 = Z.take(batch, perm)
    a = call(*batch, c["lim"], 0.8, S_HI)
    b = call(so2, T2, C2, c["lim"], 0.8, S_HI)
    segs = np.concatenate([np.arange(c["so"][p], c["so"][p + 1]) for p in perm])
    assert same((a[0][segs], a[1][segs], a[2][perm], a[3][perm]), b)


def check_seams(call, Bs=SEAMS):
    """The first B trajectories of ragged48 repeated: every row equals the full batch's to the bit."""
    c = RR.cases()["ragged48"]
    full = call(c["so"], c["T"], c["C"], c["lim"], 0.8, S_HI)
    for B in Bs:
        rows = np.arange(B) % 48
        so2, T2, C2 = Z.take((c["so"], c["T"], c["C"]), rows)
        segs = np.concatenate([np.arange(c["so"][p], c["so"][p + 1]) for p in rows])
        assert same((full[0][segs], full[1][segs], full[2][rows], full[3][rows]), call(so2, T2, C2, c["lim"], 0.8, S_HI)), B


def check_bad_rows(call):
    """A NaN coefficient, a NaN time and a zero time: FEAS_NONFINITE alone, NaN rows, the times
    copied; the other trajectories bit-identical to the clean run."""
    c = RR.cases()["ragged48"]
    so, lim = c["so"], c["lim"]
    clean = call(so, c["T"], c["C"], lim, 0.8, S_HI)
    C2, T2 = c["C"].copy(), c["T"].copy()
    C2[so[3], 1, 4] = np.nan
    T2[so[20]] = np.nan
    T2[so[42] - 1] = 0.0
    bad = [3, 20, 41]
    T_out, seg_rec, rec, flags = call(so, T2, C2, lim, 0.8, S_HI)
    keep_b = np.ones(48, bool)
    keep_b[bad] = False
    keep_s = np.repeat(keep_b, np.diff(so))
    assert (flags[bad] == NONFINITE).all() and np.isnan(rec[bad]).all() and np.isnan(seg_rec[~keep_s]).all()
    assert np.array_equal(bits(T_out[~keep_s]), bits(T2[~keep_s]))
    assert same((clean[0][keep_s], clean[1][keep_s], clean[2][keep_b], clean[3][keep_b]),
                (T_out[keep_s], seg_rec[keep_s], rec[keep_b], flags[keep_b]))


def check_in_place_repeat_and_null(call, name):
    c = RR.cases()[name]
    args = (c["so"], c["T"], c["C"])
    full = call(*args, c["lim"], 0.8, S_HI)
    assert same(full, call(*args, c["lim"], 0.8, S_HI))  # a repeated call
    assert same(full, call(*args, c["lim"], 0.8, S_HI, in_place=True))
    for k in range(3):  # no seg_rec and two limits infinite: two ladders are skipped
        one = tuple(c["lim"][q] if q == k else INF for q in range(3))
        want = call(*args, one, 0.8, S_HI)
        got = call(*args, one, 0.8, S_HI, want=(1, 0, 1, 1))
        assert got[1] is None and same((want[0], want[2], want[3]), (got[0], got[2], got[3]))
    for w in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):  # any output alone
        got = call(*args, c["lim"], 0.8, S_HI, want=w)
        assert same([x for x, k in zip(full, w) if k], [x for x in got if x is not None])


def test_permutation(host):
    check_permutation(host_call(host))


def test_batch_sizes_across_the_tile(host):
    check_seams(host_call(host))


def test_bad_rows_stay_alone(host):
    check_bad_rows(host_call(host))


@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_in_place_repeat_and_null_outputs(host, name):
    check_in_place_repeat_and_null(host_call(host), name)


# ---- 5. fixed point through the solver ----

def check_fixed_point(call, solver):
    """M = 1, rest to rest: the solution is one shape scaled in time, so re-timing is the uniform
    dilation and one round lands on the limit: |r_max - 1| <= 2e-9 wherever the first r lay in
    [s_lo, s_hi]."""
    rng = np.random.default_rng(11)
    B, s_lo, s_hi = 37, 0.5, 2.0
    so = np.arange(B + 1, dtype=np.int32)
    W = rng.uniform(-4.0, 4.0, (2 * B, 3))
    T = np.linalg.norm(W[1::2] - W[0::2], axis=1) * rng.uniform(0.6, 3.0, B)  # mean speeds of 1/3 .. 5/3
    lim = (1.5, 3.0, 30.0)
    C = solver.solve(so, W, T)[0]
    T1, _, rec1, _ = call(so, T, C, lim, s_lo, s_hi)
    C1 = solver.solve(so, W, T1)[0]
    _, _, rec2, fl2 = call(so, T1, C1, lim, s_lo, s_hi)
    inside = (rec1[:, 0] >= s_lo) & (rec1[:, 0] <= s_hi)
    print("fixed point: %d of %d inside, |r_max - 1| <= %.3g" % (inside.sum(), B, np.abs(rec2[inside, 0] - 1.0).max()))
    assert inside.sum() >= B // 2 and (~inside).any()
    assert (np.abs(rec2[inside, 0] - 1.0) <= 2e-9).all()
    assert (rec2[rec1[:, 0] > s_hi, 0] > 1.0).all() and (rec2[rec1[:, 0] < s_lo, 0] < 1.0).all()


def test_fixed_point_for_one_segment(host):
    check_fixed_point(host_call(host), host)


def test_retime_loop_reaches_the_limits(host):
    """Solver.retime_loop on host arrays: the result is feasible by the bounds call (the closing
    dilation) and no longer than the dilation alone would have made the worst trajectory."""
    from trajectory_generator_ros2_amd import Limits
    c = RR.cases()["ragged48"]
    so, W, T0 = R.ragged48()
    lim = Limits(v_max=c["lim"][0], a_max=c["lim"][1], j_max=c["lim"][2])
    T, C, hist = host.retime_loop(so, W, T0, lim, rounds=2)
    assert 1 <= len(hist) <= 2 and all(0.0 <= h["over"] <= 1.0 and h["mean_D_out"] > 0.0 for h in hist)
    ext, _ = host.bounds(so, T, C)
    assert (ext[:, 6:9] <= np.array(c["lim"]) * (1.0 + 2e-9)).all()
    assert (T >= T0 * (1.0 - 1e-12)).all()  # s_lo = 1 never shortens
    T1, C1, hist0 = host.retime_loop(so, W, T0, lim, rounds=0)  # solve + dilate
    assert hist0 == [] and (host.bounds(so, T1, C1)[0][:, 6:9] <= np.array(c["lim"]) * (1.0 + 2e-9)).all()


# ---- 6. argument errors ----

def check_bad_arguments(status_of):
    """status_of(lim, s_lo, s_hi, want=(1, 1, 1, 1), B=None) -> tgms_status of a call on a small batch."""
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG
    ok = (1.0, 1.0, 1.0)
    assert status_of(ok, 1.0, 1.0) == 0 and status_of(ok, 0.5, 4.0) == 0 and status_of((INF, INF, 2.0), 1.0, 2.0) == 0
    for s_lo, s_hi in ((0.0, 2.0), (-1.0, 2.0), (1.5, 2.0), (0.5, 0.75), (np.nan, 2.0), (1.0, np.nan), (1.0, INF),
                       (INF, INF), (-INF, 2.0)):
        assert status_of(ok, s_lo, s_hi) == ERR_INVALID_ARG, (s_lo, s_hi)
    for k in range(3):
        for x in (np.nan, 0.0, -1.0, -INF):
            assert status_of(tuple(x if q == k else 1.0 for q in range(3)), 1.0, 2.0) == ERR_INVALID_ARG, (k, x)
    assert status_of((INF, INF, INF), 1.0, 2.0) == ERR_INVALID_ARG
    assert status_of(None, 1.0, 2.0) == ERR_INVALID_ARG
    assert status_of(ok, 1.0, 2.0, want=(0, 0, 0, 0)) == ERR_INVALID_ARG
    assert status_of(ok, 1.0, 2.0, B=0) == 0
    assert status_of(ok, 1.0, 2.0, B=-1) == ERR_INVALID_ARG


def test_bad_arguments(host):
    from trajectory_generator_ros2_amd import ERR_UNSUPPORTED, Limits, TgmsError
    so, T, C = RR.knot_peak(2)

    def status_of(lim, s_lo, s_hi, want=(1, 1, 1, 1), B=None):
        return raw_call(host, so, T, C, lim, s_lo, s_hi, want)[0] if B is None else _raw_b(host, B)
    check_bad_arguments(status_of)
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.retime_device(1, so, T, C, Limits(v_max=1.0), d_rec=np.zeros((1, 3)))
    assert e.value.status == ERR_UNSUPPORTED and "tgms_retime_batch_dev" in str(e.value)


def _raw_b(solver, B):
    import ctypes
    from trajectory_generator_ros2_amd import Limits, _lib
    so, rec = np.zeros(2, np.int32), np.zeros(3)
    return _lib.load().tgms_retime_batch(solver._h, B, so.ctypes.data, None, None, ctypes.byref(Limits(v_max=1.0)), 1.0,
                                         2.0, None, None, rec.ctypes.data, None)


def test_exports_and_constants(host):
    from trajectory_generator_ros2_amd import _lib
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tgms.h")).read()
    for name in ("tgms_retime_batch", "tgms_retime_batch_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name) and re.search(r"\b%s\s*\(" % name, text)
    for name, v in (("RETIME_STRIDE", 4), ("RETIME_REC", 3), ("RT_OVER", 1), ("RT_CAPPED", 2), ("RT_CHANGED", 4),
                    ("RT_SEG_SHIFT", 8)):
        assert getattr(_lib, name) == v and re.search(r"#define TGMS_%s %d\b" % (name, v), text)
    assert (OVER, CAPPED, CHANGED, SEG_SHIFT) == (_lib.RT_OVER, _lib.RT_CAPPED, _lib.RT_CHANGED, _lib.RT_SEG_SHIFT)
    assert _lib.load().tgms_abi_version() == 2
