"""CPU: the continuous feasibility bounds on the explicit host backend (tgms_bounds_batch on a
tgms_create_host handle; csrc/tgms_host.cpp bounds(), the algorithm of csrc/tgms_bounds_core.h).

Closed-form answers first (they catch a wrong root-finder, not merely a missing one), then the
1e-9 contract of include/tgms.h against the independent reference of bounds_ref.py on 48 + 48
solved ragged trajectories, then what the record promises next to the sampled check: it
dominates it at every dt, and it sees what a coarse dt misses."""
import os
import re

import numpy as np
import pytest

import bounds_ref as R
from extrema_ref import ORACLE_TOL, durations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.build import LIB_TGMS, build_tgms
    from trajectory_generator_ros2_amd.solver import Solver
    if not os.path.exists(LIB_TGMS):
        build_tgms()
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module", params=["rest", "end_derivs"])
def case(request, host):
    """The 48-trajectory batch (every M in 1..16 three times), rest to rest or with non-zero
    end derivatives, solved by the host backend; its records and the reference, computed once."""
    so, W, T = R.ragged48()
    ED = None if request.param == "rest" else R.end_derivs48()
    C, _, worst = host.solve(so, W, T, ED)
    assert worst == 0
    assert sorted(np.diff(so)) == sorted(list(range(1, 17)) * 3)
    ext, flags = host.bounds(so, T, C)
    return dict(so=so, W=W, T=T, ED=ED, C=C, ext=ext, flags=flags, ref=R.records(so, T, C))


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_known_answer_rest_to_rest(host, T):
    p0, d = np.array([0.3, -1.0, 2.0]), -1.7
    so, Ts, C, peaks = R.rest_to_rest(p0, d, T, axis=1)
    ext, flags = host.bounds(so, Ts, C)
    assert flags[0] == 0
    assert (np.abs(ext[0, 6:9] - peaks) <= 1e-12 * peaks).all(), (ext[0, 6:9] - peaks) / peaks
    lo, hi = p0.copy(), p0.copy()
    lo[1] += d  # d < 0: the axis runs from p0 down to p0 + d
    assert np.abs(ext[0, 0:3] - lo).max() <= 1e-12 * np.abs(lo).max()
    assert np.abs(ext[0, 3:6] - hi).max() <= 1e-12 * np.abs(hi).max()
    assert np.array_equal(ext[0, [0, 2, 3, 5]], p0[[0, 2, 0, 2]])  # the constant axes: exactly the point
    assert ext[0, 4] == p0[1] and ext[0, 9] == T


def test_constructed_overshoot(host):
    so, T, C, pmin, pmax = R.overshoot()
    ext, flags = host.bounds(so, T, C)
    assert flags[0] == 0
    tol = 1e-12 * max(np.abs(pmin).max(), np.abs(pmax).max())
    assert np.abs(ext[0, 0:3] - pmin).max() <= tol, ext[0, 0:3] - pmin
    assert np.abs(ext[0, 3:6] - pmax).max() <= tol, ext[0, 3:6] - pmax


def test_ragged_batch_meets_the_contract(case):
    R.check_contract(case["ext"], case["ref"])
    assert not case["flags"].any()
    assert np.array_equal(case["ext"][:, 9].view(np.int64), durations(case["so"], case["T"]).view(np.int64))


def test_sees_what_a_coarse_dt_misses(host):
    """Rest to rest in one segment, checked by samples at dt = 2T: sample 0 and the pinned last
    one, both at rest, so v_peak == 0 and the speed limit |d|/T passes.  The continuous check
    reports 35/16 |d|/T and sets the bit."""
    from trajectory_generator_ros2_amd import FEAS_SPEED, Limits
    p0, d, T = np.array([0.3, -1.0, 2.0]), 1.7, 1.0
    so, Ts, C, peaks = R.rest_to_rest(p0, d, T, axis=0)
    W = np.array([p0, p0 + [d, 0.0, 0.0]])
    lim = Limits(v_max=abs(d) / T)
    ext_s, fl_s = host.extrema(so, W, Ts, None, C, 2 * T, lim)
    assert ext_s[0, 6] == 0.0 and not fl_s[0] & FEAS_SPEED
    ext_c, fl_c = host.bounds(so, Ts, C, lim)
    assert fl_c[0] == FEAS_SPEED and ext_c[0, 6] > 2.0 * lim.v_max


@pytest.mark.parametrize("dt", [0.01, 0.37])
def test_dominates_the_sampled_check(host, case, dt):
    """Continuous peaks >= sampled peaks and continuous extents around the sampled ones, up to
    1e-9: the slack covers the pinned last sample, which is the waypoint and the given end
    derivative, not the polynomial's value there."""
    c = case
    smp, _ = host.extrema(c["so"], c["W"], c["T"], c["ED"], c["C"], dt)
    ext = c["ext"]
    assert (ext[:, 6:9] >= smp[:, 6:9] * (1.0 - ORACLE_TOL)).all()
    slack = ORACLE_TOL * np.abs(ext[:, 0:6]).max(axis=1)[:, None]
    assert (ext[:, 0:3] <= smp[:, 0:3] + slack).all() and (ext[:, 3:6] >= smp[:, 3:6] - slack).all()
    assert np.array_equal(ext[:, 9].view(np.int64), smp[:, 9].view(np.int64))


def test_flags_follow_the_record(host, case):
    """Strict comparisons on the stored values: a limit equal to a value is inside."""
    from trajectory_generator_ros2_amd import FEAS_ACCEL, FEAS_BOX, FEAS_JERK, FEAS_SPEED, Limits
    so, T, C, ext = case["so"], case["T"], case["C"], case["ext"]
    lim = Limits(pmin=ext[:, 0:3].min(axis=0), pmax=ext[:, 3:6].max(axis=0), v_max=np.median(ext[:, 6]),
                 a_max=ext[:, 7].max(), j_max=np.nextafter(ext[:, 8].max(), 0.0))
    ext2, flags = host.bounds(so, T, C, lim)
    assert np.array_equal(ext2.view(np.int64), ext.view(np.int64))
    assert not (flags & (FEAS_BOX | FEAS_ACCEL)).any()
    assert np.array_equal((flags & FEAS_SPEED) != 0, ext[:, 6] > lim.v_max) and (flags & FEAS_SPEED).any()
    assert np.array_equal((flags & FEAS_JERK) != 0, ext[:, 8] == ext[:, 8].max())
    lim.pmin[0] = np.nextafter(lim.pmin[0], np.inf)
    _, flags = host.bounds(so, T, C, lim)
    assert np.array_equal((flags & FEAS_BOX) != 0, ext[:, 0] < lim.pmin[0]) and (flags & FEAS_BOX).any()
    assert not host.bounds(so, T, C, Limits())[1].any()  # +-inf everywhere: unchecked
    assert not host.bounds(so, T, C, Limits(v_max=float("inf"), pmin=[-np.inf] * 3, pmax=[np.inf] * 3))[1].any()
    assert not case["flags"].any()  # limits=None on clean input


def test_nonfinite_input_marks_one_trajectory(host, case):
    from trajectory_generator_ros2_amd import FEAS_NONFINITE, Limits
    so, T, C, ext = case["so"], case["T"], case["C"], case["ext"]
    lim = Limits(v_max=np.median(ext[:, 6]))
    _, fl0 = host.bounds(so, T, C, lim)
    C2, T2 = C.copy(), T.copy()
    C2[so[3], 1, 4] = np.nan          # a NaN coefficient in trajectory 3
    T2[so[20] + 0] = np.nan           # a NaN time in trajectory 20
    T2[so[41 + 1] - 1] = 0.0          # a zero time in trajectory 41
    ext2, fl = host.bounds(so, T2, C2, lim)
    bad = [3, 20, 41]
    assert (fl[bad] == FEAS_NONFINITE).all() and np.isnan(ext2[bad]).all()
    keep = np.ones(len(fl), bool)
    keep[bad] = False
    assert np.array_equal(fl[keep], fl0[keep])
    assert np.array_equal(ext2[keep].view(np.int64), ext[keep].view(np.int64))


def test_bad_arguments(host, case):
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, Limits, TgmsError, _lib
    so, T, C, ext = case["so"], case["T"], case["C"], case["ext"]
    for bad in (Limits(v_max=float("nan")), Limits(pmin=[0, 0, 1], pmax=[1, 1, 0])):
        with pytest.raises(TgmsError) as e:
            host.bounds(so, T, C, bad)
        assert e.value.status == ERR_INVALID_ARG
    st = _lib.load().tgms_bounds_batch(host._h, len(so) - 1, so.ctypes.data, T.ctypes.data, C.ctypes.data, None,
                                       None, None)
    assert st == ERR_INVALID_ARG  # both outputs NULL
    fl = np.full(len(so) - 1, -1, np.int32)  # one output alone is enough
    assert _lib.load().tgms_bounds_batch(host._h, len(so) - 1, so.ctypes.data, T.ctypes.data, C.ctypes.data, None,
                                         None, fl.ctypes.data) == 0 and not fl.any()
    so0 = np.zeros(1, np.int32)  # B == 0
    assert _lib.load().tgms_bounds_batch(host._h, 0, so0.ctypes.data, None, None, None, ext.ctypes.data, None) == 0
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.bounds_device(len(so) - 1, so, T, C, d_extrema=ext.copy())
    assert e.value.status == ERR_UNSUPPORTED


def test_constant_trajectory(host):
    """All coefficients of degree >= 1 zero: peaks exactly 0.0, extents exactly the point."""
    so = np.array([0, 3], np.int32)
    C = np.zeros((3, 3, 8))
    C[:, :, 0] = [0.1, -2.7, 3.3]
    ext, flags = host.bounds(so, [0.5, 2.0, 7.0], C)
    assert flags[0] == 0
    assert np.array_equal(ext[0, 0:3], C[0, :, 0]) and np.array_equal(ext[0, 3:6], C[0, :, 0])
    assert (ext[0, 6:9] == 0.0).all() and ext[0, 9] == (0.5 + 2.0) + 7.0


def test_exports_hold_the_two_new_entry_points(host):
    from trajectory_generator_ros2_amd import _lib
    declared = set(re.findall(r"\b(tgms_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", "tgms.h")).read()))
    for name in ("tgms_bounds_batch", "tgms_bounds_batch_device"):
        assert name in _lib.EXPORTS and name in declared and hasattr(_lib.load(), name)
    assert sorted(declared) == sorted(_lib.EXPORTS)
    assert _lib.load().tgms_abi_version() == 2
