"""CPU: the continuous thrust and tilt bounds on the explicit host backend (tgms_thrust_batch on
a tgms_create_host handle; csrc/tgms_host.cpp thrust(), the algorithm of
csrc/tgms_thrust_core.h).  Closed forms first, then the 1e-9 contract of include/tgms.h against
the independent reference of thrust_ref.py on 48 + 48 solved ragged trajectories, the reported
times, flags and argument errors.  tests/test_gpu_thrust.py repeats every case on the device."""
import os

import numpy as np
import pytest

import bounds_ref as R
import thrust_ref as TR

G = TR.G0
P0 = np.array([0.3, -1.0, 2.0])


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
    """bounds_ref.ragged48 (every M in 1..16 three times), rest to rest or with end_derivs48,
    solved by the host backend; its records and the reference, computed once."""
    so, W, T = R.ragged48()
    ED = None if request.param == "rest" else R.end_derivs48()
    C, _, worst = host.solve(so, W, T, ED)
    assert worst == 0
    rec, flags = host.thrust(so, T, C)
    return dict(so=so, T=T, C=C, rec=rec, flags=flags, ref=TR.records(so, T, C))


# ---- closed forms, shared with test_gpu_thrust.py: each takes the call under test ----

def check_horizontal(call, T):
    """f_min == g to the bit (a = 0 at u = 0), f_max and tilt_max to 1e-12 relative, and theta
    at t_tilt reproduces tilt_max."""
    d = -1.7 * max(T, 1.0) ** 2
    so, Ts, C, _ = R.rest_to_rest(P0, d, T, axis=0)
    a = TR.a_peak(d, T)
    rec, flags = call(so, Ts, C)
    assert flags[0] == 0
    assert rec[0, 0] == G
    assert abs(rec[0, 2] - np.hypot(a, G)) <= 1e-12 * np.hypot(a, G)
    assert abs(rec[0, 4] - np.arctan(a / G)) <= 1e-12 * np.arctan(a / G)
    assert (0.0 <= rec[0, [1, 3, 5]]).all() and (rec[0, [1, 3, 5]] <= T).all()
    assert abs(TR.evaluate(so, Ts, C, 0, rec[0, 5])[1] - rec[0, 4]) <= 1e-12 * rec[0, 4]
    assert abs(TR.evaluate(so, Ts, C, 0, rec[0, 3])[0] - rec[0, 2]) <= 1e-12 * rec[0, 2]


def check_vertical(call):
    from trajectory_generator_ros2_amd import THRUST_LOW, THRUST_TILT, ThrustLimits
    so, Ts, C, _ = R.rest_to_rest(P0, 0.9, 1.5, axis=2)
    a = TR.a_peak(0.9, 1.5)
    assert a < G
    rec, flags = call(so, Ts, C)
    assert flags[0] == 0 and rec[0, 4] == 0.0
    assert abs(rec[0, 2] - (G + a)) <= 1e-12 * (G + a) and abs(rec[0, 0] - (G - a)) <= 1e-12 * (G - a)
    so, Ts, C, _ = R.rest_to_rest(P0, 4.0, 1.0, axis=2)
    assert TR.a_peak(4.0, 1.0) > G  # thrust crosses zero
    rec, flags = call(so, Ts, C, limits=ThrustLimits(0.5, float("inf"), 1.0))
    assert rec[0, 0] <= np.sqrt(1e-9) * rec[0, 2]
    assert abs(rec[0, 4] - np.pi) <= 1e-15
    assert flags[0] == THRUST_LOW | THRUST_TILT


def check_constant(call):
    so = np.array([0, 3], np.int32)
    C = np.zeros((3, 3, 8))
    C[:, :, 0] = [0.1, -2.7, 3.3]
    rec, flags = call(so, np.array([0.5, 2.0, 7.0]), C)
    assert flags[0] == 0
    assert rec[0, 0] == G and rec[0, 2] == G and rec[0, 4] == 0.0
    assert (0.0 <= rec[0, [1, 3, 5]]).all() and (rec[0, [1, 3, 5]] <= (0.5 + 2.0) + 7.0).all()


def _host_call(host):
    return lambda so, T, C, limits=None: host.thrust(so, T, C, G, limits)


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_horizontal_rest_to_rest(host, T):
    check_horizontal(_host_call(host), T)


def test_vertical_rest_to_rest(host):
    check_vertical(_host_call(host))


def test_constant_trajectory(host):
    check_constant(_host_call(host))


def test_ragged_batch_meets_the_contract(case):
    """The reference's own f_min is 6.20 at the least on these batches and F / f_min 2.26 at
    the most, so the tilt bound is at most 2.3e-9 rad."""
    assert case["ref"][:, 0].min() >= 6.0 and (case["ref"][:, 1] / case["ref"][:, 0]).max() <= 2.3
    TR.check_contract(case["rec"], case["ref"])
    assert not case["flags"].any()


def test_times_attain_the_stored_values(case):
    TR.check_times(case["so"], case["T"], case["C"], case["rec"], case["ref"])


def test_the_roots_of_G_are_needed(case):
    """The reference on its 4,097-point grid alone falls short of the full one on the tilt by
    more than the library's error: no sampled implementation passes for this one."""
    grid = TR.records(case["so"], case["T"], case["C"], grid_only=True)
    short = (case["ref"][:, 2] - grid[:, 2]).max()
    err = np.abs(case["rec"][:, 4] - case["ref"][:, 2]).max()
    print("tilt: grid alone short by %.3g rad, library off by %.3g rad" % (short, err))
    assert short >= 0.0 and err < max(short, 1e-12)


def test_flags_follow_the_record(host, case):
    """Strict comparisons on the stored values: a limit equal to a value is inside, nextafter
    past it is outside; infinite entries and limits=None check nothing."""
    from trajectory_generator_ros2_amd import THRUST_HIGH, THRUST_LOW, THRUST_TILT, ThrustLimits
    so, T, C, rec = case["so"], case["T"], case["C"], case["rec"]
    lo, hi, tilt = rec[:, 0].min(), rec[:, 2].max(), rec[:, 4].max()
    rec2, fl = host.thrust(so, T, C, G, ThrustLimits(lo, hi, tilt))
    assert not fl.any() and np.array_equal(rec2.view(np.int64), rec.view(np.int64))
    fl = host.thrust(so, T, C, G, ThrustLimits(np.nextafter(lo, np.inf), hi, tilt))[1]
    assert np.array_equal(fl, np.where(rec[:, 0] == lo, THRUST_LOW, 0)) and fl.any()
    fl = host.thrust(so, T, C, G, ThrustLimits(lo, np.nextafter(hi, 0.0), tilt))[1]
    assert np.array_equal(fl, np.where(rec[:, 2] == hi, THRUST_HIGH, 0)) and fl.any()
    fl = host.thrust(so, T, C, G, ThrustLimits(lo, hi, np.nextafter(tilt, 0.0)))[1]
    assert np.array_equal(fl, np.where(rec[:, 4] == tilt, THRUST_TILT, 0)) and fl.any()
    lim = ThrustLimits(np.median(rec[:, 0]), np.median(rec[:, 2]), np.median(rec[:, 4]))
    fl = host.thrust(so, T, C, G, lim)[1]
    want = (np.where(rec[:, 0] < lim.f_min, THRUST_LOW, 0) | np.where(rec[:, 2] > lim.f_max, THRUST_HIGH, 0)
            | np.where(rec[:, 4] > lim.tilt_max, THRUST_TILT, 0))
    assert np.array_equal(fl, want)
    inf = float("inf")
    for lim in (ThrustLimits(), ThrustLimits(-inf, inf, inf), ThrustLimits(inf, -inf, -inf)):
        assert not host.thrust(so, T, C, G, lim)[1].any()
    assert not case["flags"].any()


def test_nonfinite_input_marks_one_trajectory(host, case):
    from trajectory_generator_ros2_amd import FEAS_NONFINITE, ThrustLimits
    so, T, C, rec = case["so"], case["T"], case["C"], case["rec"]
    lim = ThrustLimits(tilt_max=np.median(rec[:, 4]))
    fl0 = host.thrust(so, T, C, G, lim)[1]
    C2, T2 = C.copy(), T.copy()
    C2[so[3], 1, 4] = np.nan   # a NaN coefficient in trajectory 3
    C2[so[9], 0, 0] = np.inf   # an infinite constant term, which p'' never reads, in trajectory 9
    T2[so[20]] = np.nan        # a NaN time in trajectory 20
    T2[so[42] - 1] = 0.0       # a zero time in trajectory 41
    T2[so[30]] = -1.0          # a negative time in trajectory 30
    rec2, fl = host.thrust(so, T2, C2, G, lim)
    bad = [3, 9, 20, 30, 41]
    keep = np.ones(len(fl), bool)
    keep[bad] = False
    assert (fl[bad] == FEAS_NONFINITE).all() and np.isnan(rec2[bad]).all()
    assert np.array_equal(fl[keep], fl0[keep]) and fl0.any()
    assert np.array_equal(rec2[keep].view(np.int64), rec[keep].view(np.int64))


def test_g_zero_gives_the_acceleration_peak(host, case):
    """g == 0 is allowed: f is p'' itself, so f_max is the bounds record's a_peak (the same
    ladder on the same polynomial, evaluated through another scaling)."""
    rec0 = host.thrust(case["so"], case["T"], case["C"], 0.0)[0]
    a_peak = host.bounds(case["so"], case["T"], case["C"])[0][:, 7]
    assert (np.abs(rec0[:, 2] - a_peak) <= 1e-12 * a_peak).all()


def test_bad_arguments(host, case):
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError, ThrustLimits, _lib
    so, T, C, rec = case["so"], case["T"], case["C"], case["rec"]
    B = len(so) - 1
    for kw in (dict(limits=ThrustLimits(f_min=float("nan"))), dict(limits=ThrustLimits(tilt_max=float("nan"))),
               dict(g=float("nan")), dict(g=-1.0), dict(g=float("inf"))):
        with pytest.raises(TgmsError) as e:
            host.thrust(so, T, C, **kw)
        assert e.value.status == ERR_INVALID_ARG
    L = _lib.load()
    assert L.tgms_thrust_batch(host._h, B, so.ctypes.data, T.ctypes.data, C.ctypes.data, G, None, None,
                               None) == ERR_INVALID_ARG  # both outputs NULL
    fl = np.full(B, -1, np.int32)  # one output alone is enough
    assert L.tgms_thrust_batch(host._h, B, so.ctypes.data, T.ctypes.data, C.ctypes.data, G, None, None,
                               fl.ctypes.data) == 0 and not fl.any()
    out = np.full((B, 6), -7.0)
    so0 = np.zeros(1, np.int32)  # B == 0: TGMS_OK, the outputs untouched
    assert L.tgms_thrust_batch(host._h, 0, so0.ctypes.data, None, None, G, None, out.ctypes.data, None) == 0
    assert (out == -7.0).all()
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.thrust_device(B, so, T, C, d_rec=rec.copy())
    assert e.value.status == ERR_UNSUPPORTED


def test_exports_hold_the_two_new_entry_points(host):
    from trajectory_generator_ros2_amd import _lib
    for name in ("tgms_thrust_batch", "tgms_thrust_batch_device"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().tgms_abi_version() == 2
