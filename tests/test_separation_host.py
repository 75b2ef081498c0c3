"""CPU: the continuous swarm separation on the explicit host backend (tgms_separation_batch on a
tgms_create_host handle; csrc/tgms_host.cpp separation(), the algorithm of
csrc/tgms_separation_core.h).

Closed-form answers first (they catch a wrong root-finder, a wrong knot merge or a wrong held
end, not merely a missing one), then the 1e-9 contract of include/tgms.h against the
independent reference of separation_ref.py on 96 pairs of solved ragged trajectories, then the
all-pairs order, the flags, the argument checks and the isolation of bad input.

Measured on the 96 + 96 pairs (host backend): d_min^2 within 2.7e-15 x L^2 of the reference and
dist(t_min)^2 within 2.7e-15 x L^2 of d_min^2, against the contract's 1e-9."""
import os
import re

import numpy as np
import pytest

import separation_ref as SR
from extrema_ref import ORACLE_TOL

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
    c = dict(SR.contract_case(request.param))
    c["sep"], c["flags"] = host.separation(c["so"], c["T"], c["C"], c["pairs"], c["t0"])
    return c


def _raw(host, so, T, C, P, pairs=None, t0=None, scale=None, r_min=0.0, sep=None, flags=None):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return host._L.tgms_separation_batch(host._h, len(so) - 1, p(so), p(T), p(C), p(t0), P, p(pairs), p(scale),
                                         r_min, p(sep), p(flags))


PAIR01 = np.array([[0, 1]], np.int32)


@pytest.mark.parametrize("split", [False, True])
def test_known_answer_crossing(host, split):
    so, T, C = SR.crossing(split)
    sep, fl = host.separation(so, T, C, PAIR01)
    assert fl[0] == 0
    assert abs(sep[0, 0] - 0.5) <= 1e-12 * 0.5 and abs(sep[0, 1] - 1.0) <= 1e-12
    # the knots alone see sqrt(4.25)
    assert np.hypot(2.0, 0.5) > 2.06


def test_known_answer_shifted_starts(host):
    """i: (t, 0, 0) from t = 0, j: (2 - tau, 0.5 + tau / 4, 0) from t = 0.6: the relative motion is
    r0 + v t with r0 = (-2.6, -0.35), v = (2, -0.25) while both fly, closest at t* = -r0.v / |v|^2
    = 1.2585 (inside [0.6, 2]), where the vehicles do not meet."""
    i = SR.line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 2.0)
    j = SR.line([2.0, 0.5, 0.0], [-1.0, 0.25, 0.0], 2.0)
    so, T, C = SR.batch(i, j)
    r0, v = np.array([-2.6, -0.5 + 0.25 * 0.6]), np.array([2.0, -0.25])
    ts = -(r0 @ v) / (v @ v)
    assert 0.6 < ts < 2.0
    want = np.linalg.norm(r0 + v * ts)
    sep, fl = host.separation(so, T, C, PAIR01, start_times=[0.0, 0.6])
    assert fl[0] == 0 and abs(sep[0, 0] - want) <= 1e-12 * want and abs(sep[0, 1] - ts) <= 1e-9
    # and the order of the pair does not matter
    sep2, _ = host.separation(so, T, C, PAIR01[:, ::-1], start_times=[0.0, 0.6])
    assert abs(sep2[0, 0] - want) <= 1e-12 * want


def test_held_tail(host):
    """i ends at t = 1 at (1, 0, 0) and holds; j passes (1, 0.25, 0) at t = 3."""
    so, T, C = SR.batch(SR.line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 1.0), SR.line([-2.0, 0.25, 0.0], [1.0, 0.0, 0.0], 4.0))
    sep, fl = host.separation(so, T, C, PAIR01)
    assert fl[0] == 0 and abs(sep[0, 0] - 0.25) <= 1e-12 * 0.25 and abs(sep[0, 1] - 3.0) <= 1e-12 * 3.0


def test_disjoint_windows(host):
    """j starts at t = 3, after i has ended at (2, 0, 0): every interval has a held side.  While i
    flies, j waits at (1, 0.8, 0), never closer than 0.8; then j passes i's end point along
    (-1, 0.8) + (1, -0.3) tau relative to it, closest at tau* = 1.24 / 1.09."""
    so, T, C = SR.batch(SR.line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 2.0), SR.line([1.0, 0.8, 0.0], [1.0, -0.3, 0.0], 2.0))
    r0, v = np.array([-1.0, 0.8]), np.array([1.0, -0.3])
    ts = -(r0 @ v) / (v @ v)
    want = np.linalg.norm(r0 + v * ts)
    assert 0.0 < ts < 2.0 and want < 0.5
    sep, fl = host.separation(so, T, C, PAIR01, start_times=[0.0, 3.0])
    assert fl[0] == 0 and abs(sep[0, 0] - want) <= 1e-12 * want and abs(sep[0, 1] - (3.0 + ts)) <= 1e-9


def test_identical_trajectories_give_exactly_zero(host):
    c = SR.contract_case("end_derivs")
    so, T, C = c["so"], c["T"], c["C"]
    b = int(np.flatnonzero(np.diff(so) == 16)[0])
    one = (C[so[b]:so[b + 1]], T[so[b]:so[b + 1]])
    so2, T2, C2 = SR.batch(one, one)
    sep, fl = host.separation(so2, T2, C2, np.array([[0, 0], [0, 1], [1, 1]], np.int32), start_times=[1.7, 1.7])
    assert not fl.any() and (sep[:, 0] == 0.0).all() and not np.signbit(sep[:, 0]).any()
    assert ((sep[:, 1] >= 1.7) & (sep[:, 1] <= 1.7 + T2[:16].sum() + 1e-12)).all()
    sep, fl = host.separation(so, T, C, np.array([[b, b], [3, 3]], np.int32), start_times=c["t0"])
    assert not fl.any() and (sep[:, 0] == 0.0).all()


def test_scale(host):
    """Stacked 0.9 apart in z, flying the same line: s = (1, 1, 1/3) gives 0.3."""
    so, T, C = SR.batch(SR.line([0.0, 0.0, 1.0], [1.0, 0.5, 0.0], 2.0), SR.line([0.0, 0.0, 1.9], [1.0, 0.5, 0.0], 2.0))
    sep, _ = host.separation(so, T, C, PAIR01, scale=[1.0, 1.0, 1.0 / 3.0])
    assert abs(sep[0, 0] - 0.3) <= 1e-12 * 0.3
    sep, _ = host.separation(so, T, C, PAIR01)
    assert abs(sep[0, 0] - 0.9) <= 1e-12 * 0.9


def test_ragged_pairs_meet_the_contract(case):
    assert not case["flags"].any()
    SR.check_contract(case["sep"], case["trajs"], case["pairs"], case["refs"], what="host separation")


def test_dominates_a_10ms_grid(case):
    """d_min^2 <= the least squared reference distance over a 10 ms grid of the window, plus the
    contract's slack."""
    for n, ((i, j), (_, L, dist)) in enumerate(zip(case["pairs"], case["refs"])):
        lo, hi = SR.window(case["trajs"][i], case["trajs"][j])
        grid = np.arange(lo, hi, 0.01)
        assert case["sep"][n, 0] ** 2 <= float((dist(grid) ** 2).min()) + ORACLE_TOL * L ** 2, n


@pytest.mark.parametrize("B", [2, 3, 48])
def test_all_pairs_is_the_explicit_list(host, B):
    c = SR.contract_case("rest")
    so, T, C, t0 = c["so"][:B + 1], c["T"][:c["so"][B]], c["C"][:c["so"][B]], c["t0"][:B]
    pairs = np.array([(i, j) for i in range(B) for j in range(i + 1, B)], np.int32)
    sep_a, fl_a = host.separation(so, T, C, None, t0)
    sep_e, fl_e = host.separation(so, T, C, pairs, t0)
    assert sep_a.shape == (B * (B - 1) // 2, 2)
    assert np.array_equal(sep_a.view(np.int64), sep_e.view(np.int64)) and np.array_equal(fl_a, fl_e)
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG
    sep = np.empty((len(pairs) + 1, 2))
    for P in (len(pairs) - 1, len(pairs) + 1):
        assert _raw(host, so, T, C, P, sep=sep) == ERR_INVALID_ARG


def test_flags_and_arguments(host):
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, SEP_CLOSE, TgmsError
    so, T, C = SR.crossing()
    sep, fl = host.separation(so, T, C, PAIR01)
    d = float(sep[0, 0])
    assert host.separation(so, T, C, PAIR01, r_min=d)[1][0] == 0           # strict: equal is not close
    sep2, fl2 = host.separation(so, T, C, PAIR01, r_min=np.nextafter(d, np.inf))
    assert fl2[0] == SEP_CLOSE and np.array_equal(sep2.view(np.int64), sep.view(np.int64))
    for r in (0.0, -1.0, -np.inf):
        assert host.separation(so, T, C, PAIR01, r_min=r)[1][0] == 0       # r_min <= 0 checks nothing
    assert host.separation(so, T, C, PAIR01, r_min=np.inf)[1][0] == SEP_CLOSE
    with pytest.raises(TgmsError) as e:
        host.separation(so, T, C, PAIR01, r_min=float("nan"))
    assert e.value.status == ERR_INVALID_ARG
    for bad in ([0.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, float("nan")], [float("inf"), 1.0, 1.0]):
        with pytest.raises(TgmsError) as e:
            host.separation(so, T, C, PAIR01, scale=bad)
        assert e.value.status == ERR_INVALID_ARG
    assert _raw(host, so, T, C, 1, PAIR01) == ERR_INVALID_ARG              # both outputs NULL
    flags = np.full(1, -1, np.int32)                                       # one output alone is enough
    assert _raw(host, so, T, C, 1, PAIR01, flags=flags) == 0 and flags[0] == 0
    out = np.full((1, 2), -7.0)
    assert _raw(host, so, T, C, 0, PAIR01, sep=out) == 0 and (out == -7.0).all()   # P == 0
    assert _raw(host, so, T, C, -1, PAIR01, sep=out) == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.separation_device(2, so, T, C, 1, PAIR01, d_sep=out)
    assert e.value.status == ERR_UNSUPPORTED


def test_bad_input_marks_exactly_its_pairs(host):
    from trajectory_generator_ros2_amd import SEP_NONFINITE
    c = SR.contract_case("rest")
    so, T, C, t0 = c["so"], c["T"], c["C"], c["t0"]
    pairs = np.concatenate([c["pairs"], [[-1, 5], [5, 48], [48, -1], [7, 7]]]).astype(np.int32)
    r_min = float(np.median([r[0] ** 0.5 for r in c["refs"]]))
    sep0, fl0 = host.separation(so, T, C, pairs, t0, r_min=r_min)
    assert (fl0[:96] & 1).any() and not (fl0[:96] & 1).all()
    C2, T2, t2 = C.copy(), T.copy(), t0.copy()
    C2[so[3] + 1, 1, 4] = np.nan      # a NaN coefficient in trajectory 3
    T2[so[41 + 1] - 1] = 0.0          # a zero time in trajectory 41
    t2[20] = np.nan                   # a NaN start time in trajectory 20
    assert np.diff(so)[3] >= 2
    sep, fl = host.separation(so, T2, C2, pairs, t2, r_min=r_min)
    bad = np.isin(pairs, [3, 20, 41]).any(axis=1) | (pairs < 0).any(axis=1) | (pairs >= 48).any(axis=1)
    assert bad[96:99].all() and not bad[99] and 6 <= bad[:96].sum() < 96
    assert (fl[bad] == SEP_NONFINITE).all() and np.isnan(sep[bad]).all()
    assert (fl0[96:99] == SEP_NONFINITE).all() and np.isnan(sep0[96:99]).all()   # the indices alone
    assert np.array_equal(fl[~bad], fl0[~bad])
    assert np.array_equal(sep[~bad].view(np.int64), sep0[~bad].view(np.int64))


def test_exports_hold_the_two_new_entry_points(host):
    from trajectory_generator_ros2_amd import SEP_CLOSE, SEP_NONFINITE, SEP_STRIDE, _lib
    src = open(os.path.join(ROOT, "include", "tgms.h")).read()
    declared = set(re.findall(r"\b(tgms_[a-z_]+)\s*\(", src))
    for name in ("tgms_separation_batch", "tgms_separation_batch_device"):
        assert name in _lib.EXPORTS and name in declared and hasattr(_lib.load(), name)
    for name, v in (("STRIDE", SEP_STRIDE), ("CLOSE", SEP_CLOSE), ("NONFINITE", SEP_NONFINITE)):
        assert int(re.search(r"#define TGMS_SEP_%s (\d+)" % name, src).group(1)) == v
    assert _lib.load().tgms_abi_version() == 2
