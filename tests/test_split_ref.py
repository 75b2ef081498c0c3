"""CPU: the split reference (split_ref.py) against closed forms, before anything is held to it:
a parabola split at its peak, a rest-to-rest segment whose excursion is at its last waypoint,
and the min_frac clamp on a cubic that peaks at u = 0.02.  The seg_rec rows are the closed
forms' own."""
import numpy as np
import pytest

import bounds_ref as R
import split_ref as SR
from test_corridor_ref import parabola

K = 0.7


def cubic(T, scale=1000.0):
    """M = 1: y(u) = scale (u^3 / 3 - 1.01 u^2 + 0.04 u), y' = scale (u - 0.02)(u - 2): the
    maximum over [0, 1] is at u = 0.02.  Returns (so, W, T, C)."""
    C = np.zeros((1, 3, 8))
    C[0, 1, 1:4] = np.array([0.04, -1.01, 1.0 / 3.0]) * scale / T ** np.arange(1, 4)
    W = np.array([[0.0, 0.0, 0.0], [0.0, scale * (1.0 / 3.0 - 1.01 + 0.04), 0.0]])
    return np.array([0, 1], np.int32), W, np.array([T]), C


@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_parabola_is_split_at_its_peak(mode):
    T, d, r = 2.0, 0.1, 0.25
    so, Ts, C = parabola(K, T)
    W = np.array([[0.3, 0.0, 2.0], [0.3, 0.0, 2.0]])
    faces = np.array([[0.0, 1.0, 0.0, d]])
    seg_rec = np.array([[K * T * T / 4 - d, T / 2]])
    out = SR.split(so, W, Ts, C, faces, np.array([0, 1]), seg_rec, np.array([0]), r, mode, 0.1)
    assert list(out["so"]) == [0, 2] and list(out["parent"]) == [0, 0] and out["flags"][0] == SR.DONE
    assert abs(out["T"][0] - T / 2) <= 1e-9 * T and out["T"][0] + out["T"][1] == T
    assert np.array_equal(out["W"][[0, 2]], W)
    want_y = d - r if mode == SR.PULL else 0.0
    assert np.abs(out["W"][1] - [0.3, want_y, 2.0]).max() <= 1e-15
    assert list(out["fo"]) == [0, 1, 2] and np.array_equal(out["faces"], np.repeat(faces, 2, axis=0))
    assert list(out["inserted"]) == [True, False]


def test_an_excursion_at_the_last_waypoint_is_not_split():
    L, T = 3.0, 2.0
    so, Ts, C, _ = R.rest_to_rest(np.zeros(3), L, T, axis=0)
    W = np.array([[0.0, 0.0, 0.0], [L, 0.0, 0.0]])
    faces = np.array([[1.0, 0.0, 0.0, L / 2]])
    out = SR.split(so, W, Ts, C, faces, np.array([0, 1]), np.array([[L / 2, T]]), np.array([0]), 0.0, SR.PULL, 0.1)
    assert out["flags"][0] == SR.AT_END and list(out["so"]) == [0, 1] and list(out["parent"]) == [0]
    assert np.array_equal(out["W"], W) and np.array_equal(out["T"], Ts) and np.array_equal(out["faces"], faces)
    assert list(out["fo"]) == [0, 1]
    # one ulp inside the threshold on the left is still a waypoint, just past it is not
    for t_s, want in ((T * 2.0 ** -20, SR.AT_END), (np.nextafter(T * 2.0 ** -20, 1.0), SR.DONE)):
        out = SR.split(so, W, Ts, C, faces, np.array([0, 1]), np.array([[L / 2, t_s]]), np.array([0]), 0.0, SR.CHORD, 0.1)
        assert out["flags"][0] == want


@pytest.mark.parametrize("T", [0.3, 1.0, 7.0])
def test_min_frac_clamps_the_split_time_to_the_bit(T):
    so, W, Ts, C = cubic(T)
    faces = np.array([[0.0, 1.0, 0.0, 0.0]])
    m = 1000.0 * (0.02 ** 3 / 3 - 1.01 * 0.02 ** 2 + 0.04 * 0.02)
    out = SR.split(so, W, Ts, C, faces, None, np.array([[m, 0.02 * T]]), np.array([0]), 0.0, SR.PULL, 0.1)
    assert out["T"][0] == np.float64(0.1) * np.float64(T) and out["T"][1] == np.float64(T) - out["T"][0]
    assert out["fo"] is None and np.array_equal(out["faces"], faces) and out["flags"][0] == SR.DONE
    # p(0.1 T) is already below the face: the point is left where it is
    want = 1000.0 * (0.1 ** 3 / 3 - 1.01 * 0.1 ** 2 + 0.04 * 0.1)
    assert want < 0.0 and abs(out["W"][1, 1] - want) <= 1e-14 * 1000.0 and out["W"][1, 0] == 0.0


def test_the_cap_takes_the_larger_margin_then_the_lower_segment():
    T = np.ones(15)
    m = np.full(15, -1.0)
    m[[3, 9]] = [0.5, 0.7]
    ts = np.cumsum(T) - 0.5
    args = (np.zeros(15, np.int64), np.zeros(15, np.int64), np.ones(15, np.int64), 1, 0.0, False)
    mask, fl = SR.plan_row(T, m, ts, *args)
    assert [i for i in range(15) if mask[i]] == [9] and fl == SR.DONE | SR.FULL
    m[3] = 0.7
    mask, fl = SR.plan_row(T, m, ts, *args)
    assert [i for i in range(15) if mask[i]] == [3] and fl == SR.DONE | SR.FULL
    mask, fl = SR.plan_row(np.ones(16), np.ones(16), np.cumsum(np.ones(16)) - 0.5, np.zeros(16, np.int64),
                           np.zeros(16, np.int64), np.ones(16, np.int64), 1, 0.0, False)
    assert not any(mask) and fl == SR.FULL
