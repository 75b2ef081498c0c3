"""CPU: the corridor reference (corridor_ref.py) against closed forms, before anything is held
to it: the rest-to-rest segment against faces across and behind its motion, a parabola against
the face it rises from, and a slanted face against the projection done by hand."""
import numpy as np
import pytest

import bounds_ref as R
import corridor_ref as CR

P0 = np.zeros(3)


def parabola(k, T):
    """M = 1: p_y = k t (T - t), x and z constant."""
    C = np.zeros((1, 3, 8))
    C[0, 0, 0], C[0, 2, 0] = 0.3, 2.0
    C[0, 1, 1], C[0, 1, 2] = k * T, -k
    return np.array([0, 1], np.int32), np.array([T]), C


def test_rest_to_rest_against_faces_across_and_behind():
    L, T = 3.0, 2.0
    so, Ts, C, _ = R.rest_to_rest(P0, L, T, axis=0)
    m, u = CR.item(C[0], T, np.array([1.0, 0.0, 0.0, L / 2]))
    assert abs(m - L / 2) <= 1e-15 * L and u == 1.0
    m, u = CR.item(C[0], T, np.array([-1.0, 0.0, 0.0, 0.0]))
    assert m == 0.0 and u == 0.0
    ref = CR.records(so, Ts, C, [[1.0, 0.0, 0.0, L / 2], [-1.0, 0.0, 0.0, 0.0]])
    assert abs(ref["m"][0] - L / 2) <= 1e-15 * L and ref["face"][0] == 0 and ref["seg"][0] == 0
    assert abs(CR.evaluate(so, Ts, C, 0, T, [1.0, 0.0, 0.0, L / 2]) - L / 2) <= 1e-15 * L


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_parabola_peaks_in_the_middle(T):
    k = 0.7
    so, Ts, C = parabola(k, T)
    m, u = CR.item(C[0], T, np.array([0.0, 1.0, 0.0, 0.0]))
    assert abs(m - k * T * T / 4) <= 1e-15 * k * T * T and abs(u - 0.5) <= 1e-12
    assert abs(CR.evaluate(so, Ts, C, 0, T / 2, [0.0, 1.0, 0.0, 0.0]) - k * T * T / 4) <= 1e-15 * k * T * T


def test_slanted_face_against_the_projection_by_hand():
    """x = 0.3 + 0.5 t, y = k t (T - t): n = (3, 4, 0) / 5, d = 1 gives
    q(t) = 0.6 (0.3 + 0.5 t) + 0.8 k t (T - t) - 1, stationary at t* = T / 2 + 0.3 / (1.6 k)."""
    k, T = 0.7, 2.0
    so, Ts, C = parabola(k, T)
    C[0, 0, 1] = 0.5
    ts = T / 2 + 0.3 / (1.6 * k)
    assert 0.0 < ts < T
    want = 0.6 * (0.3 + 0.5 * ts) + 0.8 * k * ts * (T - ts) - 1.0
    m, u = CR.item(C[0], T, np.array([0.6, 0.8, 0.0, 1.0]))
    assert abs(m - want) <= 1e-15 * 3.0 and abs(u * T - ts) <= 1e-12


def test_ties_and_empty_spans():
    """A duplicated face reports the lower index, a segment without faces -inf / -1, and a
    trajectory takes its lowest segment among equal margins."""
    so, Ts, C = parabola(0.7, 1.0)
    so2 = np.array([0, 3], np.int32)
    C3, T3 = np.repeat(C, 3, axis=0), np.repeat(Ts, 3)
    f = np.array([[0.0, 1.0, 0.0, 0.0]] * 3)
    ref = CR.records(so2, T3, C3, f, np.array([0, 0, 2, 3]))
    assert list(ref["seg_face"]) == [-1, 0, 2] and np.isneginf(ref["seg_m"][0])
    assert ref["seg"][0] == 1 and ref["face"][0] == 0 and ref["m"][0] == ref["seg_m"][1] == ref["seg_m"][2]
    ref = CR.records(so2, T3, C3, f[:0], np.zeros(4, np.int64))
    assert np.isneginf(ref["m"][0]) and ref["seg"][0] == -1 and ref["face"][0] == -1
