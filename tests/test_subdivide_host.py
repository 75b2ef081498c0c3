"""CPU: the corridor subdivision on the host backend (tgms_corridor_subdivide_batch on a
tgms_create_host handle) against the brute-force NumPy reference of subdivide_ref.py, to the bit;
the round trip through the inflation call, the certificate against the field reference, then every
argument error, B == 0 and the nullable outputs on the C interface."""
import ctypes

import numpy as np
import pytest

import subdivide_ref as SR
from trajectory_generator_ros2_amd import _lib
from trajectory_generator_ros2_amd.solver import Solver, TgmsError


@pytest.fixture(scope="module")
def host():
    with Solver(host=True) as s:
        yield s


def test_empty_map_returns_the_input(host):
    SR.check_empty_map(host)


def test_hand_checked_leg(host):
    SR.check_hand(host)


def test_nodes_on_the_chord_stay_blocked(host):
    SR.check_on_chord(host)


def test_budget_takes_the_largest_fitting_depth(host):
    SR.check_budget(host)


def test_bad_legs_are_isolated(host):
    SR.check_isolation(host)


def test_times_are_exact_fractions(host):
    SR.check_times(host)


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4])
def test_random_scene_equals_the_reference(host, depth):
    SR.check_random(host, depth)


def test_random_scene_partly_outside_the_grid(host):
    SR.check_random(host, 4, shift=3.0)


def test_round_trip_through_the_inflation(host):
    SR.check_round_trip(host)


def test_unflagged_segments_are_certified_free(host):
    SR.check_certificate(host)


def test_corridor_from_map_is_subdivide_then_inflate(host):
    so, W, T, v = SR.room()
    (so2, W2, T2, faces, fo), (sub_fl, sub_seg, inf_seg, inf_fl) = host.corridor_from_map(
        so, W, T, SR.R_ORIGIN, SR.R_H, v, SR.R_FREE, 2)
    SR.assert_same((so2, W2, T2, None, sub_seg, sub_fl), SR.room_reference()[:3] + (None,) + SR.room_reference()[4:])
    want = host.corridor_inflate(so2, W2, SR.R_ORIGIN, SR.R_H, v, SR.R_FREE, 2)
    assert SR.same_bits(faces, want[1]) and np.array_equal(fo, want[2]) and np.array_equal(inf_seg, want[3])
    assert np.array_equal(inf_fl, want[4]) and len(T2) == so2[-1] == len(fo) - 1


def test_arguments(host):
    SR.check_arguments(host, TgmsError, _lib.ERR_INVALID_ARG)
    L, h = _lib.load(), host._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    so, W, T = SR.path([(0.5, 0.5, 0.5), (8.5, 8.5, 0.5)])
    v = SR.g_values([(8, 1, 0)])
    f = ctypes.byref(_lib.Field(SR.G_ORIGIN, SR.G_H, SR.G_N))
    want = SR.reference(so, W, T, SR.G_ORIGIN, SR.G_H, v, 0.3, 4)
    cap = 16

    def outs():
        return [np.full(2, -2, np.int32), np.full((cap + 1, 3), -2.0), np.full(cap, -2.0), np.full(cap, -2, np.int32),
                np.full(cap, -2, np.int32), np.full(1, -2, np.int64), np.full(1, -2, np.int32)]

    call = L.tgms_corridor_subdivide_batch
    inv = _lib.ERR_INVALID_ARG
    o = outs()
    args = lambda o: [p(x) if x is not None else None for x in o]  # noqa: E731
    assert call(h, 1, p(so), p(W), p(T), f, p(v), 0.3, 4, *args(o)) == _lib.OK
    # NULL inputs, a required output NULL, one of the two time arrays alone
    assert call(h, 1, None, p(W), p(T), f, p(v), 0.3, 4, *args(o)) == inv
    assert call(h, 1, p(so), None, p(T), f, p(v), 0.3, 4, *args(o)) == inv
    assert call(h, 1, p(so), p(W), p(T), None, p(v), 0.3, 4, *args(o)) == inv
    assert call(h, 1, p(so), p(W), p(T), f, None, 0.3, 4, *args(o)) == inv
    assert call(h, -1, p(so), p(W), p(T), f, p(v), 0.3, 4, *args(o)) == inv
    assert call(h, 1, p(so), p(W), None, f, p(v), 0.3, 4, *args(o)) == inv
    for i in (0, 1, 2, 5):
        a = args(o)
        a[i] = None
        assert call(h, 1, p(so), p(W), p(T), f, p(v), 0.3, 4, *a) == inv, i
    big = ctypes.byref(_lib.Field(SR.G_ORIGIN, SR.G_H, (1290, 1290, 1290)))
    assert call(h, 1, p(so), p(W), p(T), big, p(v), 0.3, 4, *args(o)) == inv
    # every nullable output omitted in turn (the times as a pair): the others are unchanged
    for i in (2, 3, 4, 6):
        o = outs()
        a = args(o)
        a[i] = None
        assert call(h, 1, p(so), p(W), None if i == 2 else p(T), f, p(v), 0.3, 4, *a) == _lib.OK
        assert o[5][0] == 2 and (o[i] == -2).all()
        got = [o[0], o[1][:3], o[2][:2], o[3][:2], o[4][:2], o[6]]
        for j, (g, w) in enumerate(zip(got, want)):
            if j != (i if i < 5 else 5):
                assert SR.same_bits(g, w), (i, j)
        assert (o[1][3:] == -2.0).all() and (o[3][2:] == -2).all()  # nothing past S'
    # B == 0: the first offset and the total, nothing else
    o = outs()
    assert call(h, 0, p(so[:1]), None, None, f, p(v), 0.3, 4, p(o[0]), None, None, None, None, p(o[5]), p(o[6])) == _lib.OK
    assert list(o[0]) == [0, -2] and o[5][0] == 0 and o[6][0] == -2
    # the device entry point has no host path
    tab = np.zeros((18, 18, 18), np.int32)
    assert L.tgms_corridor_subdivide_batch_device(h, 1, p(so), p(W), p(T), f, p(tab), 4, *args(outs()),
                                                  None) == _lib.ERR_UNSUPPORTED
