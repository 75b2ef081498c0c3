"""CPU: the corridor re-route on the host backend (tgms_corridor_reroute_batch on a tgms_create_host
handle) against the brute-force reference of reroute_ref.py, to the bit: the hand-checked wall, the
closed wall, the margin, the window cap, the end nodes, the degenerate leg, the tie order, the long
serpentine, the budget, isolation, times, the random mazes with the round trip through the
inflation; corridor_from_map with the re-route between its two steps; then every argument error,
B == 0 and the nullable outputs on the C interface."""
import ctypes

import numpy as np
import pytest

import reroute_ref as RR
from trajectory_generator_ros2_amd import _lib
from trajectory_generator_ros2_amd.solver import Solver, TgmsError


@pytest.fixture(scope="module")
def host():
    with Solver(host=True) as s:
        yield s


def test_wall_with_a_gap_by_hand(host):
    RR.check_wall_with_gap(host)


def test_closed_wall_has_no_path(host):
    RR.check_closed_wall(host)


def test_margin_one_short_of_the_gap(host):
    RR.check_small_margin(host)


def test_window_cap(host):
    RR.check_window_cap(host)


def test_end_node_not_free(host):
    RR.check_ends(host)


def test_degenerate_leg_is_copied(host):
    RR.check_degenerate(host)


def test_tie_order(host):
    RR.check_tie_order(host)


def test_long_path_needs_sixteen_bits(host):
    RR.check_long_path(host)


def test_budget_is_all_or_nothing(host):
    RR.check_budget(host)


def test_bad_legs_are_isolated(host):
    RR.check_isolation(host)


def test_times_follow_the_lengths(host):
    RR.check_times(host)


@pytest.mark.parametrize("margin,max_pieces", [(1, 8), (3, 4), (6, 8)])
def test_random_mazes_equal_the_reference(host, margin, max_pieces):
    RR.check_maze(host, margin, max_pieces)


def test_corridor_from_map_with_reroute(host):
    so, W, T, v = RR.maze()
    plain = host.corridor_from_map(so, W, T, RR.O, RR.H, v, RR.RF, 2, 0)
    assert len(plain) == 2 and len(plain[1]) == 4  # the default: today's shape
    (so2, W2, T2, faces, fo), (sub_fl, sub_seg, inf_seg, inf_fl, rrt_fl, rrt_seg, rrt_par, rrt_hops) = \
        host.corridor_from_map(so, W, T, RR.O, RR.H, v, RR.RF, 2, 0, reroute=(3, 4))
    RR.assert_same((so2, W2, T2, rrt_par, rrt_seg, rrt_hops, rrt_fl), RR.maze_reference(3, 4))  # depth 0: the input
    want = host.corridor_inflate(so2, W2, RR.O, RR.H, v, RR.RF, 2)
    assert RR.same_bits(faces, want[1]) and np.array_equal(inf_seg, want[3]) and len(T2) == so2[-1] == len(fo) - 1
    assert np.array_equal((inf_seg & _lib.INF_BLOCKED) != 0, (rrt_seg & _lib.RRT_BLOCKED) != 0)
    assert np.array_equal(sub_seg, plain[1][1]) and np.array_equal(sub_fl, plain[1][0])


def test_arguments(host):
    RR.check_arguments(host, TgmsError, _lib.ERR_INVALID_ARG)
    L, h = _lib.load(), host._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    so, W, T = RR.path([(2, 4, 1), (6, 4, 1)])
    v = RR.grid((16, 16, 4), [(4, 4, 1)])
    f = ctypes.byref(_lib.Field(RR.O, RR.H, (16, 16, 4)))
    want = RR.reference(so, W, T, RR.O, RR.H, v, RR.RF, 4, 8)
    cap = 8

    def outs():
        return [np.full(2, -2, np.int32), np.full((cap + 1, 3), -2.0), np.full(cap, -2.0), np.full(cap, -2, np.int32),
                np.full(cap, -2, np.int32), np.full(1, -2, np.int32), np.full(1, -2, np.int64), np.full(1, -2, np.int32)]

    call = L.tgms_corridor_reroute_batch
    inv = _lib.ERR_INVALID_ARG
    o = outs()
    args = lambda o: [p(x) if x is not None else None for x in o]  # noqa: E731
    assert call(h, 1, p(so), p(W), p(T), f, p(v), 0.3, 4, 8, *args(o)) == _lib.OK
    # NULL inputs, a required output NULL, one of the two time arrays alone
    assert call(h, 1, None, p(W), p(T), f, p(v), 0.3, 4, 8, *args(o)) == inv
    assert call(h, 1, p(so), None, p(T), f, p(v), 0.3, 4, 8, *args(o)) == inv
    assert call(h, 1, p(so), p(W), p(T), None, p(v), 0.3, 4, 8, *args(o)) == inv
    assert call(h, 1, p(so), p(W), p(T), f, None, 0.3, 4, 8, *args(o)) == inv
    assert call(h, -1, p(so), p(W), p(T), f, p(v), 0.3, 4, 8, *args(o)) == inv
    assert call(h, 1, p(so), p(W), None, f, p(v), 0.3, 4, 8, *args(o)) == inv
    assert b"NULL together" in L.tgms_last_error(h)
    for i in (0, 1, 2, 6):
        a = args(o)
        a[i] = None
        assert call(h, 1, p(so), p(W), p(T), f, p(v), 0.3, 4, 8, *a) == inv, i
    big = ctypes.byref(_lib.Field(RR.O, RR.H, (1290, 1290, 1290)))
    assert call(h, 1, p(so), p(W), p(T), big, p(v), 0.3, 4, 8, *args(o)) == inv
    # every nullable output omitted in turn (the times as a pair): the others are unchanged
    for i in (2, 3, 4, 5, 7):
        o = outs()
        a = args(o)
        a[i] = None
        assert call(h, 1, p(so), p(W), None if i == 2 else p(T), f, p(v), 0.3, 4, 8, *a) == _lib.OK
        assert o[6][0] == 3 and (o[i] == -2).all()
        got = [o[0], o[1][:4], o[2][:3], o[3][:3], o[4][:3], o[5], o[7]]
        for j, (g, w) in enumerate(zip(got, want)):
            if j != (i if i < 6 else 6):
                assert RR.same_bits(g, w), (i, j)
        assert (o[1][4:] == -2.0).all() and (o[3][3:] == -2).all()  # nothing past S'
    # B == 0: the first offset and the total, nothing else
    o = outs()
    assert call(h, 0, p(so[:1]), None, None, f, p(v), 0.3, 4, 8, p(o[0]), None, None, None, None, None, p(o[6]),
                p(o[7])) == _lib.OK
    assert list(o[0]) == [0, -2] and o[6][0] == 0 and o[7][0] == -2
    # the device entry point has no host path
    tab = np.zeros((5, 17, 17), np.int32)
    assert L.tgms_corridor_reroute_batch_dev(h, 1, p(so), p(W), p(T), f, p(tab), 4, 8, *args(outs()),
                                             None) == _lib.ERR_UNSUPPORTED
    assert b"tgms_corridor_reroute_batch_dev" in L.tgms_last_error(h)
