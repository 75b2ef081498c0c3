"""CPU: the corridor inflation on the host backend (tgms_corridor_inflate_batch on a
tgms_create_host handle) against the brute-force NumPy reference of inflate_ref.py, to the bit;
then every argument error and B == 0 on the C interface."""
import ctypes

import numpy as np
import pytest

import inflate_ref as IR
from trajectory_generator_ros2_amd import _lib
from trajectory_generator_ros2_amd.solver import Solver, TgmsError


@pytest.fixture(scope="module")
def host():
    with Solver(host=True) as s:
        yield s


@pytest.mark.parametrize("max_grow", [0, 1, 8])
def test_random_scene_equals_the_reference(host, max_grow):
    IR.check_random(host, max_grow)


def test_random_scene_partly_outside_the_grid(host):
    IR.check_random(host, 8, shift=3.0)


def test_empty_map(host):
    IR.check_empty_map(host)


def test_closed_direction_stays_closed(host):
    IR.check_closed_direction_stays_closed(host)


def test_nan_node_is_not_free(host):
    IR.check_closed_direction_stays_closed(host, bad=np.nan)


def test_blocked_seed(host):
    IR.check_blocked(host)


def test_waypoints_on_nodes(host):
    IR.check_on_a_node(host)


def test_one_ulp_either_side_of_a_node(host):
    IR.check_one_ulp(host)


def test_row_lengths_1_and_16(host):
    IR.check_row_lengths(host)


def test_nan_waypoint_spoils_its_two_segments_only(host):
    IR.check_nan_waypoint(host)


def test_far_waypoints(host):
    IR.check_far_waypoints(host)


def test_arguments(host):
    IR.check_arguments(host, TgmsError, _lib.ERR_INVALID_ARG)
    L, h = _lib.load(), host._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    so, W = IR.one_leg()
    v = IR.g_values()
    f = ctypes.byref(_lib.Field(IR.G_ORIGIN, IR.G_H, IR.G_N))
    box, faces = np.full((1, 6), -2, np.int32), np.zeros((6, 4))
    fo, seg_flags, flags = np.zeros(2, np.int64), np.full(1, -2, np.int32), np.full(1, -2, np.int32)
    call = L.tgms_corridor_inflate_batch
    inv = _lib.ERR_INVALID_ARG
    # NULL inputs, every output NULL
    assert call(h, 1, None, p(W), f, p(v), 0.3, 4, p(box), None, None, None, None) == inv
    assert call(h, 1, p(so), None, f, p(v), 0.3, 4, p(box), None, None, None, None) == inv
    assert call(h, 1, p(so), p(W), None, p(v), 0.3, 4, p(box), None, None, None, None) == inv
    assert call(h, 1, p(so), p(W), f, None, 0.3, 4, p(box), None, None, None, None) == inv
    assert call(h, 1, p(so), p(W), f, p(v), 0.3, 4, None, None, None, None, None) == inv
    assert call(h, -1, p(so), p(W), f, p(v), 0.3, 4, p(box), None, None, None, None) == inv
    # a table of more than 2^31 - 1 entries: refused before a value is read (1290^3 nodes fit, 1291^3 entries do not)
    big = ctypes.byref(_lib.Field(IR.G_ORIGIN, IR.G_H, (1290, 1290, 1290)))
    assert call(h, 1, p(so), p(W), big, p(v), 0.3, 4, p(box), None, None, None, None) == inv
    # each output alone is enough
    want = IR.reference(so, W, IR.G_ORIGIN, IR.G_H, v, 0.3, 4)
    outs = [box, faces, fo, seg_flags, flags]
    for i, o in enumerate(outs):
        a = [None] * 5
        a[i] = p(o)
        assert call(h, 1, p(so), p(W), f, p(v), 0.3, 4, *a) == _lib.OK
        assert IR.same_bits(o.reshape(want[i].shape), want[i]), (i, o)
    # B == 0: nothing is touched
    flags[:] = -2
    assert call(h, 0, p(so[:1]), None, f, p(v), 0.3, 4, None, None, None, None, p(flags)) == _lib.OK
    assert list(flags) == [-2]
    # the device entry points have no host path
    tab = np.zeros((8, 9, 10), np.int32)
    assert L.tgms_field_occupancy_device(h, f, p(v), 0.3, p(tab), None) == _lib.ERR_UNSUPPORTED
    assert L.tgms_corridor_inflate_batch_device(h, 1, p(so), p(W), f, p(tab), 4, p(box), None, None, None, None,
                                                None) == _lib.ERR_UNSUPPORTED


def test_solver_returns_what_the_corridor_loop_takes(host):
    """The faces and offsets go into Solver.corridor unchanged: a straight rest-to-rest leg inside
    its own inflated box has a margin <= 0 on every face."""
    so, W = IR.one_leg()
    _, faces, fo, _, flags = host.corridor_inflate(so, W, IR.G_ORIGIN, IR.G_H, IR.g_values(), 0.3, 1)
    T = np.array([2.0])
    C, _, worst = host.solve(so, W, T)
    assert worst == _lib.OK and list(flags) == [_lib.INF_CAPPED]
    rec, _, _, _, cfl = host.corridor(so, T, C, faces, fo, 0.0)
    assert rec[0, 0] <= 0.0 and not (cfl & _lib.COR_OUTSIDE).any()
