"""CPU: the waypoint repair on the host backend (tgms_field_nearest_free and
tgms_waypoints_repair_batch on a tgms_create_host handle, csrc/tgms_repair_core.h) against the
brute-force reference of repair_ref.py, to the bit: constructed maps with hand-computed sites, the
reach's edge, NaN nodes, random maps, grids at the seams of the kernels' tiles, and every outcome of
a waypoint.  test_gpu_repair.py runs the same cases on the device."""
import numpy as np
import pytest

import repair_ref as RP
from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, RPR_KEEP_FIRST, RPR_KEEP_LAST, TgmsError


@pytest.fixture(scope="module")
def be():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


def test_all_free_is_the_identity(be):
    RP.check_all_free(be)


def test_all_blocked_has_no_site(be):
    RP.check_all_blocked(be)


def test_one_blocked_node_takes_the_lowest_index(be):
    RP.check_one_blocked_node(be)


def test_one_free_node(be):
    RP.check_one_free_node(be)


def test_plane_line_and_corner(be):
    RP.check_plane_line_corner(be)


def test_reach_is_inclusive(be):
    RP.check_reach(be)


def test_nan_nodes_and_the_threshold(be):
    RP.check_nan_and_threshold(be)


@pytest.mark.parametrize("fill,max_shift", [(0.1, 2), (0.5, 3), (0.9, 5), (0.98, 40), (0.999, 7)])
def test_random_maps(be, fill, max_shift):
    RP.check_random(be, fill, max_shift)


@pytest.mark.parametrize("n", RP.seam_grids(), ids=lambda n: "x".join(map(str, n)))
def test_tile_seams(be, n):
    RP.check_seam(be, n, 4)
    RP.check_seam(be, n, 200)


def test_outcomes_by_hand(be):
    RP.check_outcomes(be)


def test_stuck_until_the_reach_grows(be):
    RP.check_stuck_and_reach(be)


def test_outside_and_nonfinite_are_copied(be):
    RP.check_outside_and_nonfinite(be)


def test_modes_protect_the_ends(be):
    RP.check_modes(be)


def test_two_neighbours_on_one_node(be):
    RP.check_zero_length_leg(be)


def test_times_follow_the_lengths(be):
    RP.check_times(be)


@pytest.mark.parametrize("fill,max_shift,mode", [(0.2, 2, 0), (0.5, 3, RPR_KEEP_FIRST), (0.8, 6, RPR_KEEP_LAST),
                                                  (0.95, 2, RPR_KEEP_FIRST | RPR_KEEP_LAST)])
def test_random_batches(be, fill, max_shift, mode):
    RP.check_random_batch(be, fill, max_shift, mode)


def test_no_ends_after_a_full_repair(be):
    """Guarantee 2 on a dyadic lattice: a leg whose two waypoints are clear or MOVED is never
    RRT_ENDS in the re-route with the same map and r_free; and the batch before the repair has some."""
    from trajectory_generator_ros2_amd import RPR_MOVED, RRT_ENDS
    v = RP.random_map(RP.RANDOM_N, 0.3, 21)
    so, W, T = RP.dyadic_batch(60, 8, RP.RANDOM_N)
    before = be.corridor_reroute(so, W, RP.O, RP.H, v, RP.RF, 3, 8, T)
    assert (before[4] & RRT_ENDS).any()
    W2, T2, wp, _, _ = be.waypoints_repair(so, W, RP.O, RP.H, v, RP.RF, 4, 0, T)
    after = be.corridor_reroute(so, W2, RP.O, RP.H, v, RP.RF, 3, 8, T2)
    good = (wp == 0) | (wp == RPR_MOVED)
    rows = np.arange(int(so[-1])) + np.repeat(np.arange(len(so) - 1), np.diff(so))
    leg_ok = good[rows] & good[rows + 1]
    ends = np.bincount(after[3], weights=(after[4] & RRT_ENDS) != 0, minlength=int(so[-1])) > 0
    assert leg_ok.any() and not (ends & leg_ok).any()


def test_arguments(be):
    RP.check_arguments(be, TgmsError, ERR_INVALID_ARG)


def test_device_calls_need_a_gpu_handle(be):
    z = np.zeros(8, np.int32)
    with pytest.raises(TgmsError) as e:
        be.field_nearest_free_device(RP.O, RP.H, (2, 2, 2), np.ones(8, np.float32), RP.RF, 2, z, z)
    assert e.value.status == ERR_UNSUPPORTED and "tgms_field_nearest_free_dev" in str(e.value)
    with pytest.raises(TgmsError) as e:
        be.waypoints_repair_device(1, z, np.zeros((2, 3)), RP.O, RP.H, (2, 2, 2), z, 0, np.zeros((2, 3)))
    assert e.value.status == ERR_UNSUPPORTED and "tgms_waypoints_repair_batch_dev" in str(e.value)
