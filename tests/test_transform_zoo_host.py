"""CPU: the three transforming calls of the host backend (tgms_dilate_batch, tgms_cut_batch,
tgms_corridor_split_batch on a tgms_create_host handle) on the constructed polynomials of
poly_zoo.py: the checks of transform_zoo.py, which test_gpu_transform_zoo.py repeats on the
device.  The references a case uses are first held against the long-double grid
(test_references_agree_with_the_grid), to poly_zoo.CAP in the contract's own unit."""
import os

import pytest

import poly_zoo as Z
import split_ref as SR
import transform_zoo as X


@pytest.fixture(scope="module")
def be():
    from trajectory_generator_ros2_amd.build import LIB_TGMS, build_tgms
    from trajectory_generator_ros2_amd.solver import Solver
    if not os.path.exists(LIB_TGMS):
        build_tgms()
    s = Solver(host=True)
    yield X.Host(s)
    s.close()


def test_references_agree_with_the_grid(be):
    """dilate_ref's records of the dilated zoo against the 65,537-point grid, and the contract once
    more from the grid's own records; cut_ref's Fraction states against long-double Horner."""
    X.check_dilate_contract(be, "host", grid=True)
    X.check_cut_reference_against_longdouble()


# ---- A. dilate ----

def test_dilate_peak_on_a_knot(be):
    X.check_dilate_knot_peak(be, "host")


def test_dilate_deficient_rows(be):
    X.check_dilate_deficient(be, "host")


def test_dilate_ballistic_arc_under_f_min(be):
    X.check_dilate_ballistic(be, "host")


def test_dilate_tilt_limit_at_free_fall(be):
    X.check_free_fall_tilt(be, "host")


@pytest.mark.parametrize("s_lo", [0.625, 0.875])
def test_dilate_contract_on_the_zoo(be, s_lo):
    X.check_dilate_contract(be, "host", s_lo=s_lo)


def test_dilate_translation(be):
    X.check_dilate_translation(be)


@pytest.mark.parametrize("k", Z.RESCALES)
def test_dilate_time_rescale(be, k):
    X.check_dilate_rescale(be, k)


def test_dilate_idempotence(be):
    X.check_dilate_idempotence(be, "host")


def test_dilate_then_bounds_and_thrust(be):
    X.check_dilate_round_trip(be, "host")


# ---- B. cut ----

def test_cut_zoo_against_the_reference(be):
    X.check_cut_against_ref(be, "host")


def test_cut_on_the_knot_that_is_the_extremum(be):
    X.check_cut_knot_peak(be)


def test_cut_deficient_pieces(be):
    X.check_cut_deficient(be)


def test_cut_composition(be):
    X.check_cut_composition(be, "host")


def test_cut_translation(be):
    X.check_cut_translation(be)


@pytest.mark.parametrize("k", Z.RESCALES)
def test_cut_time_rescale(be, k):
    X.check_cut_rescale(be, k)


def test_cut_then_the_analysis_calls(be):
    X.check_cut_round_trips(be, "host")


# ---- C. split ----

@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_split_cheb_in_a_corridor(be, mode):
    X.check_split_cheb(be, "host", mode)


def test_split_excursion_on_an_interior_knot(be):
    X.check_split_knot_peak(be, "host")


@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_split_deficient_row(be, mode):
    X.check_split_deficient(be, "host", mode)


@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_split_then_solve_then_corridor(be, mode):
    X.check_split_round_trip(be, "host", mode)
