"""CPU: the swarm neighbour search on the host backend (tgms_neighbors_batch on a
tgms_create_host handle), against the separation call over all ordered pairs reduced in NumPy
(neighbors_ref.py).  The `tested` assertions of the crossing and the lattice fail for an
implementation that does not cull."""
import ctypes

import numpy as np
import pytest

import neighbors_ref as NR
from trajectory_generator_ros2_amd import _lib
from trajectory_generator_ros2_amd.solver import Solver, TgmsError


@pytest.fixture(scope="module")
def host():
    with Solver(host=True) as s:
        yield s


@pytest.fixture(scope="module")
def ref_sep(host):
    """The reference d_min t_min of all 2,256 ordered pairs of a contract batch, once per module."""
    cache = {}

    def get(name, scale_name):
        if (name, scale_name) not in cache:
            so, T, C, t0, _ = NR.contract_inputs(name)
            sep, fl = host.separation(so, T, C, pairs=NR.ordered_pairs(len(so) - 1), start_times=t0,
                                      scale=NR.SCALES[scale_name])
            assert not fl.any()
            sep.setflags(write=False)
            cache[name, scale_name] = sep
        return cache[name, scale_name]
    return get


def test_crossing_and_bystander(host):
    NR.check_crossing(host)


def test_strictness_and_margin_direction(host):
    NR.check_strict(host)


@pytest.mark.parametrize("B", NR.LATTICE_B)
def test_lattice(host, B):
    NR.check_lattice(host, B)


def test_start_times_and_held_ends(host):
    NR.check_held(host)


@pytest.mark.parametrize("scale_name", sorted(NR.SCALES))
@pytest.mark.parametrize("name", ["rest", "end_derivs"])
def test_contract(host, ref_sep, name, scale_name):
    NR.check_contract(host, ref_sep, host.bounds, name, scale_name, "host")


def test_unusable_vehicles(host):
    NR.check_unusable(host)


def test_arguments(host):
    so, T, C = NR.crossing3()
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(TgmsError) as e:
            host.neighbors(so, T, C, r)
        assert e.value.status == _lib.ERR_INVALID_ARG
    for sc in ((1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        with pytest.raises(TgmsError) as e:
            host.neighbors(so, T, C, 1.0, scale=sc)
        assert e.value.status == _lib.ERR_INVALID_ARG
    L, h = _lib.load(), host._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tested = np.zeros(3, dtype=np.int32)
    assert L.tgms_neighbors_batch(h, 3, p(so), p(T), p(C), None, None, 1.0, None, None, None, p(tested),
                                  None) == _lib.ERR_INVALID_ARG
    assert L.tgms_neighbors_batch(h, 0, p(so[:1]), None, None, None, None, 1.0, None, None, p(tested), None,
                                  None) == _lib.OK
    # one output alone is enough
    count = np.full(3, -2, dtype=np.int32)
    assert L.tgms_neighbors_batch(h, 3, p(so), p(T), p(C), None, None, 1.0, None, None, p(count), None, None) == _lib.OK
    assert list(count) == [1, 1, 0]
    # the device entry point has no host path
    assert L.tgms_neighbors_batch_device(h, 3, p(so), p(T), p(C), None, None, 1.0, None, None, p(count), None, None,
                                         None) == _lib.ERR_UNSUPPORTED
