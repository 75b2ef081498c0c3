"""CPU: the obstacle clearance on the host backend (tgms_clearance_batch on a tgms_create_host
handle), against the NumPy longdouble reference of clearance_ref.py.  The `tested` assertions of
the fly-by and the lattice fail for an implementation that does not cull."""
import ctypes

import numpy as np
import pytest

import clearance_ref as CR
from trajectory_generator_ros2_amd import _lib
from trajectory_generator_ros2_amd.solver import Solver, TgmsError


@pytest.fixture(scope="module")
def host():
    with Solver(host=True) as s:
        yield s


def test_flyby(host):
    CR.check_flyby(host)


def test_strictness_and_margin_direction(host):
    CR.check_strict(host)


@pytest.mark.parametrize("B,K", CR.LATTICE)
def test_chunk_edges_and_tie_rule(host, B, K):
    CR.check_lattice(host, B, K)


@pytest.mark.parametrize("scale_name", sorted(CR.SCALES))
@pytest.mark.parametrize("name", ["rest", "end_derivs"])
def test_contract(host, name, scale_name):
    CR.check_contract(host, name, scale_name, "host")


def test_unusable_inputs(host):
    CR.check_unusable(host)


def test_arguments(host):
    so, T, C = CR.flyby()
    ob = np.array([CR.EDGE])
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(TgmsError) as e:
            host.clearance(so, T, C, ob, r)
        assert e.value.status == _lib.ERR_INVALID_ARG
    for sc in ((1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        with pytest.raises(TgmsError) as e:
            host.clearance(so, T, C, ob, 1.0, scale=sc)
        assert e.value.status == _lib.ERR_INVALID_ARG
    L, h = _lib.load(), host._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tested = np.zeros(1, dtype=np.int32)
    count = np.full(1, -2, dtype=np.int32)
    # tested alone is no output
    assert L.tgms_clearance_batch(h, 1, p(so), p(T), p(C), 1, p(ob), None, 1.0, None, None, None, p(tested),
                                  None) == _lib.ERR_INVALID_ARG
    # obstacles may be NULL only when K == 0
    assert L.tgms_clearance_batch(h, 1, p(so), p(T), p(C), 1, None, None, 1.0, None, None, p(count), None,
                                  None) == _lib.ERR_INVALID_ARG
    assert L.tgms_clearance_batch(h, 0, p(so[:1]), None, None, 0, None, None, 1.0, None, None, p(count), None,
                                  None) == _lib.OK
    # one output alone is enough
    assert L.tgms_clearance_batch(h, 1, p(so), p(T), p(C), 1, p(ob), None, 1.0, None, None, p(count), None,
                                  None) == _lib.OK
    assert list(count) == [1]
    # K == 0: the "none" row
    out = host.clearance(so, T, C, np.zeros((0, 6)), 1.0)
    CR.none_rows(out, [0])
    assert out[3][0] == 0
    # the device entry point has no host path
    assert L.tgms_clearance_batch_device(h, 1, p(so), p(T), p(C), 1, p(ob), None, 1.0, None, None, p(count), None, None,
                                         None) == _lib.ERR_UNSUPPORTED
