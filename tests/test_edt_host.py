"""CPU: the distance-field build on the host backend (tgms_field_edt on a tgms_create_host handle,
csrc/tgms_edt_core.h) against the brute-force reference of edt_ref.py, bit for bit, on the whole
matrix of shapes, maps, caps, modes and spacings; then the arguments, the agreement with
synthetic.box_field on a lattice-aligned scene, the signed field's axis differences, and the
inflation of a field the call built."""
import ctypes

import numpy as np
import pytest

import edt_ref as ER
import inflate_ref as IR
from trajectory_generator_ros2_amd import EDT_NONE, EDT_SIGNED, ERR_INVALID_ARG, ERR_UNSUPPORTED, OK, TgmsError, _lib
from trajectory_generator_ros2_amd import synthetic as S


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


@pytest.mark.parametrize("case", ER.CASES, ids=ER.case_id)
def test_matrix_equals_the_reference(host, case):
    ER.check_case(host, *case)


def test_empty_and_full_maps_by_hand(host):
    """Empty: every value max_dist and d2 = R^2 in both modes.  Full: 0 and 0 unsigned; -max_dist and
    -R^2 signed."""
    n, h, md = (9, 7, 5), 0.094, 0.3  # R = ceil(3.19...) = 4
    assert ER.cap(h, md) == 4
    for signed in (False, True):
        v, d2 = host.field_edt(ER.make_map(n, "empty"), ER.ORIGIN, h, md, signed)
        assert (v == np.float32(md)).all() and (d2 == 16).all()
    v, d2 = host.field_edt(ER.make_map(n, "full"), ER.ORIGIN, h, md)
    assert (v == 0).all() and not np.signbit(v).any() and (d2 == 0).all()
    v, d2 = host.field_edt(ER.make_map(n, "full"), ER.ORIGIN, h, md, True)
    assert (v == -np.float32(md)).all() and (d2 == -16).all()


def test_cap_is_corrected_and_clipped(host):
    """R from a quotient that rounds down to an integer, and from one far beyond 32,768."""
    occ = ER.make_map((9, 7, 5), "corner0")
    for h, md in ((0.1, 0.3), (0.094, 0.094 * 3), (1e-3, 1e9), (0.125, 1e300)):
        got = host.field_edt(occ, ER.ORIGIN, h, md)
        ER.assert_same(got, ER.reference(occ, h, md, False), (h, md))
    # signed, max_dist just below R spacings: nodes between R and R + 1/2 spacings away keep a value
    # below max_dist although their square is reported as R^2
    n, name = (40, 33, 9), "random_0.001"
    for h in ER.H_VALUES:
        got = host.field_edt(ER.make_map(n, name), ER.ORIGIN, h, 3.9 * h, True)
        want = ER.convert(*ER.squares(n, name), ER.make_map(n, name), h, 3.9 * h, True)
        ER.assert_same(got, want, h)
        assert ((want[1] == 16) & (want[0] < np.float32(3.9 * h))).any()
    assert ER.cap(1e-3, 1e9) == 32768
    _, d2 = host.field_edt(ER.make_map((9, 7, 5), "empty"), ER.ORIGIN, 1e-3, 1e9)
    assert (d2 == 32768 ** 2).all() and 32768 ** 2 < EDT_NONE


def test_arguments(host):
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    occ = np.zeros((5, 7, 9), np.uint8)
    v, d2 = np.zeros(occ.shape, np.float32), np.zeros(occ.shape, np.int32)
    good = dict(origin=ER.ORIGIN, h=0.125, n=(9, 7, 5))

    def call(field=None, o=occ, md=1.0, mode=0, vals=v, sq=d2, **kw):
        f = ctypes.byref(_lib.Field(**{**good, **kw})) if field is None else field
        return L.tgms_field_edt(host._h, f, None if o is None else p(o), md, mode, None if vals is None else p(vals),
                                None if sq is None else p(sq))

    assert call() == OK
    assert call(vals=None) == OK and call(sq=None) == OK and call(mode=EDT_SIGNED) == OK
    bad_fields = [dict(n=(1, 7, 5)), dict(n=(9, 1, 5)), dict(n=(9, 7, 1)), dict(n=(16385, 2, 2)), dict(n=(2, 16385, 2)),
                  dict(n=(2, 2, 16385)), dict(n=(16384, 16384, 8)), dict(h=0.0), dict(h=-0.125), dict(h=float("inf")),
                  dict(h=float("nan")), dict(origin=(float("nan"), 0.0, 0.0)), dict(origin=(0.0, float("inf"), 0.0)),
                  dict(origin=(0.0, 0.0, -float("inf")))]
    for kw in bad_fields:
        assert call(**kw) == ERR_INVALID_ARG, kw
        fld = _lib.Field(**{**good, **kw})
        assert L.tgms_field_edt_work_size(ctypes.byref(fld), 0) == 0, kw
    for md in (0.0, -1.0, float("inf"), float("nan")):
        assert call(md=md) == ERR_INVALID_ARG, md
    for mode in (2, 3, -1, 1 << 30):
        assert call(mode=mode) == ERR_INVALID_ARG, mode
        assert L.tgms_field_edt_work_size(ctypes.byref(_lib.Field(**good)), mode) == 0
    assert call(field=ctypes.POINTER(_lib.Field)()) == ERR_INVALID_ARG
    assert call(o=None) == ERR_INVALID_ARG
    assert call(vals=None, sq=None) == ERR_INVALID_ARG
    assert host.last_error() != ""
    assert L.tgms_field_edt_work_size(ctypes.POINTER(_lib.Field)(), 0) == 0
    # two int32 per node, in either mode; the largest grid the call takes has a size
    assert host.field_edt_work_size(**good) == host.field_edt_work_size(**good, signed=True) == 8 * 9 * 7 * 5
    assert host.field_edt_work_size(ER.ORIGIN, 0.125, (16384, 16384, 7)) == 8 * 16384 * 16384 * 7
    # the device call needs a GPU handle
    with pytest.raises(TgmsError) as e:
        host.field_edt_device(ER.ORIGIN, 0.125, (9, 7, 5), occ, 1.0, np.zeros(2 * occ.size, np.int32), d_values=v)
    assert e.value.status == ERR_UNSUPPORTED


def test_unsigned_values_equal_box_field_on_a_lattice_aligned_scene(host):
    """h = 2^-3, the origin on multiples of it and box faces on nodes: the nearest point of a box is
    a node, every coordinate difference is h times an integer exactly, and scaling by h^2, a power
    of four, passes through the square root exactly.  So the transform of box_occupancy is
    box_field of the same boxes bit for bit."""
    occ, want = ER.aligned()
    assert 0 < occ.sum() < occ.size
    v, d2 = host.field_edt(occ, ER.A_ORIGIN, ER.A_H, ER.A_FAR)
    assert ER.same_bits(v, want)
    assert np.array_equal(np.float32(ER.A_H) * np.sqrt(d2.astype(np.float64)).astype(np.float32), want)
    assert np.array_equal(occ != 0, want == 0)


def test_signed_field_is_1_lipschitz_along_the_axes_and_never_zero(host):
    """Every axis edge difference is at most h, up to the one fp32 rounding of each value; d2 is
    never 0 and its sign is the value's."""
    for n, name in (((40, 33, 9), "random_0.05"), ((40, 33, 9), "random_0.5"), ((9, 7, 5), "checker"),
                    ((40, 33, 9), "plane_y")):
        for h in ER.H_VALUES:
            for md in ER.max_dists(n, h) + (3.2 * h,):
                v, d2 = host.field_edt(ER.make_map(n, name), ER.ORIGIN, h, md, True)
                assert (d2 != 0).all() and np.array_equal(d2 < 0, ER.make_map(n, name) != 0)
                assert np.array_equal(np.signbit(v), d2 < 0) and (v != 0).all()
                top = np.abs(v).max()  # half an fp32 ulp per value, and its three fp64 roundings
                tol = float(np.spacing(np.float32(top))) + 8.0 * float(np.spacing(np.float64(top)))
                for a in range(3):
                    assert np.abs(np.diff(v.astype(np.float64), axis=a)).max() <= h + tol, (n, name, h, md, a)


def test_inflation_of_a_built_field_equals_that_of_box_field(host):
    """The corridor inflation's reference gives the same boxes at r_free = 0.3 for the values the
    call built (capped at 1 m, so they differ from box_field's far from the boxes) as for
    box_field's own."""
    occ, exact = ER.aligned()
    v, _ = host.field_edt(occ, ER.A_ORIGIN, ER.A_H, 1.0)
    assert not ER.same_bits(v, exact) and (v <= 1.0).all()
    rng = np.random.default_rng(S.SEED + 11)
    so = np.array([0, 5, 8, 16], dtype=np.int32)
    lo = np.array(ER.A_ORIGIN)
    W = lo + rng.uniform(0.02, 0.98, size=(int(so[-1]) + len(so) - 1, 3)) * ER.A_H * (np.array(ER.A_N) - 1)
    got = IR.reference(so, W, ER.A_ORIGIN, ER.A_H, v, 0.3, 8)
    want = IR.reference(so, W, ER.A_ORIGIN, ER.A_H, exact, 0.3, 8)
    IR.assert_same(got, want)
    assert (got[3] & IR.INF_BLOCKED).any() and (got[3] == 0).any()
    IR.assert_same(host.corridor_inflate(so, W, ER.A_ORIGIN, ER.A_H, v, 0.3, 8), want)
