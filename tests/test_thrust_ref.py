"""CPU, no library: the reference of thrust_ref.py against closed forms, so that what the host
and GPU tests are held to is itself pinned."""
import numpy as np
import pytest

import bounds_ref as R
import thrust_ref as TR

G = TR.G0
P0 = np.array([0.3, -1.0, 2.0])


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_horizontal_rest_to_rest(T):
    """p'' is along x alone with extremes +-a_pk and 0 at both ends: f_min = g, f_max =
    sqrt(a_pk^2 + g^2), tilt_max = atan(a_pk / g)."""
    d = -1.7 * T ** 2  # a_pk independent of T
    so, Ts, C, _ = R.rest_to_rest(P0, d, T, axis=0)
    a = TR.a_peak(d, T)
    ref = TR.records(so, Ts, C)[0]
    assert ref[0] == G
    assert abs(ref[1] - np.hypot(a, G)) <= 1e-14 * ref[1]
    assert abs(ref[2] - np.arctan(a / G)) <= 1e-14
    f, th = TR.evaluate(so, Ts, C, 0, 0.5 * T * (1 - 1 / np.sqrt(5.0)))  # where |p''| peaks
    assert abs(f - ref[1]) <= 1e-13 * ref[1] and abs(th - ref[2]) <= 1e-13


def test_vertical_rest_to_rest():
    so, Ts, C, _ = R.rest_to_rest(P0, 0.9, 1.5, axis=2)
    a = TR.a_peak(0.9, 1.5)
    assert a < G
    ref = TR.records(so, Ts, C)[0]
    assert abs(ref[0] - (G - a)) <= 1e-14 * G and abs(ref[1] - (G + a)) <= 1e-14 * G and ref[2] == 0.0
    so, Ts, C, _ = R.rest_to_rest(P0, 4.0, 1.0, axis=2)  # a_pk = 30 > g: thrust crosses zero
    ref = TR.records(so, Ts, C)[0]
    assert ref[0] <= 0.05 and abs(ref[2] - np.pi) <= 1e-15  # the grid's floor only: no root of f_z is sought


def test_constant_and_g_zero():
    so = np.array([0, 3], np.int32)
    C = np.zeros((3, 3, 8))
    C[:, :, 0] = [0.1, -2.7, 3.3]
    ref = TR.records(so, [0.5, 2.0, 7.0], C)[0]
    assert ref[0] == G and ref[1] == G and ref[2] == 0.0
    so, Ts, C, peaks = R.rest_to_rest(P0, 1.7, 2.0, axis=1)
    ref = TR.records(so, Ts, C, g=0.0)[0]  # g = 0: the extremes of |p''| itself
    assert ref[0] == 0.0 and abs(ref[1] - peaks[1]) <= 1e-14 * peaks[1]


def test_the_tilt_polynomial_has_degree_13_and_its_roots_matter():
    """On a solved-looking segment (all three axes moving) the degree-14 coefficient of G is
    rounding noise, and theta is stationary at the interior roots of G."""
    rng = np.random.default_rng(5)
    C = rng.uniform(-1, 1, (1, 3, 8))
    e = TR._force_polys(C[0], 1.3, G)
    Gp = TR.tilt_poly(e)
    assert len(Gp) == 15 and abs(Gp[14]) <= 1e-17 * np.abs(Gp).max()
    roots = TR._candidates(TR._antiderivative(Gp))
    inner = roots[(roots > 1e-3) & (roots < 1 - 1e-3)]
    assert len(inner) >= 1
    for r in inner:
        h = 1e-4
        th = [float(TR._values(e, 1.3, np.array([r + k * h], dtype=TR.LD))[1][0]) for k in (-1, 0, 1)]
        assert abs(th[2] - th[0]) <= 1e-3 * abs(th[2] - 2 * th[1] + th[0])  # odd part vanishes: stationary
