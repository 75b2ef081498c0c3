"""CPU: the body-rate reference of rate_ref.py against itself and against a closed form.  Its
two ways to the per-segment maximum of omega^2 (the roots of the degree-25 stationarity
polynomial from np.convolve and the companion matrix; 200,001 samples plus golden-section
refinement) must agree to 1e-10 relative on the three golden batches.  Measured: 3.3e-18 on
ragged.npz, 1.7e-18 on end_derivs.npz, 1.3e-17 on extreme.npz (longdouble values at both ways'
candidates), no segment excepted."""
import numpy as np
import pytest

import rate_ref as RR

AGREE = 1e-10


@pytest.mark.parametrize("name", RR.FIXTURES)
def test_roots_and_samples_agree(name):
    """On extreme.npz alone a segment over 1e-10 would be excepted (the reference takes the
    larger of the two there) and listed by index, 2 % of the segments at the most."""
    fx = RR.fixture(name)
    wa, wb = fx["w2_roots"], fx["w2_samples"]
    rel = np.abs(wa - wb) / np.maximum(wa, wb)
    over = np.flatnonzero(rel > AGREE)
    print("%s: roots vs samples on omega^2: %.3g relative at worst, excepted segments %s"
          % (name, float(rel.max()), list(over)))
    allowed = 0.02 * len(rel) if name == "extreme" else 0
    assert len(over) <= allowed, (list(over), [float(x) for x in rel[over]])
    assert np.isfinite(fx["omega"]).all() and (fx["omega"] > 0).all()


def test_closed_form():
    """p_x = a t^2 / 2 + k t^3 / 6: omega = g k / ((a + k t)^2 + g^2), k / g at t = -a / k."""
    for a, k, T in ((-3.0, 4.0, 1.5), (-0.2, 7.0, 0.05), (-30.0, 2.0, 20.0)):
        so, Ts, C, tp = RR.closed_form(a, k, T)
        omega, seg, u = RR.records(so, Ts, C)
        assert abs(omega[0] - k / RR.G0) <= 1e-14 * k / RR.G0 and seg[0] == omega[0]
        assert abs(u[0] * T - tp) <= 1e-9 * T
        for t in (0.0, 0.3 * T, T):
            want = RR.G0 * k / ((a + k * t) ** 2 + RR.G0 ** 2)
            assert abs(RR.evaluate(so, Ts, C, 0, t) - want) <= 1e-14 * want


def test_zero_cross_product_is_zero():
    """A constant and a purely vertical trajectory have omega == 0.0, at g = 0 as well."""
    so, T = np.array([0, 2], np.int32), np.array([0.7, 2.0])
    C = np.zeros((2, 3, 8))
    C[:, :, 0] = [0.1, -2.7, 3.3]
    for g in (0.0, RR.G0):
        assert RR.records(so, T, C, g)[0][0] == 0.0
    C[:, 2, 1:] = np.linspace(-1.0, 1.0, 14).reshape(2, 7)
    for g in (0.0, RR.G0):
        assert RR.records(so, T, C, g)[0][0] == 0.0
