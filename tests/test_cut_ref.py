"""CPU: what the replan cut (tgms_cut_batch) rests on, in exact arithmetic, and the bit-level
rules of its reference (cut_ref.py).

The optimality identity.  A minimum-snap trajectory is the optimum of a problem whose state is
(p, p', p'', p''') and whose control is the snap, so the tail of an optimum is the optimum of the
tail problem started from that state.  With oracle/exact.py: solve exactly, cut (cut_ref.shifted
gives the state and the shifted row as rationals), solve the tail exactly from that state, and
require equality with the Taylor-shifted originals: no tolerance, the state is passed as rationals
through exact._reduced."""
from fractions import Fraction as F
from math import factorial

import numpy as np
import pytest

import cut_ref as CR
from oracle import exact


def _problem(M, with_derivs, seed):
    rng = np.random.default_rng(seed)
    W = np.round(rng.uniform(-3, 3, (M + 1, 3)) * 64) / 64
    T = np.round(rng.uniform(0.5, 2.0, M) * 64) / 64
    ED = np.round(rng.uniform(-1, 1, (2, 3, 3)) * 16) / 16 if with_derivs else None
    return exact._as_frac_traj(W, T, ED)


@pytest.mark.parametrize("with_derivs", [False, True], ids=["rest", "end_derivs"])
@pytest.mark.parametrize("M", [1, 2, 4, 16])
def test_the_tail_of_an_optimum_is_the_optimum_of_the_tail(M, with_derivs):
    _, W, T, ED = _problem(M, with_derivs, 100 + M)
    C, _ = exact._reduced(M, W, T, ED)
    for s in sorted({0, M // 2, M - 1}):  # the first, a middle and the last segment
        t_loc = T[s] * F(3, 8)
        rows = [CR.shifted(C[s][a], t_loc)[0] for a in range(3)]
        state = [[factorial(k) * rows[a][k] for a in range(3)] for k in range(4)]  # [order][axis]
        W2 = [state[0]] + W[s + 1:]
        T2 = [T[s] - t_loc] + T[s + 1:]
        ED2 = [[state[1], state[2], state[3]], ED[1]]
        C2, _ = exact._reduced(M - s, W2, T2, ED2)
        assert C2[0] == rows, (M, s)          # the shortened segment: the Taylor shift
        assert C2[1:] == C[s + 1:], (M, s)    # the rest: unchanged


def test_a_cut_on_a_knot_needs_no_shift():
    _, W, T, ED = _problem(4, True, 7)
    C, kd = exact._reduced(4, W, T, ED)
    state = [[kd(2, a)[k] for a in range(3)] for k in range(4)]
    C2, _ = exact._reduced(2, [state[0]] + W[3:], T[2:], [[state[1], state[2], state[3]], ED[1]])
    assert C2 == C[2:]


# ---- the bit-level rules of the reference ----

T4 = np.array([0.7, 1.3, 0.9, 1.1])
K4 = CR.knots(T4)


def test_a_cut_on_a_knot_belongs_to_the_later_segment():
    fin, s, t_loc, fl, t0 = CR.decide(T4, K4[2], 0.25)
    assert (fin, s, t_loc, fl) == (False, 2, 0.0, CR.DONE) and t0 == K4[2]


def test_one_ulp_either_side_of_a_knot():
    below, above = np.nextafter(K4[2], 0.0), np.nextafter(K4[2], 10.0)
    # just after: segment 2 at one ulp of the knot
    fin, s, t_loc, fl, t0 = CR.decide(T4, above, 0.25)
    assert (fin, s, fl) == (False, 2, CR.DONE) and t_loc == above - K4[2] and t0 == K4[2] + t_loc
    # just before: what is left of segment 1 is below min_frac T: snapped onto the knot
    fin, s, t_loc, fl, t0 = CR.decide(T4, below, 0.25)
    assert (fin, s, t_loc, fl) == (False, 2, 0.0, CR.DONE | CR.SNAPPED) and t0 == K4[2]
    # with min_frac = 0 it stays in segment 1, however little is left
    fin, s, t_loc, fl, t0 = CR.decide(T4, below, 0.0)
    assert (fin, s, fl) == (False, 1, CR.DONE) and t_loc == below - K4[1] and T4[1] - t_loc > 0.0


def test_rem_just_above_and_just_below_the_least_fraction():
    mf = 0.25
    least = np.float64(mf * T4[1])
    edge = np.float64(T4[1] - least)  # t_loc with rem == least up to the rounding of two subtractions
    for t_loc in (np.nextafter(edge, 0.0), edge, np.nextafter(edge, 10.0), np.nextafter(np.nextafter(edge, 10.0), 10.0)):
        rem = np.float64(T4[1] - t_loc)
        fin, s, tl, fl, _ = CR.decide(T4, np.float64(K4[1] + t_loc), mf)
        got = np.float64(min(max(np.float64(np.float64(K4[1] + t_loc) - K4[1]), 0.0), T4[1]))
        snapped = np.float64(T4[1] - got) < least
        assert not fin and s == (2 if snapped else 1) and bool(fl & CR.SNAPPED) == bool(snapped)
        assert abs(rem - least) < 1e-15
    assert {bool(CR.decide(T4, np.float64(K4[1] + x), mf)[3] & CR.SNAPPED) for x in (edge - 1e-9, edge + 1e-9)} == {
        False, True}


def test_snapping_off_the_last_segment_finishes():
    fin, s, t_loc, fl, t0 = CR.decide(T4, K4[4] - 0.01, 0.25)
    assert fin and fl == CR.FINISHED | CR.DONE and t0 == K4[4]


@pytest.mark.parametrize("t_cut", [0.0, -0.0, -1.0, -np.inf])
def test_a_cut_at_or_before_zero_is_the_identity(t_cut):
    fin, s, t_loc, fl, t0 = CR.decide(T4, t_cut, 0.25)
    assert (fin, s, t_loc, fl, t0) == (False, 0, 0.0, 0, 0.0)
    rng = np.random.default_rng(3)
    so, W, C, ED = np.array([0, 4]), rng.normal(size=(5, 3)), rng.normal(size=(4, 3, 8)), rng.normal(size=(1, 18))
    r = CR.cut(so, W, T4, C, [t_cut], 0.25, ED)
    for k, v in (("so", so), ("W", W), ("T", T4), ("C", C), ("ED", ED)):
        assert np.array_equal(CR.bits(r[k]), CR.bits(np.asarray(v, r[k].dtype))), k
    assert not r["W_tol"].any() and not r["C_tol"].any() and not r["ED_tol"].any()


@pytest.mark.parametrize("t_cut", [float(K4[4]), float(K4[4]) + 1.0, np.inf])
def test_a_cut_at_or_beyond_the_end_finishes(t_cut):
    rng = np.random.default_rng(4)
    W, C = rng.normal(size=(5, 3)), rng.normal(size=(4, 3, 8))
    r = CR.cut([0, 4], W, T4, C, [t_cut], 0.0, rng.normal(size=(1, 18)))
    assert r["flags"][0] == CR.FINISHED | CR.DONE and list(r["so"]) == [0, 1] and r["t0"][0] == K4[4]
    assert np.array_equal(r["W"], [W[4], W[4]]) and r["T"][0] == T4[3] and r["parent"][0] == 3
    assert not r["ED"].any() and np.array_equal(r["C"][0, :, 0], W[4]) and not r["C"][0, :, 1:].any()


def test_a_nan_cut_is_copied_through():
    rng = np.random.default_rng(5)
    W, C, ED = rng.normal(size=(5, 3)), rng.normal(size=(4, 3, 8)), rng.normal(size=(1, 18))
    r = CR.cut([0, 4], W, T4, C, [np.nan], 0.25, ED)
    assert r["flags"][0] == CR.NONFINITE and np.isnan(r["t0"][0]) and list(r["parent"]) == [0, 1, 2, 3]
    assert np.array_equal(r["W"], W) and np.array_equal(r["T"], T4) and np.array_equal(r["C"], C) and np.array_equal(r["ED"], ED)


def test_the_reference_state_is_the_derivative():
    """cut()'s evaluated rows against numpy's own polynomial derivative, at 1e-12 of the scale."""
    rng = np.random.default_rng(6)
    W, C = rng.normal(size=(5, 3)), rng.normal(size=(4, 3, 8))
    r = CR.cut([0, 4], W, T4, C, [K4[1] + 0.4], 0.1)
    assert r["s"][0] == 1 and list(r["so"]) == [0, 3] and r["flags"][0] == CR.DONE
    t = r["t_loc"][0]
    for a in range(3):
        p = np.polynomial.Polynomial(C[1, a])
        assert abs(r["W"][0, a] - p(t)) <= 1e-12 * r["W_tol"][0, a] / CR.TOL
        for k in (1, 2, 3):
            assert abs(r["ED"][0, (k - 1) * 3 + a] - p.deriv(k)(t)) <= 1e-12 * r["ED_tol"][0, (k - 1) * 3 + a] / CR.TOL
        q = np.polynomial.Polynomial(r["C"][0, a])
        for x in (0.0, 0.3, 0.9):
            assert abs(q(x) - p(t + x)) <= 1e-12 * np.abs(C[1, a]).sum() * 2.0 ** 7
    assert r["T"][0] == T4[1] - t and np.array_equal(r["T"][1:], T4[2:]) and np.array_equal(r["C"][1:], C[2:])
