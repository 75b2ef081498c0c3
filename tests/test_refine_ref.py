"""CPU: the refinement-step reference (tests/refine_ref.py) meets its own conditions before the
kernels are asked to (test_gpu_refine_step.py): it reproduces the exact fixture at the
fixture's eta, the larger step sizes it is used at do reach the clamp on both sides, every
M has members to build a uniform batch from, and a correct fp64 implementation (the oracle)
passes check_step, so step_bound is a bound the arithmetic can meet."""
import numpy as np
import pytest

import refine_ref as R
from conftest import REFINE_GROUPS, load_refine_golden

ETAS = (0.02, 0.5, 2.0)


@pytest.mark.parametrize("group", REFINE_GROUPS)
def test_expected_step_reproduces_the_fixture(group):
    """At the fixture's eta = 0.02 the longdouble restatement gives the fixture's T1 (mpmath
    exp of rationals, rounded once) to 1e-15 relative."""
    k_T, eta, groups = load_refine_golden()
    d = groups[group]
    T1_ref, dtau = R.expected_step(d["seg_offsets"], d["seg_times"], d["dJ"], d["F"], k_T, eta)
    assert (k_T, eta) == (1.0, 0.02)
    assert float(np.abs(dtau).max()) < 0.5  # nothing clamps at this eta
    assert float(np.abs(d["T1"].astype(R.LD) / T1_ref - 1).max()) <= 1e-15


def _clamped(d, k_T, eta):
    so = d["seg_offsets"]
    _, dtau = R.expected_step(so, d["seg_times"], d["dJ"], d["F"], k_T, eta)
    cl = np.abs(dtau) > 0.5
    per_traj = np.maximum.reduceat(cl, so[:-1].astype(np.int64))
    return dtau, cl, per_traj


@pytest.mark.parametrize("group", ["r257", "r257e"])
def test_larger_steps_reach_the_clamp(group):
    """eta = 2: at least 9 % of the segments clamp, on both sides, in at least half the
    trajectories; eta = 0.5: at least 3 %."""
    k_T, _, groups = load_refine_golden()
    dtau, cl, per_traj = _clamped(groups[group], k_T, 2.0)
    print(f"{group} eta=2: clamped share {cl.mean():.3f}, most negative dtau {float(dtau.min()):.2f}, "
          f"most positive {float(dtau.max()):.2f}, trajectories with a clamped segment {per_traj.mean():.2f}")
    assert cl.mean() >= 0.09
    assert (dtau < -0.5).any() and (dtau > 0.5).any()
    assert per_traj.mean() >= 0.5
    dtau, cl, _ = _clamped(groups[group], k_T, 0.5)
    print(f"{group} eta=0.5: clamped share {cl.mean():.3f}")
    assert cl.mean() >= 0.03


@pytest.mark.parametrize("group", ["r257", "r257e"])
def test_every_m_has_members(group):
    _, _, groups = load_refine_golden()
    counts = np.bincount(np.diff(groups[group]["seg_offsets"]), minlength=17)
    assert counts[0] == 0 and len(counts) == 17 and (counts[1:] >= 6).all(), counts


@pytest.mark.parametrize("group", ["r257", "r257e"])
def test_uniform_from_group_is_a_gather(group):
    """uniform_from_group cycles through the group's trajectories of one M, and gather() on its
    src returns the same rows together with their exact dJ, F, T1."""
    _, _, groups = load_refine_golden()
    d = groups[group]
    so = d["seg_offsets"]
    for M in (1, 9, 16):
        W, T, ED, src = R.uniform_from_group(d, M, 70)
        n = len(R.members(d, M))
        assert W.shape == (70, M + 1, 3) and T.shape == (70, M) and (np.diff(so)[src] == M).all()
        assert np.array_equal(src[:n], R.members(d, M)) and np.array_equal(src[n:], src[:70 - n])
        b = 69
        s0 = so[src[b]]
        assert np.array_equal(T[b], d["seg_times"][s0:s0 + M])
        assert np.array_equal(W[b], d["waypoints"][s0 + src[b]:s0 + src[b] + M + 1])
        assert (ED is None) == (d["end_derivs"] is None) and (ED is None or np.array_equal(ED[b], d["end_derivs"][src[b]]))
        g = R.gather(d, src)
        assert np.array_equal(g["dJ"].reshape(70, M)[b], d["dJ"][s0:s0 + M]) and g["F"][b] == d["F"][src[b]]
        assert np.array_equal(g["seg_offsets"], M * np.arange(71))


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("group", ["r257", "r257e"])
def test_oracle_step_passes_check_step(oracle, group, eta):
    """The fp64 oracle (reduced formulation, one step; F at the input times from iters = 0)
    is inside step_bound at every eta: the bound is one a correct fp64 implementation meets.
    Its own gradient error on r257e is 8.2e-10 of the 1e-9 the bound grants, so the ratio is
    close to 1 there."""
    k_T, _, groups = load_refine_golden()
    d = groups[group]
    so, W, T, ED = d["seg_offsets"], d["waypoints"], d["seg_times"], d["end_derivs"]
    _, F0, _, st0 = oracle.refine_batch(so, W, T, ED, k_T, eta, 0, oracle.REDUCED)
    T1, _, _, st1 = oracle.refine_batch(so, W, T, ED, k_T, eta, 1, oracle.REDUCED)
    assert (st0 == 0).all() and (st1 == 0).all()
    R.check_step(so, T, T1, F0, d, k_T, eta, label=f"oracle {group}")


def test_check_step_catches_a_wrong_step():
    """check_step fails on a step that misses the clamp, on one that is 1e-8 off in one
    segment, and on a cost 1e-10 off; it passes on the reference's own rounding."""
    k_T, _, groups = load_refine_golden()
    d = groups["r257e"]
    so, T = d["seg_offsets"], d["seg_times"]
    T1_ref, dtau = R.expected_step(so, T, d["dJ"], d["F"], k_T, 2.0)
    good = T1_ref.astype(np.float64)
    assert R.check_step(so, T, good, d["F"], d, k_T, 2.0, label="rounded reference") <= 0.25
    unclamped = (T.astype(R.LD) * np.exp(dtau)).astype(np.float64)
    with pytest.raises(AssertionError):
        R.check_step(so, T, unclamped, d["F"], d, k_T, 2.0)
    off = good.copy()
    off[1234] *= 1.0 + 1e-8
    with pytest.raises(AssertionError):
        R.check_step(so, T, off, d["F"], d, k_T, 2.0)
    with pytest.raises(AssertionError):
        R.check_step(so, T, good, d["F"] * (1.0 + 1e-10), d, k_T, 2.0)
