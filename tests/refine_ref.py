"""Reference for ONE time-allocation refinement step (tgms_refine_uniform_device,
tgms_refine_batch_device), shared by test_refine_ref.py and test_gpu_refine_step.py.  NumPy
only.  The exact ingredients come from tests/golden/refine_grad.npz (oracle/exact.py: rational
solve, rational dJ_i/dT_i and F, each rounded once to fp64); the step itself,
  T_i <- T_i exp(clip(-eta T_i (dJ_i + k_T) / F, -1/2, 1/2)),
is restated here in np.longdouble for any eta, so the clamp and the whole range of the
kernels' exp polynomial get an exact value and not only the fixture's own eta = 0.02, where
no segment clamps.  F holds k_T sum T_i at the fixture's k_T, so that k_T is the one to use."""
import numpy as np

LD = np.longdouble
ULP = 2.0 ** -52
GRAD_TOL = 1e-9    # applied gradient against exact, norm-wise per trajectory (conftest.gradient_rel_err at TOL)
COST_TOL = 1e-11   # F against exact (test_refine_step_matches_exact_fixture)
ROUND_TOL = 4 * ULP  # exp_step (0.83 ulp) and the product T_i * exp: below 2 ulp; the rest for dtau's own rounding


def _per_segment(so, per_traj):
    return np.repeat(np.asarray(per_traj), np.diff(np.asarray(so, dtype=np.int64)))


def expected_step(so, T0, dJ, F, k_T, eta):
    """(T1_ref, dtau_ref), both np.longdouble [S]: dtau = -eta T0 (dJ + k_T) / F_b from the exact
    dJ and F, T1_ref = T0 exp(clip(dtau, -1/2, 1/2))."""
    T0 = np.asarray(T0, dtype=LD).reshape(-1)
    Fs = _per_segment(so, np.asarray(F, dtype=LD))
    dtau = -LD(eta) * T0 * (np.asarray(dJ, dtype=LD) + LD(k_T)) / Fs
    return T0 * np.exp(np.clip(dtau, LD(-0.5), LD(0.5))), dtau


def step_bound(so, T0, dJ, F, dtau_ref, eta):
    """Per-segment tolerance on T1 / T1_ref - 1, derived from contracts the suite already holds
    the step to, not from what any implementation gives:
      - the applied gradient g is within GRAD_TOL of the exact dJ norm-wise per trajectory,
        max_i |g_i - dJ_i| <= 1e-9 max_j |dJ_j|, so the unclamped step moves by at most
        eta T0_i / F_b * 1e-9 * max_j |dJ_j|;
      - the F the step divides by is within COST_TOL relative, which moves dtau_i by at most
        1e-11 |dtau_i|;
      - clip is 1-Lipschitz, so the clamped step moves by no more than the unclamped one;
      - T1 = T0 exp(x): an error d in x is a relative error exp(d) - 1 = d (1 + d/2 + ...) in
        T1, and d <= 2e-9 here, so the second-order term is below 2e-18 and sits inside the
        last term;
      - exp_step (0.83 ulp on [-1/2, 1/2]) and the product round below 2 ulp of 2^-52 together;
        the other 2 x 2^-52 hold the fp64 rounding of dtau itself: the sum, three products
        and the reciprocal of F, each 2^-53 of |dtau|, and |dtau| <= 1/2 where it still counts
        (beyond the clamp it does not reach the result).
    bound_i = eta T0_i / F_b * 1e-9 * max_j |dJ_j| + 1e-11 |dtau_i| + 4 x 2^-52."""
    so = np.asarray(so, dtype=np.int64)
    T0 = np.asarray(T0, dtype=np.float64).reshape(-1)
    gmax = _per_segment(so, np.maximum.reduceat(np.abs(np.asarray(dJ, dtype=np.float64)), so[:-1]))
    Fs = _per_segment(so, np.asarray(F, dtype=np.float64))
    return eta * T0 / Fs * GRAD_TOL * gmax + COST_TOL * np.abs(np.asarray(dtau_ref, dtype=np.float64)) + ROUND_TOL


def members(group, M):
    """The indices of the group's trajectories with M segments, in batch order."""
    return np.flatnonzero(np.diff(group["seg_offsets"]) == M)


def gather(group, src):
    """The trajectories `src` of a fixture group as a CSR batch: dict(seg_offsets, waypoints
    [S'+B',3], seg_times, end_derivs | None, dJ, F, T1), each trajectory's rows copied whole."""
    so = np.asarray(group["seg_offsets"], dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    Ms = np.diff(so)[src]
    so2 = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    seg = np.concatenate([np.arange(so[b], so[b + 1]) for b in src]) if len(src) else np.zeros(0, np.int64)
    wp = np.concatenate([np.arange(so[b] + b, so[b + 1] + b + 1) for b in src]) if len(src) else np.zeros(0, np.int64)
    ED = group["end_derivs"]
    return {"seg_offsets": so2, "waypoints": np.ascontiguousarray(group["waypoints"][wp]),
            "seg_times": np.ascontiguousarray(group["seg_times"][seg]),
            "end_derivs": None if ED is None else np.ascontiguousarray(ED[src]),
            "dJ": group["dJ"][seg], "F": group["F"][src], "T1": group["T1"][seg]}


def uniform_from_group(group, M, B):
    """(W [B, M+1, 3], T [B, M], ED [B, 18] or None, src [B]): trajectory b is the group's
    (b mod n_M)-th trajectory with M segments; src[b] is its index in the group, so that
    gather(group, src) holds the exact dJ, F and T1 of the uniform batch."""
    mem = members(group, M)
    assert len(mem) > 0, M
    src = mem[np.arange(B) % len(mem)]
    g = gather(group, src)
    return g["waypoints"].reshape(B, M + 1, 3), g["seg_times"].reshape(B, M), g["end_derivs"], src


def check_step(so, T0, T1, cost, group_slice, k_T, eta, label=""):
    """One step's output against exact: `cost` within 1e-11 relative of the exact F, every
    segment's T1 / T1_ref - 1 within step_bound, and every segment whose |dtau_ref| exceeds
    1/2 by more than its bound (so any implementation inside the contracts clamps it) at
    T0 e^(+-1/2) to 4 x 2^-52.  `group_slice` holds the exact dJ [S] and F [B] of the same
    trajectories (gather).  Prints and returns the worst error-to-bound ratio."""
    so = np.asarray(so, dtype=np.int64)
    T0 = np.asarray(T0, dtype=np.float64).reshape(-1)
    T1 = np.asarray(T1, dtype=np.float64).reshape(-1)
    dJ, F = group_slice["dJ"], group_slice["F"]
    assert T0.shape == T1.shape == dJ.shape and np.asarray(cost).shape == F.shape
    cerr = np.abs(np.asarray(cost, dtype=LD) / np.asarray(F, dtype=LD) - 1)
    T1_ref, dtau = expected_step(so, T0, dJ, F, k_T, eta)
    bound = step_bound(so, T0, dJ, F, dtau, eta)
    err = np.abs(np.asarray(T1, dtype=LD) / T1_ref - 1).astype(np.float64)
    ratio = err / bound
    w = int(np.argmax(ratio))
    b = int(np.searchsorted(so, w, side="right") - 1)
    sure = np.abs(dtau).astype(np.float64) > 0.5 + bound
    edge = T0.astype(LD) * np.exp(np.where(dtau > 0, LD(0.5), LD(-0.5)))
    cl = np.abs(T1.astype(LD) / edge - 1).astype(np.float64)
    clamp_worst = float(cl[sure].max()) if sure.any() else 0.0
    print(f"check_step {label} eta={eta}: worst err/bound {ratio[w]:.3f} (err {err[w]:.3e}, bound {bound[w]:.3e}) at "
          f"trajectory {b} (M = {so[b + 1] - so[b]}) segment {w - so[b]}, dtau_ref {float(dtau[w]):+.3f}; "
          f"cost err {float(cerr.max()):.2e}; {int(sure.sum())} of {len(T0)} segments surely clamped, "
          f"worst {clamp_worst:.2e}")
    assert float(cerr.max()) <= COST_TOL, float(cerr.max())
    assert ratio[w] <= 1.0, (b, w - so[b], err[w], bound[w])
    assert clamp_worst <= ROUND_TOL, clamp_worst
    return float(ratio[w])
