"""GPU: the solve kernels on the constructed problems of solve_zoo.py, against exact rational
arithmetic rounded once and against symmetries that hold to the bit.

Every method -- reduced and band for M = 1..16, dense for M = 1..10 -- solves three tiled launches
per M through solver.solve (B = 197: three full wavefronts and a tail of five; the rows recur with
an odd period or one that does not divide 64, so each lands on many lane positions); the reduced
method also through solve_uniform_device with a status buffer.  Uniform M takes the reduced method
through k_lane_uniform (even M <= 10, a trajectory per lane), k_reduced_uniform_lines (even
M >= 12, a lane pair per trajectory, whole-line output) and k_reduced_uniform (odd M, a lane pair,
axis-sequential), each with and without end derivatives; two ragged mixes take it through both
fused ragged classes, with and without the end-derivative array.

1-6 are asserted for every method; 4 and 6 hold to the bit on every variant but two, whose axes
round in different orders (axes_round_alike names the lines) and are held to the exact reference
at 1e-9 on both sides instead.  7 and 8 are asserted against the exact reference for every
method and to the bit for the reduced method: its block LDL^T is homogeneous in T and couples
through w1 - w0 (csrc/tgms_device.h KSP/KEP, segment_coeffs), so scaled times give scaled bits and
a translation changes c0 alone.  The literal-KKT methods choose pivots by comparing rows of
different units (position rows against derivative rows), which a time scale reorders, and take the
absolute waypoints as the right-hand side: for them 7 is asserted at 1e-9 against the exactly
transformed reference, 8 at the header's contract (norm-wise 1e-9 with c0 included), and the
bit-equality and the shape error under translation are printed, not asserted."""
import numpy as np
import pytest

import solve_zoo as Z
from conftest import batch_rel_err

pytestmark = pytest.mark.gpu

VARIANTS = ([("reduced", M) for M in range(1, 17)] + [("reduced_device", M) for M in range(1, 17)]
            + [("band", M) for M in range(1, 17)] + [("dense", M) for M in range(1, 11)])
IDS = ["%s-M%d" % v for v in VARIANTS]
_runs = {}


def _method(path):
    from trajectory_generator_ros2_amd import METHOD_BAND_KKT, METHOD_DENSE_KKT, METHOD_REDUCED
    return dict(reduced=METHOD_REDUCED, reduced_device=METHOD_REDUCED, band=METHOD_BAND_KKT, dense=METHOD_DENSE_KKT)[path]


def _solve_fn(solver, path):
    if path != "reduced_device":
        return lambda so, W, T, ED: solver.solve(so, W, T, ED)[:2]

    def device(so, W, T, ED):
        import torch
        B, M = len(so) - 1, int(so[1])
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        dC = torch.full((B, M, 3, 8), float("nan"), dtype=torch.float64, device="cuda")
        dS = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        dW, dT, dED = up(W), up(T), up(ED)
        solver.solve_uniform_device(B, M, dW, dT, dC, dS, dED)
        torch.cuda.synchronize()
        return dC.cpu().numpy(), dS.cpu().numpy()
    return device


def _with_method(solver, path, fn):
    from trajectory_generator_ros2_amd import METHOD_REDUCED
    solver.set_method(_method(path))
    try:
        return fn()
    finally:
        solver.set_method(METHOD_REDUCED)


def run_of(solver, path, M):
    """The variant's three launches, solved once per session and left unchanged."""
    if (path, M) not in _runs:
        _runs[path, M] = _with_method(solver, path, lambda: Z.Run(_solve_fn(solver, path), M, path))
    return _runs[path, M]


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_exact_reference(solver, path, M):
    """1. Every family within 1e-9 of the exact solve, status 0; cubic: max|c4..c7| <= 1e-9 max|c|."""
    Z.check_exact(run_of(solver, path, M), batch_rel_err)


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_placement(solver, path, M):
    """2. All copies of a row in one launch are bit-identical, coefficients and status."""
    Z.check_placement(run_of(solver, path, M))


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_waypoint_scale(solver, path, M):
    """3. Waypoints and end derivatives times 2^+-20: the same bits times 2^+-20."""
    Z.check_scale_w(run_of(solver, path, M))


def axes_round_alike(path, M):
    """False for the two kernel variants whose axes round in different orders, both measured and
    read; every other variant is held to the bit.

    k_band_kkt (every M): the three right-hand sides are slots 19..21 of a band row, so in the back
    substitution (csrc/tgms_band.hip:406-452) each axis' constant enters the eight-lane partial
    sums in another lane (3, 4, 5) and the DPP butterfly adds it at another place of the tree.  x and
    y of `twin` differ by up to ~1,300 ulp of single small coefficients (M = 1), both axes within
    2.40e-13 of the exact reference at every M.

    k_lane_uniform (even M = 4..10): the source is the same for every axis (seg_rows,
    csrc/tgms_reduced.hip:2527-2549), yet c7 of segment 0, the seven-term P7 sum of line 2540
    times r^4, comes out 1 ulp apart between x and y at M = 4, every other coefficient equal.  The
    build contracts a * b + c into fused operations where the compiler chooses (HIP's default
    -ffp-contract=fast; trajectory_generator_ros2_amd/build.py HIP_FLAGS sets none), per unrolled
    instance: a difference of that kind, read from the figures, not confirmed in the ISA.  M = 2
    on the same kernel, the lane-pair kernels and the dense method are bit-equal and stay asserted.

    Neither moves data between axes: test_still_axes holds on both (a moving axis keeps its bits
    whether the other two move or not, a constant axis gives exact zeros)."""
    return not (path == "band" or (path.startswith("reduced") and M % 2 == 0 and 4 <= M <= 10))


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_twin_axes(solver, path, M):
    """4. y a copy of x: C[:, 0] and C[:, 1] bit-identical.  On the two variants of axes_round_alike
    both axes are held to the exact reference at 1e-9 instead."""
    Z.check_twin(run_of(solver, path, M), bitwise=axes_round_alike(path, M))


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_still_axes(solver, path, M):
    """5. A constant axis gives c1..c7 == 0.0 and c0 the waypoint; the moving axis has the bits it
    has when the other two move as well."""
    Z.check_still(run_of(solver, path, M))


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_axis_permutation(solver, path, M):
    """6. All six axis permutations: the permuted result bit for bit.  On the two variants of
    axes_round_alike the permuted and the base solve are held to the exact reference at 1e-9."""
    Z.check_swap(run_of(solver, path, M), bitwise=axes_round_alike(path, M))


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_time_scale(solver, path, M):
    """7. Times scaled by 2^+-1: within 1e-9 of the exactly transformed reference; the reduced
    method to the bit.  Band and dense compare pivot candidates of different units, so only the
    tolerance is asserted for them; whether the bits agreed is printed."""
    Z.check_scale_t(run_of(solver, path, M), bitwise=path.startswith("reduced"))


@pytest.mark.parametrize("path,M", VARIANTS, ids=IDS)
def test_translation(solver, path, M):
    """8. Translated by (2^20, -2^20, 2^19): the reduced method returns c0 == w_i exactly, c1..c7 the
    untranslated bits, and meets the shape bound 1e-9 of the untranslated norm.  Band and dense
    meet include/tgms.h's contract, norm-wise 1e-9 with the offset in c0; their shape error is
    printed (measured, not guaranteed)."""
    Z.check_translate(run_of(solver, path, M), displacement=path.startswith("reduced"))


@pytest.mark.parametrize("path", ["reduced", "band"])
def test_ragged_mix(solver, path):
    """Both ragged mixes (every M in 1..16; with the end-derivative array the reduced classes split
    at M = 11 / 12, without it at 13 / 14): exact reference at 1e-9, status 0, and the 34 copies of
    a row, which span at least two tiles of their M's group, bit-identical."""
    _with_method(solver, path, lambda: Z.check_ragged(_solve_fn(solver, path), batch_rel_err, path))


def test_worst_per_family_table(solver):
    """Prints the table DESIGN.md quotes: per method, the worst value of each family over M."""
    for path in ("reduced", "reduced_device", "band", "dense"):
        worst = {}
        for p, M in VARIANTS:
            if p == path:
                for k, v in Z.check_exact(run_of(solver, p, M), batch_rel_err).items():
                    worst[k] = max(worst.get(k, 0.0), v)
        print("%s, worst per family over M: %s" % (path, "  ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
