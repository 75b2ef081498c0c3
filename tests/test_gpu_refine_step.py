"""GPU: one time-allocation refinement step on every kernel variant against exact arithmetic.

The step entry points are tgms_refine_uniform_device (k_refine_uniform<M, HAS_ED>, 32
specialisations) and tgms_refine_batch_device (ragged: k_refine_multi<MLO, MHI, HAS_ED>, one
launch per occupancy class from host-built group tables; uniform offsets: the uniform kernel).
The exact reference is tests/golden/refine_grad.npz's ragged groups r257 / r257e (257
trajectories, every M in 1..16 at least 6 times) through refine_ref.py: the trajectories of one
M gathered into a uniform batch keep their exact dJ and F, and the step is restated in
np.longdouble at eta = 0.02 (the fixture's own), 0.5 and 2.0, where 4 % and 10 % of the segments
clamp, on both sides.  check_step's tolerance is derived (refine_ref.step_bound), and
test_refine_ref.py shows the fp64 oracle inside it.

One wavefront holds 32 trajectories (a lane pair each): B = 70 is two full wavefronts and a
tail of 6.  Also here: the uniform refinement loop (tgms_refine_loop_device on a uniform batch:
ping-pong buffers, the copy back after an odd number of steps, the cached graph replayed on new
times) against chained steps, invalid trajectories, refused arguments, two streams on one
handle, and graph capture."""
import numpy as np
import pytest

import refine_ref as R
from conftest import load_refine_golden

pytestmark = pytest.mark.gpu

ETAS = (0.02, 0.5, 2.0)
B_U = 70


@pytest.fixture(scope="module")
def fx():
    """(k_T, {with_ed: group}): the exact ragged groups, left unchanged by every test."""
    k_T, eta, groups = load_refine_golden()
    assert (k_T, eta) == (1.0, 0.02)
    return k_T, {False: groups["r257"], True: groups["r257e"]}


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _outputs(S, B):
    """Prefilled outputs: NaN times and costs, -1 statuses."""
    import torch
    return (torch.full((S,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((B,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((B,), -1, dtype=torch.int32, device="cuda"))


def _untouched(*outs):
    import torch
    torch.cuda.synchronize()
    for o in outs:
        if o.dtype == torch.int32:
            assert bool((o == -1).all())
        else:
            assert bool(torch.isnan(o).all())


def uniform_step(solver, W, T, ED, k_T, eta, cost=True, status=True):
    """tgms_refine_uniform_device on host arrays W [B, M+1, 3], T [B, M] -> (T1 [B*M], cost, status)."""
    import torch
    B, M = T.shape
    dTo, dc, dst = _outputs(B * M, B)
    solver.refine_uniform_device(B, M, _dev(W), _dev(T), dTo, k_T, eta, dc if cost else None,
                                 dst if status else None, _dev(ED))
    torch.cuda.synchronize()
    return dTo.cpu().numpy(), dc.cpu().numpy(), dst.cpu().numpy()


def ragged_step(solver, g, k_T, eta, cost=True, status=True):
    """tgms_refine_batch_device on a gathered batch (refine_ref.gather) -> (T1 [S], cost, status)."""
    import torch
    so = g["seg_offsets"]
    B = len(so) - 1
    dTo, dc, dst = _outputs(int(so[-1]), B)
    solver.refine_batch_device(so, _dev(so), _dev(g["waypoints"]), _dev(g["seg_times"]), dTo, k_T, eta,
                               dc if cost else None, dst if status else None, _dev(g["end_derivs"]))
    torch.cuda.synchronize()
    return dTo.cpu().numpy(), dc.cpu().numpy(), dst.cpu().numpy()


_WHOLE = {}


def whole(solver, fx, ed, eta):
    """The ragged step on the whole group (B = 257), computed once per (ed, eta) and shared."""
    if (ed, eta) not in _WHOLE:
        k_T, groups = fx
        g = R.gather(groups[ed], np.arange(257))
        _WHOLE[(ed, eta)] = (g,) + ragged_step(solver, g, k_T, eta)
    return _WHOLE[(ed, eta)]


def _rows_of(g, idx):
    """Segment indices of the trajectories idx of a gathered batch."""
    so = g["seg_offsets"]
    return np.concatenate([np.arange(so[b], so[b + 1]) for b in idx])


# ------------------------------------------------------------------ 1. every uniform specialisation

@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("ed", [False, True])
@pytest.mark.parametrize("M", range(1, 17))
def test_uniform_step_matches_exact(solver, fx, M, ed, eta):
    """k_refine_uniform<M, ed> at B = 70 against exact; rows built from the same trajectory are
    bit-equal wherever they sit (another wavefront, the tail)."""
    k_T, groups = fx
    W, T, ED, src = R.uniform_from_group(groups[ed], M, B_U)
    T1, cost, st = uniform_step(solver, W, T, ED, k_T, eta)
    assert (st == 0).all()
    g = R.gather(groups[ed], src)
    R.check_step(g["seg_offsets"], T, T1, cost, g, k_T, eta, label=f"k_refine_uniform<{M}, {ed}>")
    if eta == 0.02:  # the fixture's own step, at the bound the other exact-fixture tests use
        assert np.abs(T1 / g["T1"] - 1).max() <= 1e-11
    n = len(R.members(groups[ed], M))
    assert n < 32  # so every trajectory recurs, the second time in another wavefront or the tail
    first = np.arange(B_U) % n
    assert np.array_equal(_bits(T1.reshape(B_U, M)), _bits(T1.reshape(B_U, M)[first]))
    assert np.array_equal(_bits(cost), _bits(cost[first]))


@pytest.mark.parametrize("ed", [False, True])
@pytest.mark.parametrize("M", range(1, 17))
def test_uniform_step_eta_zero_keeps_times(solver, fx, M, ed):
    k_T, groups = fx
    W, T, ED, src = R.uniform_from_group(groups[ed], M, B_U)
    T1, cost, st = uniform_step(solver, W, T, ED, k_T, 0.0)
    assert (st == 0).all()
    assert np.array_equal(_bits(T1), _bits(T.reshape(-1)))
    assert np.abs(cost / groups[ed]["F"][src] - 1).max() <= 1e-11


# ------------------------------------------------------------------ 2. the ragged step entry point

@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("ed", [False, True])
def test_ragged_step_matches_exact(solver, fx, ed, eta):
    """k_refine_multi (both classes of this HAS_ED) on the whole group, every M group a partial
    wavefront; and on the group tiled three times (B = 771, groups of 18..75: several wavefronts
    with partial tails), whose three copies are bit-equal to each other and to the single call."""
    k_T, groups = fx
    g, T1, cost, st = whole(solver, fx, ed, eta)
    assert (st == 0).all()
    R.check_step(g["seg_offsets"], g["seg_times"], T1, cost, g, k_T, eta, label=f"k_refine_multi ed={ed} B=257")
    if eta == 0.02:
        assert np.abs(T1 / g["T1"] - 1).max() <= 1e-11
    g3 = R.gather(groups[ed], np.tile(np.arange(257), 3))
    counts = np.bincount(np.diff(g3["seg_offsets"]))[1:]
    assert counts.min() == 18 and counts.max() == 75
    T3, c3, st3 = ragged_step(solver, g3, k_T, eta)
    assert (st3 == 0).all()
    R.check_step(g3["seg_offsets"], g3["seg_times"], T3, c3, g3, k_T, eta, label=f"k_refine_multi ed={ed} B=771")
    assert np.array_equal(_bits(T3), _bits(np.tile(T1, 3)))
    assert np.array_equal(_bits(c3), _bits(np.tile(cost, 3)))


@pytest.mark.parametrize("ed", [False, True])
def test_ragged_step_any_order(solver, fx, ed):
    """A random order of the same trajectories (other positions in every group's list, other
    offsets): each trajectory's times and cost are bit-equal to the unpermuted call's."""
    k_T, groups = fx
    eta = 2.0
    g, T1, cost, _ = whole(solver, fx, ed, eta)
    p = np.random.default_rng(17).permutation(257)
    gp = R.gather(groups[ed], p)
    Tp, cp, stp = ragged_step(solver, gp, k_T, eta)
    assert (stp == 0).all()
    assert np.array_equal(_bits(Tp), _bits(T1[_rows_of(g, p)]))
    assert np.array_equal(_bits(cp), _bits(cost[p]))


@pytest.mark.parametrize("ed", [False, True])
@pytest.mark.parametrize("keep", ["M<=11", "M>=14", "M in 12..13"])
def test_ragged_step_sub_batches(solver, fx, ed, keep):
    """Sub-batches that leave one occupancy class empty, or hold only M = 12 and 13 (the one-wave
    class with end derivatives, the two-wave class without): bit-equal to the same trajectories
    in the whole-batch call."""
    k_T, groups = fx
    eta = 0.5
    g, T1, cost, _ = whole(solver, fx, ed, eta)
    Ms = np.diff(g["seg_offsets"])
    idx = np.flatnonzero({"M<=11": Ms <= 11, "M>=14": Ms >= 14, "M in 12..13": (Ms == 12) | (Ms == 13)}[keep])
    assert len(idx) > 32
    gs = R.gather(groups[ed], idx)
    Ts, cs, sts = ragged_step(solver, gs, k_T, eta)
    assert (sts == 0).all()
    assert np.array_equal(_bits(Ts), _bits(T1[_rows_of(g, idx)]))
    assert np.array_equal(_bits(cs), _bits(cost[idx]))


@pytest.mark.parametrize("ed", [False, True])
@pytest.mark.parametrize("M", [5, 12, 16])
def test_batch_call_with_uniform_offsets_takes_the_uniform_kernel(solver, fx, M, ed):
    k_T, groups = fx
    W, T, ED, src = R.uniform_from_group(groups[ed], M, B_U)
    want = uniform_step(solver, W, T, ED, k_T, 0.5)
    got = ragged_step(solver, R.gather(groups[ed], src), k_T, 0.5)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------ 3. invalid trajectories keep their times

BAD_MS = (3, 8, 12, 13, 16)  # both classes, with and without end derivatives (boundaries 11 and 13)


def _inject(g, b, kind):
    """Make trajectory b of the gathered batch g invalid in place."""
    so = g["seg_offsets"]
    s0, s1 = int(so[b]), int(so[b + 1])
    if kind == 0:
        g["seg_times"][s1 - 1] = 0.0 if b % 2 else -1.5  # T <= 0 in the last segment
    elif kind == 1:
        g["seg_times"][s0] = np.inf if b % 2 else np.nan  # a non-finite T
    elif kind == 2:
        g["waypoints"][s1 + b, 1] = np.nan  # NaN at the last waypoint
    else:
        g["end_derivs"][b, 17] = np.nan


def _check_invalid(clean, dirty, so, T_in, bad):
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG
    B = len(so) - 1
    good = np.setdiff1d(np.arange(B), bad)
    (Tc, cc, sc), (Td, cd, sd) = clean, dirty
    assert (sc == 0).all() and (sd[bad] == ERR_INVALID_ARG).all()
    rows_bad = np.concatenate([np.arange(so[b], so[b + 1]) for b in bad])
    rows_good = np.concatenate([np.arange(so[b], so[b + 1]) for b in good])
    assert np.array_equal(_bits(Td[rows_bad]), _bits(T_in[rows_bad]))
    assert np.array_equal(_bits(Td[rows_good]), _bits(Tc[rows_good]))
    assert np.array_equal(_bits(cd[good]), _bits(cc[good])) and np.array_equal(sd[good], sc[good])


@pytest.mark.parametrize("ed", [False, True])
def test_ragged_step_invalid_trajectories_keep_their_times(solver, fx, ed):
    """T <= 0 in the last segment, a non-finite T, a NaN waypoint and (with them) a NaN end
    derivative, each in a trajectory of five M groups: those come back with
    TGMS_ERR_INVALID_ARG and their input times bit for bit, every other trajectory exactly as
    in the clean call; omitting d_cost or d_status changes nothing else."""
    k_T, groups = fx
    eta = 0.5
    g, T1, cost, st = whole(solver, fx, ed, eta)
    gd = R.gather(groups[ed], np.arange(257))
    Ms = np.diff(gd["seg_offsets"])
    bad = []
    for M in BAD_MS:
        mem = np.flatnonzero(Ms == M)
        for kind in range(4 if ed else 3):
            _inject(gd, int(mem[kind + 1]), kind)
            bad.append(int(mem[kind + 1]))
    bad = np.array(sorted(bad))
    dirty = ragged_step(solver, gd, k_T, eta)
    _check_invalid((T1, cost, st), dirty, gd["seg_offsets"], gd["seg_times"], bad)
    no_cost = ragged_step(solver, gd, k_T, eta, cost=False)
    no_st = ragged_step(solver, gd, k_T, eta, status=False)
    assert np.array_equal(_bits(no_cost[0]), _bits(dirty[0])) and np.array_equal(no_cost[2], dirty[2])
    assert np.isnan(no_cost[1]).all() and (no_st[2] == -1).all()
    good = np.setdiff1d(np.arange(257), bad)
    assert np.array_equal(_bits(no_st[0]), _bits(dirty[0])) and np.array_equal(_bits(no_st[1][good]), _bits(dirty[1][good]))


@pytest.mark.parametrize("ed", [False, True])
@pytest.mark.parametrize("M", BAD_MS)
def test_uniform_step_invalid_trajectories_keep_their_times(solver, fx, M, ed):
    """The same injections in the uniform kernel, in the first wavefront, the second and the tail."""
    k_T, groups = fx
    eta = 0.5
    W, T, ED, src = R.uniform_from_group(groups[ed], M, B_U)
    clean = uniform_step(solver, W, T, ED, k_T, eta)
    gd = R.gather(groups[ed], src)
    bad = np.array([3, 33, 40, 69] if ed else [3, 33, 69])
    for kind, b in enumerate(bad):
        _inject(gd, int(b), kind)
    Wd, Td, EDd = gd["waypoints"].reshape(B_U, M + 1, 3), gd["seg_times"].reshape(B_U, M), gd["end_derivs"]
    dirty = uniform_step(solver, Wd, Td, EDd, k_T, eta)
    _check_invalid(clean, dirty, gd["seg_offsets"], gd["seg_times"], bad)
    no_cost = uniform_step(solver, Wd, Td, EDd, k_T, eta, cost=False)
    no_st = uniform_step(solver, Wd, Td, EDd, k_T, eta, status=False)
    assert np.array_equal(_bits(no_cost[0]), _bits(dirty[0])) and np.array_equal(no_cost[2], dirty[2])
    assert np.isnan(no_cost[1]).all() and (no_st[2] == -1).all()
    good = np.setdiff1d(np.arange(B_U), bad)
    assert np.array_equal(_bits(no_st[0]), _bits(dirty[0])) and np.array_equal(_bits(no_st[1][good]), _bits(dirty[1][good]))


# ------------------------------------------------------------------ 4. the uniform refinement loop

@pytest.mark.parametrize("iters", [0, 1, 2, 3])
@pytest.mark.parametrize("ed", [False, True])
@pytest.mark.parametrize("M", [3, 10])
def test_uniform_loop_is_its_chained_steps(solver, fx, M, ed, iters):
    """tgms_refine_loop_device on a uniform batch (loop_on_device: two time buffers, the copy
    back after an odd number of steps, a graph cached by its pointers): times bit-equal to
    `iters` chained step calls, the cost to an eta = 0 step's at the final times, the
    coefficients to the uniform solve there; and again after new times were written into the
    same tensor, which replays the cached graph."""
    import torch
    k_T, groups = fx
    eta = 0.5
    W, T, ED, _ = R.uniform_from_group(groups[ed], M, B_U)
    so = (M * np.arange(B_U + 1)).astype(np.int32)
    dso, dW, dED = _dev(so), _dev(W), _dev(ED)
    dT = _dev(T)
    dC = torch.full((B_U * M, 3, 8), float("nan"), dtype=torch.float64, device="cuda")
    _, dcost, dst = _outputs(1, B_U)

    def chain(T0):
        Tk = T0
        for _ in range(iters):
            Tk, _, st = uniform_step(solver, W, Tk.reshape(B_U, M), ED, k_T, eta)
            assert (st == 0).all()
        Tk = Tk.reshape(B_U, M)
        _, cost, _ = uniform_step(solver, W, Tk, ED, k_T, 0.0)
        C = torch.empty_like(dC)
        solver.solve_uniform_device(B_U, M, dW, _dev(Tk), C, None, dED)
        torch.cuda.synchronize()
        return Tk, cost, C.cpu().numpy()

    T_b = T * np.linspace(0.8, 1.3, M)  # other times for the second call
    for T0 in (T, T_b):
        dT.copy_(_dev(T0))
        dC.fill_(float("nan"))
        dcost.fill_(float("nan"))
        dst.fill_(-1)
        solver.refine_loop_device(so, dso, dW, dT, k_T, eta, iters, dC, dcost, dst, dED)
        torch.cuda.synchronize()
        Tk, cost, C = chain(T0)
        assert (dst.cpu().numpy() == 0).all()
        assert np.array_equal(_bits(dT.cpu().numpy()), _bits(Tk))
        assert np.array_equal(_bits(dcost.cpu().numpy()), _bits(cost))
        assert np.array_equal(_bits(dC.cpu().numpy()), _bits(C))
        assert (iters == 0) == np.array_equal(Tk, T0)
        if iters == 1:  # the host call runs the same step kernels
            Th, Ch, ch, sth, worst = solver.refine(so, W, T0, ED, k_T, eta, 1)
            assert worst == 0 and np.array_equal(_bits(Th), _bits(Tk.reshape(-1)))
            assert np.array_equal(_bits(ch), _bits(cost)) and np.array_equal(_bits(Ch), _bits(C))


# ------------------------------------------------------------------ 5. arguments

def _off_by_8(t):
    """A copy of the device tensor t that starts 8 bytes past a 16-byte boundary."""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    out = buf[1:]
    out.copy_(t.reshape(-1))
    assert out.data_ptr() % 16 == 8
    return out


@pytest.mark.parametrize("entry", ["uniform", "batch"])
def test_refused_arguments_leave_the_outputs_alone(solver, fx, entry):
    import torch
    from trajectory_generator_ros2_amd import (ERR_INVALID_ARG, ERR_UNSUPPORTED, METHOD_DENSE_KKT, METHOD_REDUCED,
                                               TgmsError)
    k_T, groups = fx
    M = 7
    if entry == "uniform":
        W, T, ED, src = R.uniform_from_group(groups[True], M, B_U)
        g = R.gather(groups[True], src)
    else:
        g = R.gather(groups[True], np.arange(100))
    so = g["seg_offsets"]
    B, S = len(so) - 1, int(so[-1])
    dso, dW, dT, dED = _dev(so), _dev(g["waypoints"]), _dev(g["seg_times"]), _dev(g["end_derivs"])
    dTo, dc, dst = _outputs(S, B)

    def call(W=dW, T=dT, To=dTo, c=dc, st=dst, ED=dED, kT=k_T, eta=0.1, M=M, so=so):
        if entry == "uniform":
            solver.refine_uniform_device(B, M, W, T, To, kT, eta, c, st, ED)
        else:
            solver.refine_batch_device(so, dso, W, T, To, kT, eta, c, st, ED)

    def refused(status, **kw):
        with pytest.raises(TgmsError) as e:
            call(**kw)
        assert e.value.status == status, (kw.keys(), e.value)
        _untouched(dTo, dc, dst)

    refused(ERR_INVALID_ARG, To=dT)  # the output aliases the input
    off_To = _off_by_8(dTo)
    for kw in ({"W": _off_by_8(dW)}, {"T": _off_by_8(dT)}, {"ED": _off_by_8(dED)}, {"To": off_To},
               {"c": _off_by_8(dc)}):
        refused(ERR_INVALID_ARG, **kw)
        assert "aligned" in solver.last_error()
    _untouched(off_To)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        refused(ERR_INVALID_ARG, kT=bad)
        refused(ERR_INVALID_ARG, eta=bad)
    if entry == "uniform":
        refused(ERR_INVALID_ARG, M=0)
        refused(ERR_INVALID_ARG, M=17)
    else:
        so0 = so.copy()
        so0[41:] -= so0[41] - so0[40]  # trajectory 40 has no segment
        refused(ERR_INVALID_ARG, so=so0)
        assert "trajectory 40 has 0 segments" in solver.last_error()
        so17 = so.copy()
        so17[58:] += 17 - (so17[58] - so17[57])  # trajectory 57 has 17
        refused(ERR_INVALID_ARG, so=so17)
        assert "trajectory 57 has 17 segments" in solver.last_error()
    solver.set_method(METHOD_DENSE_KKT)
    try:
        refused(ERR_UNSUPPORTED)
    finally:
        solver.set_method(METHOD_REDUCED)
    # B = 0 is no error, and nothing is written
    if entry == "uniform":
        solver.refine_uniform_device(0, M, dW, dT, dTo, k_T, 0.1, dc, dst, dED)
    else:
        solver.refine_batch_device(np.zeros(1, np.int32), dso, dW, dT, dTo, k_T, 0.1, dc, dst, dED)
    _untouched(dTo, dc, dst)
    call()  # and the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all() and bool(torch.isfinite(dTo).all()) and bool(torch.isfinite(dc).all())


# ------------------------------------------------------------------ 6. two streams on one handle

@pytest.mark.parametrize("ed", [False, True])
def test_two_streams_share_the_plan_scratch(solver, fx, ed):
    """Two ragged step calls of one handle back to back on two streams (as
    test_two_streams_share_handle_scratch for the solve): the second uploads its own grouping
    into the handle's permutation while the first call's kernels may still read theirs.  Each
    equals its call alone."""
    import torch
    k_T, groups = fx
    eta = 0.5
    g1 = R.gather(groups[ed], np.tile(np.arange(257), 3))  # B = 771
    g2 = R.gather(groups[ed], np.arange(256, 56, -1))      # B = 200, another grouping
    alone = [ragged_step(solver, g, k_T, eta) for g in (g1, g2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    args, outs = [], []
    for g in (g1, g2):
        so = g["seg_offsets"]
        args.append((so, _dev(so), _dev(g["waypoints"]), _dev(g["seg_times"]), _dev(g["end_derivs"])))
        outs.append(_outputs(int(so[-1]), len(so) - 1))
    torch.cuda.synchronize()
    for (so, dso, dW, dT, dED), (dTo, dc, dst), s in zip(args, outs, streams):
        solver.refine_batch_device(so, dso, dW, dT, dTo, k_T, eta, dc, dst, dED, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for (dTo, dc, dst), (T1, cost, st) in zip(outs, alone):
        assert np.array_equal(_bits(dTo.cpu().numpy()), _bits(T1))
        assert np.array_equal(_bits(dc.cpu().numpy()), _bits(cost))
        assert np.array_equal(dst.cpu().numpy(), st) and (st == 0).all()


# ------------------------------------------------------------------ 7. capture

@pytest.mark.parametrize("ed", [False, True])
def test_uniform_step_captured_and_replayed(solver, fx, ed):
    """tgms_refine_uniform_device inside torch.cuda.graph (test_gpu_bounds.py's pattern),
    replayed twice with the times changed in place between the replays: each replay is
    bit-equal to the direct call on the times it saw.  (The ragged call refuses a capturing
    stream: test_gpu_capture.py.)"""
    import torch
    k_T, groups = fx
    M, eta = 9, 0.5
    W, T, ED, _ = R.uniform_from_group(groups[ed], M, B_U)
    T_b = T * np.linspace(1.2, 0.7, M)
    want = [uniform_step(solver, W, Tx, ED, k_T, eta) for Tx in (T, T_b)]
    assert not np.array_equal(want[0][0], want[1][0])
    dW, dT, dED = _dev(W), _dev(T), _dev(ED)
    dTo, dc, dst = _outputs(B_U * M, B_U)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        try:
            solver.refine_uniform_device(B_U, M, dW, dT, dTo, k_T, eta, dc, dst, dED, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for Tx, (T1, cost, st) in zip((T, T_b), want):
        dT.copy_(_dev(Tx))
        dTo.fill_(float("nan"))
        dc.fill_(float("nan"))
        dst.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dTo.cpu().numpy()), _bits(T1))
        assert np.array_equal(_bits(dc.cpu().numpy()), _bits(cost))
        assert np.array_equal(dst.cpu().numpy(), st)
    del graph
