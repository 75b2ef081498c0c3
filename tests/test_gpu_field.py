"""GPU: the distance-field clearance (tgms_field_clearance_batch on a GPU handle and
tgms_field_clearance_batch_device, csrc/tgms_field.hip).  The cases of test_field_host.py run
through both entry points (field_ref.py), then the launch's own corners: bad segment counts in
the device offsets, misaligned arrays, host / device agreement, two streams on one handle, a
captured graph of the call with a given bound, the refusal to capture the reduction, a multi
handle, the host handle's device call."""
import numpy as np
import pytest

import field_ref as FR
from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, SEP_CLOSE, SEP_NONFINITE, TgmsError

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _outs(B):
    import torch
    return (torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((B,), -2, dtype=torch.int32, device="cuda"), torch.full((B,), -2, dtype=torch.int32, device="cuda"))


class Device:
    """The device entry point behind the backend interface of field_ref.py."""

    def __init__(self, solver):
        self.s = solver

    def field_clearance(self, so, T, C, origin, h, values, r_min, tol, lip=0.0, max_evals=1 << 20):
        import torch
        B = len(so) - 1
        v = np.ascontiguousarray(values, dtype=np.float32)
        outs = _outs(B)
        self.s.field_clearance_device(B, _dev(np.asarray(so, np.int32)), _dev(np.asarray(T, np.float64).reshape(-1)),
                                      _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)), origin, h, v.shape[::-1], _dev(v),
                                      lip, r_min, tol, max_evals, *outs)
        torch.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in outs)


@pytest.fixture(scope="module", params=["host_pointers", "device"])
def be(request, solver):
    return solver if request.param == "host_pointers" else Device(solver)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


@pytest.mark.parametrize("tol", FR.AFFINE_TOLS)
@pytest.mark.parametrize("name", ["rest", "end_derivs", "ragged65"])
def test_affine_field_within_tol_of_the_exact_minimum(be, name, tol):
    FR.check_affine(be, name, tol)


def test_affine_field_with_a_given_bound(be):
    FR.check_affine(be, "ragged65", 1e-3, lip=float(np.linalg.norm(FR.AFFINE_N)))


def test_sphere_horizon_and_host_agreement(be, host):
    far = FR.check_sphere(be, FR.INF)
    close = FR.check_sphere(be, 0.3)
    assert close[1].sum() <= far[1].sum(), (close[1], far[1])
    # host and device: d_min within tol + eps of each other where both are below r_min
    so, T, C, v, L, _ = FR.sphere_case()
    h = host.field_clearance(so, T, C, FR.SPHERE_ORIGIN, FR.SPHERE_H, v, 0.3, FR.SPHERE_TOL)
    eps = np.array([FR.eps_of(FR.Row(so, T, C, b), FR.SPHERE_H, v, L) for b in range(len(so) - 1)])
    both = (h[0][:, 0] < 0.3) & (close[0][:, 0] < 0.3)
    assert both.sum() == 4 and np.array_equal(h[2] & SEP_CLOSE, close[2] & SEP_CLOSE)
    assert (np.abs(h[0][both, 0] - close[0][both, 0]) <= FR.SPHERE_TOL + eps[both]).all()


@pytest.mark.parametrize("given", [False, True])
def test_rough_field_is_sound(be, given):
    FR.check_rough(be, given)


def test_constant_field_costs_the_knots(be):
    FR.check_constant(be)


def test_degenerate_geometry(be):
    FR.check_degenerate(be)


def test_budget(be):
    FR.check_budget(be)


def test_unusable_rows(be):
    FR.check_unusable(be)


def test_arguments(be, solver):
    import torch
    FR.check_arguments(be, TgmsError, ERR_INVALID_ARG)
    so, T, C = FR.hover((0.5, 0.5, 0.5))
    dso, dT, dC, dv = _dev(so), _dev(T), _dev(C), _dev(np.zeros((3, 3, 3), np.float32))
    grid = ((0.0, 0.0, 0.0), 1.0, (3, 3, 3))
    evals = torch.full((1,), -2, dtype=torch.int32, device="cuda")
    with pytest.raises(TgmsError) as e:  # every output NULL
        solver.field_clearance_device(1, dso, dT, dC, *grid, dv, 0.0, 1.0, 1e-3, 100)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # values NULL
        solver.field_clearance_device(1, dso, dT, dC, *grid, None, 0.0, 1.0, 1e-3, 100, d_evals=evals)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # more than 2^31 - 1 nodes: refused before a value is read
        solver.field_clearance_device(1, dso, dT, dC, (0.0, 0.0, 0.0), 1.0, (2048, 2048, 512), dv, 0.0, 1.0, 1e-3, 100,
                                      d_evals=evals)
    assert e.value.status == ERR_INVALID_ARG
    solver.field_clearance_device(0, dso, dT, dC, *grid, dv, 0.0, 1.0, 1e-3, 100, d_evals=evals)  # B == 0: nothing launched
    torch.cuda.synchronize()
    assert evals.tolist() == [-2]
    solver.field_clearance_device(1, dso, dT, dC, *grid, dv, 0.0, float("inf"), 1e-3, 100, d_evals=evals)  # one output is enough
    torch.cuda.synchronize()
    assert evals.tolist() == [2]


def test_bad_segment_counts_read_nothing(solver):
    """A span of 0, of 17 and of -15 in the device offsets: those rows are flagged and nothing of
    them is read (their offsets point far outside the arrays); the others are the batch without them."""
    so, T, C, v, L, _ = FR.sphere_case()  # spans 1 2 2 3 1 4
    bad = np.array([0, 1, 1, 3, 6, 23, 8], dtype=np.int32)  # spans 1 0 2 3 17 -15
    near, evals, flags = Device(solver).field_clearance(bad, T, C, FR.SPHERE_ORIGIN, FR.SPHERE_H, v, 0.3, FR.SPHERE_TOL)
    for b in (1, 4, 5):
        assert flags[b] == SEP_NONFINITE and np.isnan(near[b]).all() and evals[b] == 0, (b, flags[b], near[b], evals[b])
    want = Device(solver).field_clearance(so, T, C, FR.SPHERE_ORIGIN, FR.SPHERE_H, v, 0.3, FR.SPHERE_TOL)
    assert np.array_equal(near[0], want[0][0]) and evals[0] == want[1][0] and flags[0] == want[2][0]  # the same row 0
    keep = np.array([0, 1, 3, 6], dtype=np.int32)  # rows 2 and 3 of the spoiled offsets as a batch of their own
    alone = Device(solver).field_clearance(keep[1:] - 1, T[1:6], C[1:6], FR.SPHERE_ORIGIN, FR.SPHERE_H, v, 0.3, FR.SPHERE_TOL)
    assert np.array_equal(near[2:4], alone[0]) and np.array_equal(evals[2:4], alone[1]) and np.array_equal(flags[2:4], alone[2])


def test_misaligned_arrays(solver):
    import torch
    so, T, C, v, _, _ = FR.sphere_case()
    B = len(so) - 1
    dso, dT, dC, dv = _dev(so), _dev(T), _dev(C), _dev(v)
    grid = (FR.SPHERE_ORIGIN, FR.SPHERE_H, v.shape[::-1])
    flags = torch.zeros(B, dtype=torch.int32, device="cuda")
    odd = torch.zeros(len(T) + 1, dtype=torch.float64, device="cuda")[1:]
    odd.copy_(dT)
    with pytest.raises(TgmsError) as e:
        solver.field_clearance_device(B, dso, odd, dC, *grid, dv, 1.8, 0.3, 1e-3, 1000, d_flags=flags)
    assert e.value.status == ERR_INVALID_ARG
    near = torch.zeros(2 * B + 1, dtype=torch.float64, device="cuda")[1:]
    with pytest.raises(TgmsError) as e:
        solver.field_clearance_device(B, dso, dT, dC, *grid, dv, 1.8, 0.3, 1e-3, 1000, d_near=near)
    assert e.value.status == ERR_INVALID_ARG
    odd_v = torch.zeros(4 * v.size + 4, dtype=torch.uint8, device="cuda")[1:4 * v.size + 1]  # not 4-byte aligned
    with pytest.raises(TgmsError) as e:
        solver.field_clearance_device(B, dso, dT, dC, *grid, odd_v, 1.8, 0.3, 1e-3, 1000, d_flags=flags)
    assert e.value.status == ERR_INVALID_ARG


def _affine_device(name):
    so, T, C, _ = FR.solved(name)
    return len(so) - 1, _dev(so), _dev(T), _dev(C)


def test_two_streams_on_one_handle(solver):
    """Two calls of one handle on two streams, the reduction on one (handle scratch) and a given
    bound on the other (none): each output is that of the call alone."""
    import torch
    d = Device(solver)
    v = FR.affine_field()
    grid = (FR.AFFINE_ORIGIN, FR.AFFINE_H, v.shape[::-1])
    L = float(np.linalg.norm(FR.AFFINE_N))
    cases = [("rest", 0.0), ("ragged65", L), ("end_derivs", 0.0)]
    want = [d.field_clearance(*FR.solved(n)[:3], FR.AFFINE_ORIGIN, FR.AFFINE_H, v, 1.0, 1e-2, lip=lip) for n, lip in cases]
    dv = _dev(v)
    args = [_affine_device(n) for n, _ in cases]
    outs = [_outs(a[0]) for a in args]
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for a, o, st, (_, lip) in zip(args, outs, streams, cases):
        solver.field_clearance_device(*a, *grid, dv, lip, 1.0, 1e-2, 1 << 20, *o, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        for x, y in zip(o, w):
            assert np.array_equal(x.cpu().numpy(), y)


def test_captured_graph_with_a_given_bound(solver):
    """The call with lip > 0 is one launch without handle scratch: captured, replayed twice, and
    equal to the eager result each time."""
    import torch
    v = FR.affine_field()
    grid = (FR.AFFINE_ORIGIN, FR.AFFINE_H, v.shape[::-1])
    L = float(np.linalg.norm(FR.AFFINE_N))
    B, dso, dT, dC = _affine_device("ragged65")
    dv = _dev(v)
    eager, outs = _outs(B), _outs(B)
    solver.field_clearance_device(B, dso, dT, dC, *grid, dv, L, 1.0, 1e-2, 1 << 20, *eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        solver.field_clearance_device(B, dso, dT, dC, *grid, dv, L, 1.0, 1e-2, 1 << 20, *outs, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        outs[0].fill_(float("nan"))
        outs[1].fill_(-2)
        outs[2].fill_(-2)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(outs, eager):
            assert torch.equal(x, y)
    assert (eager[1] > 0).all()
    del g


def test_capturing_the_reduction_is_unsupported(solver):
    import torch
    v = FR.affine_field()
    grid = (FR.AFFINE_ORIGIN, FR.AFFINE_H, v.shape[::-1])
    B, dso, dT, dC = _affine_device("ragged65")
    dv = _dev(v)
    outs = _outs(B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.field_clearance_device(B, dso, dT, dC, *grid, dv, 0.0, 1.0, 1e-2, 1 << 20, *outs, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- checked below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert isinstance(err, TgmsError) and err.status == ERR_UNSUPPORTED, err
    del g
    solver.field_clearance_device(B, dso, dT, dC, *grid, dv, 0.0, 1.0, 1e-2, 1 << 20, *outs)  # the handle still works
    torch.cuda.synchronize()
    assert (outs[1].cpu().numpy() >= np.diff(FR.solved("ragged65")[0]) + 1).all()


def test_multi_handle_runs_on_device_0(solver):
    from trajectory_generator_ros2_amd.solver import Solver
    so, T, C, v, _, _ = FR.sphere_case()
    a = (so, T, C, FR.SPHERE_ORIGIN, FR.SPHERE_H, v, 0.3, FR.SPHERE_TOL)
    want = solver.field_clearance(*a)
    with Solver(device_count=1) as m:
        got = m.field_clearance(*a)
        dgot = Device(m).field_clearance(*a)
    for w, g, d in zip(want, got, dgot):
        assert np.array_equal(w, g) and np.array_equal(w, d)


def test_host_handle_device_call_is_unsupported(host):
    so, T, C = FR.hover((0.5, 0.5, 0.5))
    with pytest.raises(TgmsError) as e:
        host.field_clearance_device(1, so, T, C, (0.0, 0.0, 0.0), 1.0, (3, 3, 3), np.zeros((3, 3, 3), np.float32), 0.0, 1.0,
                                    1e-3, 100, d_evals=np.zeros(1, np.int32))
    assert e.value.status == ERR_UNSUPPORTED
