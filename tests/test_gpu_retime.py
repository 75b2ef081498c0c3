"""GPU: the segment re-timing (tgms_retime_batch_dev / tgms_retime_batch on a GPU handle,
csrc/tgms_retime.hip): the checks of test_retime_host.py repeated on the device, agreement with
the host backend, and the launch's corners: tiles of four trajectories per wavefront, the
grid-stride loop, bad rows and bad spans in the middle of a tile, in place, NULL outputs, graph
capture."""
import numpy as np
import pytest

import retime_ref as RR
from retime_ref import NONFINITE
from test_retime_host import (S_HI, _limits, _raw_b, check_bad_arguments, check_bad_rows, check_constant,
                              check_fixed_point, check_in_place_repeat_and_null, check_permutation, check_public_calls,
                              check_reference, check_seams, check_straight, check_translation, raw_call, same)

pytestmark = pytest.mark.gpu

GRID = 4096  # workgroups of the launch at most (csrc/tgms_retime.hip launch_retime)
TILE = 4     # trajectories per workgroup


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the fixtures are read-only


def _outputs(B, S, dT, want, in_place):
    import torch
    f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    return [(dT if in_place else f64(S)) if want[0] else None, f64(S, 4) if want[1] else None,
            f64(B, 3) if want[2] else None, torch.full((B,), -9, dtype=torch.int32, device="cuda") if want[3] else None]


def device_call(solver):
    """tgms_retime_batch_dev on fresh NaN / -9 outputs (those of `want`); numpy results."""
    def call(so, T, C, lim, s_lo, s_hi, want=(1, 1, 1, 1), in_place=False, so_dev=None):
        import torch
        so = np.asarray(so, np.int32)
        B, S = len(so) - 1, len(np.asarray(T).reshape(-1))
        dso, dT = _dev(so if so_dev is None else so_dev), _dev(np.asarray(T, np.float64).reshape(-1))
        dC = _dev(np.asarray(C, np.float64).reshape(-1, 3, 8))
        outs = _outputs(B, S, dT, want, in_place)
        solver.retime_device(B, dso, dT, dC, _limits(lim), s_lo, s_hi, *outs)
        torch.cuda.synchronize()
        return tuple(None if o is None else o.cpu().numpy() for o in outs)
    return call


def staged_call(solver):
    """tgms_retime_batch on the GPU handle: one upload, the launch, one download."""
    def call(so, T, C, lim, s_lo, s_hi, want=(1, 1, 1, 1), in_place=False):
        st, outs = raw_call(solver, so, T, C, lim, s_lo, s_hi, want, in_place)
        assert st == 0, solver.last_error()
        return outs
    return call


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.mark.parametrize("s_lo", [1.0, 0.8])
@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_against_the_reference_and_the_host(solver, host, name, s_lo):
    """The reference's tolerances on the device's output, then the host backend on the same input:
    peaks within 2e-9 relative of each other (each within 1e-9 of the truth), the staged call
    bit-equal to the device call."""
    check_reference(device_call(solver), name, s_lo)
    c = RR.cases()[name]
    args = (c["so"], c["T"], c["C"], c["lim"], s_lo, S_HI)
    dev, hst = device_call(solver)(*args), raw_call(host, *args)[1]
    for d, h in zip(dev[:3], hst[:3]):
        assert (np.abs(d - h) <= 2e-9 * np.abs(h)).all()
    print("%s s_lo=%g: device and host bit-equal %s" % (name, s_lo, same(dev, hst)))
    assert same(dev, staged_call(solver)(*args))


@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_against_bounds_and_dilate(solver, name):
    check_public_calls(device_call(solver), solver, name)


def test_exact_cases(solver):
    check_straight(device_call(solver))
    check_constant(device_call(solver))
    check_straight(staged_call(solver))
    for name in ("ragged48", "zoo"):
        check_translation(device_call(solver), name)


def test_permutation_and_batch_sizes(solver):
    check_permutation(device_call(solver))
    check_seams(device_call(solver))
    check_seams(staged_call(solver), Bs=(5,))


def test_grid_stride(solver):
    """More tiles than workgroups, the last tile partial: 4 * 4096 + 5 one-segment trajectories (the
    fixed-point batch's shapes repeated); every row equals the row of a 37-trajectory call."""
    so1, T1, C1 = (np.arange(38, dtype=np.int32),) + _m1_batch()
    lim = (1.5, 3.0, 30.0)
    small = device_call(solver)(so1, T1, C1, lim, 0.5, 2.0)
    B = TILE * GRID + 5
    rows = np.arange(B) % 37
    big = device_call(solver)(np.arange(B + 1, dtype=np.int32), T1[rows], C1[rows], lim, 0.5, 2.0)
    assert same([x[rows] for x in small], big)


def _m1_batch():
    rng = np.random.default_rng(11)
    d = rng.uniform(-4.0, 4.0, (37, 3))
    T = np.linalg.norm(d, axis=1) * rng.uniform(0.6, 3.0, 37)
    C = np.zeros((37, 3, 8))
    for j, k in ((4, 35.0), (5, -84.0), (6, 70.0), (7, -20.0)):  # bounds_ref.rest_to_rest on every axis
        C[:, :, j] = d * k / T[:, None] ** j
    return T, C


def test_bad_rows_and_bad_spans(solver):
    """check_bad_rows, then offsets with a span of 0 and one of 17 segments in the middle of a tile:
    FEAS_NONFINITE alone and a NaN record for those, nothing written for their segments, the other
    trajectories bit-identical to a batch without them."""
    check_bad_rows(device_call(solver))
    c = RR.cases()["ragged48"]
    so, T, C, lim = c["so"], c["T"], c["C"], c["lim"]
    S, Ms = int(so[-1]), np.diff(so)
    k = next(k for k in range(2, 47) if Ms[k] + Ms[k + 1] == 17)  # trajectories k and k + 1 merged: a span of 17
    # an empty span after trajectory 0, which moves every later trajectory up by one
    so_bad = np.concatenate([so[:2], [so[1]], so[2:k + 1], so[k + 2:]]).astype(np.int32)
    bad = [1, k + 1]
    assert np.diff(so_bad)[bad].tolist() == [0, 17] and len(so_bad) == len(so)
    T_out, seg_rec, rec, flags = device_call(solver)(so, T, C, lim, 0.8, S_HI, so_dev=so_bad)
    assert (flags[bad] == NONFINITE).all() and np.isnan(rec[bad]).all()
    skipped = np.arange(so[k], so[k + 2])
    assert np.isnan(T_out[skipped]).all() and np.isnan(seg_rec[skipped]).all()  # the sentinels: nothing written
    clean = device_call(solver)(so, T, C, lim, 0.8, S_HI)
    keep_new = [b for b in range(48) if b not in bad]
    keep_old = [b for b in range(48) if b not in (k, k + 1)]
    segs = np.setdiff1d(np.arange(S), skipped)
    assert same((clean[0][segs], clean[1][segs], clean[2][keep_old], clean[3][keep_old]),
                (T_out[segs], seg_rec[segs], rec[keep_new], flags[keep_new]))


@pytest.mark.parametrize("name", ["ragged48", "zoo"])
def test_in_place_repeat_and_null_outputs(solver, name):
    check_in_place_repeat_and_null(device_call(solver), name)


def test_fixed_point_for_one_segment(solver):
    check_fixed_point(device_call(solver), solver)


def test_bad_arguments(solver):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, TgmsError
    so, T, C = RR.knot_peak(2)
    dso, dT, dC = _dev(so), _dev(T), _dev(C)

    def status_of(lim, s_lo, s_hi, want=(1, 1, 1, 1), B=None):
        outs = _outputs(1, 2, dT, want, False)
        try:
            solver.retime_device(1 if B is None else B, dso, dT, dC, _limits(lim), s_lo, s_hi, *outs)
        except TgmsError as e:
            return e.status
        torch.cuda.synchronize()
        return 0
    check_bad_arguments(status_of)
    check_bad_arguments(lambda lim, s_lo, s_hi, want=(1, 1, 1, 1), B=None:  # the staged call on the GPU handle
                        raw_call(solver, so, T, C, lim, s_lo, s_hi, want)[0] if B is None else _raw_b(solver, B))
    odd = torch.zeros(2 * 4 + 1, dtype=torch.float64, device="cuda")[1:]  # 8 bytes past a 16-byte boundary
    for kw in (dict(d_seg_times_out=odd[:2]), dict(d_seg_rec=odd), dict(d_rec=odd[:3])):
        with pytest.raises(TgmsError) as e:
            solver.retime_device(1, dso, dT, dC, _limits((1.0, 1.0, 1.0)), 1.0, 2.0, **kw)
        assert e.value.status == ERR_INVALID_ARG and "16-byte" in str(e.value)


def test_graph_capture(solver):
    """One kernel, no plan, no scratch: the call on a ragged batch is captured with torch.cuda.graph on
    a single stream, and one replay gives the bits of the uncaptured call."""
    import torch
    c = RR.cases()["ragged48"]
    so, T, C, lim = c["so"], c["T"], c["C"], _limits(c["lim"])
    B, S = len(so) - 1, len(T)
    want = device_call(solver)(so, T, C, c["lim"], 0.8, S_HI)
    dso, dT, dC = _dev(so), _dev(T), _dev(C)
    outs = _outputs(B, S, dT, (1, 1, 1, 1), False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        try:
            solver.retime_device(B, dso, dT, dC, lim, 0.8, S_HI, *outs, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same(want, tuple(o.cpu().numpy() for o in outs))
    del graph
