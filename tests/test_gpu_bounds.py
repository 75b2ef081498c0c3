"""GPU: the continuous feasibility bounds (tgms_bounds_batch / tgms_bounds_batch_device,
csrc/tgms_bounds.hip): closed-form answers, the 1e-9 contract of include/tgms.h against the
independent reference of bounds_ref.py, agreement with the host backend, and the launch's
corners: tiles of four trajectories per wavefront, the grid-stride loop, bad offsets, flags,
argument errors, graph capture."""
import numpy as np
import pytest

import bounds_ref as R
from extrema_ref import durations

pytestmark = pytest.mark.gpu

GRID = 4096  # workgroups of the launch at most (csrc/tgms_bounds.hip launch_bounds)
TILE = 4     # trajectories per workgroup


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device_call(solver, so, T, C, limits=None, ext=True, flags=True):
    """tgms_bounds_batch_device on fresh NaN / -1 outputs; returns numpy (ext, flags)."""
    import torch
    B = len(so) - 1
    d_ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda") if ext else None
    d_fl = torch.full((B,), -1, dtype=torch.int32, device="cuda") if flags else None
    solver.bounds_device(B, _dev(np.asarray(so, np.int32)), _dev(np.asarray(T, np.float64).reshape(-1)),
                         _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)), limits, d_ext, d_fl)
    torch.cuda.synchronize()
    return (d_ext.cpu().numpy() if ext else None), (d_fl.cpu().numpy() if flags else None)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ragged(solver):
    """The 48-trajectory batch (every M in 1..16 three times), solved on the GPU, and its
    device records without limits.  Shared, never modified."""
    so, W, T = R.ragged48()
    C, st, worst = solver.solve(so, W, T)
    assert worst == 0 and not st.any()
    ext, fl = _device_call(solver, so, T, C)
    return dict(so=so, W=W, T=T, C=C, ext=ext, fl=fl)


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_known_answer_rest_to_rest(solver, T):
    p0, d = np.array([0.3, -1.0, 2.0]), -1.7
    so, Ts, C, peaks = R.rest_to_rest(p0, d, T, axis=1)
    ext, flags = _device_call(solver, so, Ts, C)
    assert flags[0] == 0
    assert (np.abs(ext[0, 6:9] - peaks) <= 1e-12 * peaks).all(), (ext[0, 6:9] - peaks) / peaks
    lo, hi = p0.copy(), p0.copy()
    lo[1] += d
    assert np.abs(ext[0, 0:3] - lo).max() <= 1e-12 * np.abs(lo).max()
    assert np.abs(ext[0, 3:6] - hi).max() <= 1e-12 * np.abs(hi).max()
    assert np.array_equal(ext[0, [0, 2, 3, 5]], p0[[0, 2, 0, 2]]) and ext[0, 4] == p0[1] and ext[0, 9] == T


def test_constructed_overshoot_and_constant(solver):
    so, T, C, pmin, pmax = R.overshoot()
    ext, flags = _device_call(solver, so, T, C)
    tol = 1e-12 * max(np.abs(pmin).max(), np.abs(pmax).max())
    assert flags[0] == 0
    assert np.abs(ext[0, 0:3] - pmin).max() <= tol and np.abs(ext[0, 3:6] - pmax).max() <= tol
    C0 = np.zeros((3, 3, 8))
    C0[:, :, 0] = [0.1, -2.7, 3.3]
    ext, flags = _device_call(solver, [0, 3], [0.5, 2.0, 7.0], C0)
    assert flags[0] == 0 and (ext[0, 6:9] == 0.0).all() and ext[0, 9] == (0.5 + 2.0) + 7.0
    assert np.array_equal(ext[0, 0:3], C0[0, :, 0]) and np.array_equal(ext[0, 3:6], C0[0, :, 0])


def test_sees_what_a_coarse_dt_misses(solver):
    from trajectory_generator_ros2_amd import FEAS_SPEED, Limits
    p0, d, T = np.array([0.3, -1.0, 2.0]), 1.7, 1.0
    so, Ts, C, peaks = R.rest_to_rest(p0, d, T, axis=0)
    lim = Limits(v_max=abs(d) / T)
    ext_s, fl_s = solver.extrema(so, np.array([p0, p0 + [d, 0.0, 0.0]]), Ts, None, C, 2 * T, lim)
    assert ext_s[0, 6] == 0.0 and fl_s[0] == 0
    assert _device_call(solver, so, Ts, C, lim)[1][0] == FEAS_SPEED


def test_ragged_batches_meet_the_contract(solver, host, ragged):
    """Rest to rest and with non-zero end derivatives: within 1e-9 of the reference, within 2e-9
    of the host backend (both meet 1e-9), durations bit-equal to the sampled check's."""
    r = ragged
    C_ed, st, worst = solver.solve(r["so"], r["W"], r["T"], R.end_derivs48())
    assert worst == 0
    for C, ext in ((r["C"], r["ext"]), (C_ed, _device_call(solver, r["so"], r["T"], C_ed)[0])):
        R.check_contract(ext, R.records(r["so"], r["T"], C))
        assert np.array_equal(ext[:, 9].view(np.int64), durations(r["so"], r["T"]).view(np.int64))
        ext_h = host.bounds(r["so"], r["T"], C)[0]
        R.check_contract(ext, ext_h[:, 0:9], tol=2e-9)
    assert not r["fl"].any()


def test_edge_shapes(solver, host):
    """B = 1 with M = 1 and with M = 16; one trajectory mixing T = 0.05 and T = 20 (against the
    reference); B = 65 x M = 16: 17 tiles, the last one a single trajectory past sixteen full
    wavefronts of segments (against the host backend, which the CPU tests hold to the
    reference)."""
    from trajectory_generator_ros2_amd import synthetic as S
    rng = np.random.default_rng(7)
    for Ts in ([1.3], list(rng.uniform(0.5, 3.0, 16)), [0.05, 20.0, 0.05, 20.0, 3.0]):
        so = np.array([0, len(Ts)], np.int32)
        n = len(Ts) + 1
        W = np.c_[rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(0.5, 5, n)]
        C, st, worst = solver.solve(so, W, Ts)
        assert worst == 0
        ext, fl = _device_call(solver, so, Ts, C)
        assert fl[0] == 0
        R.check_contract(ext, R.records(so, Ts, C))
    so, W, T = S.uniform_batch(65, 16, seed=8)
    C, st, worst = solver.solve(so, W.reshape(-1, 3), T.reshape(-1))
    assert worst == 0
    ext, fl = _device_call(solver, so, T, C)
    assert not fl.any()
    R.check_contract(ext, host.bounds(so, T, C)[0][:, 0:9], tol=2e-9)


def test_grid_stride_and_lds_reuse(solver, ragged):
    """The launch uses min(ceil(B / 4), 4096) workgroups of one wavefront, each taking tiles of 4
    consecutive trajectories by grid-stride.  684 copies of the 48-trajectory batch are
    B = 32,832 > 2 * 4096 * 4 trajectories: every workgroup runs a third tile on the LDS its
    first two used.  Every copy's records and flags are bit-equal to the first copy's."""
    from trajectory_generator_ros2_amd import Limits
    r = ragged
    n = 684
    B = 48 * n
    assert B > 2 * GRID * TILE
    S = int(r["so"][-1])
    so = np.concatenate([[0], (r["so"][1:][None, :] + S * np.arange(n)[:, None]).reshape(-1)]).astype(np.int32)
    lim = Limits(v_max=np.median(r["ext"][:, 6]), pmax=[4.0, 4.0, 4.5])
    ext1, fl1 = _device_call(solver, r["so"], r["T"], r["C"], lim)
    assert fl1.any() and not fl1.all()
    ext, fl = _device_call(solver, so, np.tile(r["T"], n), np.tile(r["C"], (n, 1, 1)), lim)
    assert np.array_equal(ext.reshape(n, 48, 10).view(np.int64), np.broadcast_to(ext1.view(np.int64), (n, 48, 10)))
    assert np.array_equal(fl.reshape(n, 48), np.broadcast_to(fl1, (n, 48)))
    assert np.array_equal(ext1.view(np.int64), r["ext"].view(np.int64))


def test_flags(solver, ragged):
    """Each bit set alone by a limit one ulp below the stored value and cleared by one equal to
    it; either output alone; no limits and +-inf limits flag nothing."""
    from trajectory_generator_ros2_amd import FEAS_ACCEL, FEAS_BOX, FEAS_JERK, FEAS_SPEED, Limits
    r = ragged
    ext = r["ext"]
    call = lambda lim, **kw: _device_call(solver, r["so"], r["T"], r["C"], lim, **kw)
    lo, hi = ext[:, 0:3].min(axis=0), ext[:, 3:6].max(axis=0)
    top = dict(v_max=ext[:, 6].max(), a_max=ext[:, 7].max(), j_max=ext[:, 8].max())
    e2, fl = call(Limits(pmin=lo, pmax=hi, **top))  # every limit equal to the extreme value: inside
    assert not fl.any() and np.array_equal(e2.view(np.int64), ext.view(np.int64))
    for col, bit, name in ((6, FEAS_SPEED, "v_max"), (7, FEAS_ACCEL, "a_max"), (8, FEAS_JERK, "j_max")):
        kw = dict(top)
        kw[name] = np.nextafter(top[name], 0.0)
        fl = call(Limits(pmin=lo, pmax=hi, **kw))[1]
        assert np.array_equal(fl, np.where(ext[:, col] == top[name], bit, 0))
    for face in range(6):
        lim = Limits(pmin=lo, pmax=hi, **top)
        if face < 3:
            lim.pmin[face] = np.nextafter(lo[face], np.inf)
            want = ext[:, face] < lim.pmin[face]
        else:
            lim.pmax[face - 3] = np.nextafter(hi[face - 3], -np.inf)
            want = ext[:, face] > lim.pmax[face - 3]
        assert want.sum() >= 1 and np.array_equal(call(lim)[1], np.where(want, FEAS_BOX, 0))
    assert not r["fl"].any() and not call(Limits())[1].any()
    lim = Limits(v_max=np.median(ext[:, 6]), pmax=[4.0, 4.0, 4.5])
    fl = call(lim)[1]
    assert np.array_equal((fl & FEAS_SPEED) != 0, ext[:, 6] > lim.v_max) and (fl & FEAS_BOX).any()
    assert np.array_equal(call(lim, ext=False)[1], fl)
    assert np.array_equal(call(lim, flags=False)[0].view(np.int64), ext.view(np.int64))


def test_nonfinite_input_and_bad_offsets(solver, ragged):
    from trajectory_generator_ros2_amd import FEAS_NONFINITE, Limits
    r = ragged
    so, T, C, ext = r["so"], r["T"], r["C"], r["ext"]
    lim = Limits(v_max=np.median(ext[:, 6]))
    fl0 = _device_call(solver, so, T, C, lim)[1]
    C2, T2 = C.copy(), T.copy()
    C2[so[3], 1, 4] = np.nan       # a NaN coefficient in trajectory 3
    T2[so[20]] = np.nan            # a NaN time in trajectory 20
    T2[so[42] - 1] = 0.0           # a zero time in trajectory 41
    T2[so[30]] = -1.0              # a negative time in trajectory 30
    ext2, fl = _device_call(solver, so, T2, C2, lim)
    bad = [3, 20, 30, 41]
    keep = np.ones(len(fl), bool)
    keep[bad] = False
    assert (fl[bad] == FEAS_NONFINITE).all() and np.isnan(ext2[bad]).all()
    assert np.array_equal(fl[keep], fl0[keep])
    assert np.array_equal(ext2[keep].view(np.int64), ext[keep].view(np.int64))
    # device offsets with M = 0 (trajectory 1) and M = 17 (trajectory 3) between trajectories
    # 0, 1, 2 of the batch: nothing is read for the two, the others are as before
    M = np.diff(so)[:3]
    so2 = np.cumsum([0, M[0], 0, M[1], 17, M[2]]).astype(np.int32)
    T3, C3 = np.full(so2[-1], 1.0), np.full((so2[-1], 3, 8), 0.5)
    for src, dst in ((0, 0), (1, 2), (2, 4)):
        T3[so2[dst]:so2[dst + 1]] = T[so[src]:so[src + 1]]
        C3[so2[dst]:so2[dst + 1]] = C[so[src]:so[src + 1]]
    ext3, fl3 = _device_call(solver, so2, T3, C3, lim)
    assert list(fl3[[1, 3]]) == [FEAS_NONFINITE] * 2 and np.isnan(ext3[[1, 3]]).all()
    assert np.array_equal(fl3[[0, 2, 4]], fl0[:3])
    assert np.array_equal(ext3[[0, 2, 4]].view(np.int64), ext[:3].view(np.int64))


def test_argument_errors_launch_nothing(solver, ragged):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, Limits, TgmsError
    r = ragged
    B = len(r["so"]) - 1
    dso, dT, dC = _dev(r["so"]), _dev(r["T"]), _dev(r["C"])
    odd = torch.full((B * 10 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    for kw in (dict(d_extrema=odd, d_flags=fl), dict(limits=Limits(a_max=float("nan")), d_extrema=ext, d_flags=fl),
               dict(limits=Limits(pmin=[0, 0, 1], pmax=[1, 1, 0]), d_extrema=ext, d_flags=fl),
               dict(d_extrema=None, d_flags=None)):
        with pytest.raises(TgmsError) as e:
            solver.bounds_device(B, dso, dT, dC, **kw)
        assert e.value.status == ERR_INVALID_ARG
    solver.bounds_device(0, None, None, None, d_extrema=ext, d_flags=fl)  # B == 0: TGMS_OK, nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all()) and bool(torch.isnan(ext).all()) and bool((fl == -1).all())


def test_host_pointer_call_gives_the_device_call_bits(solver, ragged):
    from trajectory_generator_ros2_amd import Limits
    r = ragged
    lim = Limits(v_max=np.median(r["ext"][:, 6]))
    ext_h, fl_h = solver.bounds(r["so"], r["T"], r["C"], lim)
    ext_d, fl_d = _device_call(solver, r["so"], r["T"], r["C"], lim)
    assert np.array_equal(ext_h.view(np.int64), ext_d.view(np.int64)) and np.array_equal(fl_h, fl_d)
    assert fl_d.any()


def test_captured_into_a_graph_and_replayed(solver, ragged):
    """The device call on the ragged batch inside torch.cuda.graph (test_gpu_extrema.py's
    pattern), replayed twice with the coefficients changed in place between the replays: each
    replay is bit-equal to the direct call on the coefficients it saw."""
    import torch
    from trajectory_generator_ros2_amd import Limits
    r = ragged
    B = len(r["so"]) - 1
    lim = Limits(v_max=np.median(r["ext"][:, 6]))
    C_b = r["C"] * np.linspace(0.5, 2.0, 8)  # another polynomial per segment
    want = [_device_call(solver, r["so"], r["T"], C, lim) for C in (r["C"], C_b)]
    assert not np.array_equal(want[0][0], want[1][0])
    dso, dT, dC = _dev(r["so"]), _dev(r["T"]), _dev(r["C"])
    ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.bounds_device(B, dso, dT, dC, lim, ext, fl, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for C, (ext0, fl0) in zip((r["C"], C_b), want):
        dC.copy_(_dev(C))
        ext.fill_(float("nan"))
        fl.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ext.cpu().numpy().view(np.int64), ext0.view(np.int64))
        assert np.array_equal(fl.cpu().numpy(), fl0)
    del g
