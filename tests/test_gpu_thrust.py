"""GPU: the continuous thrust and tilt bounds (tgms_thrust_batch / tgms_thrust_batch_device,
csrc/tgms_thrust.hip): the closed forms and the 1e-9 contract of test_thrust_host.py repeated on
the device, agreement with the host backend, and the launch's corners: tiles of four
trajectories per wavefront, the grid-stride loop, bad rows in the middle of a tile, limits,
argument errors, graph capture, and what a coarse dt misses."""
import numpy as np
import pytest

import bounds_ref as R
import thrust_ref as TR
from test_thrust_host import check_constant, check_horizontal, check_vertical

pytestmark = pytest.mark.gpu

G = TR.G0
GRID = 4096  # workgroups of the launch at most (csrc/tgms_thrust.hip launch_thrust)
TILE = 4     # trajectories per workgroup


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the fixtures are read-only


def _device_call(solver, so, T, C, limits=None, g=G, rec=True, flags=True):
    """tgms_thrust_batch_device on fresh NaN / -1 outputs; returns numpy (rec, flags)."""
    import torch
    B = len(so) - 1
    d_rec = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda") if rec else None
    d_fl = torch.full((B,), -1, dtype=torch.int32, device="cuda") if flags else None
    solver.thrust_device(B, _dev(np.asarray(so, np.int32)), _dev(np.asarray(T, np.float64).reshape(-1)),
                         _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)), g, limits, d_rec, d_fl)
    torch.cuda.synchronize()
    return (d_rec.cpu().numpy() if rec else None), (d_fl.cpu().numpy() if flags else None)


def _call(solver):
    return lambda so, T, C, limits=None: _device_call(solver, so, T, C, limits)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ragged(solver):
    """bounds_ref.ragged48 solved on the GPU, rest to rest (C) and with end_derivs48 (C_ed), and
    the device records of C without limits.  Shared, never modified."""
    so, W, T = R.ragged48()
    C, st, worst = solver.solve(so, W, T)
    assert worst == 0 and not st.any()
    C_ed, st, worst = solver.solve(so, W, T, R.end_derivs48())
    assert worst == 0
    rec, fl = _device_call(solver, so, T, C)
    for a in (C, C_ed, rec, fl):
        a.setflags(write=False)
    return dict(so=so, W=W, T=T, C=C, C_ed=C_ed, rec=rec, fl=fl)


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_horizontal_rest_to_rest(solver, T):
    check_horizontal(_call(solver), T)


def test_vertical_rest_to_rest(solver):
    check_vertical(_call(solver))


def test_constant_trajectory(solver):
    check_constant(_call(solver))


def test_ragged_batches_meet_the_contract(solver, host, ragged):
    """Rest to rest and with end derivatives: within 1e-9 of the reference, within 2e-9 of the
    host backend, the times in [0, D_b] and attaining the stored values, no flags."""
    r = ragged
    for C, rec in ((r["C"], r["rec"]), (r["C_ed"], _device_call(solver, r["so"], r["T"], r["C_ed"])[0])):
        ref = TR.records(r["so"], r["T"], C)
        TR.check_contract(rec, ref)
        TR.check_times(r["so"], r["T"], C, rec, ref)
        rec_h, fl_h = host.thrust(r["so"], r["T"], C)
        TR.check_contract(rec, rec_h[:, [0, 2, 4]], tol=2e-9)
        assert not fl_h.any()
    assert not r["fl"].any()


def test_edge_shapes(solver, host):
    """B = 1 with M = 1 and with M = 16; one trajectory mixing T = 0.05 and T = 20 (against the
    reference); B = 65 x M = 16: 17 tiles, the last one a single trajectory (against the host
    backend, which the CPU tests hold to the reference)."""
    from trajectory_generator_ros2_amd import synthetic as S
    rng = np.random.default_rng(7)
    for Ts in ([1.3], list(rng.uniform(0.5, 3.0, 16)), [0.05, 20.0, 0.05, 20.0, 3.0]):
        so = np.array([0, len(Ts)], np.int32)
        n = len(Ts) + 1
        W = np.c_[rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(0.5, 5, n)]
        C, st, worst = solver.solve(so, W, Ts)
        assert worst == 0
        rec, fl = _device_call(solver, so, Ts, C)
        assert fl[0] == 0
        ref = TR.records(so, Ts, C)
        TR.check_contract(rec, ref)
        TR.check_times(so, Ts, C, rec, ref)
    so, W, T = S.uniform_batch(65, 16, seed=8)
    C, st, worst = solver.solve(so, W.reshape(-1, 3), T.reshape(-1))
    assert worst == 0
    rec, fl = _device_call(solver, so, T, C)
    assert not fl.any()
    TR.check_contract(rec, host.thrust(so, T, C)[0][:, [0, 2, 4]], tol=2e-9)


def test_grid_stride_and_lds_reuse(solver, ragged):
    """B = 4 * 4096 + 5 rows repeating the 48: every workgroup runs a second tile on the LDS its
    first used, five rows more start a third round, and the last tile holds one row.  Every row
    is bit-equal to its original from the 48-row call."""
    from trajectory_generator_ros2_amd import ThrustLimits
    r = ragged
    B = TILE * GRID + 5
    src = np.arange(B) % 48
    M = np.diff(r["so"])[src]
    so = np.concatenate([[0], np.cumsum(M)]).astype(np.int32)
    seg = np.concatenate([np.arange(r["so"][b], r["so"][b + 1]) for b in range(48)] * (B // 48 + 1))[:so[-1]]
    assert np.array_equal(np.diff(r["so"])[src], np.diff(so)) and len(seg) == so[-1]
    lim = ThrustLimits(np.median(r["rec"][:, 0]), np.median(r["rec"][:, 2]), np.median(r["rec"][:, 4]))
    rec1, fl1 = _device_call(solver, r["so"], r["T"], r["C"], lim)
    assert fl1.any() and not fl1.all()
    assert np.array_equal(_bits(rec1), _bits(r["rec"]))
    rec, fl = _device_call(solver, so, r["T"][seg], r["C"][seg], lim)
    assert np.array_equal(_bits(rec), _bits(rec1[src])) and np.array_equal(fl, fl1[src])


def test_bad_rows_in_the_middle_of_a_tile(solver, ragged):
    """M = 0 and M = 17 from the offsets, a NaN coefficient, a time of 0 and of -1: each such row
    has NONFINITE alone and an all-NaN record, every other row is bit-equal to the clean
    batch's."""
    from trajectory_generator_ros2_amd import FEAS_NONFINITE, ThrustLimits
    r = ragged
    so, T, C, rec0 = r["so"], r["T"], r["C"], r["rec"]
    lim = ThrustLimits(tilt_max=np.median(rec0[:, 4]))
    fl0 = _device_call(solver, so, T, C, lim)[1]
    assert fl0.any()
    C2, T2 = C.copy(), T.copy()
    C2[so[5] + 0, 1, 4] = np.nan   # rows 5, 22, 30 and 41 are second or third in their tiles
    T2[so[23] - 1] = 0.0
    T2[so[30]] = -1.0
    T2[so[41]] = np.nan
    rec, fl = _device_call(solver, so, T2, C2, lim)
    bad = [5, 22, 30, 41]
    keep = np.ones(len(fl), bool)
    keep[bad] = False
    assert (fl[bad] == FEAS_NONFINITE).all() and np.isnan(rec[bad]).all()
    assert np.array_equal(fl[keep], fl0[keep]) and np.array_equal(_bits(rec[keep]), _bits(rec0[keep]))
    # device offsets with M = 0 (row 1) and M = 17 (row 2) inside the first tile, between rows
    # 0 and 1 of the batch; rows 2.. of the batch follow
    M = np.diff(so)
    so2 = np.cumsum(np.concatenate([[0, M[0], 0, 17], M[1:]])).astype(np.int32)
    T3, C3 = np.full(so2[-1], 1.0), np.full((so2[-1], 3, 8), 0.5)
    T3[:M[0]], C3[:M[0]] = T[:M[0]], C[:M[0]]
    T3[so2[3]:], C3[so2[3]:] = T[M[0]:], C[M[0]:]
    rec3, fl3 = _device_call(solver, so2, T3, C3, lim)
    assert list(fl3[[1, 2]]) == [FEAS_NONFINITE] * 2 and np.isnan(rec3[[1, 2]]).all()
    rest = np.r_[0, 3:len(fl3)]
    assert np.array_equal(fl3[rest], fl0) and np.array_equal(_bits(rec3[rest]), _bits(rec0))


def test_limits(solver, ragged):
    """A limit equal to the stored value raises no flag, nextafter past it raises it, infinite
    entries are unchecked; either output alone."""
    from trajectory_generator_ros2_amd import THRUST_HIGH, THRUST_LOW, THRUST_TILT, ThrustLimits
    r = ragged
    rec = r["rec"]
    call = lambda lim, **kw: _device_call(solver, r["so"], r["T"], r["C"], lim, **kw)
    lo, hi, tilt = rec[:, 0].min(), rec[:, 2].max(), rec[:, 4].max()
    rec2, fl = call(ThrustLimits(lo, hi, tilt))
    assert not fl.any() and np.array_equal(_bits(rec2), _bits(rec))
    assert np.array_equal(call(ThrustLimits(np.nextafter(lo, np.inf), hi, tilt))[1],
                          np.where(rec[:, 0] == lo, THRUST_LOW, 0))
    assert np.array_equal(call(ThrustLimits(lo, np.nextafter(hi, 0.0), tilt))[1],
                          np.where(rec[:, 2] == hi, THRUST_HIGH, 0))
    assert np.array_equal(call(ThrustLimits(lo, hi, np.nextafter(tilt, 0.0)))[1],
                          np.where(rec[:, 4] == tilt, THRUST_TILT, 0))
    inf = float("inf")
    for lim in (None, ThrustLimits(), ThrustLimits(-inf, inf, inf), ThrustLimits(inf, -inf, -inf)):
        assert not call(lim)[1].any()
    lim = ThrustLimits(np.median(rec[:, 0]), np.median(rec[:, 2]), np.median(rec[:, 4]))
    fl = call(lim)[1]
    want = (np.where(rec[:, 0] < lim.f_min, THRUST_LOW, 0) | np.where(rec[:, 2] > lim.f_max, THRUST_HIGH, 0)
            | np.where(rec[:, 4] > lim.tilt_max, THRUST_TILT, 0))
    assert np.array_equal(fl, want) and len(set(fl)) > 2
    assert np.array_equal(call(lim, rec=False)[1], fl)
    assert np.array_equal(_bits(call(lim, flags=False)[0]), _bits(rec))


def test_argument_errors_launch_nothing(solver, host, ragged):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError, ThrustLimits
    r = ragged
    B = len(r["so"]) - 1
    dso, dT, dC = _dev(r["so"]), _dev(r["T"]), _dev(r["C"])
    odd = torch.full((B * 6 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    rec = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    for kw in (dict(d_rec=odd, d_flags=fl), dict(limits=ThrustLimits(f_max=float("nan")), d_rec=rec, d_flags=fl),
               dict(g=float("nan"), d_rec=rec, d_flags=fl), dict(g=-1.0, d_rec=rec, d_flags=fl),
               dict(g=float("inf"), d_rec=rec, d_flags=fl), dict(d_rec=None, d_flags=None)):
        with pytest.raises(TgmsError) as e:
            solver.thrust_device(B, dso, dT, dC, **kw)
        assert e.value.status == ERR_INVALID_ARG
    solver.thrust_device(0, None, None, None, d_rec=rec, d_flags=fl)  # B == 0: TGMS_OK, nothing launched
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.thrust_device(B, dso, dT, dC, d_rec=rec, d_flags=fl)
    assert e.value.status == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all()) and bool(torch.isnan(rec).all()) and bool((fl == -1).all())


def test_host_pointer_call_gives_the_device_call_bits(solver, ragged):
    from trajectory_generator_ros2_amd import ThrustLimits
    r = ragged
    lim = ThrustLimits(tilt_max=np.median(r["rec"][:, 4]))
    rec_h, fl_h = solver.thrust(r["so"], r["T"], r["C"], G, lim)
    rec_d, fl_d = _device_call(solver, r["so"], r["T"], r["C"], lim)
    assert np.array_equal(_bits(rec_h), _bits(rec_d)) and np.array_equal(fl_h, fl_d) and fl_d.any()


def test_captured_into_a_graph_and_replayed(solver, ragged):
    """The device call on the ragged batch inside torch.cuda.graph; the replay after the inputs
    were overwritten in place with the end-derivative coefficients is bit-equal to a direct call
    on them."""
    import torch
    from trajectory_generator_ros2_amd import ThrustLimits
    r = ragged
    B = len(r["so"]) - 1
    lim = ThrustLimits(tilt_max=np.median(r["rec"][:, 4]))
    want = [_device_call(solver, r["so"], r["T"], C, lim) for C in (r["C"], r["C_ed"])]
    assert not np.array_equal(want[0][0], want[1][0])
    dso, dT, dC = _dev(r["so"]), _dev(r["T"]), _dev(r["C"])
    rec = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.thrust_device(B, dso, dT, dC, G, lim, rec, fl, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for C, (rec0, fl0) in zip((r["C"], r["C_ed"]), want):
        dC.copy_(_dev(C))
        rec.fill_(float("nan"))
        fl.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(rec.cpu().numpy()), _bits(rec0))
        assert np.array_equal(fl.cpu().numpy(), fl0)
    del g


def test_sees_what_a_coarse_dt_misses(solver):
    """The horizontal closed form sampled at dt = 2T: sample 0 and the pinned last one, both at
    rest, so the reduction of the sampler's output reports tilt == 0 and raises nothing.  The
    continuous call flags THRUST_TILT against half the true tilt."""
    from trajectory_generator_ros2_amd import THRUST_TILT, ThrustLimits
    d, T = 1.7, 1.0
    so, Ts, C, _ = R.rest_to_rest(np.array([0.3, -1.0, 2.0]), d, T, axis=0)
    lim = ThrustLimits(tilt_max=np.arctan(TR.a_peak(d, T) / G) / 2)
    W = np.array([[0.3, -1.0, 2.0], [0.3 + d, -1.0, 2.0]])
    offs, out = solver.sample(so, W, Ts, None, C, 2 * T)
    a = out[:, 6:9]
    tilt = np.arctan2(np.hypot(a[:, 0], a[:, 1]), a[:, 2] + G)
    assert len(out) == 2 and tilt.max() == 0.0 and not tilt.max() > lim.tilt_max
    rec, fl = _device_call(solver, so, Ts, C, lim)
    assert fl[0] == THRUST_TILT and rec[0, 4] > 2 * lim.tilt_max * (1 - 1e-12)
