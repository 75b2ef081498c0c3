"""GPU: the fused feasibility check (tgms_extrema_batch / tgms_extrema_batch_device,
csrc/tgms_extrema.hip) against the sampler it is defined by, and against the oracle.

Every record must be what a reduction over `Solver.sample`'s output of the same batch gives:
extents equal, peaks within 1e-14 relative (only the three-term sum and the square root may
round differently), duration bit-equal to the prefix sum of T; and within the project's
1e-9 of the same reduction over the oracle's samples.  The flags are strict comparisons on
the stored record."""
import numpy as np
import pytest

from extrema_ref import PEAK_RTOL, bit_equal, check_against_oracle, check_against_samples

pytestmark = pytest.mark.gpu
DT = 0.01


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device_call(solver, so, W, T, ED, C, dt, limits=None, ext=True, flags=True, stream=0, bufs=None):
    """tgms_extrema_batch_device on fresh NaN / -1 outputs; returns numpy (ext, flags)."""
    import torch
    B = len(so) - 1
    d_ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda") if ext else None
    d_fl = torch.full((B,), -1, dtype=torch.int32, device="cuda") if flags else None
    args = bufs or (_dev(np.asarray(so, np.int32)), _dev(np.asarray(W).reshape(-1, 3)), _dev(np.asarray(T).reshape(-1)),
                    _dev(np.asarray(C).reshape(-1, 3, 8)), _dev(None if ED is None else np.asarray(ED).reshape(-1, 18)))
    solver.extrema_device(B, args[0], args[1], args[2], args[3], dt, limits, d_ext, d_fl, args[4], stream=stream)
    torch.cuda.synchronize()
    return (d_ext.cpu().numpy() if ext else None), (d_fl.cpu().numpy() if flags else None)


def _solve(solver, so, W, T, ED=None):
    C, st, worst = solver.solve(so, W, T, ED)
    assert worst == 0 and not st.any()
    return C


@pytest.fixture(scope="module")
def ragged(solver):
    """The ragged 40-trajectory batch (M = 1..16): inputs, GPU samples, and the records of the
    host-pointer and the device call without limits.  Shared, never modified."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = S.ragged_batch(40, 1, 16, seed=12)
    C = _solve(solver, so, W, T)
    offs, out = solver.sample(so, W, T, None, C, DT)
    ext_h, fl_h = solver.extrema(so, W, T, None, C, DT)
    ext_d, fl_d = _device_call(solver, so, W, T, None, C, DT)
    return dict(so=so, W=W, T=T, C=C, offs=offs, out=out, ext_h=ext_h, fl_h=fl_h, ext_d=ext_d, fl_d=fl_d)


def test_ragged_matches_sampler_and_oracle(ragged, oracle):
    r = ragged
    for ext, fl in ((r["ext_h"], r["fl_h"]), (r["ext_d"], r["fl_d"])):
        check_against_samples(ext, r["so"], r["T"], r["offs"], r["out"])
        check_against_oracle(ext, r["so"], r["W"], r["T"], None, r["C"], DT, oracle)
        assert not fl.any()
    assert np.array_equal(r["ext_h"].view(np.int64), r["ext_d"].view(np.int64))


def test_edge_shapes(solver, oracle):
    """One batch of B = 5 (not a multiple of 4): M = 1 with sum T < dt (ns = 2: sample 0 and
    the pinned one), ns = 64, ns = 65, ns = 193 = 3*64 + 1 with segment times that are exact
    multiples of dt (samples land on the knots), and M = 16."""
    rng = np.random.default_rng(5)
    Ts = [[0.004], [0.3, 0.33], [0.32, 0.32], [0.5, 0.25, 0.75, 0.42], list(rng.uniform(0.5, 3.0, 16))]
    so = np.cumsum([0] + [len(t) for t in Ts]).astype(np.int32)
    T = np.concatenate(Ts)
    n = int(so[-1]) + 5
    W = np.c_[rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(0.5, 5, n)]
    C = _solve(solver, so, W, T)
    offs, out = solver.sample(so, W, T, None, C, DT)
    assert list(np.diff(offs)[:4]) == [2, 64, 65, 193]
    knots = np.cumsum(Ts[3])[:-1] / DT  # 50, 75, 150: k*dt equals the knot time exactly
    assert all(float(k) * DT == t for k, t in zip(np.rint(knots), np.cumsum(Ts[3])[:-1]))
    for ext in (solver.extrema(so, W, T, None, C, DT)[0], _device_call(solver, so, W, T, None, C, DT)[0]):
        check_against_samples(ext, so, T, offs, out)
        check_against_oracle(ext, so, W, T, None, C, DT, oracle)


def test_pinned_final_sample_is_counted(solver):
    """Final end velocity above every sampled speed: v_peak is the pinned sample's."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = S.uniform_batch(6, 2, seed=31)
    d = W[:, -1] - W[:, -2]
    d /= np.linalg.norm(d, axis=1)[:, None]
    ED = np.zeros((6, 18))
    ED[:, 9:12] = 40.0 * d   # final velocity along the last segment ...
    ED[:, 12:15] = 40.0 * d  # ... still accelerating, so the speed peaks at the very end
    W, T = W.reshape(-1, 3), T.reshape(-1)
    C = _solve(solver, so, W, T, ED)
    offs, out = solver.sample(so, W, T, ED, C, DT)
    final = np.sqrt((ED[:, 9:12] ** 2).sum(axis=1))
    for b in range(6):
        s = out[offs[b]:offs[b + 1]]
        assert np.sqrt((s[:-1, 3:6] ** 2).sum(axis=1)).max() < final[b]
    for ext in (solver.extrema(so, W, T, ED, C, DT)[0], _device_call(solver, so, W, T, ED, C, DT)[0]):
        assert (np.abs(ext[:, 6] - final) <= PEAK_RTOL * final).all()
        check_against_samples(ext, so, T, offs, out)


def _device_reduction(out, offs):
    """[B,9] pmin pmax peaks from the device sampler's output `out`, reduced by torch on the
    device (extrema_ref.reduce_samples in numpy would take seconds at these sizes)."""
    import torch
    B = len(offs) - 1
    idx = torch.repeat_interleave(torch.arange(B, device="cuda"), _dev(np.diff(offs)))
    i3 = idx[:, None].expand(-1, 3)
    new = lambda v, w: torch.full((B, w) if w else (B,), v, dtype=torch.float64, device="cuda")
    lo = new(float("inf"), 3).scatter_reduce_(0, i3, out[:, 0:3], "amin")
    hi = new(float("-inf"), 3).scatter_reduce_(0, i3, out[:, 0:3], "amax")
    pk = [new(0.0, 0).scatter_reduce_(0, idx, (out[:, 3 + 3 * q:6 + 3 * q] ** 2).sum(dim=1), "amax").sqrt()
          for q in range(3)]
    return torch.cat([lo, hi, torch.stack(pk, dim=1)], dim=1).cpu().numpy()


def _check_against_reduction(ext, ref, dur):
    assert np.isfinite(ext).all()
    assert bit_equal(ext[:, 0:6], ref[:, 0:6])
    assert (np.abs(ext[:, 6:9] - ref[:, 6:9]) <= PEAK_RTOL * ref[:, 6:9]).all()
    assert np.array_equal(ext[:, 9].view(np.int64), dur.view(np.int64))


def test_multi_block_against_device_reduction(solver):
    """B = 1,027 x M = 3 at dt = 0.05: many workgroups, one trajectory each (the grid-stride
    loop is test_grid_stride_and_lds_reuse's), against a torch reduction of the device
    sampler's output, on the device."""
    import torch
    from trajectory_generator_ros2_amd import synthetic as S
    from trajectory_generator_ros2_amd.solver import sample_offsets
    B, M, dt = 1027, 3, 0.05
    so, W, T = S.uniform_batch(B, M, seed=33)
    dso, dW, dT = _dev(so), _dev(W), _dev(T)
    dC = torch.empty((B, M, 3, 8), dtype=torch.float64, device="cuda")
    solver.solve_uniform_device(B, M, dW, dT, dC)
    offs = sample_offsets(so, T.reshape(-1), dt)
    out = torch.empty((int(offs[-1]), 14), dtype=torch.float64, device="cuda")
    solver.sample_device(B, dso, dW, dT, dC, dt, _dev(offs), out)
    ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda")
    solver.extrema_device(B, dso, dW, dT, dC, dt, None, ext)
    torch.cuda.synchronize()
    _check_against_reduction(ext.cpu().numpy(), _device_reduction(out, offs), ((T[:, 0] + T[:, 1]) + T[:, 2]))


def test_grid_stride_and_lds_reuse(solver):
    """B = 16,400 x M = 1..2 at dt = 0.1: more trajectories than the launch's 15,360
    workgroups, so workgroups 0..1,039 take a second trajectory (b + 15,360) on the LDS
    arrays the first one used.  Every record against the device sampler's reduction; then
    with a NaN coefficient in trajectory 100 (its workgroup goes on to the clean 15,460) and
    in 15,560 (the second trajectory of workgroup 200, after the clean 200): those two are
    flagged, every other record keeps its bits."""
    import torch
    from extrema_ref import durations
    from trajectory_generator_ros2_amd import FEAS_NONFINITE
    from trajectory_generator_ros2_amd import synthetic as S
    from trajectory_generator_ros2_amd.solver import sample_offsets
    B, dt, grid = 16400, 0.1, 15360
    so, W, T = S.ragged_batch(B, 1, 2, seed=34)
    C = _solve(solver, so, W, T)
    bufs = (_dev(so), _dev(W), _dev(T), _dev(C), None)
    offs = sample_offsets(so, T, dt)
    out = torch.empty((int(offs[-1]), 14), dtype=torch.float64, device="cuda")
    solver.sample_device(B, bufs[0], bufs[1], bufs[2], bufs[3], dt, _dev(offs), out)
    ext, fl = _device_call(solver, so, W, T, None, C, dt, bufs=bufs)
    assert not fl.any()
    _check_against_reduction(ext, _device_reduction(out, offs), durations(so, T))
    bad = [100, grid + 200]
    assert bad[0] + grid < B and bad[1] < B  # both workgroups do run a second trajectory
    C2 = C.copy()
    for b in bad:
        C2[so[b], 2, 5] = np.nan
    ext2, fl2 = _device_call(solver, so, W, T, None, C2, dt)
    want = np.zeros(B, np.int32)
    want[bad] = FEAS_NONFINITE
    assert np.array_equal(fl2, want)
    keep = want == 0
    assert np.array_equal(ext2[keep].view(np.int64), ext[keep].view(np.int64))


def test_flags_box(solver, ragged):
    from trajectory_generator_ros2_amd import FEAS_BOX, Limits
    r = ragged
    ext = r["ext_d"]
    lo, hi = ext[:, 0:3].min(axis=0), ext[:, 3:6].max(axis=0)
    call = lambda lim: _device_call(solver, r["so"], r["W"], r["T"], None, r["C"], DT, lim)
    e2, fl = call(Limits(pmin=lo, pmax=hi))  # exactly the returned extents: everything inside
    assert not fl.any() and np.array_equal(e2, ext)
    for face in range(6):  # shrink one face by one ulp: exactly the trajectories beyond it
        lim = Limits(pmin=lo, pmax=hi)
        if face < 3:
            lim.pmin[face] = np.nextafter(lo[face], np.inf)
            want = ext[:, face] < lim.pmin[face]
        else:
            lim.pmax[face - 3] = np.nextafter(hi[face - 3], -np.inf)
            want = ext[:, face] > lim.pmax[face - 3]
        fl = call(lim)[1]
        assert 1 <= want.sum() < len(want) and np.array_equal(fl, np.where(want, FEAS_BOX, 0))
    for b in (0, 17, 39):  # a chosen trajectory's own extents, then one face one ulp inside them
        assert call(Limits(pmin=ext[b, 0:3], pmax=ext[b, 3:6]))[1][b] == 0
        lim = Limits(pmin=ext[b, 0:3], pmax=ext[b, 3:6])
        lim.pmax[1] = np.nextafter(ext[b, 4], -np.inf)
        assert call(lim)[1][b] == FEAS_BOX


def test_flags_speed_limits(solver, ragged):
    from trajectory_generator_ros2_amd import FEAS_ACCEL, FEAS_JERK, FEAS_SPEED, Limits
    r = ragged
    ext = r["ext_d"]
    lim = Limits(v_max=np.median(ext[:, 6]), a_max=np.median(ext[:, 7]), j_max=np.median(ext[:, 8]))
    for fl in (_device_call(solver, r["so"], r["W"], r["T"], None, r["C"], DT, lim)[1],
               solver.extrema(r["so"], r["W"], r["T"], None, r["C"], DT, lim)[1]):
        want = np.zeros(len(fl), np.int32)
        for col, bit, m in ((6, FEAS_SPEED, lim.v_max), (7, FEAS_ACCEL, lim.a_max), (8, FEAS_JERK, lim.j_max)):
            over = ext[:, col] > m
            assert len(fl) // 4 <= over.sum() <= len(fl) - len(fl) // 4  # both sides populated
            want |= np.where(over, bit, 0).astype(np.int32)
        assert np.array_equal(fl, want)


def test_flags_null_and_infinite_limits(solver, ragged):
    from trajectory_generator_ros2_amd import Limits
    r = ragged
    args = (solver, r["so"], r["W"], r["T"], None, r["C"], DT)
    assert not _device_call(*args, Limits())[1].any()  # +-inf everywhere
    lim = Limits(v_max=np.median(r["ext_d"][:, 6]), pmax=[4.0, 4.0, 4.5])
    ext, fl = _device_call(*args, lim)
    assert fl.any() and np.array_equal(ext, r["ext_d"])
    assert np.array_equal(_device_call(*args, lim, ext=False)[1], fl)
    assert np.array_equal(_device_call(*args, lim, flags=False)[0].view(np.int64), ext.view(np.int64))


def test_nonfinite_input_marks_one_trajectory(solver, ragged):
    from trajectory_generator_ros2_amd import FEAS_NONFINITE, Limits
    r = ragged
    lim = Limits(v_max=np.median(r["ext_d"][:, 6]))
    _, fl0 = _device_call(solver, r["so"], r["W"], r["T"], None, r["C"], DT, lim)
    C2 = r["C"].copy()
    C2[r["so"][7] + 1, 1, 3] = np.nan
    ext, fl = _device_call(solver, r["so"], r["W"], r["T"], None, C2, DT, lim)
    assert fl[7] == FEAS_NONFINITE and not (np.delete(fl, 7) & FEAS_NONFINITE).any()
    assert np.array_equal(np.delete(fl, 7), np.delete(fl0, 7))
    keep = np.arange(len(fl)) != 7
    assert np.array_equal(ext[keep].view(np.int64), r["ext_d"][keep].view(np.int64))


def test_argument_errors_launch_nothing(solver, ragged):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, Limits, TgmsError
    r = ragged
    B = len(r["so"]) - 1
    dso, dW, dT, dC = _dev(r["so"]), _dev(r["W"]), _dev(r["T"]), _dev(r["C"])
    odd = torch.full((B * 10 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    for kw in (dict(d_extrema=odd, d_flags=fl), dict(limits=Limits(a_max=float("nan")), d_extrema=ext, d_flags=fl),
               dict(d_extrema=None, d_flags=None)):
        with pytest.raises(TgmsError) as e:
            solver.extrema_device(B, dso, dW, dT, dC, DT, **kw)
        assert e.value.status == ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all()) and bool(torch.isnan(ext).all()) and bool((fl == -1).all())


def test_captured_into_a_graph_and_replayed(solver, ragged):
    """The device call on a ragged batch inside torch.cuda.graph (tests/test_gpu_capture.py's
    pattern): outputs reset to NaN / -1, replayed, bit-equal to the direct call."""
    import torch
    from trajectory_generator_ros2_amd import Limits
    r = ragged
    B = len(r["so"]) - 1
    lim = Limits(v_max=np.median(r["ext_d"][:, 6]))
    ext0, fl0 = _device_call(solver, r["so"], r["W"], r["T"], None, r["C"], DT, lim)
    dso, dW, dT, dC = _dev(r["so"]), _dev(r["W"]), _dev(r["T"]), _dev(r["C"])
    ext = torch.full((B, 10), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.extrema_device(B, dso, dW, dT, dC, DT, lim, ext, fl, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for _ in range(2):
        ext.fill_(float("nan"))
        fl.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ext.cpu().numpy().view(np.int64), ext0.view(np.int64))
        assert np.array_equal(fl.cpu().numpy(), fl0)
    del g
