"""GPU: the continuous swarm separation (tgms_separation_batch / tgms_separation_batch_device,
csrc/tgms_separation.hip): closed-form answers, the 1e-9 contract of include/tgms.h against the
independent reference of separation_ref.py, agreement with the host backend, and the launch's
corners: tiles of sixteen pairs per wavefront, 33-interval pairs, zero-length intervals, the
grid-stride loop, the all-pairs decode, bad indices and offsets, flags, argument errors, graph
capture."""
import numpy as np
import pytest

import separation_ref as SR

pytestmark = pytest.mark.gpu

GRID = 4096  # workgroups of the launch at most (csrc/tgms_separation.hip GRID_CAP)
TILE = 16    # pairs per workgroup (csrc/tgms_separation.hip TILE)

PAIR01 = np.array([[0, 1]], np.int32)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device_call(solver, so, T, C, pairs=None, t0=None, scale=None, r_min=0.0, sep=True, flags=True):
    """tgms_separation_batch_device on fresh NaN / -1 outputs; returns numpy (sep, flags)."""
    import torch
    B = len(so) - 1
    P = B * (B - 1) // 2 if pairs is None else len(pairs)
    d_sep = torch.full((P, 2), float("nan"), dtype=torch.float64, device="cuda") if sep else None
    d_fl = torch.full((P,), -1, dtype=torch.int32, device="cuda") if flags else None
    solver.separation_device(B, _dev(np.asarray(so, np.int32)), _dev(np.asarray(T, np.float64).reshape(-1)),
                             _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)), P,
                             None if pairs is None else _dev(np.asarray(pairs, np.int32).reshape(-1, 2)),
                             None if t0 is None else _dev(np.asarray(t0, np.float64)), scale, r_min, d_sep, d_fl)
    torch.cuda.synchronize()
    return (d_sep.cpu().numpy() if sep else None), (d_fl.cpu().numpy() if flags else None)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def rest(solver):
    """The rest-to-rest contract case and its device records.  Shared, never modified."""
    c = dict(SR.contract_case("rest"))
    c["sep"], c["fl"] = _device_call(solver, c["so"], c["T"], c["C"], c["pairs"], c["t0"])
    return c


def test_known_answers(solver):
    """The closed forms of test_separation_host.py through the device call: the crossing (whole
    and with j split at a knot that is not i's), shifted starts, the held tail, disjoint
    windows, the scale."""
    for split in (False, True):
        so, T, C = SR.crossing(split)
        sep, fl = _device_call(solver, so, T, C, PAIR01)
        assert fl[0] == 0 and abs(sep[0, 0] - 0.5) <= 1e-12 * 0.5 and abs(sep[0, 1] - 1.0) <= 1e-12
    so, T, C = SR.batch(SR.line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 2.0), SR.line([2.0, 0.5, 0.0], [-1.0, 0.25, 0.0], 2.0))
    r0, v = np.array([-2.6, -0.35]), np.array([2.0, -0.25])
    ts = -(r0 @ v) / (v @ v)
    want = np.linalg.norm(r0 + v * ts)
    sep, fl = _device_call(solver, so, T, C, PAIR01, t0=[0.0, 0.6])
    assert fl[0] == 0 and abs(sep[0, 0] - want) <= 1e-12 * want and abs(sep[0, 1] - ts) <= 1e-9
    so, T, C = SR.batch(SR.line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 1.0), SR.line([-2.0, 0.25, 0.0], [1.0, 0.0, 0.0], 4.0))
    sep, fl = _device_call(solver, so, T, C, PAIR01)
    assert fl[0] == 0 and abs(sep[0, 0] - 0.25) <= 1e-12 * 0.25 and abs(sep[0, 1] - 3.0) <= 1e-12 * 3.0
    so, T, C = SR.batch(SR.line([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 2.0), SR.line([1.0, 0.8, 0.0], [1.0, -0.3, 0.0], 2.0))
    r0, v = np.array([-1.0, 0.8]), np.array([1.0, -0.3])
    ts = -(r0 @ v) / (v @ v)
    want = np.linalg.norm(r0 + v * ts)
    sep, fl = _device_call(solver, so, T, C, PAIR01, t0=[0.0, 3.0])
    assert fl[0] == 0 and abs(sep[0, 0] - want) <= 1e-12 * want and abs(sep[0, 1] - (3.0 + ts)) <= 1e-9
    so, T, C = SR.batch(SR.line([0.0, 0.0, 1.0], [1.0, 0.5, 0.0], 2.0), SR.line([0.0, 0.0, 1.9], [1.0, 0.5, 0.0], 2.0))
    sep, _ = _device_call(solver, so, T, C, PAIR01, scale=[1.0, 1.0, 1.0 / 3.0])
    assert abs(sep[0, 0] - 0.3) <= 1e-12 * 0.3


def test_identical_trajectories_give_exactly_zero(solver, rest):
    so, T, C = rest["so"], rest["T"], rest["C"]
    b = int(np.flatnonzero(np.diff(so) == 16)[0])
    one = (C[so[b]:so[b + 1]], T[so[b]:so[b + 1]])
    so2, T2, C2 = SR.batch(one, one)
    sep, fl = _device_call(solver, so2, T2, C2, [[0, 0], [0, 1], [1, 1]], t0=[1.7, 1.7])
    assert not fl.any() and (sep[:, 0] == 0.0).all() and not np.signbit(sep[:, 0]).any()
    sep, fl = _device_call(solver, so, T, C, [[b, b], [3, 3]], t0=rest["t0"])
    assert not fl.any() and (sep[:, 0] == 0.0).all()


def test_ragged_pairs_meet_the_contract(solver, host, rest):
    """Rest to rest and with non-zero end derivatives: within 1e-9 L^2 of the reference, within
    2e-9 L^2 of the host backend (both meet 1e-9)."""
    for c in (rest, SR.contract_case("end_derivs")):
        sep, fl = (c["sep"], c["fl"]) if "sep" in c else _device_call(solver, c["so"], c["T"], c["C"], c["pairs"], c["t0"])
        assert not fl.any()
        SR.check_contract(sep, c["trajs"], c["pairs"], c["refs"], what="device separation")
        sep_h, _ = host.separation(c["so"], c["T"], c["C"], c["pairs"], c["t0"])
        L = np.array([r[1] for r in c["refs"]])
        err = np.abs(sep[:, 0] ** 2 - sep_h[:, 0] ** 2) / L ** 2
        print("device vs host: d_min^2 off by %.3g x L^2" % err.max())
        assert (err <= 2e-9).all()


def test_host_pointer_call_gives_the_device_call_bits(solver, rest):
    c = rest
    r_min = float(np.median(c["sep"][:, 0]))
    sep_h, fl_h = solver.separation(c["so"], c["T"], c["C"], c["pairs"], c["t0"], r_min=r_min)
    sep_d, fl_d = _device_call(solver, c["so"], c["T"], c["C"], c["pairs"], c["t0"], r_min=r_min)
    assert _same(sep_h, sep_d) and np.array_equal(fl_h, fl_d) and fl_d.any() and not fl_d.all()
    assert _same(sep_d, c["sep"])
    sep_a, fl_a = solver.separation(c["so"][:6], c["T"][:c["so"][5]], c["C"][:c["so"][5]], None, c["t0"][:5])
    sep_b, fl_b = _device_call(solver, c["so"][:6], c["T"][:c["so"][5]], c["C"][:c["so"][5]], None, c["t0"][:5])
    assert sep_a.shape == (10, 2) and _same(sep_a, sep_b) and np.array_equal(fl_a, fl_b)


def test_edge_shapes(solver, host):
    """P = 1; two M = 16 trajectories with no coincident knots (33 intervals, the most a pair
    has); the same two with all knots coincident (zero-length intervals); P = 17 (a one-pair
    last tile).  Against the reference and the host backend."""
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = S.uniform_batch(3, 16, seed=11)
    W, T = W.reshape(-1, 3), T.reshape(-1).copy()
    T[32:48] = T[0:16]  # trajectory 2 has trajectory 0's times: with equal starts every knot coincides
    C, st, worst = solver.solve(so, W, T)
    assert worst == 0
    t0 = np.array([0.0, 0.3, 0.0])
    k0, k1 = np.cumsum(T[:16]), 0.3 + np.cumsum(T[16:32])
    assert len(np.unique(np.concatenate([[0.0, 0.3], k0, k1]))) == 34
    pairs = np.array([[0, 1], [0, 2], [2, 0], [1, 2]] * 4 + [[1, 0]], np.int32)  # P = 17
    trajs = SR.batch_trajs(so, T, C, t0)
    refs4 = SR.references(trajs, pairs[:4])
    refs = (refs4 * 4) + [refs4[0]]
    sep1, fl1 = _device_call(solver, so, T, C, pairs[:1], t0)  # P = 1
    sep, fl = _device_call(solver, so, T, C, pairs, t0)
    assert not fl.any() and fl1[0] == 0 and _same(sep[:1], sep1)
    SR.check_contract(sep, trajs, pairs, refs, what="device separation, M = 16 pairs")
    assert _same(sep[:4], sep[4:8]) and _same(sep[:4], sep[12:16])
    sep_h, _ = host.separation(so, T, C, pairs, t0)
    L = np.array([r[1] for r in refs])
    assert (np.abs(sep[:, 0] ** 2 - sep_h[:, 0] ** 2) <= 2e-9 * L ** 2).all()


def test_grid_stride_and_lds_reuse(solver, host):
    """The launch uses min(ceil(P / 16), 4096) workgroups of one wavefront, each taking tiles of 16
    consecutive pairs by grid-stride.  P = 4096 * 16 + 5 leaves a partial tile to the second pass
    of workgroup 0, on the LDS its first tile used.  The pairs are cheap M = 1 linear motions
    cycled with period 7 (coprime to the tile), so the records are a tiling of seven host-backend
    answers; the device's own seven must also be bit-equal throughout."""
    from trajectory_generator_ros2_amd import SEP_CLOSE
    rng = np.random.default_rng(5)
    lines = [SR.line(rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3), rng.uniform(1.0, 3.0)) for _ in range(8)]
    so, T, C = SR.batch(*lines)
    t0 = rng.uniform(0.0, 1.0, 8)
    seven = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [1, 2], [3, 4], [5, 6]], np.int32)
    P = GRID * TILE + 5
    pairs = seven[np.arange(P) % 7]
    sep7_h, _ = host.separation(so, T, C, seven, t0)
    r_min = float(np.median(sep7_h[:, 0]))
    sep7, fl7 = _device_call(solver, so, T, C, seven, t0, r_min=r_min)
    assert (np.abs(sep7[:, 0] - sep7_h[:, 0]) <= 1e-12 * sep7_h[:, 0]).all()
    assert np.array_equal(fl7, np.where(sep7[:, 0] < r_min, SEP_CLOSE, 0)) and fl7.any() and not fl7.all()
    sep, fl = _device_call(solver, so, T, C, pairs, t0, r_min=r_min)
    assert _same(sep, sep7[np.arange(P) % 7]) and np.array_equal(fl, fl7[np.arange(P) % 7])


def test_all_pairs_is_the_explicit_list(solver, rest):
    """B = 65: 2,080 pairs decoded on the device, bit-equal to the explicit list in the stated
    order (trajectories 48..64 repeat the first 17 with other start times)."""
    c = rest
    so, T, C = c["so"], c["T"], c["C"]
    S17 = int(so[17])
    so65 = np.concatenate([so, so[-1] + so[1:18]]).astype(np.int32)
    T65, C65 = np.concatenate([T, T[:S17]]), np.concatenate([C, C[:S17]])
    t65 = np.concatenate([c["t0"], c["t0"][:17] + 0.5])
    pairs = np.array([(i, j) for i in range(65) for j in range(i + 1, 65)], np.int32)
    assert len(pairs) == 2080
    r_min = 1.0
    sep_a, fl_a = _device_call(solver, so65, T65, C65, None, t65, r_min=r_min)
    sep_e, fl_e = _device_call(solver, so65, T65, C65, pairs, t65, r_min=r_min)
    assert _same(sep_a, sep_e) and np.array_equal(fl_a, fl_e) and np.isfinite(sep_a).all()
    assert fl_a.any() and not fl_a.all()


def test_flags(solver):
    from trajectory_generator_ros2_amd import SEP_CLOSE
    so, T, C = SR.crossing()
    sep, fl = _device_call(solver, so, T, C, PAIR01)
    d = float(sep[0, 0])
    assert fl[0] == 0
    assert _device_call(solver, so, T, C, PAIR01, r_min=d)[1][0] == 0  # strict
    sep2, fl2 = _device_call(solver, so, T, C, PAIR01, r_min=np.nextafter(d, np.inf))
    assert fl2[0] == SEP_CLOSE and _same(sep2, sep)
    for r in (0.0, -1.0):
        assert _device_call(solver, so, T, C, PAIR01, r_min=r)[1][0] == 0
    assert _device_call(solver, so, T, C, PAIR01, r_min=1.0, sep=False)[1][0] == SEP_CLOSE
    assert _same(_device_call(solver, so, T, C, PAIR01, r_min=1.0, flags=False)[0], sep)


def test_bad_input_marks_exactly_its_pairs(solver, rest):
    from trajectory_generator_ros2_amd import SEP_NONFINITE
    c = rest
    so, T, C, t0 = c["so"], c["T"], c["C"], c["t0"]
    pairs = np.concatenate([c["pairs"], [[-1, 5], [5, 48], [48, -1], [7, 7]]]).astype(np.int32)
    r_min = float(np.median(c["sep"][:, 0]))
    sep0, fl0 = _device_call(solver, so, T, C, pairs, t0, r_min=r_min)
    assert _same(sep0[:96], c["sep"]) and (fl0[96:99] == SEP_NONFINITE).all() and np.isnan(sep0[96:99]).all()
    assert fl0[99] == 1 and sep0[99, 0] == 0.0
    C2, T2, t2 = C.copy(), T.copy(), t0.copy()
    C2[so[3] + 1, 1, 4] = np.nan      # a NaN coefficient in trajectory 3
    T2[so[41 + 1] - 1] = 0.0          # a zero time in trajectory 41
    T2[so[30]] = np.inf               # an infinite time in trajectory 30
    t2[20] = np.nan                   # a NaN start time in trajectory 20
    sep, fl = _device_call(solver, so, T2, C2, pairs, t2, r_min=r_min)
    bad = np.isin(pairs, [3, 20, 30, 41]).any(axis=1) | (pairs < 0).any(axis=1) | (pairs >= 48).any(axis=1)
    assert (fl[bad] == SEP_NONFINITE).all() and np.isnan(sep[bad]).all()
    assert np.array_equal(fl[~bad], fl0[~bad]) and _same(sep[~bad], sep0[~bad])
    # device offsets with M = 0 (trajectory 1) and M = 17 (trajectory 3) between trajectories
    # 0, 1, 2 of the batch: nothing is read for the two, the pairs of the others are as before
    M = np.diff(so)[:3]
    so2 = np.cumsum([0, M[0], 0, M[1], 17, M[2]]).astype(np.int32)
    T3, C3 = np.full(so2[-1], 1.0), np.full((so2[-1], 3, 8), 0.5)
    for src, dst in ((0, 0), (1, 2), (2, 4)):
        T3[so2[dst]:so2[dst + 1]] = T[so[src]:so[src + 1]]
        C3[so2[dst]:so2[dst + 1]] = C[so[src]:so[src + 1]]
    t3 = np.array([t0[0], 0.0, t0[1], 0.0, t0[2]])
    sep3, fl3 = _device_call(solver, so2, T3, C3, None, t3)
    want, _ = _device_call(solver, so[:4], T[:so[3]], C[:so[3]], None, t0[:3])
    p5 = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    good = np.array([i in (0, 2, 4) and j in (0, 2, 4) for i, j in p5])
    assert good.sum() == 3 and _same(sep3[good], want) and not fl3[good].any()
    assert (fl3[~good] == SEP_NONFINITE).all() and np.isnan(sep3[~good]).all()


def test_argument_errors_launch_nothing(solver, rest):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, TgmsError
    c = rest
    B, P = 48, 96
    dso, dT, dC, dP, dt0 = _dev(c["so"]), _dev(c["T"]), _dev(c["C"]), _dev(c["pairs"]), _dev(c["t0"])
    odd = torch.full((P * 2 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    sep = torch.full((P, 2), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    for kw in (dict(d_sep=odd, d_flags=fl), dict(d_sep=None, d_flags=None), dict(r_min=float("nan"), d_sep=sep),
               dict(scale=[1.0, 0.0, 1.0], d_sep=sep), dict(scale=[1.0, float("nan"), 1.0], d_flags=fl),
               dict(scale=[-1.0, 1.0, 1.0], d_sep=sep, d_flags=fl)):
        with pytest.raises(TgmsError) as e:
            solver.separation_device(B, dso, dT, dC, P, dP, dt0, **kw)
        assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # pairs == NULL needs P == B (B - 1) / 2
        solver.separation_device(B, dso, dT, dC, P, None, dt0, d_sep=sep, d_flags=fl)
    assert e.value.status == ERR_INVALID_ARG
    solver.separation_device(B, dso, dT, dC, 0, dP, dt0, d_sep=sep, d_flags=fl)  # P == 0: TGMS_OK, nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all()) and bool(torch.isnan(sep).all()) and bool((fl == -1).all())


def test_captured_into_a_graph_and_replayed(solver, rest):
    """The device call on the ragged batch inside torch.cuda.graph (test_gpu_bounds.py's pattern),
    replayed twice with the start times changed in place between the replays: each replay is
    bit-equal to the direct call on the start times it saw."""
    import torch
    c = rest
    r_min = float(np.median(c["sep"][:, 0]))
    t_b = c["t0"][::-1].copy()
    want = [_device_call(solver, c["so"], c["T"], c["C"], c["pairs"], t, r_min=r_min) for t in (c["t0"], t_b)]
    assert not np.array_equal(want[0][0], want[1][0])
    dso, dT, dC, dP, dt0 = _dev(c["so"]), _dev(c["T"]), _dev(c["C"]), _dev(c["pairs"]), _dev(c["t0"])
    sep = torch.full((96, 2), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((96,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.separation_device(48, dso, dT, dC, 96, dP, dt0, None, r_min, sep, fl, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for t, (sep0, fl0) in zip((c["t0"], t_b), want):
        dt0.copy_(_dev(t))
        sep.fill_(float("nan"))
        fl.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert _same(sep.cpu().numpy(), sep0) and np.array_equal(fl.cpu().numpy(), fl0)
    del g
