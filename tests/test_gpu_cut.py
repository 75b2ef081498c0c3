"""GPU: the replan cut (tgms_cut_batch / tgms_cut_batch_device, csrc/tgms_cut.hip): the checks of
test_cut_host.py through the device call, the integers, flags, times and t0 bit-equal to the host
backend, and the launches' corners: one row, two tiles, a full tile, the seams of the scan (SCAN
entries per workgroup, SCAN workgroup sums per chunk of the top level), the grid-stride loop, a
bad segment count in the middle of a tile, capacity sentinels, omitted outputs, argument errors,
graph capture, a repeated call, and the whole tick on the device with only the new offsets on the
host."""
import numpy as np
import pytest

import cut_ref as CR
import test_cut_host as H

pytestmark = pytest.mark.gpu

GRID, TILE, SCAN = 4096, 4, 256  # csrc/tgms_cut.hip, csrc/tgms_corridor_split.hip
NAMES = ("d_seg_offsets_out", "d_waypoints_out", "d_seg_times_out", "d_end_derivs_out", "d_coeffs_out", "d_parent",
         "d_t0_out", "d_totals", "d_flags")


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()


def _outputs(B, S, omit=()):
    """Fresh device outputs at the header's capacities: NaN in the fp64 rows, -7 in the others."""
    import torch
    sh = dict(d_seg_offsets_out=((B + 1,), torch.int32), d_waypoints_out=((S + B, 3), torch.float64),
              d_seg_times_out=((S,), torch.float64), d_end_derivs_out=((B, 18), torch.float64),
              d_coeffs_out=((S, 3, 8), torch.float64), d_parent=((S,), torch.int32), d_t0_out=((B,), torch.float64),
              d_totals=((1,), torch.int64), d_flags=((B,), torch.int32))
    return {k: None if k in omit else torch.full(s, float("nan") if dt == torch.float64 else -7, dtype=dt, device="cuda")
            for k, (s, dt) in sh.items()}


def _raw(solver, so, W, T, C, tc, mf, ED=None, omit=()):
    """tgms_cut_batch_device on fresh outputs; returns the untrimmed numpy outputs."""
    import torch
    so = np.asarray(so, np.int32)
    B, S = len(so) - 1, int(so[-1])
    out = _outputs(B, S, omit)
    solver.cut_device(B, _dev(so), _dev(np.asarray(W, np.float64).reshape(-1, 3)),
                      _dev(np.asarray(T, np.float64).reshape(-1)), _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)),
                      _dev(np.asarray(tc, np.float64)), mf, d_end_derivs=None if ED is None else _dev(ED), **out)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def dev_cut(solver):
    """Solver.cut's tuple from the device call, after checking that nothing beyond the totals was
    written."""
    def call(so, W, T, C, tc, mf, ED=None, want_coeffs=True):
        raw = _raw(solver, so, W, T, C, tc, mf, ED, () if want_coeffs else ("d_coeffs_out",))
        B, S2 = len(so) - 1, int(raw["d_totals"][0])
        assert S2 == raw["d_seg_offsets_out"][-1]
        assert np.isnan(raw["d_seg_times_out"][S2:]).all() and (raw["d_parent"][S2:] == -7).all()
        assert np.isnan(raw["d_waypoints_out"][S2 + B:]).all()
        if want_coeffs:
            assert np.isnan(raw["d_coeffs_out"][S2:]).all()
        return (raw["d_seg_offsets_out"], raw["d_waypoints_out"][:S2 + B], raw["d_seg_times_out"][:S2],
                raw["d_end_derivs_out"], raw["d_coeffs_out"][:S2] if want_coeffs else None, raw["d_parent"][:S2],
                raw["d_t0_out"], raw["d_flags"])
    return call


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module", params=["rest", "end_derivs"])
def case(request, solver):
    return H.ragged_case(solver.solve, request.param == "end_derivs")


@pytest.fixture(scope="module")
def rest(solver):
    return H.ragged_case(solver.solve, False)


@pytest.fixture(scope="module")
def Cut(solver):
    return dev_cut(solver)


def bit_equal_to_host(dev, hst):
    """Integers, flags, times and t0 to the bit."""
    for i in (0, 2, 5, 6, 7):
        assert np.array_equal(CR.bits(dev[i]), CR.bits(hst[i])), i


# ---- every host check through the device call ----

def test_against_the_reference_and_the_host_backend(Cut, host, case):
    H.check_against_ref(Cut, case)
    for mf in (H.MIN_FRAC, 0.0):
        bit_equal_to_host(H.run(Cut, case, mf), H.run(H.host_cut(host), case, mf))


def test_a_cut_at_or_before_zero_reproduces_the_batch(Cut, case):
    H.check_identity(Cut, case)


def test_finished_rows_hold_the_end_point(Cut, case):
    H.check_finished(Cut, case)


def test_unusable_rows_are_copied_through(Cut, case):
    H.check_unusable(Cut, case)


def test_cut_then_solve_reproduces_the_tail(Cut, solver, case):
    H.check_resolve(Cut, solver.solve, case)


def test_the_join_is_smooth(Cut, solver, case):
    H.check_join(Cut, solver.solve, case)


# ---- the launches' corners ----

def small_batch(B, seed=5):
    """M of 1 or 2, random polynomials (no solve is needed for the cut itself), cuts of every kind."""
    rng = np.random.default_rng(seed)
    M = 1 + (np.arange(B) * 7 // 3) % 2
    so = np.concatenate([[0], np.cumsum(M)]).astype(np.int32)
    S = int(so[-1])
    W, T, C = rng.uniform(-2, 2, (S + B, 3)), rng.uniform(0.5, 2.0, S), rng.uniform(-1, 1, (S, 3, 8))
    D = np.add.reduceat(T, so[:-1])
    kind = np.arange(B) % 5
    tc = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.0 * D, 0.3 * D, 0.62 * D, np.inf * D], 0.97 * D)
    return so, W, T, C, tc


@pytest.mark.parametrize("B", [1, TILE, TILE + 1, SCAN, SCAN + 1, SCAN * SCAN + 1],
                         ids=["one", "full_tile", "two_tiles", "scan", "scan+1", "scan^2+1"])
def test_tiles_and_the_seams_of_the_scan(solver, host, B):
    so, W, T, C, tc = small_batch(B)
    dev = dev_cut(solver)(so, W, T, C, tc, 0.25)
    hst = host.cut(so, W, T, C, tc, 0.25)
    bit_equal_to_host(dev, hst)
    assert np.array_equal(dev[0], np.concatenate([[0], np.cumsum(np.diff(hst[0]))]))
    n = min(B, 600)  # the reference in rationals on the first rows, the host backend on all
    CR.compare(tuple(x[:k] if x is not None else x for x, k in zip(
        dev, (n + 1, dev[0][n] + n, dev[0][n], n, dev[0][n], dev[0][n], n, n))),
        CR.cut(so[:n + 1], W[:so[n] + n], T[:so[n]], C[:so[n]], tc[:n], 0.25))
    for i in (1, 3, 4):
        assert np.allclose(dev[i], hst[i], rtol=0, atol=1e-9 * 2.0 ** 8 * 8)  # |c| <= 1, t <= 2: the condition sums


def test_grid_stride_and_lds_reuse(solver, host):
    """B = 4 * 4096 + 1: every workgroup runs a second tile, the last tile holds one row."""
    B = TILE * GRID + 1
    so, W, T, C, tc = small_batch(B, seed=6)
    dev = dev_cut(solver)(so, W, T, C, tc, 0.25)
    hst = host.cut(so, W, T, C, tc, 0.25)
    bit_equal_to_host(dev, hst)
    for i in (1, 3, 4):
        assert np.allclose(dev[i], hst[i], rtol=0, atol=1e-9 * 2.0 ** 8 * 8)
    five = dev_cut(solver)(so[:6], W[:so[5] + 5], T[:so[5]], C[:so[5]], tc[:5], 0.25)
    for b in range(5):
        assert H.same(H.rows_of(dev, b), H.rows_of(five, b)), b


def test_a_bad_segment_count_in_the_middle_of_a_tile(Cut, solver, rest):
    """M = 17 from the offsets between rows 0 and 1: one placeholder segment with a NaN time, two
    NaN waypoints, NaN end derivatives and coefficients, parent -1, a NaN t0 and NONFINITE alone;
    every other row as in the clean batch."""
    c = rest
    so, M = c["so"], np.diff(c["so"])
    m0 = int(M[0])
    so2 = np.cumsum(np.concatenate([[0, m0, 17], M[1:]])).astype(np.int32)
    ins = lambda a, fill, at: np.concatenate([a[:at], fill, a[at:]])
    W2 = ins(c["W"], np.zeros((18, 3)), m0 + 1)
    T2, C2 = ins(c["T"], np.ones(17), m0), ins(c["C"], np.full((17, 3, 8), 0.5), m0)
    tc2 = ins(c["tc"], np.array([0.5]), 1)
    out = Cut(so2, W2, T2, C2, tc2, H.MIN_FRAC)
    clean = H.run(Cut, c)
    a = out[0][1]
    assert out[0][2] - a == 1 and np.isnan(out[2][a]) and np.isnan(out[1][a + 1:a + 3]).all() and out[5][a] == -1
    assert np.isnan(out[3][1]).all() and np.isnan(out[4][a]).all() and np.isnan(out[6][1]) and out[7][1] == CR.NONFINITE
    for b in range(H.B0):
        x, y = H.rows_of(out, b + (b > 0)), H.rows_of(clean, b)
        assert H.same(x, y), b
    # the solve that follows rejects that row alone
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG
    _, st, _ = solver.solve(out[0], out[1], out[2], out[3], check=False)
    assert st[1] == ERR_INVALID_ARG and not st[np.r_[0, 2:H.B0 + 1]].any()


def test_nullable_outputs_omitted_in_turn(solver, case):
    c = case
    args = (c["so"], c["W"], c["T"], c["C"], c["tc"], H.MIN_FRAC, c["ED"])
    full = _raw(solver, *args)
    for name in ("d_coeffs_out", "d_parent", "d_t0_out", "d_flags"):
        part = _raw(solver, *args, omit=(name,))
        assert part[name] is None
        assert all(np.array_equal(CR.bits(part[k]), CR.bits(full[k])) for k in NAMES if k != name), name


def test_host_pointer_call_and_a_repeat_give_the_device_call_bits(solver, Cut, case):
    dev = H.run(Cut, case)
    assert H.same(H.run(Cut, case), dev)
    assert H.same(H.run(H.host_cut(solver), case), dev)


def test_argument_errors_launch_nothing(solver, host, rest):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError
    c = rest
    B, S = H.B0, int(c["so"][-1])
    d = [_dev(c[k]) for k in ("so", "W", "T", "C", "tc")]
    out = _outputs(B, S)
    odd = torch.full((S + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]
    for mf, o in ((-0.1, out), (1.0, out), (float("nan"), out), (0.25, dict(out, d_seg_times_out=odd)),
                  (0.25, dict(out, d_totals=None)), (0.25, dict(out, d_end_derivs_out=None)),
                  (0.25, dict(out, d_seg_offsets_out=None))):
        with pytest.raises(TgmsError) as e:
            solver.cut_device(B, *d, mf, **o)
        assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.cut_device(B, *d, 0.25, **out)
    assert e.value.status == ERR_UNSUPPORTED
    # not capturable: TGMS_ERR_UNSUPPORTED inside a capture, which ends normally
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.cut_device(B, *d, 0.25, stream=side.cuda_stream, **out)
        except TgmsError as e:
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is not None and err.status == ERR_UNSUPPORTED
    del g
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all())
    for k, v in out.items():
        assert bool(torch.isnan(v).all()) if v.dtype == torch.float64 else bool((v == -7).all()), k
    # B == 0: TGMS_OK, the total and the first offset
    solver.cut_device(0, None, None, None, None, None, 0.25, **out)
    torch.cuda.synchronize()
    assert out["d_totals"].tolist() == [0] and int(out["d_seg_offsets_out"][0]) == 0
    assert bool(torch.isnan(out["d_seg_times_out"]).all()) and bool((out["d_seg_offsets_out"][1:] == -7).all())


def test_the_tick_on_the_device_with_only_the_offsets_on_the_host(solver, case):
    """cut -> solve_batch_device with device buffers: the re-solve reproduces coeffs_out at 1e-9; the
    new offsets are the only thing copied to the host (the ragged solve's plan needs them)."""
    import torch
    from conftest import batch_rel_err
    c = case
    B, S = H.B0, int(c["so"][-1])
    d = [_dev(c[k]) for k in ("so", "W", "T", "C", "tc")]
    out = _outputs(B, S)
    solver.cut_device(B, *d, H.MIN_FRAC, d_end_derivs=_dev(c["ED"]), **out)
    so2 = out["d_seg_offsets_out"].cpu().numpy()  # the 4 B per trajectory that cross
    S2 = int(so2[-1])
    assert 0 < S2 < S and (np.diff(so2) >= 1).all() and (np.diff(so2) <= np.diff(c["so"])).all()
    dC2 = torch.zeros((S2, 3, 8), dtype=torch.float64, device="cuda")
    dSt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    solver.solve_batch_device(so2, out["d_seg_offsets_out"], out["d_waypoints_out"], out["d_seg_times_out"], dC2, dSt,
                              d_end_derivs=out["d_end_derivs_out"])
    torch.cuda.synchronize()
    assert not dSt.cpu().numpy().any() and int(out["d_totals"][0]) == S2
    err = batch_rel_err(so2, dC2.cpu().numpy(), out["d_coeffs_out"][:S2].cpu().numpy())
    print("re-solve on the device against coeffs_out:", err)
    assert err <= 1e-9
