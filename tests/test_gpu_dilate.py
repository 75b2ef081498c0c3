"""GPU: the time dilation (tgms_dilate_batch / tgms_dilate_batch_device, csrc/tgms_dilate.hip):
the closed forms and the contract of test_dilate_host.py repeated on the device, agreement with
the host backend, and the launch's corners: tiles of four trajectories per wavefront, the
grid-stride loop with a partial tile, rows that finish at different rounds of one tile, bad rows
in the middle of a tile, in place, NULL outputs, graph capture."""
import numpy as np
import pytest

import bounds_ref as R
import dilate_ref as DR
import thrust_ref as TR
from test_dilate_host import (LIM, S_HI, TIGHT, check_closed_forms, check_constant, check_hover_excluded, check_ragged,
                              check_search_heavy, limits_of)

pytestmark = pytest.mark.gpu

G = TR.G0
INF = float("inf")
GRID = 4096  # workgroups of the launch at most (csrc/tgms_dilate.hip launch_dilate)
TILE = 4     # trajectories per workgroup
P0 = np.array([0.3, -1.0, 2.0])


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the fixtures are read-only


def _device_call(solver, so, T, C, lim, s_lo, s_hi=S_HI, g=G, want=(1, 1, 1, 1, 1), in_place=False):
    """tgms_dilate_batch_device on fresh NaN / -9 outputs (those of `want`); numpy results, None
    for an output that was not asked for."""
    import torch
    so = np.asarray(so, np.int32)
    B, S = len(so) - 1, len(np.asarray(T).reshape(-1))
    dso, dT, dC = _dev(so), _dev(np.asarray(T, np.float64).reshape(-1)), _dev(np.asarray(C, np.float64).reshape(-1, 3, 8))
    f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    i32 = lambda n: torch.full((n,), -9, dtype=torch.int32, device="cuda")
    outs = [f64(B) if want[0] else None, i32(B) if want[1] else None, i32(B) if want[2] else None,
            (dT if in_place else f64(S)) if want[3] else None, (dC if in_place else f64(S, 3, 8)) if want[4] else None]
    lk, lt = limits_of(lim)
    solver.dilate_device(B, dso, dT, dC, g, lk, lt, s_lo, s_hi, *outs)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in outs)


def _call(solver):
    return lambda so, T, C, lim, s_lo, s_hi=S_HI, g=G: _device_call(solver, so, T, C, lim, s_lo, s_hi, g)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(x, y):
    return all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(x, y))


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ragged(solver):
    """bounds_ref.ragged48 solved on the GPU, rest to rest and with end_derivs48.  Shared, never
    modified."""
    so, W, T = R.ragged48()
    cases = []
    for name, ED in (("rest", None), ("end_derivs", R.end_derivs48())):
        C, st, worst = solver.solve(so, W, T, ED)
        assert worst == 0
        C.setflags(write=False)
        cases.append(dict(so=so, T=T, C=C, ED=ED, name=name))
    return cases


@pytest.fixture(scope="module")
def mixed():
    """Three M = 1 rest-to-rest rows against f_max = 16: feasible at s_lo (one evaluation),
    capped by s_hi = 3 (two or three), and one that needs the whole search."""
    rows = [R.rest_to_rest(P0, d, 1.0, axis=0) for d in (0.2, 400.0, 4.0)]
    so = np.arange(4, dtype=np.int32)
    return so, np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows])


MIXED_LIM = (INF, INF, INF, 0, 16.0, INF)


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_closed_forms(solver, T):
    check_closed_forms(_call(solver), T)


def test_constant_trajectory(solver):
    check_constant(_call(solver))


def test_limits_that_exclude_hover_are_capped(solver):
    check_hover_excluded(_call(solver))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("s_lo", [1.0, 0.25])
def test_ragged_batches_meet_the_contract_and_the_host(solver, host, ragged, which, s_lo):
    """The contract on the device's output, then the host backend on the same input: s within
    2e-9 relative; active and the flag bits equal wherever the two leading limits of the output
    differ by more than 1e-9 (the excesses of dilate_ref on the device's output say which)."""
    c = ragged[which]
    dev = check_ragged(_call(solver), c, s_lo)
    lk, lt = limits_of(LIM)
    hst = host.dilate(c["so"], c["T"], c["C"], G, lk, lt, s_lo, S_HI)
    _agree(c, dev, hst, LIM)


def _agree(c, dev, hst, lim):
    assert np.abs(dev[0] - hst[0]).max() <= 2e-9 * np.abs(hst[0]).max() and (np.abs(dev[0] / hst[0] - 1) <= 2e-9).all()
    e = np.sort(DR.excesses(DR.quantities(c["so"], dev[3], dev[4]), lim), axis=1)
    clear = np.where(dev[1] == DR.NONE, e[:, -1] < -1e-9, e[:, -1] - e[:, -2] > 1e-9)
    assert clear.sum() >= len(clear) // 2
    assert np.array_equal(dev[1][clear], hst[1][clear])
    assert np.array_equal(dev[2][clear] & DR.MASK, hst[2][clear] & DR.MASK)


@pytest.mark.parametrize("which", [0, 1])
def test_search_heavy_batch(solver, host, ragged, which):
    c = ragged[which]
    dev = check_search_heavy(_call(solver), c)
    lk, lt = limits_of(TIGHT)
    _agree(c, dev, host.dilate(c["so"], c["T"], c["C"], G, lk, lt, 0.25, S_HI), TIGHT)


@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_small_batches(solver, ragged, B):
    """The first B rows alone are bit-equal to the same rows of the 48-row call."""
    c = ragged[0]
    so = c["so"][:B + 1]
    full = _device_call(solver, c["so"], c["T"], c["C"], TIGHT, 0.25)
    part = _device_call(solver, so, c["T"][:so[-1]], c["C"][:so[-1]], TIGHT, 0.25)
    assert _same(part, (full[0][:B], full[1][:B], full[2][:B], full[3][:so[-1]], full[4][:so[-1]]))


def test_grid_stride_with_a_partial_tile(solver, mixed):
    """B = 4 * 4096 + 5 rows of M = 1 repeating the three mixed rows: every workgroup runs a
    second tile on the LDS its first used, the last tile holds one row, and consecutive tiles mix
    the rows differently.  Every row is bit-equal to the row solved alone."""
    so3, T3, C3 = mixed
    alone = [_device_call(solver, so3[:2], T3[i:i + 1], C3[i:i + 1], MIXED_LIM, 1.0, 3.0) for i in range(3)]
    B = TILE * GRID + 5
    src = np.arange(B) % 3
    so = np.arange(B + 1, dtype=np.int32)
    out = _device_call(solver, so, T3[src], C3[src], MIXED_LIM, 1.0, 3.0)
    for k in range(5):
        want = np.concatenate([alone[i][k] for i in range(3)])[src]
        assert np.array_equal(_bits(out[k]), _bits(want)), k


def test_rows_of_one_tile_finish_independently(solver, mixed):
    """One tile: feasible at s_lo, capped, the full search, in every order of the three.  Each
    row is bit-equal to the same trajectory solved alone, and the three took different numbers of
    evaluations."""
    so3, T3, C3 = mixed
    alone = [_device_call(solver, so3[:2], T3[i:i + 1], C3[i:i + 1], MIXED_LIM, 1.0, 3.0) for i in range(3)]
    ev = [int(a[2][0]) >> DR.EVALS_SHIFT for a in alone]
    assert [int(a[2][0]) & DR.MASK for a in alone] == [0, DR.CAPPED, 0]
    assert alone[0][0][0] == 1.0 and alone[1][0][0] == 3.0 and 1.0 < alone[2][0][0] < 3.0
    assert ev[0] == 1 and ev[1] in (2, 3) and ev[2] > ev[1]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1]):
        out = _device_call(solver, so3, T3[order], C3[order], MIXED_LIM, 1.0, 3.0)
        for k in range(5):
            assert np.array_equal(_bits(out[k]), _bits(np.concatenate([alone[i][k] for i in order]))), (order, k)


def test_m1_and_m16_in_one_tile(solver, host):
    """M = 1, 16, 1, 16 in one tile, solved rest to rest: the contract, and each row bit-equal to
    the row alone."""
    rng = np.random.default_rng(11)
    Ms = np.array([1, 16, 1, 16])
    so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    n = so[-1] + 4
    W = np.c_[rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(0.5, 5, n)]
    T = rng.uniform(0.5, 3.0, so[-1])
    C, st, worst = solver.solve(so, W, T)
    assert worst == 0
    out = _device_call(solver, so, T, C, TIGHT, 0.25)
    DR.check_contract(so, out[3], out[4], out[0], out[1], out[2], TIGHT, 0.25, label="M = 1, 16, 1, 16")
    for b in range(4):
        sl = slice(so[b], so[b + 1])
        one = _device_call(solver, np.array([0, Ms[b]], np.int32), T[sl], C[sl], TIGHT, 0.25)
        assert _same(one, (out[0][b:b + 1], out[1][b:b + 1], out[2][b:b + 1], out[3][sl], out[4][sl]))


def test_bad_rows_in_the_middle_of_a_tile(solver, ragged):
    """A NaN coefficient, a time of 0 and a NaN time, then M = 0 and M = 17 from the offsets: each
    such row has s = NaN, active = -1, NONFINITE alone; the rows of a bad trajectory are copied
    unchanged, those of a bad segment count are not written; every other row is bit-equal to the
    clean batch's."""
    c = ragged[0]
    so, T, C = c["so"], c["T"], c["C"]
    ref = _device_call(solver, so, T, C, TIGHT, 0.25)
    C2, T2 = C.copy(), T.copy()
    C2[so[5], 1, 4] = np.nan   # rows 5, 22 and 41 are second or third in their tiles
    T2[so[23] - 1] = 0.0
    T2[so[41]] = np.nan
    bad = [5, 22, 41]
    out = _device_call(solver, so, T2, C2, TIGHT, 0.25)
    keep = np.ones(48, bool)
    keep[bad] = False
    assert np.isnan(out[0][bad]).all() and (out[1][bad] == -1).all() and (out[2][bad] == DR.NONFINITE).all()
    assert _same([o[keep] for o in out[:3]], [o[keep] for o in ref[:3]])
    seg_bad = np.concatenate([np.arange(so[b], so[b + 1]) for b in bad])
    seg_keep = np.setdiff1d(np.arange(so[-1]), seg_bad)
    assert np.array_equal(_bits(out[3][seg_bad]), _bits(T2[seg_bad])) and np.array_equal(_bits(out[4][seg_bad]), _bits(C2[seg_bad]))
    assert _same((out[3][seg_keep], out[4][seg_keep]), (ref[3][seg_keep], ref[4][seg_keep]))
    # device offsets with M = 0 (row 1) and M = 17 (row 2) inside the first tile; the 17 rows keep their fill
    M = np.diff(so)
    so2 = np.cumsum(np.concatenate([[0, M[0], 0, 17], M[1:]])).astype(np.int32)
    T3, C3 = np.full(so2[-1], 1.0), np.full((so2[-1], 3, 8), 0.5)
    T3[:M[0]], C3[:M[0]] = T[:M[0]], C[:M[0]]
    T3[so2[3]:], C3[so2[3]:] = T[M[0]:], C[M[0]:]
    out3 = _device_call(solver, so2, T3, C3, TIGHT, 0.25)
    assert np.isnan(out3[0][[1, 2]]).all() and (out3[1][[1, 2]] == -1).all() and (out3[2][[1, 2]] == DR.NONFINITE).all()
    rest = np.r_[0, 3:50]
    assert _same([o[rest] for o in out3[:3]], ref[:3])
    gap = slice(so2[2], so2[3])
    assert np.isnan(out3[3][gap]).all() and np.isnan(out3[4][gap]).all()  # nothing written for M = 17
    segs = np.r_[0:M[0], so2[3]:so2[-1]]
    assert _same((out3[3][segs], out3[4][segs]), ref[3:])


def test_in_place_and_null_outputs(solver, ragged):
    """In place is bit-equal to out of place; each output alone gives the bits of the full call,
    and the others stay untouched (they are not allocated here)."""
    c = ragged[1]
    full = _device_call(solver, c["so"], c["T"], c["C"], TIGHT, 0.25)
    inpl = _device_call(solver, c["so"], c["T"], c["C"], TIGHT, 0.25, in_place=True)
    assert _same(full, inpl) and not np.array_equal(full[4], c["C"])
    for k in range(5):
        want = [0] * 5
        want[k] = 1
        out = _device_call(solver, c["so"], c["T"], c["C"], TIGHT, 0.25, want=want)
        assert np.array_equal(_bits(out[k]), _bits(full[k])) and all(out[j] is None for j in range(5) if j != k)


def test_host_pointer_call_gives_the_device_call_bits(solver, ragged):
    c = ragged[0]
    lk, lt = limits_of(TIGHT)
    assert _same(solver.dilate(c["so"], c["T"], c["C"], G, lk, lt, 0.25, S_HI),
                 _device_call(solver, c["so"], c["T"], c["C"], TIGHT, 0.25))


def test_argument_errors_launch_nothing(solver, host, ragged):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, Limits, TgmsError, ThrustLimits
    c = ragged[0]
    B = 48
    dso, dT, dC = _dev(c["so"]), _dev(c["T"]), _dev(c["C"])
    sc = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    odd = torch.full((B + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    nan = float("nan")
    for kw in (dict(d_scale=odd), dict(limits=Limits(a_max=nan), d_scale=sc), dict(tlimits=ThrustLimits(f_max=nan), d_scale=sc),
               dict(s_lo=0.0, d_scale=sc), dict(s_lo=2.0, s_hi=1.0, d_scale=sc), dict(s_hi=INF, d_scale=sc),
               dict(tlimits=ThrustLimits(tilt_max=np.pi / 2), d_scale=sc), dict(g=-1.0, d_scale=sc), dict()):
        with pytest.raises(TgmsError) as e:
            solver.dilate_device(B, dso, dT, dC, **kw)
        assert e.value.status == ERR_INVALID_ARG, kw
    solver.dilate_device(0, None, None, None, d_scale=sc)  # B == 0: TGMS_OK, nothing launched
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.dilate_device(B, dso, dT, dC, d_scale=sc)
    assert e.value.status == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(sc).all()) and bool(torch.isnan(odd).all())


def test_captured_into_a_graph_and_replayed(solver, ragged):
    """The device call on the ragged batch inside torch.cuda.graph; the replay after the inputs
    were overwritten with the end-derivative coefficients is bit-equal to a direct call on them."""
    import torch
    want = [_device_call(solver, c["so"], c["T"], c["C"], TIGHT, 0.25) for c in ragged]
    assert not np.array_equal(want[0][0], want[1][0])
    c = ragged[0]
    B, S = 48, int(c["so"][-1])
    dso, dT, dC = _dev(c["so"]), _dev(c["T"]), _dev(c["C"])
    outs = [torch.full((B,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((B,), -9, dtype=torch.int32, device="cuda"), torch.full((B,), -9, dtype=torch.int32, device="cuda"),
            torch.full((S,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((S, 3, 8), float("nan"), dtype=torch.float64, device="cuda")]
    lk, lt = limits_of(TIGHT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.dilate_device(B, dso, dT, dC, G, lk, lt, 0.25, S_HI, *outs, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for cc, w in zip(ragged, want):
        dC.copy_(_dev(cc["C"]))
        for o in outs:
            o.fill_(float("nan") if o.dtype == torch.float64 else -9)
        g.replay()
        torch.cuda.synchronize()
        assert _same([o.cpu().numpy() for o in outs], w)
    del g
