"""GPU: the continuous body-rate bound (tgms_rate_batch / tgms_rate_batch_device,
csrc/tgms_rate.hip): the closed form, the exact zeros and the 1e-9 F J / m^2 contract of
test_rate_host.py repeated on the device, agreement with the host backend, and the launch's
corners: a full 64-lane tile beside a tail tile, the grid-stride loop, bad rows in the middle of
a tile, nullable outputs, argument errors, graph capture and the host-pointer call."""
import numpy as np
import pytest

import rate_ref as RR
from test_rate_host import bad_rows, check_bad_rows, check_closed_form, check_exact_zeros

pytestmark = pytest.mark.gpu

G = RR.G0
GRID = 4096  # workgroups of the launch at most (csrc/tgms_rate.hip launch_rate)
TILE = 4     # trajectories per workgroup


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the fixtures are read-only


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _device_call(solver, so, T, C, g=G, limit=float("inf"), rec=True, seg=True, flags=True):
    """tgms_rate_batch_device on fresh NaN / -7 outputs; returns numpy (rec, seg_rec, flags), None
    for an output left out."""
    import torch
    B, S = len(so) - 1, int(np.asarray(T).size)
    d_rec = torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda") if rec else None
    d_seg = torch.full((S, 2), float("nan"), dtype=torch.float64, device="cuda") if seg else None
    d_fl = torch.full((B,), -7, dtype=torch.int32, device="cuda") if flags else None
    solver.rate_device(B, _dev(np.asarray(so, np.int32)), _dev(np.asarray(T, np.float64).reshape(-1)),
                       _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)), g, limit, d_rec, d_seg, d_fl)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (d_rec, d_seg, d_fl))


def _call(solver, limit=float("inf")):
    return lambda so, T, C, g: _device_call(solver, so, T, C, g, limit)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ragged(solver):
    """ragged.npz with its reference, a limit that flags about half of it, and the device's
    outputs under that limit.  Shared, never modified."""
    fx = RR.fixture("ragged")
    lim = float(np.median(fx["omega"]))
    out = _device_call(solver, fx["so"], fx["T"], fx["C"], G, lim)
    for a in out:
        a.setflags(write=False)
    return dict(fx=fx, lim=lim, out=out)


def test_closed_form_single_segment(solver):
    check_closed_form(_call(solver))


def test_constant_and_vertical_give_zero(solver):
    check_exact_zeros(_call(solver))


@pytest.mark.parametrize("name", RR.FIXTURES)
def test_golden_batches_meet_the_contract(solver, host, name):
    """Within 1e-9 F J / m^2 of the reference and of the host backend, the times in range and
    attaining the stored values, the segment rows consistent with the records."""
    fx = RR.fixture(name)
    rec, seg, fl = _device_call(solver, fx["so"], fx["T"], fx["C"])
    assert not fl.any()
    RR.check_contract(rec, seg, fx, name + ", device")
    rec_h, seg_h, _ = host.rate(fx["so"], fx["T"], fx["C"])
    e = np.abs(rec[:, 0] - rec_h[:, 0]) / fx["scale"]
    e_seg = np.abs(seg[:, 0] - seg_h[:, 0]) / np.repeat(fx["scale"], np.diff(fx["so"]))
    print("rate, device vs host (%s): %.3g, segment rows %.3g x F J / m^2" % (name, e.max(), e_seg.max()))
    assert (e <= 1e-9).all() and (e_seg <= 1e-9).all()


def test_full_tile_and_tail_tile(solver):
    """B = 5 with segment counts 16, 16, 16, 16, 1: all 64 lanes of the first tile, one lane of
    the second.  Every row is bit-equal to the row of the batch it came from."""
    ex, rg = RR.fixture("extreme"), RR.fixture("ragged")
    assert list(np.diff(ex["so"])) == [16] * 4 and rg["so"][1] == 1
    so = np.array([0, 16, 32, 48, 64, 65], np.int32)
    T, C = np.concatenate([ex["T"], rg["T"][:1]]), np.concatenate([ex["C"], rg["C"][:1]])
    rec, seg, fl = _device_call(solver, so, T, C)
    rec_e, seg_e, _ = _device_call(solver, ex["so"], ex["T"], ex["C"])
    rec_r, seg_r, _ = _device_call(solver, rg["so"], rg["T"], rg["C"])
    assert not fl.any() and np.isfinite(rec).all()
    assert np.array_equal(_bits(rec), _bits(np.concatenate([rec_e, rec_r[:1]])))
    assert np.array_equal(_bits(seg), _bits(np.concatenate([seg_e, seg_r[:1]])))


def test_bad_rows_in_the_middle_of_a_tile(solver, ragged):
    """A NaN coefficient, a time of 0, of -1 and NaN, then M = 0 and M = 17 from the offsets:
    each such row has NONFINITE alone and a NaN record, every other row is bit-equal to the clean
    batch's; for a bad segment count no segment row is written."""
    from trajectory_generator_ros2_amd import FEAS_NONFINITE
    fx, lim = ragged["fx"], ragged["lim"]
    rec0, seg0, fl0 = ragged["out"]
    check_bad_rows(_call(solver, lim), fx, ragged["out"])
    # device offsets with M = 0 (row 1) and M = 17 (row 2) inside the first tile, between rows 0
    # and 1 of the batch; rows 2.. of the batch follow
    so, T, C = fx["so"], fx["T"], fx["C"]
    M = np.diff(so)
    so2 = np.cumsum(np.concatenate([[0, M[0], 0, 17], M[1:]])).astype(np.int32)
    T3, C3 = np.full(so2[-1], 1.0), np.full((so2[-1], 3, 8), 0.5)
    T3[:M[0]], C3[:M[0]] = T[:M[0]], C[:M[0]]
    T3[so2[3]:], C3[so2[3]:] = T[M[0]:], C[M[0]:]
    rec3, seg3, fl3 = _device_call(solver, so2, T3, C3, G, lim)
    assert list(fl3[[1, 2]]) == [FEAS_NONFINITE] * 2 and np.isnan(rec3[[1, 2]]).all()
    rest = np.r_[0, 3:len(fl3)]
    assert np.array_equal(fl3[rest], fl0) and np.array_equal(_bits(rec3[rest]), _bits(rec0))
    assert np.isnan(seg3[so2[2]:so2[3]]).all()  # the prefill: nothing written for the 17 rows
    assert np.array_equal(_bits(np.concatenate([seg3[:so2[1]], seg3[so2[3]:]])), _bits(seg0))


def test_grid_stride_and_lds_reuse(solver, ragged):
    """B = 4 * 4096 + 3 copies of one golden trajectory (M = 7): every workgroup runs a second
    tile on the LDS its first used, three rows more start a third round.  Every row is bit-equal
    to row 0, which is the trajectory's row in the 24-row call."""
    fx, lim = ragged["fx"], ragged["lim"]
    b, B = 6, TILE * GRID + 3
    s0, s1 = int(fx["so"][b]), int(fx["so"][b + 1])
    M = s1 - s0
    assert M == 7
    so = (np.arange(B + 1) * M).astype(np.int32)
    rec, seg, fl = _device_call(solver, so, np.tile(fx["T"][s0:s1], B), np.tile(fx["C"][s0:s1], (B, 1, 1)), G, lim)
    assert np.array_equal(_bits(rec[0]), _bits(ragged["out"][0][b])) and fl[0] == ragged["out"][2][b]
    assert np.array_equal(_bits(seg[:M]), _bits(ragged["out"][1][s0:s1]))
    assert (_bits(rec) == _bits(rec[0])).all() and (fl == fl[0]).all()
    assert (_bits(seg).reshape(B, M * 2) == _bits(seg[:M]).reshape(-1)).all()


def test_nullable_outputs(solver, ragged):
    """Each output omitted in turn, and each alone: what is asked for is bit-equal to the full
    call's (the prefill of NaN / -7 is gone from all of it)."""
    fx, lim = ragged["fx"], ragged["lim"]
    rec0, seg0, fl0 = ragged["out"]
    assert fl0.any() and not fl0.all() and not np.isnan(rec0).any() and not np.isnan(seg0).any()
    for mask in (0b110, 0b101, 0b011, 0b001, 0b010, 0b100):
        rec, seg, fl = _device_call(solver, fx["so"], fx["T"], fx["C"], G, lim, rec=bool(mask & 1), seg=bool(mask & 2),
                                    flags=bool(mask & 4))
        assert (rec is None) == (not mask & 1) and (seg is None) == (not mask & 2) and (fl is None) == (not mask & 4)
        assert rec is None or np.array_equal(_bits(rec), _bits(rec0))
        assert seg is None or np.array_equal(_bits(seg), _bits(seg0))
        assert fl is None or np.array_equal(fl, fl0)


def test_flag_is_strict_on_the_stored_value(solver, ragged):
    from trajectory_generator_ros2_amd import RATE_HIGH
    fx = ragged["fx"]
    rec0, _, fl0 = ragged["out"]
    assert np.array_equal(fl0, np.where(rec0[:, 0] > ragged["lim"], RATE_HIGH, 0))
    top = rec0[:, 0].max()
    assert not _device_call(solver, fx["so"], fx["T"], fx["C"], G, top)[2].any()
    fl = _device_call(solver, fx["so"], fx["T"], fx["C"], G, np.nextafter(top, 0.0))[2]
    assert np.array_equal(fl, np.where(rec0[:, 0] == top, RATE_HIGH, 0)) and fl.any()
    for lim in (float("inf"), -float("inf")):
        assert not _device_call(solver, fx["so"], fx["T"], fx["C"], G, lim)[2].any()


def test_argument_errors_launch_nothing(solver, host, ragged):
    import torch
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError
    fx = ragged["fx"]
    B, S = len(fx["so"]) - 1, int(fx["so"][-1])
    dso, dT, dC = _dev(fx["so"]), _dev(fx["T"]), _dev(fx["C"])
    odd = torch.full((S * 2 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    rec = torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    for kw in (dict(d_rec=rec, d_seg_rec=odd, d_flags=fl), dict(omega_limit=float("nan"), d_rec=rec, d_flags=fl),
               dict(g=float("nan"), d_rec=rec, d_flags=fl), dict(g=-1.0, d_rec=rec, d_flags=fl),
               dict(g=float("inf"), d_rec=rec, d_flags=fl), dict(d_rec=None, d_seg_rec=None, d_flags=None)):
        with pytest.raises(TgmsError) as e:
            solver.rate_device(B, dso, dT, dC, **kw)
        assert e.value.status == ERR_INVALID_ARG
    solver.rate_device(0, None, None, None, d_rec=rec, d_flags=fl)  # B == 0: TGMS_OK, nothing launched
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.rate_device(B, dso, dT, dC, d_rec=rec, d_flags=fl)
    assert e.value.status == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all()) and bool(torch.isnan(rec).all()) and bool((fl == -7).all())


def test_host_pointer_call_gives_the_device_call_bits(solver, ragged):
    fx, lim = ragged["fx"], ragged["lim"]
    rec_h, seg_h, fl_h = solver.rate(fx["so"], fx["T"], fx["C"], G, lim)
    rec_d, seg_d, fl_d = ragged["out"]
    assert np.array_equal(_bits(rec_h), _bits(rec_d)) and np.array_equal(_bits(seg_h), _bits(seg_d))
    assert np.array_equal(fl_h, fl_d) and fl_d.any()


def test_captured_into_a_graph_and_replayed(solver, ragged):
    """One capture of the device call on the ragged batch inside torch.cuda.graph and one replay
    onto prefilled outputs: bit-equal to the direct call."""
    import torch
    fx, lim = ragged["fx"], ragged["lim"]
    rec0, seg0, fl0 = ragged["out"]
    B, S = len(fx["so"]) - 1, int(fx["so"][-1])
    dso, dT, dC = _dev(fx["so"]), _dev(fx["T"]), _dev(fx["C"])
    rec = torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda")
    seg = torch.full((S, 2), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.rate_device(B, dso, dT, dC, G, lim, rec, seg, fl, stream=side.cuda_stream)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    rec.fill_(float("nan"))
    seg.fill_(float("nan"))
    fl.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rec.cpu().numpy()), _bits(rec0))
    assert np.array_equal(_bits(seg.cpu().numpy()), _bits(seg0))
    assert np.array_equal(fl.cpu().numpy(), fl0)
    del g
