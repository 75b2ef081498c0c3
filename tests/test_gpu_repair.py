"""GPU: the waypoint repair (tgms_field_nearest_free / tgms_waypoints_repair_batch on a GPU handle and
the two `_dev` entry points, csrc/tgms_repair.hip).  The cases of test_repair_host.py run through both
(repair_ref.py), then the launch's own corners: host / device equality on a batch larger than one
launch tile and on B = 1, a bad segment count between good neighbours, sentinels around every device
output, a repeated call, both calls captured into one HIP graph and replayed, a host handle, the
invalid arguments of each call, and the chain nearest_free -> repair -> subdivide -> re-route ->
inflate -> solve on device buffers."""
import numpy as np
import pytest

import repair_ref as RP
from conftest import check_spline_properties
from trajectory_generator_ros2_amd import (ERR_INVALID_ARG, ERR_UNSUPPORTED, FEAS_NONFINITE, INF_BLOCKED, INF_OUTSIDE,
                                           OK, RPR_KEEP_FIRST, RPR_KEEP_LAST, RPR_MOVED, RRT_BLOCKED, RRT_ENDS,
                                           RRT_OUTSIDE, TgmsError)

pytestmark = pytest.mark.gpu
PAD = 8  # sentinel rows on either side of every device output


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).cuda()  # a copy: the shared inputs are read-only


def _padded(rows, cols, dtype, fill):
    """A buffer of `rows` rows between PAD sentinel rows: (whole, the caller's view); with PAD = 8
    every view is 16-byte aligned."""
    import torch
    shape = (rows + 2 * PAD,) + ((cols,) if cols else ())
    whole = torch.full(shape, fill, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + rows]


def _intact(whole, used):
    w = whole.cpu().numpy()
    assert (w[:PAD] == -9).all() and (w[PAD + used:] == -9).all(), "a sentinel was written"


def map_device(solver, values, origin, h, r_free, max_shift, want_dsq=True):
    """tgms_field_nearest_free_dev between sentinels: (n, nearest, dsq) with the maps on the device."""
    import torch
    v = np.ascontiguousarray(values, dtype=np.float32)
    n, N = v.shape[::-1], v.size
    assert solver.field_nearest_free_work_size(origin, h, n) == 4 * N
    near_w, near = _padded(N, 0, torch.int32, -9)
    dsq_w, dsq = _padded(N, 0, torch.int32, -9)
    work_w, work = _padded(N, 0, torch.int32, -9)
    solver.field_nearest_free_device(origin, h, n, _dev(v), r_free, max_shift, near, work, dsq if want_dsq else None)
    torch.cuda.synchronize()
    for whole in (near_w, dsq_w, work_w):
        _intact(whole, N)
    assert want_dsq or (dsq == -9).all()
    return n, near, dsq


def repair_device(solver, so, W, T, origin, h, values, r_free, max_shift, mode, so_dev=None):
    """The two device calls, the second between sentinels; the five outputs as a Solver returns them."""
    import torch
    so = np.asarray(so, np.int32)
    B, rows = len(so) - 1, len(np.asarray(W).reshape(-1, 3))
    S = rows - B
    n, near, _ = map_device(solver, values, origin, h, r_free, max_shift, want_dsq=False)
    W_w, W_o = _padded(rows, 3, torch.float64, -9.0)
    T_w, T_o = _padded(S, 0, torch.float64, -9.0)
    wf_w, wf_o = _padded(rows, 0, torch.int32, -9)
    sh_w, sh_o = _padded(rows, 0, torch.int32, -9)
    fl_w, fl_o = _padded(B, 0, torch.int32, -9)
    dT = None if T is None else _dev(np.asarray(T, np.float64))
    solver.waypoints_repair_device(B, _dev(so if so_dev is None else so_dev), _dev(np.asarray(W, np.float64).reshape(-1, 3)),
                                   origin, h, n, near, mode, W_o, d_seg_times=dT,
                                   d_seg_times_out=None if T is None else T_o, d_wp_flags=wf_o, d_shift=sh_o, d_flags=fl_o)
    torch.cuda.synchronize()
    for whole, used in ((W_w, rows), (T_w, S if T is not None else 0), (wf_w, rows), (sh_w, rows), (fl_w, B)):
        _intact(whole, used)
    c = lambda x: x.cpu().numpy()  # noqa: E731
    return c(W_o), None if T is None else c(T_o), c(wf_o), c(fl_o), c(sh_o)


class Device:
    """The device entry points behind the backend interface of repair_ref.py."""

    def __init__(self, solver):
        self.s = solver

    def field_nearest_free(self, values, origin, h, r_free, max_shift):
        _, near, dsq = map_device(self.s, values, origin, h, r_free, max_shift)
        shape = np.asarray(values).shape
        return near.cpu().numpy().reshape(shape), dsq.cpu().numpy().reshape(shape)

    def waypoints_repair(self, so, W, origin, h, values, r_free, max_shift, mode=0, seg_times=None):
        return repair_device(self.s, so, W, seg_times, origin, h, values, r_free, max_shift, mode)


@pytest.fixture(scope="module", params=["host_pointers", "device"])
def be(request, solver):
    return solver if request.param == "host_pointers" else Device(solver)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


def test_constructed_maps(be):
    RP.check_all_free(be)
    RP.check_all_blocked(be)
    RP.check_one_blocked_node(be)
    RP.check_one_free_node(be)
    RP.check_plane_line_corner(be)
    RP.check_reach(be)
    RP.check_nan_and_threshold(be)


@pytest.mark.parametrize("fill,max_shift", [(0.1, 2), (0.5, 3), (0.9, 5), (0.98, 40), (0.999, 7)])
def test_random_maps(be, fill, max_shift):
    RP.check_random(be, fill, max_shift)


def test_tile_seams(be, host):
    """Every seam grid at a short and a long reach, against the host backend (which test_repair_host.py
    holds to the brute-force reference on the same grids)."""
    for n in RP.seam_grids():
        v = RP.random_map(n, 0.93, n[0] + 7 * n[1] + 13 * n[2])
        for reach in (4, 200):
            got, want = be.field_nearest_free(v, RP.O, RP.H, RP.RF, reach), host.field_nearest_free(v, RP.O, RP.H, RP.RF, reach)
            assert RP.same_bits(got[0], want[0]) and RP.same_bits(got[1], want[1]), (n, reach)


def test_waypoint_outcomes(be):
    RP.check_outcomes(be)
    RP.check_stuck_and_reach(be)
    RP.check_outside_and_nonfinite(be)
    RP.check_modes(be)
    RP.check_zero_length_leg(be)
    RP.check_times(be)


@pytest.mark.parametrize("fill,max_shift,mode", [(0.2, 2, 0), (0.5, 3, RPR_KEEP_FIRST), (0.8, 6, RPR_KEEP_LAST),
                                                  (0.95, 2, RPR_KEEP_FIRST | RPR_KEEP_LAST)])
def test_random_batches(be, fill, max_shift, mode):
    RP.check_random_batch(be, fill, max_shift, mode)


def test_arguments(solver):
    RP.check_arguments(solver, TgmsError, ERR_INVALID_ARG)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 1500])
def test_batch_sizes_equal_the_host_and_repeat(solver, host, B):
    """A workgroup takes 16 trajectories; B = 1, one workgroup's seam and many workgroups.  Twice: the
    bits repeat."""
    v = RP.random_map(RP.RANDOM_N, 0.4, 5)
    so, W, T = RP.dyadic_batch(B, B, RP.RANDOM_N, m_hi=16 if B < 100 else 5)
    a = (so, W, RP.O, RP.H, v, RP.RF, 3, RPR_KEEP_FIRST, T)
    want = host.waypoints_repair(*a)
    assert B < 15 or (want[2] == RPR_MOVED).any()
    first = Device(solver).waypoints_repair(*a)
    RP.assert_same(first, want, "device")
    RP.assert_same(Device(solver).waypoints_repair(*a), first, "repeated")
    RP.assert_same(solver.waypoints_repair(*a), want, "host pointers")


@pytest.mark.parametrize("count", [0, 17])
def test_bad_segment_count_between_good_neighbours(solver, host, count):
    """A trajectory with `count` segments inserted at position 5: its rows keep the sentinel, its flag
    is FEAS_NONFINITE, the neighbours are bit-equal to the batch without it."""
    v = RP.random_map(RP.RANDOM_N, 0.4, 5)
    so, W, T = RP.dyadic_batch(11, 31, RP.RANDOM_N)
    want = host.waypoints_repair(so, W, RP.O, RP.H, v, RP.RF, 3, 0, T)
    at = 5
    s, w = int(so[at]), int(so[at]) + at
    so_bad = np.concatenate([so[:at + 1], so[at:] + count]).astype(np.int32)
    W_bad = np.concatenate([W[:w], np.full((count + 1, 3), 3.5), W[w:]])
    T_bad = np.concatenate([T[:s], np.ones(count), T[s:]])
    got = repair_device(solver, so_bad, W_bad, T_bad, RP.O, RP.H, v, RP.RF, 3, 0)
    for g, e, cut, gap in ((got[0], want[0], w, count + 1), (got[1], want[1], s, count), (got[2], want[2], w, count + 1),
                           (got[4], want[4], w, count + 1)):
        assert RP.same_bits(g[:cut], e[:cut]) and RP.same_bits(g[cut + gap:], e[cut:])
        assert (g[cut:cut + gap] == -9).all()
    assert np.array_equal(got[3], np.concatenate([want[3][:at], [FEAS_NONFINITE], want[3][at:]]))


def test_both_calls_in_one_graph(solver, host):
    """Neither call uses handle scratch: map and repair are captured into one HIP graph and replayed
    on new values and waypoints in the same buffers."""
    import torch
    v = RP.random_map(RP.RANDOM_N, 0.4, 5)
    so, W, T = RP.dyadic_batch(50, 2, RP.RANDOM_N)
    n, N, rows = RP.RANDOM_N, v.size, len(W)
    dv, dso, dW, dT = _dev(v), _dev(so), _dev(W), _dev(T)
    near, work = _dev(np.full(N, -9, np.int32)), _dev(np.full(N, -9, np.int32))
    W_o, T_o = _dev(np.full((rows, 3), -9.0)), _dev(np.full(len(T), -9.0))
    wf, sh, fl = (_dev(np.full(k, -9, np.int32)) for k in (rows, rows, 50))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        solver.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 3, near, work, stream=side.cuda_stream)
        solver.waypoints_repair_device(50, dso, dW, RP.O, RP.H, n, near, RPR_KEEP_LAST, W_o, d_seg_times=dT,
                                       d_seg_times_out=T_o, d_wp_flags=wf, d_shift=sh, d_flags=fl, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    c = lambda x: x.cpu().numpy()  # noqa: E731
    for vals, (_, Wk, Tk) in ((v, (so, W, T)), (RP.random_map(n, 0.6, 9), RP.dyadic_batch(50, 2, n, frac=4))):
        dv.copy_(torch.from_numpy(vals))
        dW.copy_(torch.from_numpy(Wk))
        dT.copy_(torch.from_numpy(Tk))
        g.replay()
        torch.cuda.synchronize()
        want = host.waypoints_repair(so, Wk, RP.O, RP.H, vals, RP.RF, 3, RPR_KEEP_LAST, Tk)
        RP.assert_same((c(W_o), c(T_o), c(wf), c(fl), c(sh)), want, "replay")
    del g


def test_host_handle_and_invalid_arguments_of_the_device_calls(solver, host):
    import torch
    v = RP.block()
    so, W, T = RP.path([(1, 1, 2), (6, 5, 2), (10, 10, 2)])
    n, N = (12, 12, 6), v.size
    dv, dso, dW, dT = _dev(v), _dev(so), _dev(W), _dev(T)
    near, work, W_o, T_o = _dev(np.zeros(N, np.int32)), _dev(np.zeros(N, np.int32)), _dev(np.zeros((3, 3))), _dev(np.zeros(2))
    with pytest.raises(TgmsError) as e:
        host.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 3, near, work)
    assert e.value.status == ERR_UNSUPPORTED and "tgms_field_nearest_free_dev" in str(e.value)
    with pytest.raises(TgmsError) as e:
        host.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, near, 0, W_o)
    assert e.value.status == ERR_UNSUPPORTED and "tgms_waypoints_repair_batch_dev" in str(e.value)
    odd4 = torch.zeros(4 * N + 4, dtype=torch.uint8, device="cuda")[1:4 * N + 1]
    odd8 = torch.zeros(10, dtype=torch.float64, device="cuda")[1:].reshape(3, 3)
    big = (16385, 2, 2)
    bad = [lambda: solver.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 0, near, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 32769, near, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, n, dv, float("nan"), 3, near, work),
           lambda: solver.field_nearest_free_device(RP.O, 0.0, n, dv, RP.RF, 3, near, work),
           lambda: solver.field_nearest_free_device((0.0, 0.0, float("inf")), RP.H, n, dv, RP.RF, 3, near, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, (12, 1, 6), dv, RP.RF, 3, near, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, big, dv, RP.RF, 3, near, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, n, None, RP.RF, 3, near, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 3, None, work),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 3, near, None),
           lambda: solver.field_nearest_free_device(RP.O, RP.H, n, dv, RP.RF, 3, odd4, work),
           lambda: solver.waypoints_repair_device(-1, dso, dW, RP.O, RP.H, n, near, 0, W_o),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, near, 4, W_o),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, None, 0, W_o),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, near, 0, None),
           lambda: solver.waypoints_repair_device(1, None, dW, RP.O, RP.H, n, near, 0, W_o),
           lambda: solver.waypoints_repair_device(1, dso, None, RP.O, RP.H, n, near, 0, W_o),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, near, 0, W_o, d_seg_times=dT),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, near, 0, W_o, d_seg_times_out=T_o),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, n, near, 0, odd8),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, -1.0, n, near, 0, W_o),
           lambda: solver.waypoints_repair_device(1, dso, dW, RP.O, RP.H, big, near, 0, W_o)]
    for i, call in enumerate(bad):
        with pytest.raises(TgmsError) as e:
            call()
        assert e.value.status == ERR_INVALID_ARG, i
    solver.waypoints_repair_device(0, None, None, RP.O, RP.H, n, near, 0, None)  # B == 0: nothing to do
    torch.cuda.synchronize()
    assert not W_o.any()


def test_chain_on_device_buffers(solver, host):
    """The scene of repair_ref.chain_scene (h = 0.125, dyadic): nearest_free -> repair -> table ->
    subdivide -> re-route -> inflate on device buffers, then the solve.  The parent chain reports
    RRT_ENDS; after the repair no re-route input leg whose two waypoints are clear carries it, and no
    unsplit leg whose two waypoints were clear or MOVED."""
    import torch
    v, so, W, T = RP.chain_scene()
    o, h, rf, c = RP.CHAIN_O, RP.CHAIN_H, RP.CHAIN_RF, RP.CHAIN
    sub0 = host.corridor_subdivide(so, W, o, h, v, rf, c["max_depth"], T)
    rr0 = solver.corridor_reroute(sub0[0], sub0[1], o, h, v, rf, c["margin"], c["max_pieces"], sub0[2])
    assert (rr0[4] & RRT_ENDS).any(), "the scene must show the parent chain's gap"
    B, S, n, N = len(so) - 1, int(so[-1]), RP.CHAIN_N, v.size
    i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")
    dv, dso = _dev(v), _dev(so)
    near, work = torch.zeros(N, **i32), torch.zeros(N, **i32)
    solver.field_nearest_free_device(o, h, n, dv, rf, c["max_shift"], near, work)
    Wr, Tr, wp = torch.zeros((S + B, 3), **f64), torch.zeros(S, **f64), torch.zeros(S + B, **i32)
    solver.waypoints_repair_device(B, dso, _dev(W), o, h, n, near, 0, Wr, d_seg_times=_dev(T), d_seg_times_out=Tr,
                                   d_wp_flags=wp)
    t = torch.zeros((n[2] + 1, n[1] + 1, n[0] + 1), **i32)
    solver.field_occupancy_device(o, h, n, dv, rf, t)
    cap1 = min(S << c["max_depth"], 16 * B)
    so1, W1, T1 = torch.zeros(B + 1, **i32), torch.zeros((cap1 + B, 3), **f64), torch.ones(cap1, **f64)
    par1, tot1 = torch.zeros(cap1, **i32), torch.zeros(2, **i64)
    solver.corridor_subdivide_device(B, dso, Wr, o, h, n, t, c["max_depth"], so1, W1, tot1, d_seg_times=Tr,
                                     d_seg_times_out=T1, d_parent=par1)
    wp1 = torch.zeros(cap1 + B, **i32)  # the repair once more, as a classifier of the subdivision's waypoints
    scratch_W = torch.zeros((cap1 + B, 3), **f64)
    solver.waypoints_repair_device(B, so1, W1, o, h, n, near, 0, scratch_W, d_wp_flags=wp1)
    cap2 = 16 * B
    so2, W2, T2 = torch.zeros(B + 1, **i32), torch.zeros((cap2 + B, 3), **f64), torch.ones(cap2, **f64)
    par2, rrt_seg, tot2 = torch.full((cap2,), -1, **i32), torch.zeros(cap2, **i32), torch.zeros(2, **i64)
    solver.corridor_reroute_device(B, so1, W1, o, h, n, t, c["margin"], c["max_pieces"], so2, W2, tot2, d_seg_times=T1,
                                   d_seg_times_out=T2, d_parent=par2, d_seg_flags_out=rrt_seg)
    faces, fo, inf_seg = torch.zeros((6 * cap2, 4), **f64), torch.zeros(cap2 + 1, **i64), torch.zeros(cap2, **i32)
    solver.corridor_inflate_device(B, so2, W2, o, h, n, t, c["max_grow"], d_faces=faces, d_face_offsets=fo,
                                   d_seg_flags=inf_seg)
    torch.cuda.synchronize()
    S1, S2 = int(tot1[0]), int(tot2[0])
    h_so1, h_so2 = so1.cpu().numpy(), so2.cpu().numpy()
    # the repair on the device is the host backend's
    want = host.waypoints_repair(so, W, o, h, v, rf, c["max_shift"], 0, T)
    assert RP.same_bits(Wr.cpu().numpy(), want[0]) and RP.same_bits(Tr.cpu().numpy(), want[1])
    h_wp, h_par1 = wp.cpu().numpy(), par1[:S1].cpu().numpy()
    assert RP.same_bits(h_wp, want[2]) and (h_wp == RPR_MOVED).any()
    clear = wp1[:S1 + B].cpu().numpy() == 0
    ok = RP.legs_with_good_ends(h_so1, np.where(clear, 0, RPR_MOVED + 1))
    whole = RP.legs_with_good_ends(so, h_wp)[h_par1] & (np.bincount(h_par1, minlength=S)[h_par1] == 1)
    assert whole.any() and not (whole & ~ok).any()
    a, b, p = rrt_seg[:S2].cpu().numpy(), inf_seg[:S2].cpu().numpy(), par2[:S2].cpu().numpy()
    assert ok.any() and not ((a & RRT_ENDS) != 0)[ok[p]].any()
    # guarantee 2 of the re-route still holds on the repaired batch
    assert np.array_equal((a & RRT_BLOCKED) != 0, (b & INF_BLOCKED) != 0)
    assert np.array_equal((a & RRT_OUTSIDE) != 0, (b & INF_OUTSIDE) != 0)
    C, st = torch.zeros((S2, 3, 8), **f64), torch.full((B,), -1, **i32)
    solver.solve_batch_device(h_so2, so2, W2, T2, C, st)
    torch.cuda.synchronize()
    solved = st.cpu().numpy() == OK
    assert solved.sum() >= B // 2
    check_spline_properties(*RP.subset(h_so2, W2[:S2 + B].cpu().numpy(), T2[:S2].cpu().numpy(), C.cpu().numpy(), solved))
