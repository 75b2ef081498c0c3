"""GPU: the corridor re-route (tgms_corridor_reroute_batch on a GPU handle and
tgms_corridor_reroute_batch_dev, csrc/tgms_reroute.hip).  The cases of test_reroute_host.py run
through both entry points (reroute_ref.py), then the launch's own corners: host / device equality at
the seams of the 256-entry scan, no candidate, one candidate, more candidates than the persistent
grid has workgroups, a bad segment count between good neighbours, sentinels around every device
output and rows past S' untouched, a repeated call, a capturing stream, a host handle, and the
pipeline subdivide -> re-route -> inflate -> solve -> containment on device buffers."""
import numpy as np
import pytest

import reroute_ref as RR
from trajectory_generator_ros2_amd import (ERR_INVALID_ARG, ERR_UNSUPPORTED, FEAS_NONFINITE, INF_BLOCKED, INF_OUTSIDE,
                                           NEAR_NONE, OK, RRT_BLOCKED, RRT_DONE, RRT_OUTSIDE, SUB_BLOCKED, TgmsError)

pytestmark = pytest.mark.gpu
PAD = 8  # sentinel rows on either side of every device output


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).cuda()  # a copy: the shared inputs are read-only


def _table(solver, origin, h, values, r_free):
    import torch
    v = np.ascontiguousarray(values, dtype=np.float32)
    n = v.shape[::-1]
    t = torch.full((n[2] + 1, n[1] + 1, n[0] + 1), -7, dtype=torch.int32, device="cuda")
    solver.field_occupancy_device(origin, h, n, _dev(v), r_free, t)
    return n, t


def _padded(rows, cols, dtype, fill):
    """A buffer of `rows` rows between PAD sentinel rows: (whole, the caller's view); with PAD = 8
    every view is 16-byte aligned."""
    import torch
    shape = (rows + 2 * PAD,) + ((cols,) if cols else ())
    whole = torch.full(shape, fill, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + rows]


def run_device(solver, so, W, T, origin, h, values, r_free, margin, max_pieces, so_dev=None, S_in=None):
    """The device call between sentinels.  Returns the seven outputs trimmed to S' (seg_times None
    without T); asserts that no sentinel and no row past S' was touched."""
    import torch
    so = np.asarray(so, np.int32)
    B, S = len(so) - 1, int(so[-1]) if len(so) > 1 else 0
    S = S if S_in is None else S_in
    cap = min(S * max_pieces, 16 * B)
    n, t = _table(solver, origin, h, values, r_free)
    f64, i32 = torch.float64, torch.int32
    so_w, so_o = _padded(B + 1, 0, i32, -9)
    W_w, W_o = _padded(cap + B, 3, f64, -9.0)
    T_w, T_o = _padded(cap, 0, f64, -9.0)
    par_w, par_o = _padded(cap, 0, i32, -9)
    sf_w, sf_o = _padded(cap, 0, i32, -9)
    hp_w, hp_o = _padded(S, 0, i32, -9)
    tot_w, tot_o = _padded(1, 0, torch.int64, -9)
    fl_w, fl_o = _padded(B, 0, i32, -9)
    dT = None if T is None else _dev(np.asarray(T, np.float64))
    solver.corridor_reroute_device(B, _dev(so if so_dev is None else so_dev), _dev(np.asarray(W, np.float64).reshape(-1, 3)),
                                   origin, h, n, t, margin, max_pieces, so_o, W_o, tot_o, d_seg_times=dT,
                                   d_seg_times_out=None if T is None else T_o, d_parent=par_o, d_seg_flags_out=sf_o,
                                   d_hops=hp_o, d_flags=fl_o)
    torch.cuda.synchronize()
    S1 = int(tot_o[0])
    assert 0 <= S1 <= cap
    for whole, used in ((so_w, B + 1), (W_w, S1 + B), (T_w, S1 if T is not None else 0), (par_w, S1), (sf_w, S1),
                        (tot_w, 1), (fl_w, B)):
        w = whole.cpu().numpy()
        assert (w[:PAD] == -9).all() and (w[PAD + used:] == -9).all(), "a sentinel or a row past S' was written"
    w = hp_w.cpu().numpy()
    assert (w[:PAD] == -9).all() and (w[PAD + S:] == -9).all()
    c = lambda x, k: x[:k].cpu().numpy()  # noqa: E731
    return (c(so_o, B + 1), c(W_o, S1 + B), None if T is None else c(T_o, S1), c(par_o, S1), c(sf_o, S1), c(hp_o, S),
            c(fl_o, B))


class Device:
    """The device entry point behind the backend interface of reroute_ref.py."""

    def __init__(self, solver):
        self.s = solver

    def corridor_reroute(self, so, W, origin, h, values, r_free, margin, max_pieces, seg_times=None):
        return run_device(self.s, so, W, seg_times, origin, h, values, r_free, margin, max_pieces)

    def corridor_inflate(self, *a):
        return self.s.corridor_inflate(*a)


@pytest.fixture(scope="module", params=["host_pointers", "device"])
def be(request, solver):
    return solver if request.param == "host_pointers" else Device(solver)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


def test_wall_with_a_gap_by_hand(be):
    RR.check_wall_with_gap(be)


def test_closed_wall_has_no_path(be):
    RR.check_closed_wall(be)


def test_margin_one_short_of_the_gap(be):
    RR.check_small_margin(be)


def test_window_cap(be):
    RR.check_window_cap(be)


def test_end_node_not_free(be):
    RR.check_ends(be)


def test_degenerate_leg_is_copied(be):
    RR.check_degenerate(be)


def test_tie_order(be):
    RR.check_tie_order(be)


def test_long_path_needs_sixteen_bits(be):
    RR.check_long_path(be)


def test_budget_is_all_or_nothing(be):
    RR.check_budget(be)


def test_bad_legs_are_isolated(be):
    RR.check_isolation(be)


def test_times_follow_the_lengths(be):
    RR.check_times(be)


@pytest.mark.parametrize("margin,max_pieces", [(1, 8), (3, 4), (6, 8)])
def test_random_mazes_equal_the_reference(be, margin, max_pieces):
    RR.check_maze(be, margin, max_pieces)


def test_arguments(solver):
    RR.check_arguments(solver, TgmsError, ERR_INVALID_ARG)


def short_legs(B, seed, m_hi=3):
    """B ragged trajectories of short legs inside the maze's grid."""
    rng = np.random.default_rng(seed)
    Ms = rng.integers(1, m_hi + 1, size=B)
    so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    p = rng.uniform(2.0, 21.0, size=(int(so[-1]) + B, 3))
    first = np.zeros(len(p), bool)
    first[so[:-1] + np.arange(B)] = True
    step = np.where(first[:, None], 0.0, rng.uniform(-3.0, 3.0, size=p.shape))
    start = np.maximum.accumulate(np.where(first, np.arange(len(p)), 0))
    W = np.clip(p[start] + step, 0.25, 22.75) * RR.H  # every waypoint within three nodes of its trajectory's first
    return so, W, rng.uniform(0.5, 4.0, size=int(so[-1]))


@pytest.mark.parametrize("B", [255, 256, 257])
def test_scan_seams(solver, host, B):
    """The 256-entry workgroups of the scan; host, host pointers and device agree to the bit."""
    so, W, T = short_legs(B, seed=B)
    v = RR.maze()[3]
    a = (so, W, RR.O, RR.H, v, RR.RF, 3, 8, T)
    want = host.corridor_reroute(*a)
    assert (want[6] & RRT_DONE).any()
    RR.assert_same(Device(solver).corridor_reroute(*a), want, "device")
    RR.assert_same(solver.corridor_reroute(*a), want, "host pointers")


def test_no_candidate_and_one_candidate(solver, host):
    so, W, T = short_legs(9, seed=4)
    free = RR.grid(RR.MAZE_N)
    got = Device(solver).corridor_reroute(so, W, RR.O, RR.H, free, RR.RF, 3, 8, T)
    S = int(so[-1])
    RR.assert_same(got, (so, W, T, np.arange(S, dtype=np.int32), np.zeros(S, np.int32), np.full(S, NEAR_NONE, np.int32),
                         np.zeros(9, np.int32)), "no candidate")
    so1, W1, T1 = RR.path([(2, 2, 1), (2, 4, 1), (6, 4, 1), (6, 2, 1)])
    one = RR.grid((16, 16, 4), [(4, 4, 1)])
    got = Device(solver).corridor_reroute(so1, W1, RR.O, RR.H, one, RR.RF, 4, 8, T1)
    RR.assert_same(got, host.corridor_reroute(so1, W1, RR.O, RR.H, one, RR.RF, 4, 8, T1), "one candidate")
    assert list(got[5]) == [NEAR_NONE, 6, NEAR_NONE]


def test_more_candidates_than_the_persistent_grid(solver, host):
    """The search's grid has 512 workgroups; 4,096 trajectories in the maze leave several thousand
    candidates, so every workgroup strides over several.  Twice: the bits repeat."""
    so, W, T = short_legs(4096, seed=9, m_hi=2)
    v = RR.maze()[3]
    a = (so, W, RR.O, RR.H, v, RR.RF, 2, 8, T)
    want = host.corridor_reroute(*a)
    assert (want[5] >= 0).sum() > 1024
    first = Device(solver).corridor_reroute(*a)
    RR.assert_same(first, want, "device")
    RR.assert_same(Device(solver).corridor_reroute(*a), first, "repeated")


@pytest.mark.parametrize("count", [0, 17])
def test_bad_segment_count_between_good_neighbours(solver, host, count):
    """A trajectory with `count` segments inserted at position 5: one placeholder row, the
    neighbours bit-equal to the batch without it, every sentinel intact."""
    so, W, T = short_legs(11, seed=31)
    v = RR.maze()[3]
    want = host.corridor_reroute(so, W, RR.O, RR.H, v, RR.RF, 3, 8, T)
    at = 5
    s, w = int(so[at]), int(so[at]) + at
    so_bad = np.concatenate([so[:at + 1], so[at:] + count]).astype(np.int32)
    W_bad = np.concatenate([W[:w], np.full((count + 1, 3), 3.5), W[w:]])
    T_bad = np.concatenate([T[:s], np.ones(count), T[s:]])
    got = run_device(solver, so_bad, W_bad, T_bad, RR.O, RR.H, v, RR.RF, 3, 8)
    s2, w2 = int(want[0][at]), int(want[0][at]) + at
    parent = want[3].copy()
    parent[s2:] += count  # the input rows behind the inserted trajectory moved
    exp = (np.concatenate([want[0][:at + 1], want[0][at:] + 1]).astype(np.int32),
           np.concatenate([want[1][:w2], np.full((2, 3), np.nan), want[1][w2:]]),
           np.concatenate([want[2][:s2], [np.nan], want[2][s2:]]),
           np.concatenate([parent[:s2], [NEAR_NONE], parent[s2:]]).astype(np.int32),
           np.concatenate([want[4][:s2], [FEAS_NONFINITE], want[4][s2:]]).astype(np.int32),
           None,
           np.concatenate([want[6][:at], [FEAS_NONFINITE], want[6][at:]]).astype(np.int32))
    for name, g, e in zip(RR.NAMES, got, exp):
        if e is not None:
            assert g.shape == e.shape and np.array_equal(g, e, equal_nan=g.dtype.kind == "f"), name
    keep = ~np.isnan(exp[2])
    assert RR.same_bits(got[2][keep], exp[2][keep]) and RR.same_bits(got[1][~np.isnan(exp[1])], exp[1][~np.isnan(exp[1])])
    hops = got[5]  # the rows of the inserted trajectory are not written: they keep the sentinel
    assert np.array_equal(hops[:s], want[5][:s]) and np.array_equal(hops[s + count:], want[5][s:])
    assert (hops[s:s + count] == -9).all()


def test_capturing_stream_and_host_handle(solver, host):
    import torch
    so, W, T = RR.path([(2, 4, 1), (6, 4, 1)])
    n, t = _table(solver, RR.O, RR.H, RR.grid((16, 16, 4), [(4, 4, 1)]), RR.RF)
    outs = dict(d_seg_offsets_out=_dev(np.zeros(2, np.int32)), d_waypoints_out=_dev(np.zeros((9, 3))),
                d_totals=_dev(np.zeros(2, np.int64)))
    dso, dW = _dev(so), _dev(W)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        with pytest.raises(TgmsError) as e:
            solver.corridor_reroute_device(1, dso, dW, RR.O, RR.H, n, t, 4, 8, stream=side.cuda_stream, **outs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert e.value.status == ERR_UNSUPPORTED
    del g
    with pytest.raises(TgmsError) as e:  # a misaligned fp64 array
        odd = torch.zeros(9 * 3 + 1, dtype=torch.float64, device="cuda")[1:]
        solver.corridor_reroute_device(1, dso, dW, RR.O, RR.H, n, t, 4, 8, **dict(outs, d_waypoints_out=odd))
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # a host handle has no device path
        host.corridor_reroute_device(1, dso, dW, RR.O, RR.H, n, t, 4, 8, **outs)
    assert e.value.status == ERR_UNSUPPORTED and "tgms_corridor_reroute_batch_dev" in str(e.value)


def test_pipeline_on_device_buffers(solver):
    """256 trajectories of short legs in the maze, every step on device buffers: subdivide, re-route,
    the same table again for the inflation, solve, corridor containment.  A leaf the subdivision
    leaves blocked is a candidate of the re-route; the inflation's BLOCKED and OUTSIDE are the
    re-route's, segment by segment."""
    import torch
    so, W, T = short_legs(256, seed=12, m_hi=4)
    v = RR.maze()[3]
    B, S = len(so) - 1, int(so[-1])
    n, t = _table(solver, RR.O, RR.H, v, RR.RF)
    i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")
    cap1 = min(S << 1, 16 * B)
    so1, W1, T1 = torch.zeros(B + 1, **i32), torch.zeros((cap1 + B, 3), **f64), torch.ones(cap1, **f64)
    sub_seg, tot1 = torch.zeros(cap1, **i32), torch.zeros(2, **i64)
    solver.corridor_subdivide_device(B, _dev(so), _dev(W), RR.O, RR.H, n, t, 1, so1, W1, tot1, d_seg_times=_dev(T),
                                     d_seg_times_out=T1, d_seg_flags_out=sub_seg)
    cap2 = 16 * B  # min(8 S1, 16 B) without reading S1 back
    so2, W2, T2 = torch.zeros(B + 1, **i32), torch.zeros((cap2 + B, 3), **f64), torch.ones(cap2, **f64)
    par, rrt_seg, rrt_fl = torch.full((cap2,), -1, **i32), torch.zeros(cap2, **i32), torch.zeros(B, **i32)
    hops, tot2 = torch.full((cap1,), -5, **i32), torch.zeros(2, **i64)
    solver.corridor_reroute_device(B, so1, W1, RR.O, RR.H, n, t, 3, 8, so2, W2, tot2, d_seg_times=T1, d_seg_times_out=T2,
                                   d_parent=par, d_seg_flags_out=rrt_seg, d_hops=hops, d_flags=rrt_fl)
    faces, fo = torch.zeros((6 * cap2, 4), **f64), torch.zeros(cap2 + 1, **i64)
    inf_seg, inf_fl = torch.zeros(cap2, **i32), torch.zeros(B, **i32)
    solver.corridor_inflate_device(B, so2, W2, RR.O, RR.H, n, t, 2, d_faces=faces, d_face_offsets=fo, d_seg_flags=inf_seg,
                                   d_flags=inf_fl)
    torch.cuda.synchronize()
    S1, S2 = int(tot1[0]), int(tot2[0])
    h_so2 = so2.cpu().numpy()
    assert h_so2[-1] == S2 and S1 < S2 <= cap2 and (np.diff(h_so2) <= 16).all()
    a, b, p = rrt_seg[:S2].cpu().numpy(), inf_seg[:S2].cpu().numpy(), par[:S2].cpu().numpy()
    assert np.array_equal((a & RRT_BLOCKED) != 0, (b & INF_BLOCKED) != 0)
    assert np.array_equal((a & RRT_OUTSIDE) != 0, (b & INF_OUTSIDE) != 0)
    assert np.array_equal((rrt_fl.cpu().numpy() & RRT_BLOCKED) != 0, (inf_fl.cpu().numpy() & INF_BLOCKED) != 0)
    # a segment the re-route searched or left blocked was a blocked leaf of the subdivision, and the others were not
    sub_blocked = (sub_seg[:S1].cpu().numpy() & SUB_BLOCKED) != 0
    pieces = np.bincount(p, minlength=S1)
    assert np.array_equal(sub_blocked, (pieces > 1) | (np.bincount(p, weights=((a & RRT_BLOCKED) != 0).astype(float), minlength=S1) > 0))
    assert (pieces > 1).any() and (hops[:S1].cpu().numpy()[pieces > 1] >= 0).all()
    C, st = torch.zeros((S2, 3, 8), **f64), torch.full((B,), -1, **i32)
    solver.solve_batch_device(h_so2, so2, W2, T2, C, st)
    rec, cfl = torch.zeros((B, 2), **f64), torch.zeros(B, **i32)
    solver.corridor_device(B, so2, T2, C, 6 * S2, faces, fo, 0.0, d_rec=rec, d_flags=cfl)
    torch.cuda.synchronize()
    solved = st.cpu().numpy() == OK  # the rebuilt batch is one the later steps take as it is
    assert solved.any() and np.isfinite(rec.cpu().numpy()[solved]).all()
    assert not (cfl.cpu().numpy()[solved] & FEAS_NONFINITE).any()
