"""GPU: the corridor inflation (tgms_corridor_inflate_batch on a GPU handle, and
tgms_field_occupancy_device + tgms_corridor_inflate_batch_device, csrc/tgms_inflate.hip).  The
cases of test_inflate_host.py run through both entry points (inflate_ref.py), then the table on
its own and the launch's own corners: host / device equality, a bad segment count in the device
offsets, misaligned arrays, each output alone, two streams on one handle, table build and
inflation in one captured graph, a multi handle, the host handle's device calls, and the
pipeline map -> corridors -> solve -> containment -> split."""
import numpy as np
import pytest

import inflate_ref as IR
from trajectory_generator_ros2_amd import (COR_OUTSIDE, ERR_INVALID_ARG, ERR_UNSUPPORTED, FEAS_NONFINITE, INF_BLOCKED,
                                           INF_CAPPED, OK, TgmsError)

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).cuda()  # a copy: the shared inputs are read-only


def _outs(S, B):
    import torch
    i32 = dict(dtype=torch.int32, device="cuda")
    return (torch.full((S, 6), -2, **i32), torch.full((6 * S, 4), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((S + 1,), -2, dtype=torch.int64, device="cuda"), torch.full((S,), -2, **i32),
            torch.full((B,), -2, **i32))


def _table(n):
    import torch
    return torch.full((n[2] + 1, n[1] + 1, n[0] + 1), -7, dtype=torch.int32, device="cuda")


class Device:
    """The two device entry points behind the backend interface of inflate_ref.py."""

    def __init__(self, solver):
        self.s = solver

    def occupancy(self, origin, h, values, r_free):
        import torch
        v = np.ascontiguousarray(values, dtype=np.float32)
        t = _table(v.shape[::-1])
        self.s.field_occupancy_device(origin, h, v.shape[::-1], _dev(v), r_free, t)
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def corridor_inflate(self, so, W, origin, h, values, r_free, max_grow):
        import torch
        so = np.asarray(so, np.int32)
        B, S = len(so) - 1, int(so[-1])
        v = np.ascontiguousarray(values, dtype=np.float32)
        n = v.shape[::-1]
        t = _table(n)
        outs = _outs(S, B)
        self.s.field_occupancy_device(origin, h, n, _dev(v), r_free, t)
        self.s.corridor_inflate_device(B, _dev(so), _dev(np.asarray(W, np.float64).reshape(-1, 3)), origin, h, n, t,
                                       max_grow, *outs)
        torch.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in outs)


@pytest.fixture(scope="module", params=["host_pointers", "device"])
def be(request, solver):
    return solver if request.param == "host_pointers" else Device(solver)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


@pytest.mark.parametrize("max_grow", [0, 1, 8])
def test_random_scene_equals_the_reference(be, max_grow):
    IR.check_random(be, max_grow)


def test_random_scene_partly_outside_the_grid(be):
    IR.check_random(be, 8, shift=3.0)


def test_empty_map(be):
    IR.check_empty_map(be)


def test_closed_direction_stays_closed(be):
    IR.check_closed_direction_stays_closed(be)


def test_nan_node_is_not_free(be):
    IR.check_closed_direction_stays_closed(be, bad=np.nan)


def test_blocked_seed(be):
    IR.check_blocked(be)


def test_waypoints_on_nodes(be):
    IR.check_on_a_node(be)


def test_one_ulp_either_side_of_a_node(be):
    IR.check_one_ulp(be)


def test_row_lengths_1_and_16(be):
    IR.check_row_lengths(be)


def test_nan_waypoint_spoils_its_two_segments_only(be):
    IR.check_nan_waypoint(be)


def test_far_waypoints(be):
    IR.check_far_waypoints(be)


def test_arguments(be):
    IR.check_arguments(be, TgmsError, ERR_INVALID_ARG)


@pytest.mark.parametrize("n", IR.TABLE_GRIDS, ids=lambda n: "x".join(map(str, n)))
def test_table_equals_cumsum(solver, n):
    IR.check_table(Device(solver).occupancy, n)


def test_host_and_device_agree_to_the_bit(solver, host):
    for shift in (0.0, 3.0):
        so, W = IR.ragged(shift)
        a = (so, W, IR.SCENE_ORIGIN, IR.SCENE_H, IR.scene(), IR.SCENE_R, 8)
        want = host.corridor_inflate(*a)
        IR.assert_same(solver.corridor_inflate(*a), want)
        IR.assert_same(Device(solver).corridor_inflate(*a), want)


def _scene_device(shift=0.0):
    so, W = IR.ragged(shift)
    return len(so) - 1, int(so[-1]), _dev(so), _dev(W)


GRID = (IR.SCENE_ORIGIN, IR.SCENE_H, IR.SCENE_N)


def _scene_table(solver):
    import torch
    t = _table(IR.SCENE_N)
    solver.field_occupancy_device(*GRID, _dev(IR.scene()), IR.SCENE_R, t)
    torch.cuda.synchronize()
    return t


def test_bad_segment_count_writes_no_row(solver):
    """A span of 17 and a span of 0 in the device offsets: those trajectories carry FEAS_NONFINITE
    alone, none of their segment rows is written, and every other row is the batch's own."""
    import torch
    so, W = IR.ragged()
    want = IR.reference(so, W, *GRID[:2], IR.scene(), IR.SCENE_R, 8)
    t = _scene_table(solver)
    B, S = len(so) - 1, int(so[-1])
    # trajectories 1 and 2 merged into one span too long for a trajectory, trajectory 2 left empty;
    # the waypoint rows of the others are where they were
    assert so[3] - so[1] > 16
    bad = so.copy()
    bad[2] = so[3]
    outs = _outs(S, B)
    solver.corridor_inflate_device(B, _dev(bad), _dev(W), *GRID, t, 8, *outs)
    torch.cuda.synchronize()
    box, faces, fo, seg_flags, flags = (o.cpu().numpy() for o in outs)
    gone = np.arange(so[1], so[3])
    keep = np.setdiff1d(np.arange(S), gone)
    assert list(flags[1:3]) == [FEAS_NONFINITE] * 2
    assert (box[gone] == -2).all() and (seg_flags[gone] == -2).all() and (fo[gone] == -2).all()
    assert np.isnan(faces.reshape(S, 24)[gone]).all()
    assert np.array_equal(box[keep], want[0][keep]) and np.array_equal(seg_flags[keep], want[3][keep])
    assert IR.same_bits(faces.reshape(S, 24)[keep], want[1].reshape(S, 24)[keep])
    assert np.array_equal(fo[keep], want[2][keep]) and fo[S] == 6 * S
    others = np.setdiff1d(np.arange(B), [1, 2])
    assert np.array_equal(flags[others], want[4][others])


def test_misaligned_arrays(solver):
    import torch
    B, S, dso, dW = _scene_device()
    t = _scene_table(solver)
    flags = torch.zeros(B, dtype=torch.int32, device="cuda")
    odd_w = torch.zeros(dW.numel() + 1, dtype=torch.float64, device="cuda")[1:]
    odd_faces = torch.zeros(24 * S + 1, dtype=torch.float64, device="cuda")[1:]
    odd_fo = torch.zeros(S + 2, dtype=torch.int64, device="cuda")[1:]
    for kw in (dict(d_waypoints=odd_w), dict(d_faces=odd_faces), dict(d_face_offsets=odd_fo)):
        w = kw.pop("d_waypoints", dW)
        with pytest.raises(TgmsError) as e:
            solver.corridor_inflate_device(B, dso, w, *GRID, t, 8, d_flags=flags, **kw)
        assert e.value.status == ERR_INVALID_ARG, kw
    with pytest.raises(TgmsError) as e:  # every output NULL
        solver.corridor_inflate_device(B, dso, dW, *GRID, t, 8)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # the table NULL
        solver.corridor_inflate_device(B, dso, dW, *GRID, None, 8, d_flags=flags)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:
        solver.field_occupancy_device(*GRID, _dev(IR.scene()), float("nan"), t)
    assert e.value.status == ERR_INVALID_ARG
    with pytest.raises(TgmsError) as e:  # more than 2^31 - 1 table entries: refused before a value is read
        solver.field_occupancy_device(*GRID[:2], (1290, 1290, 1290), _dev(IR.scene()), 0.3, t)
    assert e.value.status == ERR_INVALID_ARG
    flags.fill_(-2)
    solver.corridor_inflate_device(0, dso, dW, *GRID, t, 8, d_flags=flags)  # B == 0: nothing launched
    torch.cuda.synchronize()
    assert (flags == -2).all()


def test_each_output_alone(solver):
    import torch
    so, W = IR.ragged()
    want = IR.reference(so, W, *GRID[:2], IR.scene(), IR.SCENE_R, 8)
    B, S, dso, dW = _scene_device()
    t = _scene_table(solver)
    names = ("d_box", "d_faces", "d_face_offsets", "d_seg_flags", "d_flags")
    for i, name in enumerate(names):
        o = _outs(S, B)[i]
        solver.corridor_inflate_device(B, dso, dW, *GRID, t, 8, **{name: o})
        torch.cuda.synchronize()
        assert IR.same_bits(o.cpu().numpy(), want[i]), name
    # and through host pointers, where the staging lays out only what was asked for
    from trajectory_generator_ros2_amd import _lib
    import ctypes
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    v = np.ascontiguousarray(IR.scene())
    f = ctypes.byref(_lib.Field(*GRID))
    Wc = np.ascontiguousarray(W)
    for i in range(5):
        o = np.zeros_like(want[i])
        a = [None] * 5
        a[i] = p(o)
        assert L.tgms_corridor_inflate_batch(solver._h, B, p(so), p(Wc), f, p(v), IR.SCENE_R, 8, *a) == OK
        assert IR.same_bits(o, want[i]), names[i]


def test_two_streams_on_one_handle(solver):
    """Neither call uses handle scratch: two tables and two batches on two streams at once, each
    output that of the call alone."""
    import torch
    cases = [(0.0, 8, 0.3), (3.0, 1, 0.45)]
    want = [IR.reference(*IR.ragged(sh), *GRID[:2], IR.scene(), r, mg) for sh, mg, r in cases]
    dv = _dev(IR.scene())
    args = [_scene_device(sh) for sh, _, _ in cases]
    outs = [_outs(a[1], a[0]) for a in args]
    tabs = [_table(IR.SCENE_N) for _ in cases]
    streams = [torch.cuda.Stream() for _ in cases]
    torch.cuda.synchronize()
    for (B, S, dso, dW), o, t, st, (_, mg, r) in zip(args, outs, tabs, streams, cases):
        solver.field_occupancy_device(*GRID, dv, r, t, stream=st.cuda_stream)
        solver.corridor_inflate_device(B, dso, dW, *GRID, t, mg, *o, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        IR.assert_same(tuple(x.cpu().numpy() for x in o), w)


def test_table_and_inflation_in_one_graph(solver):
    """Table build and inflation captured into one graph; replayed after the waypoints and the map
    change in place, each replay equal to the reference of what is in the buffers then."""
    import torch
    so, W = IR.ragged()
    B, S, dso, dW = _scene_device()
    dv = _dev(IR.scene())
    t = _table(IR.SCENE_N)
    outs = _outs(S, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        solver.field_occupancy_device(*GRID, dv, IR.SCENE_R, t, stream=side.cuda_stream)
        solver.corridor_inflate_device(B, dso, dW, *GRID, t, 8, *outs, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    v2 = IR.scene().copy()
    v2[10:14, 12:15, 20:22] = 0.0  # a new obstacle
    for W_now, v_now in ((W, IR.scene()), (IR.ragged(3.0)[1], IR.scene()), (W, v2)):
        dW.copy_(_dev(W_now))
        dv.copy_(_dev(v_now))
        for o in outs:
            o.fill_(-2)
        g.replay()
        torch.cuda.synchronize()
        IR.assert_same(tuple(o.cpu().numpy() for o in outs), IR.reference(so, W_now, *GRID[:2], v_now, IR.SCENE_R, 8))
    del g


def test_multi_handle_runs_on_device_0(solver):
    from trajectory_generator_ros2_amd.solver import Solver
    so, W = IR.ragged()
    a = (so, W, *GRID[:2], IR.scene(), IR.SCENE_R, 8)
    want = solver.corridor_inflate(*a)
    with Solver(device_count=1) as m:
        IR.assert_same(m.corridor_inflate(*a), want)
        IR.assert_same(Device(m).corridor_inflate(*a), want)


def test_host_handle_device_calls_are_unsupported(host):
    so, W = IR.one_leg()
    tab = np.zeros((8, 9, 10), np.int32)
    with pytest.raises(TgmsError) as e:
        host.field_occupancy_device(IR.G_ORIGIN, IR.G_H, IR.G_N, IR.g_values(), 0.3, tab)
    assert e.value.status == ERR_UNSUPPORTED
    with pytest.raises(TgmsError) as e:
        host.corridor_inflate_device(1, so, W, IR.G_ORIGIN, IR.G_H, IR.G_N, tab, 4, d_flags=np.zeros(1, np.int32))
    assert e.value.status == ERR_UNSUPPORTED


def test_map_to_corridor_to_solve_to_split(solver):
    """An empty room with one box beside a leg: inflate, then solve, corridor and corridor_split on
    the returned faces.  The margins equal those of a corridor call on the reference's faces."""
    origin, h, n = (-5.0, -5.0, 0.0), 0.25, (41, 41, 21)
    v = IR.S.box_field([[0.5, -1.0, 0.0, 1.5, 1.0, 3.0]], origin, h, n)
    so = np.array([0, 3], dtype=np.int32)
    W = np.array([[-3.0, -2.1, 1.0], [-0.6, 0.2, 1.5], [-0.4, 2.3, 2.0], [2.6, 3.1, 1.2]])
    T = np.array([2.5, 2.0, 2.5])
    a = (so, W, origin, h, v, 0.3, 32)
    box, faces, fo, seg_flags, flags = solver.corridor_inflate(*a)
    want = IR.reference(*a)
    IR.assert_same((box, faces, fo, seg_flags, flags), want)
    assert not (seg_flags & (INF_BLOCKED | INF_CAPPED)).any()
    assert box[1, 3] < (0.5 - 0.3 - origin[0]) / h  # the box of the leg beside the obstacle stops short of it
    C, _, worst = solver.solve(so, W, T)
    assert worst == OK
    rec, where, seg_rec, seg_face, cfl = solver.corridor(so, T, C, faces, fo, 0.0)
    ref = solver.corridor(so, T, C, want[1], want[2], 0.0)
    for x, y in zip((rec, where, seg_rec, seg_face, cfl), ref):
        assert IR.same_bits(x, y)
    assert np.isfinite(seg_rec).all()
    so2, W2, T2, f2, fo2, parent, sfl = solver.corridor_split(so, W, T, C, faces, fo, seg_rec, seg_face, 0.0)
    assert len(T2) == so2[-1] >= 3 and len(fo2) == len(T2) + 1 and not (sfl & FEAS_NONFINITE).any()
    assert (len(T2) > 3) <= bool(((cfl & COR_OUTSIDE) != 0).any())  # a split only where something stuck out
    (so3, W3, T3, f3, fo3), C3, flagged = solver.corridor_loop(so, W, T, faces, fo, 0.0, 2)
    assert len(flagged) >= 1 and np.isfinite(C3).all()
