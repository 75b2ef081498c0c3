"""GPU: the distance-field build (tgms_field_edt_device, csrc/tgms_edt.hip, and tgms_field_edt on
a GPU handle).  The matrix of test_edt_host.py runs through the device entry point against the
brute-force reference (edt_ref.py), bit for bit; then a larger non-cubic map against the host
backend, each output alone, a captured graph replayed after the occupancy changed in place, the
arguments, the host-pointer call, a multi handle, and the chain occupancy -> field -> table ->
boxes on the device against the same chain on the host backend."""
import numpy as np
import pytest

import edt_ref as ER
import inflate_ref as IR
from trajectory_generator_ros2_amd import ERR_INVALID_ARG, TgmsError
from trajectory_generator_ros2_amd import synthetic as S

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).cuda()  # a copy: the shared inputs are read-only


def _work(solver, n, signed=False):
    import torch
    nbytes = solver.field_edt_work_size(ER.ORIGIN, 1.0, n, signed)
    assert nbytes == 8 * n[0] * n[1] * n[2]
    return torch.full((nbytes // 4,), -3, dtype=torch.int32, device="cuda")


def _outs(shape):
    import torch
    return (torch.full(shape, float("nan"), dtype=torch.float32, device="cuda"),
            torch.full(shape, 0, dtype=torch.int32, device="cuda"))


class Device:
    """The device entry point behind the backend interface of edt_ref.py."""

    def __init__(self, solver):
        self.s = solver

    def field_edt(self, occ, origin, h, max_dist, signed=False):
        import torch
        o = np.ascontiguousarray(occ, dtype=np.uint8)
        n = o.shape[::-1]
        v, d2 = _outs(o.shape)
        self.s.field_edt_device(origin, h, n, _dev(o), max_dist, _work(self.s, n, signed), v, d2, signed)
        torch.cuda.synchronize()
        return v.cpu().numpy(), d2.cpu().numpy()


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    with Solver(host=True) as s:
        yield s


@pytest.mark.parametrize("case", ER.CASES, ids=ER.case_id)
def test_matrix_equals_the_reference(solver, case):
    ER.check_case(Device(solver), *case)


def test_signed_cap_just_below_a_whole_number_of_spacings(solver):
    """Nodes between R and R + 1/2 spacings away keep a value below max_dist (edt_ref.py has the case)."""
    n, name = (40, 33, 9), "random_0.001"
    for h in ER.H_VALUES:
        got = Device(solver).field_edt(ER.make_map(n, name), ER.ORIGIN, h, 3.9 * h, True)
        ER.assert_same(got, ER.convert(*ER.squares(n, name), ER.make_map(n, name), h, 3.9 * h, True), h)


def test_non_cubic_map_of_several_tiles_equals_the_host_backend(solver, host):
    """64 x 48 x 40 at 2 %: several tiles per pass on every axis; caps of a few nodes, of a window
    that crosses tiles, and none; both modes."""
    rng = np.random.default_rng(S.SEED + 13)
    occ = (rng.random((40, 48, 64)) < 0.02).astype(np.uint8)
    h = 0.094
    for md in (2.5 * h, 1.0, 20.0):
        for signed in (False, True):
            got = Device(solver).field_edt(occ, ER.ORIGIN, h, md, signed)
            ER.assert_same(got, host.field_edt(occ, ER.ORIGIN, h, md, signed), (md, signed))
            ER.assert_same(solver.field_edt(occ, ER.ORIGIN, h, md, signed), got, ("host pointers", md, signed))


def test_each_output_alone(solver):
    import torch
    n, name, h, md = (40, 33, 9), "random_0.05", 0.094, 1.0
    occ = ER.make_map(n, name)
    for signed in (False, True):
        want = ER.convert(*ER.squares(n, name), occ, h, md, signed)
        for i, key in enumerate(("d_values", "d_d2")):
            o = _outs(occ.shape)[i]
            solver.field_edt_device(ER.ORIGIN, h, n, _dev(occ), md, _work(solver, n, signed), signed=signed, **{key: o})
            torch.cuda.synchronize()
            assert ER.same_bits(o.cpu().numpy(), want[i]), (key, signed)
    # and through host pointers, where the staging lays out only what was asked for
    import ctypes
    from trajectory_generator_ros2_amd import OK, _lib
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    f = ctypes.byref(_lib.Field(ER.ORIGIN, h, n))
    for i in range(2):
        o = np.zeros_like(want[i])
        a = [None, None]
        a[i] = p(o)
        assert L.tgms_field_edt(solver._h, f, p(np.ascontiguousarray(occ)), md, 1, *a) == OK
        assert ER.same_bits(o, want[i]), i


def test_captured_graph_replayed_after_the_map_changed(solver):
    """No handle scratch and no host plan: both modes captured into one graph, replayed after the
    occupancy changed in place, each replay equal to the reference of what is in the buffer then."""
    import torch
    n, h, md = (40, 33, 9), 0.094, 1.0
    maps = [ER.make_map(n, m) for m in ("random_0.05", "plane_y", "random_0.5")]
    d_occ = _dev(maps[0])
    wu, ws = _work(solver, n), _work(solver, n, True)
    (vu, du), (vs, ds) = _outs(maps[0].shape), _outs(maps[0].shape)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        solver.field_edt_device(ER.ORIGIN, h, n, d_occ, md, wu, vu, du, stream=side.cuda_stream)
        solver.field_edt_device(ER.ORIGIN, h, n, d_occ, md, ws, vs, ds, signed=True, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for m, name in zip(maps, ("random_0.05", "plane_y", "random_0.5")):
        d_occ.copy_(_dev(m))
        for o in (vu, du, vs, ds):
            o.fill_(-2)
        g.replay()
        torch.cuda.synchronize()
        sq = ER.squares(n, name)
        ER.assert_same((vu.cpu().numpy(), du.cpu().numpy()), ER.convert(*sq, m, h, md, False), name)
        ER.assert_same((vs.cpu().numpy(), ds.cpu().numpy()), ER.convert(*sq, m, h, md, True), name)
    del g


def test_arguments_are_refused_before_any_launch(solver):
    import torch
    n, h = (9, 7, 5), 0.125
    occ = _dev(ER.make_map(n, "checker"))
    w = _work(solver, n)
    v, d2 = _outs((5, 7, 9))
    raw = torch.zeros(4 * 9 * 7 * 5 * 3 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = [dict(d_values=None, d_d2=None), dict(d_occ=None), dict(d_work=None), dict(d_values=raw[1:]),
           dict(d_d2=raw[2:]), dict(d_work=raw[3:]), dict(max_dist=0.0), dict(max_dist=float("nan")),
           dict(n=(1, 7, 5)), dict(n=(16385, 2, 2)), dict(n=(16384, 16384, 8)), dict(h=0.0),
           dict(origin=(0.0, float("nan"), 0.0))]
    for kw in bad:
        a = dict(origin=ER.ORIGIN, h=h, n=n, d_occ=occ, max_dist=1.0, d_work=w, d_values=v, d_d2=d2)
        a.update(kw)
        with pytest.raises(TgmsError) as e:
            solver.field_edt_device(**a)
        assert e.value.status == ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert torch.isnan(v).all() and (d2 == 0).all() and (w == -3).all()  # nothing ran
    assert solver.field_edt_work_size(ER.ORIGIN, h, (16385, 2, 2)) == 0


def test_multi_handle_runs_on_device_0(solver):
    from trajectory_generator_ros2_amd.solver import Solver
    n, name, h, md = (9, 7, 5), "checker", 0.125, 1.0
    want = ER.convert(*ER.squares(n, name), ER.make_map(n, name), h, md, True)
    with Solver(device_count=1) as m:
        ER.assert_same(m.field_edt(ER.make_map(n, name), ER.ORIGIN, h, md, True), want)
        ER.assert_same(Device(m).field_edt(ER.make_map(n, name), ER.ORIGIN, h, md, True), want)


def test_chain_occupancy_to_field_to_table_to_boxes_equals_the_host_backend(solver, host):
    """Everything on the device, nothing downloaded in between: field_edt_device ->
    field_occupancy_device -> corridor_inflate_device.  The host backend runs the same chain; boxes,
    faces, offsets and flags agree bit for bit."""
    import torch
    origin, h, n, r_free = IR.SCENE_ORIGIN, IR.SCENE_H, IR.SCENE_N, IR.SCENE_R
    occ = (IR.scene() == 0).astype(np.uint8)  # the nodes inside the scene's boxes
    assert 0 < occ.sum() < occ.size
    so, W = IR.ragged()
    B, Sg = len(so) - 1, int(so[-1])
    v_host, _ = host.field_edt(occ, origin, h, 1.0)
    want = host.corridor_inflate(so, W, origin, h, v_host, r_free, 8)
    d_v = torch.full(occ.shape, float("nan"), dtype=torch.float32, device="cuda")
    table = torch.full((n[2] + 1, n[1] + 1, n[0] + 1), -7, dtype=torch.int32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    outs = (torch.full((Sg, 6), -2, **i32), torch.full((6 * Sg, 4), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((Sg + 1,), -2, dtype=torch.int64, device="cuda"), torch.full((Sg,), -2, **i32),
            torch.full((B,), -2, **i32))
    solver.field_edt_device(origin, h, n, _dev(occ), 1.0, _work(solver, n), d_values=d_v)
    solver.field_occupancy_device(origin, h, n, d_v, r_free, table)
    solver.corridor_inflate_device(B, _dev(so), _dev(W), origin, h, n, table, 8, *outs)
    torch.cuda.synchronize()
    assert ER.same_bits(d_v.cpu().numpy(), v_host)
    IR.assert_same(tuple(o.cpu().numpy() for o in outs), want)
    assert (want[3] & IR.INF_BLOCKED).any() and (want[3] == 0).any()
