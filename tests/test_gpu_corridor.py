"""GPU: corridor containment (tgms_corridor_batch / tgms_corridor_batch_device,
csrc/tgms_corridor.hip): the closed forms and the 1e-9 L_h contract of test_corridor_host.py
repeated on the device, agreement with the host backend, and the launch's corners: tiles of four
trajectories per wavefront, items numbered through the face counts and taken 64 at a time, tiles
without items, the grid-stride loop, bad rows in the middle of a tile, omitted outputs, argument
errors and graph capture."""
import numpy as np
import pytest

import corridor_ref as CR
import test_corridor_host as H

pytestmark = pytest.mark.gpu

GRID = 4096  # workgroups of the launch at most (csrc/tgms_corridor.hip launch_corridor)
TILE = 4     # trajectories per workgroup
NAMES = ("d_rec", "d_where", "d_seg_rec", "d_seg_face", "d_flags")


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the fixtures are read-only


def _outputs(B, S, omit=()):
    """Fresh device outputs: NaN in the fp64 rows, -7 in the int32 ones (no result is -7)."""
    import torch
    shapes = dict(d_rec=((B, 2), torch.float64), d_where=((B, 2), torch.int32), d_seg_rec=((S, 2), torch.float64),
                  d_seg_face=((S,), torch.int32), d_flags=((B,), torch.int32))
    return {k: None if k in omit else torch.full(sh, float("nan") if dt == torch.float64 else -7, dtype=dt,
                                                 device="cuda") for k, (sh, dt) in shapes.items()}


def _device_call(solver, so, T, C, faces, fo=None, r=0.0, omit=()):
    """tgms_corridor_batch_device on fresh outputs; returns numpy (rec, where, seg_rec, seg_face,
    flags), None for an omitted one."""
    import torch
    so = np.asarray(so, np.int32)
    faces = np.asarray(faces, np.float64).reshape(-1, 4)
    B, S = len(so) - 1, int(so[-1])
    out = _outputs(B, S, omit)
    solver.corridor_device(B, _dev(so), _dev(np.asarray(T, np.float64).reshape(-1)),
                           _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)), len(faces),
                           _dev(faces) if len(faces) else None,
                           None if fo is None else _dev(np.asarray(fo, np.int64)), r, **out)
    torch.cuda.synchronize()
    return tuple(None if out[k] is None else out[k].cpu().numpy() for k in NAMES)


def _call(solver):
    return lambda so, T, C, faces, fo=None, r=0.0: _device_call(solver, so, T, C, faces, fo, r)


def _same(a, b):
    """Two results equal to the bit (NaN rows included)."""
    return all((x is None and y is None) or np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                                           y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.fixture(scope="module", params=["rest", "end_derivs"])
def case(request, solver):
    """test_corridor_host.ragged_case solved and checked on the device.  Shared, never modified."""
    return H.ragged_case(solver.solve, _call(solver), request.param == "end_derivs")


@pytest.fixture(scope="module")
def rest(solver):
    return H.ragged_case(solver.solve, _call(solver), False)


def gather(c, rows):
    """The fixture's rows `rows` as a batch of their own: (so, T, C, faces, fo).  Every segment
    has six faces, so a face index keeps its value modulo 6."""
    so = c["so"]
    seg = np.concatenate([np.arange(so[b], so[b + 1]) for b in rows])
    so2 = np.concatenate([[0], np.cumsum(np.diff(so)[rows])]).astype(np.int32)
    return (so2, c["T"][seg], c["C"][seg], c["faces"].reshape(-1, 6, 4)[seg].reshape(-1, 4),
            6 * np.arange(len(seg) + 1, dtype=np.int64)), seg


def local(out, so, fo):
    """A result with its face indices relative to the owning segment's span, for comparing the
    same rows between two batches; so and fo are those of the call that gave `out`."""
    rec, where, seg_rec, seg_face, fl = out
    fo = np.asarray(fo)
    first = fo[np.asarray(so[:-1], np.int64) + np.maximum(where[:, 0], 0)]
    w = where.copy()
    w[:, 1] = np.where(where[:, 1] >= 0, where[:, 1] - first, where[:, 1])
    return rec, w, seg_rec, np.where(seg_face >= 0, seg_face - fo[:-1], seg_face).astype(np.int32), fl


def pick(out, so, rows):
    """Rows `rows` (and their segments) of a result."""
    seg = np.concatenate([np.arange(so[b], so[b + 1]) for b in rows]) if len(rows) else np.zeros(0, np.int64)
    return out[0][rows], out[1][rows], out[2][seg], out[3][seg], out[4][rows]


def against_host(solver, host, so, T, C, faces, fo, r=0.0):
    """Within 2e-9 L_h of the host backend (which the CPU tests hold to the reference), the same
    flags, and the reported places attain the stored margins."""
    out = _device_call(solver, so, T, C, faces, fo, r)
    ref = CR.records(so, T, C, faces, fo)
    hst = host.corridor(so, T, C, faces, fo, r)
    for k, L in ((0, ref["L"]), (2, ref["seg_L"])):
        fin = np.isfinite(hst[k][:, 0])
        assert np.array_equal(np.isfinite(out[k][:, 0]), fin)
        assert np.array_equal(out[k][~fin, 0].view(np.int64), hst[k][~fin, 0].view(np.int64))
        assert (np.abs(out[k][fin, 0] - hst[k][fin, 0]) <= 2e-9 * L[fin]).all()
    assert np.array_equal(out[4], hst[4])
    CR.check_times(so, T, C, faces, out[0], out[1], ref, out[2], out[3])
    return out


def test_rest_to_rest(solver):
    H.check_rest_to_rest(_call(solver))


@pytest.mark.parametrize("T", [0.05, 1.0, 20.0])
def test_parabola(solver, T):
    H.check_parabola(_call(solver), T)


def test_slanted_face(solver):
    H.check_slanted(_call(solver))


def test_constant_trajectory_gives_the_exact_value(solver):
    H.check_constant(_call(solver))


def test_ragged_batches_meet_the_contract(solver, host, case):
    """Within 1e-9 L_h of the reference, within 2e-9 L_h of the host backend, the times in
    range and attaining the stored values, the flags those of the reference."""
    H.check_ragged_contract(case)
    c = case
    against_host(solver, host, c["so"], c["T"], c["C"], c["faces"], c["fo"], H.RADIUS)


def test_ragged_face_counts(solver):
    H.check_ragged_face_counts(solver.solve, _call(solver))


def test_shared_mode_equals_the_repeated_csr(solver, rest):
    H.check_shared_equals_repeated(rest, _call(solver))


def test_ties_go_to_the_lowest_segment_then_face(solver):
    H.check_ties(_call(solver))


def test_no_faces(solver):
    H.check_no_faces(_call(solver))


def test_unusable_rows_in_the_middle_of_a_tile(solver, rest):
    """Rows 3, 21, 30, 41 and 47 are not the first of their tiles."""
    H.check_bad_rows(rest, _call(solver))


def test_unusable_faces_are_left_out(solver, rest):
    H.check_bad_faces(rest, _call(solver))


def test_small_batches(solver, host, rest):
    """B = 1 with M = 1 and one face; B = 1 with M = 16; B = 5: two tiles, the second holding
    one trajectory."""
    c = rest
    M = np.diff(c["so"])
    one, sixteen = int(np.flatnonzero(M == 1)[0]), int(np.flatnonzero(M == 16)[0])
    (so, T, C, faces, fo), _ = gather(c, [one])
    against_host(solver, host, so, T, C, faces[3:4], np.array([0, 1]))
    for rows in ([sixteen], [sixteen, one, 2, 5, 23]):
        (so, T, C, faces, fo), _ = gather(c, rows)
        out = against_host(solver, host, so, T, C, faces, fo, H.RADIUS)
        assert _same(local(out, so, fo), pick(local(c["out"], c["so"], c["fo"]), c["so"], rows))


def test_full_tile_with_items_straddling_the_passes(solver, host, rest):
    """B = 4 x M = 16: 64 segments.  Face counts 0..9 and one segment of 70: the tile's items
    are no multiple of 64, and the 70 faces straddle two passes whatever comes before."""
    c = rest
    rows = list(np.flatnonzero(np.diff(c["so"]) == 16)[:3]) + [16, int(np.flatnonzero(np.diff(c["so"]) == 1)[0])]
    (so, T, C, _, _), _ = gather(c, rows)  # 16 + 16 + 16 + 15 + 1 segments ...
    so = np.array([0, 16, 32, 48, 64], np.int32)  # ... as four trajectories of 16 (each segment stands alone)
    rng = np.random.default_rng(17)
    counts = rng.integers(0, 10, 64)
    counts[37] = 70
    assert counts.sum() % 64 != 0 and counts[:37].sum() % 64 + 70 > 64
    faces, fo = H.ragged_faces(rng, counts)
    out = against_host(solver, host, so, T, C, faces, fo)
    assert ((out[3] == -1) == (counts == 0)).all()


def test_a_tile_without_items_between_two_with_items(solver, rest):
    """B = 12: rows 4..7 own no face; every row as in the batch of its own tile's rows alone."""
    c = rest
    rows = [1, 2, 3, 5, 7, 9, 10, 11, 12, 14, 17, 18]
    (so, T, C, faces, fo), _ = gather(c, rows)
    cnt = np.diff(fo)
    cnt[so[4]:so[8]] = 0
    fo2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    faces2 = np.concatenate([faces[:fo[so[4]]], faces[fo[so[8]]:]])
    out = _device_call(solver, so, T, C, faces2, fo2, H.RADIUS)
    assert np.isneginf(out[0][4:8, 0]).all() and (out[1][4:8] == -1).all() and not out[4][4:8].any()
    assert np.isneginf(out[2][so[4]:so[8], 0]).all() and (out[3][so[4]:so[8]] == -1).all()
    keep = [0, 1, 2, 3, 8, 9, 10, 11]
    assert _same(pick(local(out, so, fo2), so, keep),
                 pick(local(c["out"], c["so"], c["fo"]), c["so"], [rows[k] for k in keep]))


def test_grid_stride_and_lds_reuse(solver):
    """B = 4 * 4096 + 1 with M = 1: every workgroup runs a second tile on the LDS its first used,
    and the last tile holds one row.  Rows repeat five parabolas and three shared faces; every
    row is bit-equal to its original from the five-row call."""
    B = TILE * GRID + 1
    ks = np.array([0.3, 0.7, 3.0, -0.4, 2.0])
    C5 = np.concatenate([H.parabola(k, 1.5)[2] for k in ks])
    faces = np.array([[0.0, 1.0, 0.0, 0.2], [0.6, 0.8, 0.0, 0.1], [0.0, -1.0, 0.0, 0.1]])
    small = _device_call(solver, np.arange(6, dtype=np.int32), np.full(5, 1.5), C5, faces, None, -0.3)
    assert len(set(small[1][:, 1])) == 3 and len(set(small[4])) == 2
    src = np.arange(B) % 5
    out = _device_call(solver, np.arange(B + 1, dtype=np.int32), np.full(B, 1.5), C5[src], faces, None, -0.3)
    assert _same(out, tuple(a[src] for a in small))


def test_a_bad_segment_count_in_the_middle_of_a_tile(solver, rest):
    """M = 17 from the offsets between rows 0 and 1: NONFINITE alone, NaN, -1, its 17 segment
    rows not written at all; every other row bit-equal to the clean batch's."""
    from trajectory_generator_ros2_amd import FEAS_NONFINITE
    c = rest
    so, T, C, fo = c["so"], c["T"], c["C"], c["fo"]
    M = np.diff(so)
    so2 = np.cumsum(np.concatenate([[0, M[0], 17], M[1:]])).astype(np.int32)
    T2 = np.concatenate([T[:M[0]], np.ones(17), T[M[0]:]])
    C2 = np.concatenate([C[:M[0]], np.full((17, 3, 8), 0.5), C[M[0]:]])
    fo2 = np.concatenate([fo[:M[0] + 1], np.repeat(fo[M[0]], 17), fo[M[0] + 1:]])
    out = _device_call(solver, so2, T2, C2, c["faces"], fo2, H.RADIUS)
    assert out[4][1] == FEAS_NONFINITE and np.isnan(out[0][1]).all() and (out[1][1] == -1).all()
    assert np.isnan(out[2][M[0]:M[0] + 17]).all() and (out[3][M[0]:M[0] + 17] == -7).all()
    rest_rows = np.r_[0, 2:49]
    assert _same(pick(out, so2, rest_rows), c["out"])


def test_a_row_alone_and_at_position_37_of_65(solver, rest):
    c = rest
    rows = list(np.arange(65) % 48)
    rows[37] = 23
    (so, T, C, faces, fo), _ = gather(c, rows)
    big = _device_call(solver, so, T, C, faces, fo, H.RADIUS)
    (so1, T1, C1, faces1, fo1), _ = gather(c, [23])
    alone = _device_call(solver, so1, T1, C1, faces1, fo1, H.RADIUS)
    assert _same(pick(local(big, so, fo), so, [37]), local(alone, so1, fo1))
    assert _same(local(big, so, fo), pick(local(c["out"], c["so"], c["fo"]), c["so"], rows))


def test_each_output_omitted_in_turn(solver, rest):
    c = rest
    for k, name in enumerate(NAMES):
        out = _device_call(solver, c["so"], c["T"], c["C"], c["faces"], c["fo"], H.RADIUS, omit=(name,))
        assert out[k] is None and _same(out[:k] + out[k + 1:], c["out"][:k] + c["out"][k + 1:])
    out = _device_call(solver, c["so"], c["T"], c["C"], c["faces"], c["fo"], H.RADIUS, omit=NAMES[:4])
    assert np.array_equal(out[4], c["out"][4])


def test_host_pointer_call_gives_the_device_call_bits(solver, rest):
    c = rest
    assert _same(solver.corridor(c["so"], c["T"], c["C"], c["faces"], c["fo"], H.RADIUS), c["out"])
    shared = c["faces"][:7]
    assert _same(solver.corridor(c["so"], c["T"], c["C"], shared, None, H.RADIUS),
                 _device_call(solver, c["so"], c["T"], c["C"], shared, None, H.RADIUS))


def test_argument_errors_launch_nothing(solver, host, rest):
    import torch
    from trajectory_generator_ros2_amd import COR_MAX_FACES, ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError
    c = rest
    B, S, F = 48, int(c["so"][-1]), len(c["faces"])
    dso, dT, dC, dF, dFo = _dev(c["so"]), _dev(c["T"]), _dev(c["C"]), _dev(c["faces"]), _dev(c["fo"])
    out = _outputs(B, S)
    odd = torch.full((B * 2 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:]  # 8 B past 16-B alignment
    odd_fo = torch.zeros(S + 2, dtype=torch.int64, device="cuda")[1:]
    none = dict.fromkeys(NAMES)
    for F_, dF_, dFo_, r, o in ((F, dF, dFo, float("nan"), out), (F, dF, dFo, float("inf"), out), (F, dF, dFo, 0.0, none),
                                (F, None, dFo, 0.0, out), (COR_MAX_FACES + 1, dF, None, 0.0, out), (-1, dF, dFo, 0.0, out),
                                (F, dF, dFo, 0.0, dict(out, d_rec=odd)), (F, dF, odd_fo, 0.0, out)):
        with pytest.raises(TgmsError) as e:
            solver.corridor_device(B, dso, dT, dC, F_, dF_, dFo_, r, **o)
        assert e.value.status == ERR_INVALID_ARG
    solver.corridor_device(0, None, None, None, 0, None, None, 0.0, **out)  # B == 0: TGMS_OK, nothing launched
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.corridor_device(B, dso, dT, dC, F, dF, dFo, 0.0, **out)
    assert e.value.status == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(odd).all()) and bool(torch.isnan(out["d_rec"]).all()) and bool(torch.isnan(out["d_seg_rec"]).all())
    assert all(bool((out[k] == -7).all()) for k in ("d_where", "d_seg_face", "d_flags"))


def test_captured_into_a_graph_and_replayed(solver, case, rest):
    """The device call inside torch.cuda.graph, replayed twice on fresh NaN / -7 outputs: each
    replay is bit-equal to the direct call."""
    import torch
    c = case
    B, S = 48, int(c["so"][-1])
    dso, dT, dC, dF, dFo = _dev(c["so"]), _dev(c["T"]), _dev(c["C"]), _dev(c["faces"]), _dev(c["fo"])
    out = _outputs(B, S)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        try:
            solver.corridor_device(B, dso, dT, dC, len(c["faces"]), dF, dFo, H.RADIUS, stream=side.cuda_stream, **out)
        except Exception as e:  # noqa: BLE001 -- reported below, the capture ends normally
            err = e
    torch.cuda.current_stream().wait_stream(side)
    assert err is None, err
    torch.cuda.synchronize()
    for _ in range(2):
        for k in NAMES:
            out[k].fill_(float("nan") if out[k].dtype == torch.float64 else -7)
        g.replay()
        torch.cuda.synchronize()
        assert _same(tuple(out[k].cpu().numpy() for k in NAMES), c["out"])
    del g
