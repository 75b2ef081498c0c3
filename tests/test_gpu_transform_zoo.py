"""GPU: the three transforming device calls (tgms_dilate_batch_device, tgms_cut_batch_device,
tgms_corridor_split_batch_device) on the constructed polynomials of poly_zoo.py: the checks of
transform_zoo.py through a backend that wraps the device entry points, with outputs prefilled
with NaN / -7 (-9) at the header's capacities and nothing written beyond the totals (the wrappers
of test_gpu_cut.py and test_gpu_split.py assert it).  Every call is also made on the host backend:
integers, flags (dilate's evaluation count excepted), times and t0_out agree to the bit, values
to twice the call's contract bound.  The round trips keep the transforming call's output buffers
on the device and hand them to the analysis call as they are.  Then the host-pointer entry points
on the GPU handle, and placement: the zoo rows mixed into the solved 48-row batch at the first, a
middle and the last lane of a tile of four and alone in a tail tile are bit-equal to the same
rows run alone.

References: test_poly_zoo_host.zoo_reference() and transform_zoo's cached zoo, built once per
session on the CPU; the long-double grid that caps them runs in the host file only."""
import numpy as np
import pytest

import cut_ref as CR
import dilate_ref as DR
import poly_zoo as Z
import split_ref as SR
import test_gpu_cut as GC
import test_gpu_dilate as GD
import test_gpu_poly_zoo as GP
import test_gpu_split as GS
import test_poly_zoo_host as H
import test_split_host as SH
import transform_zoo as X
from extrema_ref import bit_equal

pytestmark = pytest.mark.gpu

TILE = 4  # trajectories per workgroup of the three kernels


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()


def _full(shape, dt):
    import torch
    return torch.full(shape, float("nan") if dt == "f" else -7, dtype=torch.float64 if dt == "f" else torch.int32,
                      device="cuda")


class Device(X.Host):
    """transform_zoo's backend protocol on the *_batch_device entry points; with `host`, every
    transforming call is repeated on the host backend and compared."""

    def __init__(self, solver, host=None):
        self.s, self.h = solver, host
        self._cut, self._split, self._an = GC.dev_cut(solver), GS._split(solver), GP.Device(solver)

    def dilate(self, so, T, C, lim, s_lo, s_hi=X.S_HI, g=X.G):
        out = GD._device_call(self.s, so, T, C, lim, s_lo, s_hi, g)
        if self.h is not None:
            ref = self.h.dilate(so, T, C, lim, s_lo, s_hi, g)
            assert np.array_equal(out[1], ref[1]) and np.array_equal(out[2] & DR.MASK, ref[2] & DR.MASK)
            same = out[0] == ref[0]  # the same s gives the same bits (the power rule of include/tgms.h)
            seg = np.repeat(same, np.diff(so))
            assert bit_equal(out[3][seg], ref[3][seg]) and bit_equal(out[4][seg], ref[4][seg])
        return out

    def cut(self, so, W, T, C, tc, mf=0.0, ED=None):
        out = self._cut(so, W, T, C, tc, mf, ED)
        if self.h is not None:
            hst = self.h.cut(so, W, T, C, tc, mf, ED)
            GC.bit_equal_to_host(out, hst)
            ref = CR.cut(so, W, T, C, tc, mf, ED)
            for i, key in ((1, "W"), (3, "ED"), (4, "C")):  # twice the header's condition bound
                a, b = np.asarray(out[i]).reshape(ref[key].shape), np.asarray(hst[i]).reshape(ref[key].shape)
                assert (np.abs(a - b) <= 2 * ref[key + "_tol"]).all(), key
        return out

    def corridor(self, so, T, C, faces, fo, r=0.0):
        B, dso, dT, dC = self._an._in(so, T, C)
        S, fc = int(so[-1]), np.asarray(faces, np.float64).reshape(-1, 4)
        o = self._an._out(((B, 2), "f"), ((B, 2), "i"), ((S, 2), "f"), ((S,), "i"), ((B,), "i"))
        self.s.corridor_device(B, dso, dT, dC, len(fc), _dev(fc), None if fo is None else _dev(np.asarray(fo, np.int64)),
                               float(r), *o)
        return self._an._np(o)

    def split(self, so, W, T, C, faces, fo, seg_rec, seg_face, r=0.0, mode=SR.PULL, min_frac=0.1):
        out = self._split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac)
        if self.h is not None:
            hst = self.h.split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac)
            ref = SR.split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac)
            SH.compare(out, dict(ref, W=hst[1]), tol=2e-9)
            assert GS._same((out[0], out[2], out[4], out[5], out[6]), (hst[0], hst[2], hst[4], hst[5], hst[6]))
        return out

    def bounds(self, so, T, C):
        return self._an.bounds(so, T, C)

    def thrust(self, so, T, C, g):
        return self._an.thrust(so, T, C, g)

    def separation(self, so, T, C, pairs, t0):
        return self._an.separation(so, T, C, pairs, t0)

    def dilate_records(self, so, T, C, lim, s_lo, g=X.G):
        """The dilate call's own output buffers, still on the device, into bounds and thrust."""
        import torch
        from test_dilate_host import limits_of
        so = np.asarray(so, np.int32)
        B, S = len(so) - 1, int(so[-1])
        dso, dT, dC = _dev(so), _dev(np.asarray(T, np.float64).reshape(-1)), _dev(np.asarray(C, np.float64).reshape(-1, 3, 8))
        o = [_full((B,), "f"), _full((B,), "i"), _full((B,), "i"), _full((S,), "f"), _full((S, 3, 8), "f")]
        lk, lt = limits_of(lim)
        self.s.dilate_device(B, dso, dT, dC, g, lk, lt, s_lo, X.S_HI, *o)
        ext, fb, th, ft = _full((B, 10), "f"), _full((B,), "i"), _full((B, 6), "f"), _full((B,), "i")
        self.s.bounds_device(B, dso, o[3], o[4], None, ext, fb)
        self.s.thrust_device(B, dso, o[3], o[4], float(g), None, th, ft)
        torch.cuda.synchronize()
        assert not fb.cpu().numpy().any() and not ft.cpu().numpy().any()
        return tuple(x.cpu().numpy() for x in o), ext.cpu().numpy(), th.cpu().numpy()

    def cut_then(self, so, W, T, C, tc, kind, g=X.G, pairs=None):
        """The cut's output buffers at their capacities, still on the device, into one analysis call
        (seg_offsets_out says how much of them holds rows)."""
        import torch
        so = np.asarray(so, np.int32)
        B, S = len(so) - 1, int(so[-1])
        o = GC._outputs(B, S)
        self.s.cut_device(B, _dev(so), _dev(np.asarray(W, np.float64).reshape(-1, 3)),
                          _dev(np.asarray(T, np.float64).reshape(-1)), _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)),
                          _dev(np.asarray(tc, np.float64)), 0.0, **o)
        d = (B, o["d_seg_offsets_out"], o["d_seg_times_out"], o["d_coeffs_out"])
        fl = _full((B if kind != "separation" else len(pairs),), "i")
        if kind == "bounds":
            rec = _full((B, 10), "f")
            self.s.bounds_device(*d, None, rec, fl)
        elif kind == "thrust":
            rec = _full((B, 6), "f")
            self.s.thrust_device(*d, float(g), None, rec, fl)
        else:
            rec = _full((len(pairs), 2), "f")
            self.s.separation_device(*d, len(pairs), _dev(np.asarray(pairs, np.int32)), o["d_t0_out"], None, 0.0, rec, fl)
        torch.cuda.synchronize()
        assert not fl.cpu().numpy().any()
        raw = {k: v.cpu().numpy() for k, v in o.items()}
        S2 = int(raw["d_totals"][0])
        out = (raw["d_seg_offsets_out"], raw["d_waypoints_out"][:S2 + B], raw["d_seg_times_out"][:S2],
               raw["d_end_derivs_out"], raw["d_coeffs_out"][:S2], raw["d_parent"][:S2], raw["d_t0_out"], raw["d_flags"])
        return out, rec.cpu().numpy()


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield X.Host(s)
    s.close()


@pytest.fixture(scope="module")
def be(solver, host):
    return Device(solver, host)


def _agree(dev, hst, tol_of):
    """Closed-form scales of the two backends: each within its tolerance of s*, so within twice
    that of each other."""
    assert dev.keys() == hst.keys()
    for k in dev:
        assert abs(dev[k] - hst[k]) <= 2 * tol_of(k) * hst[k], (k, dev[k], hst[k])


# ---- A. dilate ----

def test_dilate_peak_on_a_knot(be, host):
    tol = {"f_hi": X.s_tolerance(DR.THRUST_HIGH, None, 10.0), "tilt": X.s_tolerance(DR.TILT, None, 0.25),
           "a": X.s_tolerance(DR.ACCEL, None)}
    _agree(X.check_dilate_knot_peak(be, "device"), X.check_dilate_knot_peak(host, "host"), lambda k: tol[k[1]])


def test_dilate_deficient_rows(be, host):
    _agree(X.check_dilate_deficient(be, "device"), X.check_dilate_deficient(host, "host"), lambda k: 2e-9)


def test_dilate_ballistic_arc_under_f_min(be, host):
    # the larger of the two rows' derived tolerances (3e-9 on the arc, 3.03e-9 on row 0), rounded up
    _agree(X.check_dilate_ballistic(be, "device"), X.check_dilate_ballistic(host, "host"), lambda k: 3.1e-9)


def test_dilate_tilt_limit_at_free_fall(be, host):
    """Both backends: finite, no NONFINITE, feasible, and the same active code and low flag bits."""
    d, h = X.check_free_fall_tilt(be, "device"), X.check_free_fall_tilt(host, "host")
    for r in d:
        assert d[r][1:] == h[r][1:], (r, d[r], h[r])


@pytest.mark.parametrize("s_lo", [0.625, 0.875])
def test_dilate_contract_on_the_zoo(be, s_lo):
    X.check_dilate_contract(be, "device", s_lo=s_lo)


def test_dilate_translation(be):
    X.check_dilate_translation(be)


@pytest.mark.parametrize("k", Z.RESCALES)
def test_dilate_time_rescale(be, k):
    X.check_dilate_rescale(be, k)


def test_dilate_idempotence(be):
    X.check_dilate_idempotence(be, "device")


def test_dilate_then_bounds_and_thrust_on_the_device(be):
    X.check_dilate_round_trip(be, "device")


# ---- B. cut ----

def test_cut_zoo_against_the_reference(be):
    X.check_cut_against_ref(be, "device")


def test_cut_on_the_knot_that_is_the_extremum(be):
    X.check_cut_knot_peak(be)


def test_cut_deficient_pieces(be):
    X.check_cut_deficient(be)


def test_cut_composition(be):
    X.check_cut_composition(be, "device")


def test_cut_translation(be):
    X.check_cut_translation(be)


@pytest.mark.parametrize("k", Z.RESCALES)
def test_cut_time_rescale(be, k):
    X.check_cut_rescale(be, k)


def test_cut_then_the_analysis_calls_on_the_device(be):
    X.check_cut_round_trips(be, "device")


# ---- C. split ----

@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_split_cheb_in_a_corridor(be, mode):
    X.check_split_cheb(be, "device", mode)


def test_split_excursion_on_an_interior_knot(be):
    X.check_split_knot_peak(be, "device")


@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_split_deficient_row(be, mode):
    X.check_split_deficient(be, "device", mode)


@pytest.mark.parametrize("mode", [SR.PULL, SR.CHORD])
def test_split_then_solve_then_corridor(be, mode):
    X.check_split_round_trip(be, "device", mode)


# ---- the host-pointer entry points on the GPU handle ----

def test_host_pointer_calls_on_the_gpu_handle(solver):
    hp = X.Host(solver)
    X.check_dilate_knot_peak(hp, "host-pointer")
    X.check_dilate_ballistic(hp, "host-pointer")
    X.check_free_fall_tilt(hp, "host-pointer")
    X.check_cut_against_ref(hp, "host-pointer")
    X.check_cut_knot_peak(hp)
    X.check_cut_deficient(hp)
    X.check_split_knot_peak(hp, "host-pointer")
    for mode in (SR.PULL, SR.CHORD):
        X.check_split_cheb(hp, "host-pointer", mode)
        X.check_split_deficient(hp, "host-pointer", mode)


# ---- D. placement ----

def _placed_with_waypoints():
    """test_gpu_poly_zoo._placed()'s 65 rows with their waypoints, and the mixed batch they come
    from: ((so, T, C), W) twice, and the order."""
    (so, T, C), _, _ = H.mixed()
    so48, W48, _ = Z.ragged48_times()
    W = np.concatenate([X.zoo_w()[1], W48])
    placed, order = GP._placed()
    _, Wp = X.rows((so, T, C), W, order)
    return (placed, Wp), ((so, T, C), W), order


def _per_row(so, rows_of):
    return np.concatenate([np.arange(so[b], so[b + 1]) for b in rows_of]) if len(rows_of) else np.zeros(0, int)


def test_dilate_placement_in_tiles(solver):
    """Every row's scale, active, flags and output rows are bit-equal to the same row among the ten
    zoo rows run alone, or among the 48 solved rows run without zoo rows."""
    dev = Device(solver)
    (placed, _), (mixed, _), order = _placed_with_waypoints()
    alone, solved = Z.take(mixed, list(range(10))), Z.take(mixed, list(range(10, 58)))
    zpos, rpos = np.flatnonzero(order < 10), np.flatnonzero(order >= 10)
    assert len(order) % TILE == 1 and len(zpos) == 17 and list(order[rpos]) == list(range(10, 58))
    m, a, s = (dev.dilate(*b, X.LIM6, 0.75, X.S_HI, X.G) for b in (placed, alone, solved))
    assert (m[1] != DR.NONE).any() and not (m[2] & DR.MASK).any()
    for q in range(3):
        assert np.array_equal(CR.bits(m[q][zpos]), CR.bits(a[q][order[zpos]])), q
        assert np.array_equal(CR.bits(m[q][rpos]), CR.bits(s[q])), q
    for q in (3, 4):
        assert bit_equal(m[q][_per_row(placed[0], zpos)], a[q][_per_row(alone[0], order[zpos])])
        assert bit_equal(m[q][_per_row(placed[0], rpos)], s[q])


def _cut_row(out, b, so_in):
    """Row b of a cut result, its parents relative to the row's first input segment."""
    so, W, T, ED, C, parent, t0, fl = out
    a0, a1 = so[b], so[b + 1]
    return (W[a0 + b:a1 + b + 1], T[a0:a1], np.asarray(ED).reshape(-1, 18)[b], C[a0:a1], parent[a0:a1] - so_in[b],
            t0[b:b + 1], fl[b:b + 1])


def test_cut_placement_in_tiles(solver):
    """The placed batch cut at a special time per zoo row and at 0.4 D per solved row: each row's own
    output rows, found through seg_offsets_out, are bit-equal to the row cut alone, and
    seg_offsets_out is the cumulative sum of the per-row counts."""
    dev = Device(solver)
    (placed, Wp), (mixed, W), order = _placed_with_waypoints()
    times = X.cut_times()
    D = np.array([float(CR.knots(mixed[1][mixed[0][b]:mixed[0][b + 1]])[-1]) for b in range(58)])
    tc_mixed = np.array([times[b][3 % len(times[b])] if b < 10 else 0.4 * D[b] for b in range(58)])
    tc = tc_mixed[order]
    out = dev.cut(placed[0], Wp, placed[1], placed[2], tc, 0.0)
    counts = []
    for pos, b in enumerate(order):
        one, W1 = X.rows(mixed, W, [b])
        ref = dev.cut(one[0], W1, one[1], one[2], tc[pos:pos + 1], 0.0)
        counts.append(int(ref[0][1]))
        for x, y in zip(_cut_row(out, pos, placed[0]), _cut_row(ref, 0, one[0])):
            assert np.array_equal(CR.bits(x), CR.bits(y)), (pos, b)
    assert np.array_equal(out[0], np.concatenate([[0], np.cumsum(counts)]))
    assert len(set(counts)) > 3 and (out[7] & CR.DONE).any()


def test_split_placement_in_tiles(solver):
    """Two faces per segment (x <= 1, -x <= 128), r = 0: each row's own output rows, with parents
    and face offsets relative to the row, are bit-equal to the row split alone."""
    dev = Device(solver)
    (placed, Wp), (mixed, W), order = _placed_with_waypoints()
    two = np.array([[1.0, 0.0, 0.0, 1.0], [-1.0, 0.0, 0.0, 128.0]])

    def run(batch, Wb):
        faces, fo = X.per_segment(two, int(batch[0][-1]))
        seg = dev.corridor(*batch, faces, fo, 0.0)[2:4]
        return dev.split(batch[0], Wb, batch[1], batch[2], faces, fo, seg[0], seg[1], 0.0, SR.PULL, 0.1)
    out = run(placed, Wp)
    assert (out[6] & SR.DONE).any() and (out[6] & SR.AT_END).any() and (out[6] == 0).any()
    counts = []
    for pos, b in enumerate(order):
        ref = run(*X.rows(mixed, W, [b]))
        counts.append(int(ref[0][1]))
        for x, y in zip(GS.row_of(out, pos), GS.row_of(ref, 0)):
            assert np.array_equal(CR.bits(x), CR.bits(y)), (pos, b)
    assert np.array_equal(out[0], np.concatenate([[0], np.cumsum(counts)]))
