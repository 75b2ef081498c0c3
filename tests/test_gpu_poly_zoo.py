"""GPU: the seven continuous-analysis device calls (tgms_*_batch_device) on the constructed
polynomials of poly_zoo.py and under its transforms.  The assertions are test_poly_zoo_host.py's,
run through a backend that wraps the device entry points: the 1e-9 contract of include/tgms.h
against exact answers and grid-checked references, and the metamorphic relations.  Then
agreement with the host backend to 2e-9, and placement: the zoo rows mixed into the solved
48-row batch at the first, a middle and the last lane of a tile and alone in a tail tile are
bit-equal to the same rows run alone, and the 48 rows to the batch without them.

The references come from test_poly_zoo_host.zoo_reference(), computed once per session on the CPU
(np.roots and long-double polish on 17 segments, about 5 s, charged to the first test that asks)
and shared; the long-double grid that caps them runs in the host file only.  H.mixed() adds one
host solve of 48 trajectories."""
import numpy as np
import pytest

import poly_zoo as Z
import test_poly_zoo_host as H
from extrema_ref import bit_equal

pytestmark = pytest.mark.gpu

TILE = 4       # trajectories per workgroup: bounds, thrust, rate, corridor (the TILE of their GPU tests)
SEP_TILE = 16  # pairs per workgroup (test_gpu_separation.py)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the fixtures are read-only


class Device:
    """A Solver's numpy methods on the *_batch_device entry points, outputs prefilled with NaN / -7."""

    def __init__(self, solver):
        self.s = solver

    def _in(self, so, T, C):
        return (len(so) - 1, _dev(np.asarray(so, np.int32)), _dev(np.asarray(T, np.float64).reshape(-1)),
                _dev(np.asarray(C, np.float64).reshape(-1, 3, 8)))

    @staticmethod
    def _out(*shapes):
        import torch
        return [torch.full(s, float("nan") if dt == "f" else -7, dtype=torch.float64 if dt == "f" else torch.int32,
                           device="cuda") for s, dt in shapes]

    @staticmethod
    def _np(outs):
        import torch
        torch.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in outs)

    def bounds(self, so, T, C, limits=None):
        B, dso, dT, dC = self._in(so, T, C)
        o = self._out(((B, 10), "f"), ((B,), "i"))
        self.s.bounds_device(B, dso, dT, dC, limits, *o)
        return self._np(o)

    def thrust(self, so, T, C, g, limits=None):
        B, dso, dT, dC = self._in(so, T, C)
        o = self._out(((B, 6), "f"), ((B,), "i"))
        self.s.thrust_device(B, dso, dT, dC, float(g), limits, *o)
        return self._np(o)

    def rate(self, so, T, C, g):
        B, dso, dT, dC = self._in(so, T, C)
        o = self._out(((B, 2), "f"), ((int(so[-1]), 2), "f"), ((B,), "i"))
        self.s.rate_device(B, dso, dT, dC, float(g), float("inf"), *o)
        return self._np(o)

    def corridor(self, so, T, C, faces):
        B, dso, dT, dC = self._in(so, T, C)
        S, fc = int(so[-1]), np.asarray(faces, np.float64).reshape(-1, 4)
        o = self._out(((B, 2), "f"), ((B, 2), "i"), ((S, 2), "f"), ((S,), "i"), ((B,), "i"))
        self.s.corridor_device(B, dso, dT, dC, len(fc), _dev(fc), None, 0.0, *o)
        return self._np(o)

    def separation(self, so, T, C, pairs=None, start_times=None, scale=None, r_min=0.0):
        B, dso, dT, dC = self._in(so, T, C)
        P = B * (B - 1) // 2 if pairs is None else len(pairs)
        o = self._out(((P, 2), "f"), ((P,), "i"))
        self.s.separation_device(B, dso, dT, dC, P, None if pairs is None else _dev(np.asarray(pairs, np.int32)),
                                 None if start_times is None else _dev(np.asarray(start_times, np.float64)), scale,
                                 float(r_min), *o)
        return self._np(o)

    def neighbors(self, so, T, C, r_min, start_times=None, scale=None):
        B, dso, dT, dC = self._in(so, T, C)
        o = self._out(((B, 2), "f"), ((B,), "i"), ((B,), "i"), ((B,), "i"), ((B,), "i"))
        self.s.neighbors_device(B, dso, dT, dC, float(r_min),
                                None if start_times is None else _dev(np.asarray(start_times, np.float64)), scale, *o)
        return self._np(o)

    def clearance(self, so, T, C, obstacles, r_min, scale=None):
        B, dso, dT, dC = self._in(so, T, C)
        ob = np.asarray(obstacles, np.float64).reshape(-1, 6)
        o = self._out(((B, 2), "f"), ((B,), "i"), ((B,), "i"), ((B,), "i"), ((B,), "i"))
        self.s.clearance_device(B, dso, dT, dC, len(ob), _dev(ob), float(r_min), scale, *o)
        return self._np(o)


@pytest.fixture(scope="module")
def dev(solver):
    return Device(solver)


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


@pytest.mark.parametrize("kind,k", H.VARIANTS)
def test_zoo_meets_the_contract(dev, kind, k):
    H.run_variant(dev, kind, k, "device")


def test_rate_on_cheb_meets_the_contract(dev):
    """test_poly_zoo_host.py's test of this name on the device: the row whose root location needed
    the polish of csrc/tgms_rate_core.h."""
    H.check_rate_on_cheb(dev, "device")


def test_translation(dev):
    H.check_translation(dev)


@pytest.mark.parametrize("k", Z.RESCALES)
def test_time_rescale(dev, k):
    H.check_rescale(dev, k)


@pytest.mark.parametrize("s", Z.CLOCKS)
def test_clock_shift(dev, s):
    H.check_clock(dev, s)


def test_device_agrees_with_the_host_backend(dev, host):
    """To 2e-9 in each contract's own unit, on the zoo and the 48 solved rows together."""
    (so, T, C), t0, pairs = H.mixed()
    eh, ed = host.bounds(so, T, C)[0], dev.bounds(so, T, C)[0]
    pm = np.abs(eh[:, 0:6]).max(axis=1)
    e_p = (np.abs(ed[:, 0:6] - eh[:, 0:6]).max(axis=1) / pm).max()
    pk = np.where(eh[:, 6:9] == 0, 1.0, eh[:, 6:9])
    e_k = (np.abs(ed[:, 6:9] - eh[:, 6:9]) / pk).max()
    th, td = host.thrust(so, T, C, H.G)[0], dev.thrust(so, T, C, H.G)[0]
    F2 = np.where(th[:, 2] > 1e-12, th[:, 2], 1.0) ** 2
    e_f = (np.abs(td[:, [0, 2]] ** 2 - th[:, [0, 2]] ** 2) / F2[:, None]).max()
    pos = th[:, 0] > 1e-3
    e_t = (np.abs(td[pos, 4] - th[pos, 4]) / (th[pos, 2] / th[pos, 0])).max()
    rh, rd = host.rate(so, T, C, H.G), dev.rate(so, T, C, H.G)
    unit = np.where(pos, th[:, 2] * eh[:, 8] / np.where(pos, th[:, 0], 1.0) ** 2, np.inf)
    unit = np.where(unit > 0, unit, 1.0)
    e_r = max((np.abs(rd[0][:, 0] - rh[0][:, 0]) / unit).max(),
              (np.abs(rd[1][:, 0] - rh[1][:, 0]) / np.repeat(unit, np.diff(so))).max())  # records and segment rows
    ch, cd = host.corridor(so, T, C, H.FACES), dev.corridor(so, T, C, H.FACES)
    Lh = (np.abs(H.FACES[ch[1][:, 1], 0:3]) * np.maximum(np.abs(eh[:, 0:3]), np.abs(eh[:, 3:6]))).sum(axis=1) \
        + np.abs(H.FACES[ch[1][:, 1], 3])
    e_c = (np.abs(cd[0][:, 0] - ch[0][:, 0]) / Lh).max()
    sh, sd = host.separation(so, T, C, pairs, t0)[0], dev.separation(so, T, C, pairs, t0)[0]
    L = np.maximum(np.abs(eh[:, 0:3]), np.abs(eh[:, 3:6])).max(axis=1)
    L2 = np.maximum(L[pairs[:, 0]], L[pairs[:, 1]]) ** 2
    e_s = (np.abs(sd[:, 0] ** 2 - sh[:, 0] ** 2) / L2).max()
    ob = H.cheb_boxes()
    kh, kd = host.clearance(so, T, C, ob, 8.0), dev.clearance(so, T, C, ob, 8.0)
    assert np.array_equal(kh[2], kd[2])
    hit = kh[2] > 0
    e_o = (np.abs(kd[0][hit, 0] ** 2 - kh[0][hit, 0] ** 2) / np.maximum(L[hit], np.abs(ob).max()) ** 2).max()
    nh, nd = host.neighbors(so, T, C, 1.0, t0), dev.neighbors(so, T, C, 1.0, t0)
    assert np.array_equal(nh[2], nd[2]) and np.array_equal(nh[1], nd[1]) and np.array_equal(nh[4], nd[4])
    hit = nh[2] > 0
    e_n = (np.abs(nd[0][hit, 0] ** 2 - nh[0][hit, 0] ** 2) / np.maximum(L[hit], L[nh[1][hit]]) ** 2).max()
    print("device vs host: neighbours %.3g" % e_n)
    assert e_n <= 2e-9
    print("device vs host: extents %.3g, peaks %.3g, thrust^2 %.3g, tilt %.3g, rate %.3g, corridor %.3g, "
          "separation %.3g, clearance %.3g" % (e_p, e_k, e_f, e_t, e_r, e_c, e_s, e_o))
    assert max(e_p, e_k, e_f, e_t, e_r, e_c, e_s, e_o) <= 2e-9


def _placed():
    """65 rows: the 48 solved rows with sixteen zoo rows (the ten, the first six again) put in at
    the first, a middle and the last lane of tiles of four and of groups of sixteen, and zoo row 9
    once more as row 64, alone in the tail tile of either width (65 = 16 * 4 + 1 = 4 * 16 + 1).
    Returns the batch and, per position, the row of H.mixed() that sits there."""
    (so, T, C), _, _ = H.mixed()
    at = (0, 5, 7, 15, 16, 21, 23, 31, 32, 37, 39, 47, 48, 53, 55, 63)  # lanes 0, 1, 3 of a tile; 0, 5, 7, 15 of a group
    zoo_at = {pos: n % 10 for n, pos in enumerate(at)}
    solved = iter(range(10, 58))
    order = [zoo_at[pos] if pos in zoo_at else next(solved) for pos in range(64)] + [9]
    assert len(order) % TILE == 1 and len(order) % SEP_TILE == 1 and set(order) == set(range(58))
    return Z.take((so, T, C), order), np.array(order)


def test_placement_in_tiles(dev):
    """Every row of the placed batch holds the bits of the same row elsewhere: a zoo row those of
    the ten zoo rows run alone, a solved row those of the 48 solved rows run without zoo rows.
    Clearance works in groups of sixteen rows, the other four calls in tiles of four."""
    (so, T, C), _, _ = H.mixed()
    placed, order = _placed()
    alone = Z.take((so, T, C), list(range(10)))
    solved = Z.take((so, T, C), list(range(10, 58)))
    ob = H.cheb_boxes()

    def segs(batch, rows):
        return np.concatenate([np.arange(batch[0][r], batch[0][r + 1]) for r in rows])
    zpos, rpos = np.flatnonzero(order < 10), np.flatnonzero(order >= 10)
    assert len(zpos) == 17 and len(rpos) == 48 and list(order[rpos]) == list(range(10, 58))
    calls = (("bounds", lambda b: dev.bounds(*b), ()), ("thrust", lambda b: dev.thrust(*b, H.G), ()),
             ("rate", lambda b: dev.rate(*b, H.G), (1,)), ("corridor", lambda b: dev.corridor(*b, H.FACES), (2, 3)),
             ("clearance", lambda b: dev.clearance(*b, ob, 8.0), ()))
    for name, call, per_segment in calls:
        m, a, s = call(placed), call(alone), call(solved)
        for q in range(len(m)):
            if name == "clearance" and q == 3:
                continue  # tested: how many boxes the culling looked at depends on the batch's bounding boxes
            if q in per_segment:
                pairs = ((m[q][segs(placed, zpos)], a[q][segs(alone, order[zpos])]), (m[q][segs(placed, rpos)], s[q]))
            else:
                pairs = ((m[q][zpos], a[q][order[zpos]]), (m[q][rpos], s[q]))
            for got, want in pairs:
                if got.dtype == np.float64:
                    assert bit_equal(got, want), (name, q)
                else:
                    assert np.array_equal(got, want), (name, q)


def _check_neighbors_against_all_pairs(dev, b, t, r_min):
    """Neighbours of a batch against the device's own separation over all ordered pairs, reduced
    by neighbors_ref's rule: count, nbr and flags equal, d_min within 1e-9 L^2, t_min in the
    pair's window.  Asserted first: no pair lies on the threshold."""
    import neighbors_ref as NR
    import separation_ref as SR
    from trajectory_generator_ros2_amd import NEAR_NONE, SEP_CLOSE
    B = len(b[0]) - 1
    pairs = NR.ordered_pairs(B)
    sep, _ = dev.separation(*b, pairs, t)
    Lb = NR.pair_L(dev.bounds, *b, None)
    L2 = np.maximum(Lb[pairs[:, 0]], Lb[pairs[:, 1]]) ** 2
    assert not (np.abs(sep[:, 0] ** 2 - r_min ** 2) <= 1e-9 * L2).any()
    d, _, nbr_ref, count_ref = NR.reduce_rows(B, pairs, sep, r_min)
    near, nbr, count, tested, flags = dev.neighbors(*b, r_min, t)
    assert count_ref.sum() > 0 and np.array_equal(count, count_ref) and np.array_equal(nbr, nbr_ref)
    assert np.array_equal(flags, np.where(count_ref > 0, SEP_CLOSE, 0))
    assert ((count <= tested) & (tested <= B - 1)).all()
    trajs = SR.batch_trajs(*b, t)
    for i in range(B):
        if nbr_ref[i] == NEAR_NONE:
            assert near[i, 0] == np.inf and near[i, 1] == 0.0
            continue
        assert abs(near[i, 0] ** 2 - d[i] ** 2) <= 1e-9 * max(Lb[i], Lb[nbr[i]]) ** 2, i
        lo, hi = SR.window(trajs[i], trajs[nbr[i]])
        assert lo <= near[i, 1] <= hi, (i, near[i, 1], lo, hi)


def test_neighbours_of_the_placed_batch(dev):
    """The 65-row placed batch through the neighbour search (rows in groups of sixteen, the last
    alone): equal to the all-pairs reduction.  The repeated zoo rows start 2^-8 s apart per copy,
    so no two rows are the same vehicle."""
    _, t0, _ = H.mixed()
    placed, order = _placed()
    t = t0[order] + np.arange(65) * 2.0 ** -8
    _check_neighbors_against_all_pairs(dev, placed, t, 1.0)


def test_pairs_of_zoo_and_solved_rows(dev):
    """Zoo rows paired with solved rows: the explicit list holds what all-pairs holds for the same
    pair, to the bit, wherever the pair lands in a tile of sixteen; neighbours agree with the
    all-pairs reduction."""
    (so, T, C), t0, _ = H.mixed()
    rows = list(range(10)) + [10, 13, 22, 31, 40, 49, 57]  # the zoo and seven solved rows, every M class mixed
    b = Z.take((so, T, C), rows)
    t = t0[rows]
    B = len(rows)
    allp, fl_all = dev.separation(*b, None, t, r_min=1.0)
    ij = np.array([(i, j) for i in range(B) for j in range(i + 1, B)], np.int32)
    pick = np.array([n for n, (i, j) in enumerate(ij) if (i < 10) != (j < 10)])  # one zoo row, one solved row
    assert len(pick) == 70 and len(pick) % SEP_TILE != 0
    lst, fl_lst = dev.separation(*b, ij[pick], t, r_min=1.0)
    assert bit_equal(lst, allp[pick]) and np.array_equal(fl_lst, fl_all[pick])
    one, _ = dev.separation(*b, ij[pick[-1:]], t, r_min=1.0)  # alone in its tile
    assert bit_equal(one, allp[pick[-1:]])
    _check_neighbors_against_all_pairs(dev, b, t, 1.0)
