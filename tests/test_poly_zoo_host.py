"""CPU: the continuous-analysis calls of the host backend on the constructed polynomials of
poly_zoo.py (full ladder depth, extrema on knots, deficient degree, a touch without a sign
change) and under a planner's transforms (a large translation, time rescaled by 2^k, start times
on a wall clock).  Exact answers where poly_zoo has them, else the call's own *_ref.py reference,
which is first held against poly_zoo's long-double grid to 1e-10 on the very case; the tolerance
forms are those of include/tgms.h, 1e-9 each.  Then the metamorphic relations, which need no
reference.  The check_* functions take a backend (anything with a Solver's numpy methods), so
test_gpu_poly_zoo.py runs them on the device entry points."""
import functools

import numpy as np
import pytest

import bounds_ref as R
import clearance_ref as CL
import corridor_ref as CR
import neighbors_ref as NR
import poly_zoo as Z
import rate_ref as RR
import separation_ref as SR
import thrust_ref as TR
from extrema_ref import bit_equal

TOL = 1e-9
G = Z.G
# rows of the zoo batch
CHEB, DEF4, LIN, BALL, CUBIC, HOLD, KP2, KP3, TOUCH, PARTNER = range(10)
ZOO_T0 = np.array([0.5, 1.25, 0.0, 2.0, 0.75, 3.5, 1.0, 0.25, 0.5, 0.5])  # multiples of 2^-8; the touch pair together
ZOO_PAIRS = np.array([[TOUCH, PARTNER], [CHEB, KP2], [DEF4, KP3], [LIN, TOUCH], [KP2, KP3], [BALL, CHEB], [CUBIC, HOLD],
                      [KP3, PARTNER], [PARTNER, TOUCH]], np.int32)
FACES = np.array([[1.0, 0.0, 0.0, 2.0], [-1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 1.5], [0.5, 0.5, -0.25, 3.0]])
X_FACE = np.array([[1.0, 0.0, 0.0, 1.0]])  # x <= 1: the margin of a knot_peak row is pmax_x - 1 exactly


@functools.lru_cache(maxsize=None)
def zoo():
    """The ten rows in one CSR batch with their exact answers: (so, T, C), {member: exact}."""
    parts = dict(cheb=Z.cheb(), deficient=Z.deficient(), kp2=Z.knot_peak(2), kp3=Z.knot_peak(3), touch=Z.touch())
    batch = Z.concat(*[p[:3] for p in parts.values()])
    for a in batch:
        a.setflags(write=False)
    assert len(batch[0]) - 1 == 10
    return batch, {k: p[3] for k, p in parts.items()}


def cheb_boxes():
    """The three boxes placed from cheb's exact x maximum X, wide enough in y and z that the
    distance is the x gap alone: one the trajectory enters by 2^-10, one it misses by 2^-10, one
    plate at X itself; then a point and a box near the other rows."""
    X = zoo()[1]["cheb"]["pmax"][0]
    wide = lambda lo, hi: [lo, -4.0, 0.0, hi, 4.0, 4.0]  # noqa: E731
    return np.array([wide(X - 2.0 ** -10, X + 1.0), wide(X + 2.0 ** -10, X + 1.0), wide(X, X),
                     [1.0, 0.5, 1.5, 1.0, 0.5, 1.5], [1.5, 0.25, 3.25, 1.75, 0.75, 3.5]])


def _cap(what, got, want, unit):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / unit
    err = np.where(np.asarray(got) == np.asarray(want), 0.0, err)
    print("reference cap, %s: reference vs 65,537-point grid %.3g" % (what, np.max(err)))
    assert (err <= Z.CAP).all(), (what, np.argmax(err), np.max(err))


def build_reference(caps):
    """Every reference of the untransformed zoo batch with the exact answers laid over it.  caps:
    each *_ref.py value is first held against poly_zoo's long-double grid to 1e-10 (the costly
    part: test_references_agree_with_the_grid does it once, on the CPU)."""
    (so, T, C), ex = zoo()
    B, S = len(so) - 1, int(so[-1])
    ref = {}
    # bounds
    b = R.records(so, T, C)
    pm = np.abs(b[:, 0:6]).max(axis=1)
    if caps:
        gb = Z.grid_bounds(so, T, C)
        _cap("bounds extents", b[:, 0:6], gb[:, 0:6], pm[:, None])
        _cap("bounds peaks", b[:, 6:9], gb[:, 6:9], np.where(b[:, 6:9] == 0, 1.0, b[:, 6:9]))
    b[CHEB, 0:3], b[CHEB, 3:6] = ex["cheb"]["pmin"], ex["cheb"]["pmax"]
    b[DEF4:HOLD + 1] = ex["deficient"]["ext"]
    b[[KP2, KP3], 3] = ex["kp2"]["pmax_x"]
    b[[TOUCH, PARTNER], 0], b[[TOUCH, PARTNER], 3] = ex["touch"]["pmin_x"], ex["touch"]["pmax_x"]
    ref["bounds"] = b
    # thrust: rows with F == 0 (the free-falling arc alone) have no ratio to form
    live = np.array([r for r in range(B) if r != BALL])
    th = np.zeros((B, 3))
    th[live] = TR.records(*Z.take((so, T, C), live), g=G)
    if caps:
        gt = np.zeros((B, 3))
        gt[live] = Z.grid_thrust(*Z.take((so, T, C), live), g=G)
        F = th[live, 1]
        _cap("thrust squares", th[live, 0:2] ** 2, gt[live, 0:2] ** 2, (F * F)[:, None])
        pos = live[th[live, 0] > 1e-3]
        _cap("tilt", th[pos, 2], gt[pos, 2], th[pos, 1] / th[pos, 0])
    th[DEF4:HOLD + 1, 0], th[DEF4:HOLD + 1, 1] = ex["deficient"]["f_min"], ex["deficient"]["f_max"]
    for r, k in ((KP2, "kp2"), (KP3, "kp3")):
        th[r, 1], th[r, 2] = ex[k]["f_max"], ex[k]["tilt_max"]
    ref["thrust"] = th
    # rate: per segment; the scale F J / m^2 where m > 0
    wa, wb, _ = RR.segments(so, T, C, G)
    seg = np.sqrt(np.maximum(wa, wb)).astype(np.float64)
    m_pos = th[:, 0] > 0
    scale = np.where(m_pos, th[:, 1] * b[:, 8] / np.where(m_pos, th[:, 0], 1.0) ** 2, np.inf)
    seg_scale = np.repeat(scale, np.diff(so))
    ok = np.isfinite(seg_scale) & (seg_scale > 0)
    if caps:
        _cap("rate", seg[ok], Z.grid_rate(so, T, C, G)[ok], seg_scale[ok])
    ref["rate"] = dict(seg=seg, scale=scale, omega=np.array([seg[so[r]:so[r + 1]].max() for r in range(B)]))
    # corridor: every (segment, face) item against the grid, then the records
    cr = CR.records(so, T, C, FACES)
    for s in range(S if caps else 0):
        items = [CR.item(C[s], T[s], f)[0] for f in FACES]
        grid = [Z.grid_corridor(T, C, s, f) for f in FACES]
        assert max(abs(i - g) for i, g in zip(items, grid)) <= Z.CAP * cr["seg_L"][s], s
    ref["corridor"] = cr
    # separation
    trajs = SR.batch_trajs(so, T, C, ZOO_T0)
    refs = SR.references(trajs, ZOO_PAIRS)
    for n, ((i, j), (d2, L, dist)) in enumerate(zip(ZOO_PAIRS, refs)):
        if {i, j} == {TOUCH, PARTNER}:
            refs[n] = (0.0, L, dist)  # exact: one touch at the quadruple root; np.roots degrades there
        elif caps:
            assert abs(d2 - Z.grid_pair(trajs[i], trajs[j], dist)) <= Z.CAP * L * L, (i, j)
    ref["separation"] = (trajs, refs)
    # clearance
    ob = cheb_boxes()
    tr0 = SR.batch_trajs(so, T, C)
    d2, L = np.empty((B, len(ob))), np.empty((B, len(ob)))
    for r in range(B):
        for k in range(len(ob)):
            x, y = CL.pair_ref(tr0[r], ob[k], [None])
            d2[r, k], L[r, k] = x[0], y[0]
            assert not caps or abs(d2[r, k] - Z.grid_clearance(tr0[r], ob[k])) <= Z.CAP * L[r, k] ** 2, (r, k)
    d2[CHEB, 0:3] = [0.0, 2.0 ** -20, 0.0]  # exact: entered, missed by 2^-10, touched
    ref["clearance"] = (tr0, ob, d2, L)
    return ref


@functools.lru_cache(maxsize=None)
def zoo_reference():
    """build_reference without the grid, computed once per session and left unchanged: what the
    contract tests of both backends use."""
    return build_reference(False)


def test_references_agree_with_the_grid():
    """The cap of every *_ref.py reference used on the zoo: within 1e-10, in the contract's own
    unit, of the 65,537-point long-double grid of the same quantity."""
    build_reference(True)


# ---- the contract checks (backend-agnostic) ----

def check_bounds(be, batch, ref, what):
    ext, fl = be.bounds(*batch)
    assert not fl.any() and np.isfinite(ext).all()
    pmax = np.abs(ref[:, 0:6]).max(axis=1)
    err_p = np.abs(ext[:, 0:6] - ref[:, 0:6]).max(axis=1) / pmax
    zero = ref[:, 6:9] == 0.0
    assert (ext[:, 6:9][zero] == 0.0).all()  # an identically zero derivative: exactly 0.0
    err_k = np.where(zero, 0.0, np.abs(ext[:, 6:9] - ref[:, 6:9]) / np.where(zero, 1.0, ref[:, 6:9])).max(axis=1)
    print("%s bounds: extents %.3g x max|p|, peaks %.3g relative" % (what, err_p.max(), err_k.max()))
    assert (err_p <= TOL).all(), (int(err_p.argmax()), float(err_p.max()))
    assert (err_k <= TOL).all(), (int(err_k.argmax()), float(err_k.max()))
    return ext


def check_thrust(be, batch, ref, g, what, knot_times=None):
    from trajectory_generator_ros2_amd import THRUST_LOW, ThrustLimits
    rec, fl = be.thrust(*batch, g)
    assert not fl.any() and np.isfinite(rec).all()
    live = ref[:, 1] > 0
    e_lo, e_hi, e_tilt = TR.contract_errors(rec[live], ref[live])
    print("%s thrust: f_min^2 %.3g F^2, f_max^2 %.3g F^2, tilt %.3g F / f_min rad" % (what, e_lo.max(), e_hi.max(),
                                                                                      e_tilt.max()))
    assert (e_lo <= TOL).all() and (e_hi <= TOL).all() and (e_tilt <= TOL).all(), (e_lo, e_hi, e_tilt)
    # the arc alone: the true thrust is 0 throughout, F == 0 and the ratio cannot be formed.  What the
    # evaluation leaves is the rounding of 1 / T^2 (two roundings of 1 / T and a product, < 2 ulp)
    # and of one fma against g: below 4 ulp of g.
    assert rec[BALL, 2] <= 4.0 * 2.0 ** -52 * g, rec[BALL]
    assert rec[DEF4, 0] ** 2 <= TOL * ref[DEF4, 1] ** 2  # the arc inside the M = 4 row: f_min^2 <= 1e-9 F^2
    assert (rec[[LIN, HOLD], 0] == g).all() and (rec[[LIN, HOLD], 2] == g).all() and (rec[[LIN, HOLD], 4] == 0.0).all()
    _, fl = be.thrust(*batch, g, ThrustLimits(f_min=1e-12 * g))
    assert (fl[[DEF4, BALL]] == THRUST_LOW).all() and not fl[[r for r in range(len(fl)) if r not in (DEF4, BALL)]].any()
    if knot_times is not None:  # the extremes that fall on a knot carry the knot's prefix sum
        for r, t in knot_times:
            assert rec[r, 3] == t and rec[r, 5] == t, (r, rec[r], t)
    return rec


def check_rate(be, batch, ref, g, what, knot_times=None):
    """Where F J / m^2 is 0 (no jerk) the value must be the reference's exactly; where m == 0 there
    is no claim."""
    so = batch[0]
    rec, seg, fl = be.rate(*batch, g)
    assert not fl.any() and np.isfinite(rec).all() and np.isfinite(seg).all()
    has = np.isfinite(ref["scale"])
    unit = np.where(ref["scale"] > 0, ref["scale"], 1.0)
    e = np.abs(rec[has, 0] - ref["omega"][has]) / unit[has]
    hs = np.repeat(has, np.diff(so))
    e_seg = np.abs(seg[hs, 0] - ref["seg"][hs]) / np.repeat(unit, np.diff(so))[hs]
    print("%s rate: omega_max %.3g, segment rows %.3g x F J / m^2" % (what, e.max(), e_seg.max()))
    assert (e <= TOL).all() and (e_seg <= TOL).all(), (e, e_seg)
    low = zoo()[1]["deficient"]["low_segments"] + so[DEF4]
    assert (seg[low] == 0.0).all()  # p''' == 0: exactly 0.0 whatever the denominator
    assert (rec[[LIN, BALL, HOLD], 0] == 0.0).all()
    for r in range(len(so) - 1):
        assert seg[so[r]:so[r + 1], 0].max() == rec[r, 0]
    # the M = 4 row's cubic is the M = 1 cubic row: the same coefficients, the same bits
    assert bit_equal(seg[so[DEF4] + 2, 0], seg[so[CUBIC], 0])
    if knot_times is not None:
        for r, t in knot_times:
            assert rec[r, 1] == t, (r, rec[r], t)
    return rec, seg


def check_corridor(be, batch, ref, faces, what, x_face=None, x_want=None):
    rec, where, seg_rec, seg_face, fl = be.corridor(*batch, faces)
    CR.check_contract(rec, ref, seg_rec=seg_rec)
    err = np.abs(rec[:, 0] - ref["m"]) / ref["L"]
    print("%s corridor: %.3g x L_h" % (what, err.max()))
    CR.check_times(*batch, faces, rec, where, ref, seg_rec, seg_face)
    if x_face is not None:
        # the maximum sits on a knot: two segments hold it, the lowest is reported (include/tgms.h)
        rec1, where1, _, _, _ = be.corridor(*batch, x_face)
        ex = zoo()[1]
        for r, k in ((KP2, "kp2"), (KP3, "kp3")):
            assert abs(rec1[r, 0] - x_want) <= TOL * (abs(x_want) + 2.0 * abs(x_face[0, 3])), (r, rec1[r])
            assert list(where1[r]) == [ex[k]["seg"], 0], (r, where1[r])
    return rec, seg_rec


def pair_references(batch, t0, L_rows):
    """(trajs, refs) of ZOO_PAIRS for a transformed zoo batch: d_min^2 is the untransformed
    reference's (a common translation, a time rescale and a clock leave it unchanged), L the larger
    of the two rows' largest coordinate magnitudes, dist the transformed trajectories' own."""
    trajs = SR.batch_trajs(*batch, t0)
    base = zoo_reference()["separation"][1]

    def dist_of(ti, tj):
        return lambda t: np.sqrt((((ti.pos(t) - tj.pos(t))) ** 2).sum(axis=1))
    return trajs, [(base[n][0], float(max(L_rows[i], L_rows[j])), dist_of(trajs[i], trajs[j]))
                   for n, (i, j) in enumerate(ZOO_PAIRS)]


def check_separation(be, batch, t0, trajs, refs, what):
    from trajectory_generator_ros2_amd import SEP_CLOSE
    sep, fl = be.separation(*batch, ZOO_PAIRS, t0)
    e1, e3 = SR.check_contract(sep, trajs, ZOO_PAIRS, refs, what=what + " separation")
    L = refs[0][1]
    assert sep[0, 0] ** 2 <= TOL * L * L and sep[8, 0] ** 2 <= TOL * L * L  # the touch, either order
    _, fl = be.separation(*batch, ZOO_PAIRS, t0, r_min=2.0 * np.sqrt(TOL) * L)
    assert fl[0] == SEP_CLOSE and fl[8] == SEP_CLOSE
    return sep


def check_neighbors(be, batch, t0, what, L_gap=None):
    """The reference is the backend's own separation call over all ordered pairs, reduced in NumPy
    (neighbors_ref's rule); that call is pinned by check_separation.  L_gap [B]: the rows' L in
    which no pair may lie on the threshold; None takes the batch's own.  The translated batch
    passes the untranslated rows' L: in its own (2^15) the unit 1e-9 L^2 is 1.07 m^2 and every
    pair lies on every threshold, while what the translation does to d_min^2 is the cancellation
    of the shift in fp64, 2^15 x 2^-52 x d = 7e-12 d, far inside 1e-9 of the untranslated L^2."""
    so, T, C = batch
    B = len(so) - 1
    pairs = NR.ordered_pairs(B)
    sep, _ = be.separation(so, T, C, pairs, t0)
    Lb = NR.pair_L(be.bounds, so, T, C, None)
    Lg = Lb if L_gap is None else np.asarray(L_gap)
    L2 = np.maximum(Lg[pairs[:, 0]], Lg[pairs[:, 1]]) ** 2
    r_min = 0.4375
    assert not (np.abs(sep[:, 0] ** 2 - r_min ** 2) <= TOL * L2).any()  # no pair on the threshold
    d, t, nbr_ref, count_ref = NR.reduce_rows(B, pairs, sep, r_min)
    near, nbr, count, tested, flags = be.neighbors(so, T, C, r_min, t0)
    assert count_ref.sum() > 0 and np.array_equal(count, count_ref), (count, count_ref)
    assert np.array_equal(nbr, nbr_ref), (nbr, nbr_ref)
    hit = count_ref > 0
    e = np.abs(near[hit, 0] ** 2 - d[hit] ** 2) / Lb[hit] ** 2
    print("%s neighbours: d_min^2 off the all-pairs reduction by %.3g x L^2, %d within r_min" % (what, e.max(), count.sum()))
    assert (e <= TOL).all()
    assert nbr[TOUCH] == PARTNER and nbr[PARTNER] == TOUCH
    assert (near[[TOUCH, PARTNER], 0] ** 2 <= TOL * Lb[[TOUCH, PARTNER]] ** 2).all()
    return near, nbr, count, flags


def check_clearance(be, batch, tr0, ob, d2_ref, L, what, threshold=True):
    from trajectory_generator_ros2_amd import NEAR_NONE
    B, K = d2_ref.shape
    L2 = L * L
    worst = 0.0
    for k in range(K):  # one box at a time, every row against it: no culling by a nearer box
        near, obs, count, tested, flags = be.clearance(*batch, ob[k:k + 1], 8.0)
        assert (count == 1).all() and (obs == 0).all()
        e = np.abs(near[:, 0] ** 2 - d2_ref[:, k]) / L2[:, k]
        worst = max(worst, e.max())
        assert (e <= TOL).all(), (k, int(e.argmax()), float(e.max()))
    print("%s clearance: d_min^2 off by %.3g x L^2" % (what, worst))
    if not threshold:  # translated by 2^15: 1e-9 L^2 is 1.07 m^2, the contract cannot tell 2^-10 from 0
        return worst
    # the three boxes at cheb's maximum under a threshold between the miss and the entry
    r_min = 2.0 ** -11
    assert not (np.abs(d2_ref - r_min ** 2) <= TOL * L2).any()
    near, obs, count, tested, flags = be.clearance(*batch, ob, r_min)
    assert np.array_equal(count, (np.sqrt(d2_ref) < r_min).sum(axis=1)), count
    assert count[CHEB] == 2 and obs[CHEB] in (0, 2) and near[CHEB, 0] ** 2 <= TOL * L2[CHEB, 0]
    near1, _, count1, _, _ = be.clearance(*batch, ob[1:2], r_min)
    assert count1[CHEB] == 0 and near1[CHEB, 0] == np.inf  # missed by 2^-10: outside 2^-11
    assert (obs[count == 0] == NEAR_NONE).all()
    return worst


# ---- transforms of the references (exact: powers of two and one translation) ----

def transformed(kind, k):
    """(batch, g, references, faces, x_face, boxes) of the zoo under one transform: the true values
    follow exactly from the untransformed ones."""
    (so, T, C), ex = zoo()
    ref = zoo_reference()
    b, th, ra, cr = ref["bounds"].copy(), ref["thrust"].copy(), dict(ref["rate"]), dict(ref["corridor"])
    tr0, ob, d2, L = ref["clearance"]
    faces, x_face, g = FACES.copy(), X_FACE.copy(), G
    if kind == "translate":
        d = np.asarray(Z.SHIFT)
        C = Z.translate(C, d)
        b[:, 0:3] += d
        b[:, 3:6] += d
        faces[:, 3] += faces[:, 0:3] @ d  # exact: dyadic normals, a dyadic shift
        x_face[:, 3] += x_face[:, 0:3] @ d
        ob = ob + np.tile(d, 2)
        pmax = np.maximum(np.abs(b[:, 0:3]), np.abs(b[:, 3:6]))
        for key, rows in (("L", np.arange(len(so) - 1)), ("seg_L", np.repeat(np.arange(len(so) - 1), np.diff(so)))):
            fc = faces[cr["face" if key == "L" else "seg_face"]]
            cr[key] = (np.abs(fc[:, 0:3]) * pmax[rows]).sum(axis=1) + np.abs(fc[:, 3])
        L = np.maximum(L, np.abs(ob).max())  # the translated scene's largest coordinate: a lower bound of it
        tr0 = SR.batch_trajs(so, T, C)
    elif kind == "rescale":
        T, C = Z.rescale_time(T, C, k)
        g = np.ldexp(G, -2 * k)
        b[:, 6:9] = np.ldexp(b[:, 6:9], -k * np.arange(1, 4))
        th[:, 0:2] = np.ldexp(th[:, 0:2], -2 * k)
        ra = {key: np.ldexp(v, -k) for key, v in ra.items()}
        tr0 = SR.batch_trajs(so, T, C)
    return (so, T, C), g, dict(bounds=b, thrust=th, rate=ra, corridor=cr, clearance=(tr0, ob, d2, L)), faces, x_face


VARIANTS = [("identity", 0), ("translate", 0)] + [("rescale", k) for k in Z.RESCALES]


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.build import LIB_TGMS, build_tgms
    from trajectory_generator_ros2_amd.solver import Solver
    import os
    if not os.path.exists(LIB_TGMS):
        build_tgms()
    s = Solver(host=True)
    yield s
    s.close()


def run_variant(be, kind, k, what):
    """All seven calls on the zoo under one transform, against the transformed references.  The
    start times scale with the time rescale (exactly: a power of two), so d_min is unchanged and
    every knot and t_min scales by 2^k."""
    batch, g, ref, faces, x_face = transformed(kind, k)
    ex = zoo()[1]
    scale_t = 2.0 ** k if kind == "rescale" else 1.0
    knots = [(KP2, ex["kp2"]["t_knot"] * scale_t), (KP3, ex["kp3"]["t_knot"] * scale_t)]
    label = "%s %s%s" % (what, kind, "" if kind != "rescale" else " 2^%d" % k)
    check_bounds(be, batch, ref["bounds"], label)
    check_thrust(be, batch, ref["thrust"], g, label, knots)
    check_rate(be, batch, ref["rate"], g, label, knots)
    check_corridor(be, batch, ref["corridor"], faces, label, x_face, ex["kp2"]["pmax_x"] - 1.0)
    check_clearance(be, batch, *ref["clearance"], label, threshold=kind != "translate")
    t0 = np.ldexp(ZOO_T0, k) if kind == "rescale" else ZOO_T0
    L_rows = np.abs(ref["bounds"][:, 0:6]).max(axis=1)
    trajs, refs = pair_references(batch, t0, L_rows)
    check_separation(be, batch, t0, trajs, refs, label)
    check_neighbors(be, batch, t0, label, np.abs(zoo_reference()["bounds"][:, 0:6]).max(axis=1))


@pytest.mark.parametrize("kind,k", VARIANTS)
def test_zoo_meets_the_contract(host, kind, k):
    run_variant(host, kind, k, "host")


def check_rate_on_cheb(be, what):
    (so, T, C), _ = zoo()
    ref = zoo_reference()["rate"]
    rec, _, _ = be.rate(so, T, C, G)
    e = abs(rec[CHEB, 0] - ref["omega"][CHEB]) / ref["scale"][CHEB]
    print("%s rate on cheb: omega_max %.17g, reference %.17g, off by %.3g x F J / m^2" % (what, rec[CHEB, 0],
                                                                                       ref["omega"][CHEB], e))
    assert e <= TOL, (rec[CHEB], ref["omega"][CHEB], e)


def test_rate_on_cheb_meets_the_contract(host):
    """The row that exposed the rate call's root location: the stationary points are the roots of G
    = N' D - 2 N D' (degree 25) from fp64 coefficients in the monomial basis, which reach 3.3e34 on
    this row while |G| within 0.01 of the root is below 1e16.  Horner's rounding moved the located
    root by 1.1e-3 in u and omega_max came out as 41.98857 against 42.08016: 1.41e-6 F J / m^2
    against the 1e-9 of include/tgms.h.  With the slots polished on omega^2 itself
    (csrc/tgms_rate_core.h, polish) the row is 5.6e-18 off."""
    check_rate_on_cheb(host, "host")


# ---- metamorphic relations: the zoo and the solved 48-row batch, no reference ----

@functools.lru_cache(maxsize=None)
def mixed():
    """The zoo's ten rows followed by bounds_ref.ragged48 with times on the 2^-8 lattice, solved by
    the host backend: (so, T, C), start times, pairs."""
    from trajectory_generator_ros2_amd.solver import Solver
    so, W, T = Z.ragged48_times()
    with Solver(host=True) as s:
        C, _, worst = s.solve(so, W, T)
    assert worst == 0
    batch = Z.concat(zoo()[0], (so, T, C))
    t0 = np.concatenate([ZOO_T0, Z.start_times(48)])
    rng = np.random.default_rng(58)
    B = len(batch[0]) - 1
    pairs = np.concatenate([ZOO_PAIRS, np.stack([rng.permutation(B), rng.permutation(B)], axis=1)]).astype(np.int32)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    for a in batch + (t0, pairs):
        a.setflags(write=False)
    return batch, t0, pairs


def check_translation(be):
    (so, T, C), t0, pairs = mixed()
    d = np.asarray(Z.SHIFT)
    C2 = Z.translate(C, d)
    e0, _ = be.bounds(so, T, C)
    e1, _ = be.bounds(so, T, C2)
    assert bit_equal(e1[:, 6:10], e0[:, 6:10])
    pm = np.maximum(np.abs(e1[:, 0:3]), np.abs(e1[:, 3:6])).max(axis=1)
    err = np.abs(e1[:, 0:6] - (e0[:, 0:6] + np.tile(d, 2))).max(axis=1) / pm
    print("translation: extents off the untranslated ones + d by %.3g x max|p|" % err.max())
    assert (err <= TOL).all()
    assert bit_equal(be.thrust(so, T, C2, G)[0], be.thrust(so, T, C, G)[0])
    r0, r1 = be.rate(so, T, C, G), be.rate(so, T, C2, G)
    assert bit_equal(r1[0], r0[0]) and bit_equal(r1[1], r0[1])
    s0, _ = be.separation(so, T, C, pairs, t0)
    s1, _ = be.separation(so, T, C2, pairs, t0)
    L0 = np.maximum(np.abs(e0[:, 0:3]), np.abs(e0[:, 3:6])).max(axis=1)
    L2 = np.maximum(L0[pairs[:, 0]], L0[pairs[:, 1]]) ** 2
    err = np.abs(s1[:, 0] ** 2 - s0[:, 0] ** 2) / L2
    print("translation: d_min^2 of pairs moved together off by %.3g x L^2 (L untranslated)" % err.max())
    assert (err <= TOL).all()


def check_rescale(be, k):
    (so, T, C), _, _ = mixed()
    T2, C2 = Z.rescale_time(T, C, k)
    g2 = float(np.ldexp(G, -2 * k))
    e0, _ = be.bounds(so, T, C)
    e1, _ = be.bounds(so, T2, C2)
    assert bit_equal(e1[:, 0:6], e0[:, 0:6])
    assert bit_equal(np.ldexp(e1[:, 6:9], k * np.arange(1, 4)), e0[:, 6:9])
    assert bit_equal(np.ldexp(e1[:, 9], -k), e0[:, 9])
    t0, t1 = be.thrust(so, T, C, G)[0], be.thrust(so, T2, C2, g2)[0]
    assert bit_equal(np.ldexp(t1[:, [0, 2]], 2 * k), t0[:, [0, 2]]) and bit_equal(t1[:, 4], t0[:, 4])
    assert bit_equal(np.ldexp(t1[:, [1, 3, 5]], -k), t0[:, [1, 3, 5]])
    r0, r1 = be.rate(so, T, C, G), be.rate(so, T2, C2, g2)
    for a, b in zip(r0[:2], r1[:2]):
        assert bit_equal(np.ldexp(b[:, 0], k), a[:, 0]) and bit_equal(np.ldexp(b[:, 1], -k), a[:, 1])
    c0, c1 = be.corridor(so, T, C, FACES), be.corridor(so, T2, C2, FACES)
    assert bit_equal(c1[0][:, 0], c0[0][:, 0]) and bit_equal(c1[2][:, 0], c0[2][:, 0])
    assert np.array_equal(c1[1], c0[1]) and np.array_equal(c1[3], c0[3])


def check_clock(be, s):
    (so, T, C), t0, pairs = mixed()
    t1 = Z.shift_clock(t0, s)
    a, fa = be.separation(so, T, C, pairs, t0, r_min=1.0)
    b, fb = be.separation(so, T, C, pairs, t1, r_min=1.0)
    assert bit_equal(b[:, 0], a[:, 0]) and np.array_equal(fa, fb) and fa.any() and not fa.all()
    ulp = np.spacing(s)
    dt = np.abs(b[:, 1] - s - a[:, 1])
    print("clock + %g: t_min off by %.3g ulp(s)" % (s, dt.max() / ulp))
    assert (dt <= 2.0 * ulp).all()
    na, nb = be.neighbors(so, T, C, 1.0, t0), be.neighbors(so, T, C, 1.0, t1)
    assert bit_equal(nb[0][:, 0], na[0][:, 0]) and na[2].sum() > 0
    for q in (1, 2, 4):  # nbr, count, flags
        assert np.array_equal(na[q], nb[q])
    hit = na[2] > 0
    assert (np.abs(nb[0][hit, 1] - s - na[0][hit, 1]) <= 2.0 * ulp).all()


def test_translation(host):
    check_translation(host)


@pytest.mark.parametrize("k", Z.RESCALES)
def test_time_rescale(host, k):
    check_rescale(host, k)


@pytest.mark.parametrize("s", Z.CLOCKS)
def test_clock_shift(host, s):
    check_clock(host, s)
