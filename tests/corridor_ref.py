"""Reference for the corridor containment (tgms_corridor_batch*), shared by
test_corridor_ref.py, test_corridor_host.py and test_gpu_corridor.py.  NumPy only, and
independent of the library's derivative ladder: per (segment, face) item the polynomial
q(u) = n . p(u) - d in u = t / T, its stationary points from np.roots of the projected derivative
(bounds_ref._candidates: real roots in [0, 1], polished in np.longdouble), and the values at
those and at the two ends evaluated from the three axis polynomials in np.longdouble.  No grid:
the candidates are what the contract names.

A reference is a dict of arrays:
    seg_m [S], seg_face [S], seg_L [S]   per segment: margin, winning face, its scale L_h
    m [B], seg [B], face [B], L [B]      per trajectory
with the tie rule of include/tgms.h (the lowest segment, then the lowest face index) and
-inf / -1 where there is no face; L_h = sum_a |n_a| max_t |p_a| + |d| over the trajectory."""
import numpy as np

from bounds_ref import LD, _candidates, _polyval
from extrema_ref import ORACLE_TOL

NONE = -1


def _axis_polys(c, T):
    """A segment's coefficients in u: [3][8] longdouble."""
    return np.asarray(c, dtype=LD) * LD(T) ** np.arange(8, dtype=LD)


def item(c, T, face):
    """(margin, u) of one segment against one face: the largest n . p(u) - d over u = 0, 1 and
    the stationary points, the first such u."""
    a = _axis_polys(c, T)
    n = np.asarray(face[:3], dtype=LD)
    q = n @ a
    q[0] -= LD(face[3])
    u = np.concatenate([np.array([0, 1], dtype=LD), _candidates(q)])
    v = sum(n[ax] * _polyval(a[ax], u) for ax in range(3)) - LD(face[3])
    k = int(np.argmax(v))
    return float(v[k]), float(u[k])


def spans(so, F, face_offsets):
    """Per segment the face span (first, end) of a call: CSR, or all F for None."""
    S = int(so[-1])
    if face_offsets is None:
        return np.zeros(S, np.int64), np.full(S, F, np.int64)
    fo = np.asarray(face_offsets, dtype=np.int64)
    return fo[:-1].copy(), fo[1:].copy()


def face_ok(face):
    return bool(np.isfinite(face).all() and np.any(np.asarray(face[:3]) != 0.0))


def records(so, T, C, faces, face_offsets=None):
    """The reference of a CSR batch with usable trajectories; unusable faces are left out."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    faces = np.asarray(faces, dtype=np.float64).reshape(-1, 4)
    B, S = len(so) - 1, int(so[-1])
    fb, fe = spans(so, len(faces), face_offsets)
    ref = dict(seg_m=np.full(S, -np.inf), seg_face=np.full(S, NONE, np.int64), seg_L=np.zeros(S),
               m=np.full(B, -np.inf), seg=np.full(B, NONE, np.int64), face=np.full(B, NONE, np.int64), L=np.zeros(B))
    grid = np.linspace(0.0, 1.0, 257).astype(LD)
    for b in range(B):
        s0, s1 = int(so[b]), int(so[b + 1])
        pmax = np.zeros(3)  # max_t |p_a| of the trajectory, from a grid and the knots: a scale only
        for s in range(s0, s1):
            a = _axis_polys(C[s], T[s])
            pmax = np.maximum(pmax, [float(np.abs(_polyval(a[ax], grid)).max()) for ax in range(3)])
        for s in range(s0, s1):
            for h in range(int(fb[s]), int(fe[s])):
                if not face_ok(faces[h]):
                    continue
                m, _ = item(C[s], T[s], faces[h])
                if m > ref["seg_m"][s]:  # ascending h: the lowest face wins a tie
                    ref["seg_m"][s], ref["seg_face"][s] = m, h
                    ref["seg_L"][s] = np.abs(faces[h, :3]) @ pmax + abs(faces[h, 3])
            if ref["seg_face"][s] != NONE and ref["seg_m"][s] > ref["m"][b]:  # ascending s
                ref["m"][b], ref["seg"][b], ref["face"][b] = ref["seg_m"][s], s - s0, ref["seg_face"][s]
                ref["L"][b] = ref["seg_L"][s]
    return ref


def face_scale(so, T, C, faces, b, h):
    """L_h of face h for trajectory b."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    grid = np.linspace(0.0, 1.0, 257).astype(LD)
    pmax = np.zeros(3)
    for s in range(int(so[b]), int(so[b + 1])):
        a = _axis_polys(C[s], T[s])
        pmax = np.maximum(pmax, [float(np.abs(_polyval(a[ax], grid)).max()) for ax in range(3)])
    f = np.asarray(faces, dtype=np.float64).reshape(-1, 4)[h]
    return float(np.abs(f[:3]) @ pmax + abs(f[3]))


def evaluate(so, T, C, b, t, face, seg=None):
    """n . p - d of trajectory b at its global time t, as a float.  seg (local index): evaluate on
    that segment, with t clamped into its span; None: the last segment whose closed interval
    [knot, knot + T] holds t.  Knots by the left-to-right float64 prefix sum the library uses."""
    T, C = np.asarray(T, dtype=np.float64).reshape(-1), np.asarray(C, dtype=np.float64).reshape(-1, 3, 8)
    s0, s1 = int(so[b]), int(so[b + 1])
    knot, at, k0 = 0.0, s0, 0.0
    for s in range(s0, s1):
        if (seg is None and t >= knot) or (seg is not None and s - s0 == seg):
            at, k0 = s, knot
        knot += T[s]
    u = np.clip((LD(t) - LD(k0)) / LD(T[at]), 0, 1)
    a = _axis_polys(C[at], T[at])
    n = np.asarray(face[:3], dtype=LD)
    return float(sum(n[ax] * _polyval(a[ax], np.array([u], dtype=LD))[0] for ax in range(3)) - LD(face[3]))


def check_contract(rec, ref, tol=ORACLE_TOL, seg_rec=None):
    """include/tgms.h: |m - m_true| <= tol L_h per trajectory (rec [B, 2]) and, given seg_rec
    [S, 2], per segment; -inf where the reference has no face."""
    rec = np.asarray(rec)
    assert rec.shape == (len(ref["m"]), 2) and not np.isnan(rec).any()
    for got, want, L, what in ((rec[:, 0], ref["m"], ref["L"], "trajectories"),) + (
            () if seg_rec is None else ((np.asarray(seg_rec)[:, 0], ref["seg_m"], ref["seg_L"], "segments"),)):
        none = np.isneginf(want)
        assert np.array_equal(np.isneginf(got), none)
        err = np.abs(got[~none] - want[~none]) / L[~none]
        if err.size:
            print("corridor vs reference, %s: %.3g x L_h" % (what, err.max()))
            assert (err <= tol).all(), (what, int(err.argmax()), float(err.max()))


def check_times(so, T, C, faces, rec, where, ref, seg_rec=None, seg_face=None, tol=ORACLE_TOL, face_base=None):
    """Every stored time lies in [0, D_b] (per segment: in the segment's span, clamped to D_b),
    and n . p - d of the reported face evaluated there reproduces the stored margin within the
    contract.  Times are not compared with the reference's: they are unspecified among ties.
    face_base [S]: added to a reported face to index `faces` (shared mode reports 0..F-1)."""
    from extrema_ref import durations
    faces = np.asarray(faces, dtype=np.float64).reshape(-1, 4)
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    D = durations(so, T)
    rec, where = np.asarray(rec), np.asarray(where)
    for b in range(len(so) - 1):
        if where[b, 1] == NONE:
            assert rec[b, 1] == 0.0 and where[b, 0] == NONE and np.isneginf(rec[b, 0])
            continue
        assert 0.0 <= rec[b, 1] <= D[b], (b, rec[b, 1], D[b])
        f = faces[where[b, 1] + (0 if face_base is None else face_base[int(so[b]) + where[b, 0]])]
        L = face_scale(so, T, C, f[None], b, 0)
        assert abs(evaluate(so, T, C, b, rec[b, 1], f, seg=int(where[b, 0])) - rec[b, 0]) <= tol * L, (b, "m_max")
    if seg_rec is None:
        return
    seg_rec, seg_face = np.asarray(seg_rec), np.asarray(seg_face)
    for b in range(len(so) - 1):
        knot = 0.0
        for s in range(int(so[b]), int(so[b + 1])):
            if seg_face[s] == NONE:
                assert seg_rec[s, 1] == 0.0 and np.isneginf(seg_rec[s, 0])
            else:
                lo, hi = knot, min(knot + T[s], D[b])
                assert lo <= seg_rec[s, 1] <= hi, (s, seg_rec[s, 1], lo, hi)
                f = faces[seg_face[s] + (0 if face_base is None else face_base[s])]
                L = face_scale(so, T, C, f[None], b, 0)
                got = evaluate(so, T, C, b, seg_rec[s, 1], f, seg=s - int(so[b]))
                assert abs(got - seg_rec[s, 0]) <= tol * L, (s, "m_s")
            knot += T[s]
