"""Reference for the corridor split (tgms_corridor_split_batch*), shared by test_split_ref.py,
test_split_host.py and test_gpu_split.py.  NumPy only: the decisions exactly as include/tgms.h
states them (fp64, every operation rounded on its own, which is what numpy scalars do), Horner in
np.longdouble for the inserted waypoint, offsets by np.cumsum.  It takes the seg_rec / seg_face
arrays of a corridor call as the library does, so every integer and every time must equal the
library's to the bit.

split(...) returns a dict:
    so [B+1], W [S'+B,3], T [S'], faces [F',4], fo [S'+1] (None in shared mode), parent [S'],
    flags [B], inserted [S'] bool (the segment's END waypoint was inserted: it is a left child),
    L [S'] (max |p| over the parent segment: the scale of the waypoint tolerance)."""
import numpy as np

from bounds_ref import LD, _polyval

PULL, CHORD = 0, 1
DONE, FULL, AT_END, NONFINITE = 1, 2, 4, 16
MAX_SEGMENTS, MAX_FACES = 16, 256
END_FRAC = 2.0 ** -20


def span_ok(a, b, F):
    return a >= 0 and b >= a and b <= F and b - a <= MAX_FACES


def local_time(t_s, knot, T):
    return np.float64(min(max(np.float64(t_s) - np.float64(knot), np.float64(0.0)), np.float64(T)))


def split_times(t_loc, T, min_frac):
    T = np.float64(T)
    lo = np.float64(min_frac) * T
    hi = T - lo
    t_left = np.float64(min(max(np.float64(t_loc), lo), hi))
    return t_left, T - t_left


def pull_point(c, t_left, face, r):
    """p(t_left) in longdouble, pulled back along -n to margin -r where it is above it."""
    n, d = np.asarray(face[:3], dtype=LD), LD(face[3])
    x = np.array([_polyval(np.asarray(c[ax], dtype=LD), LD(t_left)) for ax in range(3)], dtype=LD).reshape(3)
    q = n @ x - d
    if q > -LD(r):
        x = x - ((q + LD(r)) / (n @ n)) * n
    return x.astype(np.float64)


def chord_point(w0, w1, t_left, T):
    w0, w1 = np.asarray(w0, dtype=LD), np.asarray(w1, dtype=LD)
    return (w0 + (LD(t_left) / LD(T)) * (w1 - w0)).astype(np.float64)


def plan_row(T, m, t_s, face, fb, fe, F, r, bad):
    """(mask as a bool list, flags) of one trajectory."""
    M = len(T)
    ok = [span_ok(int(fb[i]), int(fe[i]), F) for i in range(M)]
    bad = bad or not all(ok) or bool(np.isnan(m).any() or np.isnan(t_s).any())
    want = [bool(m[i] > -r) for i in range(M)] if not bad else [False] * M
    for i in range(M):
        if want[i] and not (fb[i] <= face[i] < fe[i]):
            bad = True
    if bad:
        return [False] * M, NONFINITE
    flags, knot, cand = 0, np.float64(0.0), []
    for i in range(M):
        t_loc = local_time(t_s[i], knot, T[i])
        end = bool(t_loc <= np.float64(END_FRAC) * T[i] or t_loc >= np.float64(1.0 - END_FRAC) * T[i])
        if want[i] and end:
            flags |= AT_END
        elif want[i]:
            cand.append(i)
        knot = knot + np.float64(T[i])
    order = sorted(cand, key=lambda i: (-m[i], i))
    room = MAX_SEGMENTS - M
    mask = [False] * M
    for i in order[:room]:
        mask[i] = True
    if len(order) > room:
        flags |= FULL
    if any(mask):
        flags |= DONE
    return mask, flags


def split(so, W, T, C, faces, fo, seg_rec, seg_face, r, mode, min_frac):
    so = np.asarray(so, np.int64)
    W = np.asarray(W, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1)
    C = np.asarray(C, np.float64).reshape(-1, 3, 8)
    faces = np.asarray(faces, np.float64).reshape(-1, 4)
    seg_rec = np.asarray(seg_rec, np.float64).reshape(-1, 2)
    B, S, F = len(so) - 1, int(so[-1]), len(faces)
    fb = np.zeros(S, np.int64) if fo is None else np.asarray(fo, np.int64)[:-1]
    fe = np.full(S, F, np.int64) if fo is None else np.asarray(fo, np.int64)[1:]
    counts, flags = [], np.zeros(B, np.int32)
    Wn, Tn, Fn, fcnt, parent, inserted, Ls = [], [], [], [], [], [], []
    for b in range(B):
        s0, s1 = int(so[b]), int(so[b + 1])
        M = s1 - s0
        Tb, Wb = T[s0:s1], W[s0 + b:s1 + b + 1]
        bad = not (np.isfinite(Tb).all() and (Tb > 0).all() and np.isfinite(C[s0:s1]).all() and np.isfinite(Wb).all())
        mask, flags[b] = plan_row(Tb, seg_rec[s0:s1, 0], seg_rec[s0:s1, 1], seg_face[s0:s1], fb[s0:s1], fe[s0:s1], F,
                                  r, bad)
        knot, n_new = np.float64(0.0), 0
        for i in range(M):
            s = s0 + i
            span = faces[fb[s]:fe[s]] if span_ok(int(fb[s]), int(fe[s]), F) else faces[:0]
            Wn.append(Wb[i])
            if mask[i]:
                tl, tr = split_times(local_time(seg_rec[s, 1], knot, Tb[i]), Tb[i], min_frac)
                w = (pull_point(C[s], tl, faces[seg_face[s]], r) if mode == PULL
                     else chord_point(Wb[i], Wb[i + 1], tl, Tb[i]))
                Wn.append(w)
                Tn += [tl, tr]
            else:
                Tn.append(Tb[i])
            grid = np.linspace(0.0, float(Tb[i]), 129).astype(LD)
            L = max(float(np.abs(_polyval(np.asarray(C[s, ax], dtype=LD), grid)).max()) for ax in range(3))
            for k in range(2 if mask[i] else 1):
                parent.append(s)
                inserted.append(bool(mask[i]) and k == 0)
                Ls.append(L)
                Fn.append(span)
                fcnt.append(len(span))
                n_new += 1
            knot = knot + np.float64(Tb[i])
        Wn.append(Wb[M])
        counts.append(n_new)
    out = dict(so=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), W=np.array(Wn, np.float64).reshape(-1, 3),
               T=np.array(Tn, np.float64), parent=np.array(parent, np.int32), flags=flags,
               inserted=np.array(inserted, bool), L=np.array(Ls, np.float64))
    if fo is None:
        out["faces"], out["fo"] = faces, None
    else:
        out["faces"] = np.concatenate(Fn).reshape(-1, 4) if Fn else faces[:0]
        out["fo"] = np.concatenate([[0], np.cumsum(fcnt)]).astype(np.int64)
    return out
