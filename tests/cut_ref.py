"""Reference for the replan cut (tgms_cut_batch*), shared by test_cut_ref.py, test_cut_host.py
and test_gpu_cut.py.  Independent of the library: the decisions and the times in plain fp64
exactly as include/tgms.h states them (numpy float64 scalars, one rounded operation per line),
the evaluated values in fractions.Fraction with the header's Horner condition sums as their
tolerances."""
from fractions import Fraction as F
from math import comb, factorial

import numpy as np

DONE, SNAPPED, FINISHED, NONFINITE = 1, 2, 4, 16
NONE = -1
TOL = 1e-9


def knots(T):
    k = [np.float64(0.0)]
    for t in T:
        k.append(np.float64(k[-1] + np.float64(t)))
    return k


def decide(T, t_cut, min_frac):
    """One usable trajectory: (finished, s, t_loc, flags, t0), every operation rounded once."""
    T = [np.float64(t) for t in T]
    M, k = len(T), knots(T)
    D, t_cut, min_frac = k[M], np.float64(t_cut), np.float64(min_frac)
    if t_cut >= D:
        return True, 0, np.float64(0.0), FINISHED | DONE, D
    t_c = min(max(t_cut, np.float64(0.0)), D)
    s = sum(1 for m in range(1, M) if k[m] <= t_c)
    t_loc = min(max(np.float64(t_c - k[s]), np.float64(0.0)), T[s])
    rem = np.float64(T[s] - t_loc)
    least = np.float64(min_frac * T[s])
    flags = 0
    if rem <= 0.0 or rem < least:
        if s == M - 1:
            return True, 0, np.float64(0.0), FINISHED | DONE, D
        s, t_loc, flags = s + 1, np.float64(0.0), SNAPPED
    if s > 0 or t_loc > 0.0:
        flags |= DONE
    return False, s, t_loc, flags, np.float64(k[s] + t_loc)


def shifted(c, t):
    """Exact Taylor shift of c [8] (floats or Fractions) to t: (values [8] as Fractions, condition
    sums [8])."""
    fr = lambda x: x if isinstance(x, F) else F(float(x))
    cf, tf = [fr(x) for x in c], fr(t)
    val = [sum(comb(j, k) * cf[j] * tf ** (j - k) for j in range(k, 8)) for k in range(8)]
    cond = [float(sum(comb(j, k) * abs(cf[j]) * abs(tf) ** (j - k) for j in range(k, 8))) for k in range(8)]
    return val, cond


def cut(so, W, T, C, t_cut, min_frac, ED=None):
    """The whole call.  Returns a dict: so, T, parent, t0, flags (exact to the bit), W, ED, C with
    W_tol, ED_tol, C_tol (0.0: a copy, equal to the bit), and s, t_loc, kind per trajectory."""
    so = np.asarray(so, np.int64)
    W = np.asarray(W, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1)
    C = np.asarray(C, np.float64).reshape(-1, 3, 8)
    ED = None if ED is None else np.asarray(ED, np.float64).reshape(-1, 18)
    B = len(so) - 1
    o = dict(so=[0], T=[], parent=[], t0=[], flags=[], W=[], W_tol=[], ED=[], ED_tol=[], C=[], C_tol=[], s=[], t_loc=[],
             kind=[])
    for b in range(B):
        s0, s1 = int(so[b]), int(so[b + 1])
        M = s1 - s0
        Tb, Cb, Wb = T[s0:s1], C[s0:s1], W[s0 + b:s1 + b + 1]
        Eb = np.zeros(18) if ED is None else ED[b]
        bad = not (np.isfinite(Tb).all() and np.isfinite(Cb).all() and np.isfinite(Wb).all() and np.isfinite(Eb).all()
                   and (Tb > 0).all()) or np.isnan(t_cut[b])
        if bad:
            fin, s, t_loc, fl, t0 = False, 0, np.float64(0.0), NONFINITE, np.float64("nan")
        else:
            fin, s, t_loc, fl, t0 = decide(Tb, t_cut[b], min_frac)
        o["flags"].append(fl)
        o["t0"].append(t0)
        o["s"].append(s)
        o["t_loc"].append(t_loc)
        o["kind"].append("through" if bad else "finished" if fin else "keep")
        ed, ed_tol = Eb.copy(), np.zeros(18)
        if fin:
            o["T"].append(Tb[M - 1:])
            o["parent"].append([s1 - 1])
            o["W"].append(np.stack([Wb[M], Wb[M]]))
            o["W_tol"].append(np.zeros((2, 3)))
            c = np.zeros((1, 3, 8))
            c[0, :, 0] = Wb[M]
            o["C"].append(c)
            o["C_tol"].append(np.zeros((1, 3, 8)))
            ed[:] = 0.0
        else:
            inside = t_loc > 0.0
            Tn = Tb[s:].copy()
            if inside:
                Tn[0] = np.float64(Tb[s] - t_loc)
            Wn, Wt = Wb[s:].copy(), np.zeros((M - s + 1, 3))
            Cn, Ct = Cb[s:].copy(), np.zeros((M - s, 3, 8))
            if s > 0 or inside:
                for a in range(3):
                    val, cond = shifted(Cb[s, a], t_loc)
                    for k in (1, 2, 3):
                        ed[(k - 1) * 3 + a] = float(factorial(k) * val[k])
                        ed_tol[(k - 1) * 3 + a] = TOL * factorial(k) * cond[k]
                    if inside:
                        Wn[0, a], Wt[0, a] = float(val[0]), TOL * cond[0]
                        Cn[0, a], Ct[0, a] = [float(v) for v in val], [TOL * x for x in cond]
            o["T"].append(Tn)
            o["parent"].append(np.arange(s0 + s, s1))
            o["W"].append(Wn)
            o["W_tol"].append(Wt)
            o["C"].append(Cn)
            o["C_tol"].append(Ct)
        o["ED"].append(ed)
        o["ED_tol"].append(ed_tol)
        o["so"].append(o["so"][-1] + len(o["T"][-1]))
    cat = lambda k, shape, dt: (np.concatenate(o[k]).astype(dt) if B else np.zeros(0, dt)).reshape(shape)
    return dict(so=np.array(o["so"], np.int32), T=cat("T", (-1,), np.float64), parent=cat("parent", (-1,), np.int32),
                t0=np.array(o["t0"], np.float64), flags=np.array(o["flags"], np.int32),
                W=cat("W", (-1, 3), np.float64), W_tol=cat("W_tol", (-1, 3), np.float64),
                ED=np.array(o["ED"], np.float64).reshape(B, 18), ED_tol=np.array(o["ED_tol"], np.float64).reshape(B, 18),
                C=cat("C", (-1, 3, 8), np.float64), C_tol=cat("C_tol", (-1, 3, 8), np.float64),
                s=np.array(o["s"]), t_loc=np.array(o["t_loc"], np.float64), kind=o["kind"])


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def compare(out, ref):
    """out: Solver.cut's tuple (so, W, T, ED, C or None, parent, t0, flags) against cut()'s dict:
    integers, flags, times and t0 to the bit, copies to the bit, evaluated values within their
    condition sums."""
    so, W, T, ED, C, parent, t0, flags = out
    assert np.array_equal(so, ref["so"])
    assert np.array_equal(flags, ref["flags"])
    assert np.array_equal(parent, ref["parent"])
    assert np.array_equal(bits(T), bits(ref["T"]))
    nan = np.isnan(ref["t0"])
    assert np.array_equal(np.isnan(t0), nan) and np.array_equal(bits(t0[~nan]), bits(ref["t0"][~nan]))
    for x, key in ((W, "W"), (np.asarray(ED).reshape(-1, 18), "ED"), (C, "C")):
        if x is None:
            continue
        r, tol = ref[key], ref[key + "_tol"]
        assert x.shape == r.shape, key
        copy = tol == 0.0
        assert np.array_equal(bits(x)[copy], bits(r)[copy]), key
        assert (np.abs(x[~copy] - r[~copy]) <= tol[~copy]).all(), key
