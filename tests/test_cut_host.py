"""CPU: the replan cut on the explicit host backend (tgms_cut_batch on a tgms_create_host handle;
csrc/tgms_host.cpp cut(), the decisions of csrc/tgms_cut_core.h) against the reference of
cut_ref.py: integers, flags, times and t0 to the bit, copied rows to the bit, evaluated states
and shifted coefficients within the header's Horner condition sums at 1e-9.

The re-solve check rests on Bellman's principle (test_cut_ref.py): cut, solve, and the solve
reproduces coeffs_out.  Its inputs are ragged, M = 1..16 three times over, T in [0.5, 2] s,
min_frac = 0.25, seeded; before the seed was fixed the host solve alone was measured against the
exact rational solve (oracle/exact.py) of the very batches the cut produces, rest-to-rest and
with end derivatives: its worst norm-wise error per (trajectory, axis) was 9.8e-12, below 1e-10
(and coeffs_out, which inherits the error of the first solve, was within 4.2e-11 of that exact
solve), so the 1e-9 of the check is the solver's contract and not a number fitted to this test.

The checks take the call as a parameter (`Cut`): test_gpu_cut.py runs them through the device."""
from math import factorial

import numpy as np
import pytest

import cut_ref as CR
from conftest import batch_rel_err

B0 = 48
MIN_FRAC = 0.25


@pytest.fixture(scope="module")
def host():
    from trajectory_generator_ros2_amd.solver import Solver
    s = Solver(host=True)
    yield s
    s.close()


def ragged_case(solve, with_derivs, seed=20261020):
    """48 trajectories, M = 1..16 three times; the three rows of an M are cut in its first, a
    middle and its last segment, far enough from the segment's end not to snap.  A few rows are
    then moved onto the special places: at and before 0, at and beyond the end, on a knot, close
    before a knot (snapped) and close before the end (finished)."""
    rng = np.random.default_rng(seed)
    M = 1 + np.arange(B0) % 16
    so = np.concatenate([[0], np.cumsum(M)]).astype(np.int32)
    S = int(so[-1])
    W = rng.uniform(-3.0, 3.0, (S + B0, 3))
    T = rng.uniform(0.5, 2.0, S)
    ED = rng.uniform(-1.0, 1.0, (B0, 18)) if with_derivs else None
    C, st, worst = solve(so, W, T, ED)
    assert worst == 0 and not st.any()
    tc = np.zeros(B0)
    for b in range(B0):
        k = CR.knots(T[so[b]:so[b + 1]])
        m = int(M[b])
        s = (0, m // 2, m - 1)[b // 16]
        tc[b] = k[s] + rng.uniform(0.05, 0.7) * T[so[b] + s]
    kn = lambda b: CR.knots(T[so[b]:so[b + 1]])
    tc[3], tc[5], tc[20] = 0.0, -1.0, -np.inf
    tc[7], tc[9], tc[22] = np.inf, kn(9)[-1], kn(22)[-1] + 0.5
    tc[11] = kn(11)[2]                                  # on a knot
    tc[13] = kn(13)[5] - 0.1 * T[so[13] + 4]            # 10 % of segment 4 left: snapped
    tc[15] = kn(15)[-1] - 0.1 * T[so[16] - 1]           # 10 % of the last segment left: finished
    return dict(so=so, W=W, T=T, ED=ED, C=C, tc=tc)


def host_cut(host):
    return lambda so, W, T, C, tc, mf, ED=None, want_coeffs=True: host.cut(so, W, T, C, tc, mf, ED, want_coeffs)


@pytest.fixture(scope="module", params=["rest", "end_derivs"])
def case(request, host):
    return ragged_case(host.solve, request.param == "end_derivs")


@pytest.fixture(scope="module")
def Cut(host):
    return host_cut(host)


@pytest.fixture(scope="module")
def solve(host):
    return host.solve


def run(Cut, c, mf=MIN_FRAC, **kw):
    return Cut(c["so"], c["W"], c["T"], c["C"], c["tc"], mf, c["ED"], **kw)


# ---- the checks, shared with the device tests ----

def check_against_ref(Cut, c):
    for mf in (MIN_FRAC, 0.0):
        out = run(Cut, c, mf)
        ref = CR.cut(c["so"], c["W"], c["T"], c["C"], c["tc"], mf, c["ED"])
        CR.compare(out, ref)
    fl = out[7]
    assert fl[3] == 0 and fl[5] == 0 and fl[20] == 0 and fl[11] == CR.DONE
    assert (fl[[7, 9, 22]] == CR.FINISHED | CR.DONE).all()
    out = run(Cut, c)
    assert out[7][13] == CR.DONE | CR.SNAPPED and out[7][15] == CR.FINISHED | CR.DONE
    assert set(out[7]) == {0, CR.DONE, CR.DONE | CR.SNAPPED, CR.DONE | CR.FINISHED}


def check_identity(Cut, c):
    for t in (0.0, -2.5, -np.inf):
        out = Cut(c["so"], c["W"], c["T"], c["C"], np.full(B0, t), MIN_FRAC, c["ED"])
        ED = np.zeros((B0, 18)) if c["ED"] is None else c["ED"]
        for x, y in zip(out[:5], (c["so"], c["W"], c["T"], ED, c["C"])):
            assert np.array_equal(CR.bits(x), CR.bits(np.asarray(y, x.dtype).reshape(x.shape)))
        assert np.array_equal(out[5], np.arange(c["so"][-1])) and not out[6].any() and not out[7].any()


def check_finished(Cut, c):
    so, W, T = c["so"], c["W"], c["T"]
    out = Cut(so, W, T, c["C"], np.full(B0, np.inf), MIN_FRAC, c["ED"])
    last = so[1:] - 1
    wM = W[so[1:] + np.arange(B0)]
    assert np.array_equal(out[0], np.arange(B0 + 1)) and (out[7] == CR.FINISHED | CR.DONE).all()
    assert np.array_equal(out[1].reshape(B0, 2, 3), np.stack([wM, wM], axis=1))
    assert np.array_equal(out[2], T[last]) and not out[3].any() and np.array_equal(out[5], last)
    assert np.array_equal(out[4][:, :, 0], wM) and not out[4][:, :, 1:].any()
    D = np.array([CR.knots(T[so[b]:so[b + 1]])[-1] for b in range(B0)])
    assert np.array_equal(out[6], D)


def rows_of(out, b):
    so = out[0]
    a, e = int(so[b]), int(so[b + 1])
    return (out[1][a + b:e + b + 1], out[2][a:e], out[3][b], None if out[4] is None else out[4][a:e], out[5][a:e] - out[5][a],
            out[6][b:b + 1], out[7][b:b + 1])


def same(x, y):
    return all((p is None and q is None) or np.array_equal(CR.bits(p), CR.bits(q)) for p, q in zip(x, y))


def check_unusable(Cut, c):
    """A NaN coefficient, an infinite waypoint, a zero time, a NaN end derivative and a NaN t_cut, one
    row each: copied through with NONFINITE alone and a NaN t0; every other row as in the clean call."""
    so = c["so"]
    W, T, C, tc = c["W"].copy(), c["T"].copy(), c["C"].copy(), c["tc"].copy()
    ED = None if c["ED"] is None else c["ED"].copy()
    C[so[6] + 2, 1, 4] = np.nan
    W[so[17] + 17 + 1, 2] = np.inf
    T[so[26]] = 0.0
    tc[33] = np.nan
    bad = [6, 17, 26, 33]
    if ED is not None:
        ED[40, 11] = np.nan
        bad.append(40)
    out = Cut(so, W, T, C, tc, MIN_FRAC, ED)
    clean = run(Cut, c)
    CR.compare(out, CR.cut(so, W, T, C, tc, MIN_FRAC, ED))
    for b in range(B0):
        if b not in bad:
            assert same(rows_of(out, b), rows_of(clean, b)), b
            continue
        assert out[7][b] == CR.NONFINITE and np.isnan(out[6][b])
        a, e = int(out[0][b]), int(out[0][b + 1])
        assert e - a == so[b + 1] - so[b]
        assert same((out[1][a + b:e + b + 1], out[2][a:e], out[4][a:e]),
                    (W[so[b] + b:so[b + 1] + b + 1], T[so[b]:so[b + 1]], C[so[b]:so[b + 1]]))
        assert np.array_equal(CR.bits(out[3][b]), CR.bits(np.zeros(18) if ED is None else ED[b]))


def check_resolve(Cut, solve, c):
    """Cut, solve: the solve reproduces coeffs_out at 1e-9 norm-wise per (trajectory, axis); no
    row is left out."""
    so2, W2, T2, ED2, C2, _, _, fl = run(Cut, c)
    assert not (fl & CR.NONFINITE).any()
    R, st, worst = solve(so2, W2, T2, ED2)
    assert worst == 0 and not st.any()
    err = batch_rel_err(so2, R, C2)
    print("re-solve against coeffs_out:", err)
    assert err <= 1e-9
    return so2, R, C2


def check_join(Cut, solve, c):
    """p, v, a, j of the new first segment at 0 are those of the old trajectory at t0_out, within
    1e-9 of the Horner condition sums of the old segment; from coeffs_out and from the re-solved
    coefficients.  Every row that still flies; a finished row holds the end point instead."""
    so, T, C = c["so"], c["T"], c["C"]
    so2, W2, T2, ED2, C2, parent, t0, fl = run(Cut, c)
    R = solve(so2, W2, T2, ED2)[0]
    ref = CR.cut(so, c["W"], T, C, c["tc"], MIN_FRAC, c["ED"])
    n = 0
    for b in range(B0):
        if fl[b] & CR.FINISHED:
            continue
        seg, t_loc = int(parent[so2[b]]), ref["t_loc"][b]
        assert seg == so[b] + ref["s"][b] and t0[b] == CR.knots(T[so[b]:so[b + 1]])[ref["s"][b]] + t_loc
        for a in range(3):
            val, cond = CR.shifted(C[seg, a], t_loc)
            for q in range(4):
                want, tol = float(factorial(q) * val[q]), CR.TOL * factorial(q) * cond[q]
                for got in (C2[so2[b], a, q], R[so2[b], a, q]):
                    assert abs(factorial(q) * got - want) <= tol, (b, a, q)
        n += 1
    assert n >= 40


# ---- on the host backend ----

def test_against_the_reference(Cut, case):
    check_against_ref(Cut, case)


def test_a_cut_at_or_before_zero_reproduces_the_batch(Cut, case):
    check_identity(Cut, case)


def test_finished_rows_hold_the_end_point(Cut, case):
    check_finished(Cut, case)


def test_unusable_rows_are_copied_through(Cut, case):
    check_unusable(Cut, case)


def test_cut_then_solve_reproduces_the_tail(Cut, solve, case):
    check_resolve(Cut, solve, case)


def test_the_join_is_smooth(Cut, solve, case):
    check_join(Cut, solve, case)


def test_without_coeffs_out(Cut, case):
    full, part = run(Cut, case), run(Cut, case, want_coeffs=False)
    assert part[4] is None and same(full[:4] + full[5:], part[:4] + part[5:])


def _raw(host, c, omit=(), mf=MIN_FRAC, B=B0):
    """tgms_cut_batch through ctypes with outputs of NaN and -7, some of them omitted."""
    from trajectory_generator_ros2_amd import _lib
    L = _lib.load()
    S = int(c["so"][-1])
    o = dict(so=np.full(B0 + 1, -7, np.int32), W=np.full((S + B0, 3), np.nan), T=np.full(S, np.nan),
             ED=np.full((B0, 18), np.nan), C=np.full((S, 3, 8), np.nan), parent=np.full(S, -7, np.int32),
             t0=np.full(B0, np.nan), totals=np.full(1, -7, np.int64), flags=np.full(B0, -7, np.int32))
    p = lambda a: None if a is None else a.ctypes.data
    g = lambda k: None if k in omit else p(o[k])
    st = L.tgms_cut_batch(host._h, B, p(c["so"]), p(c["W"]), p(c["T"]), p(c["ED"]), p(c["C"]), p(c["tc"]), mf,
                          g("so"), g("W"), g("T"), g("ED"), g("C"), g("parent"), g("t0"), g("totals"), g("flags"))
    return st, o


def test_nullable_outputs_omitted_in_turn_and_nothing_written_beyond_the_totals(host, case):
    st, full = _raw(host, case)
    assert st == 0
    S2 = int(full["totals"][0])
    assert S2 == full["so"][-1] < case["so"][-1]
    assert np.isnan(full["T"][S2:]).all() and np.isnan(full["W"][S2 + B0:]).all() and np.isnan(full["C"][S2:]).all()
    assert (full["parent"][S2:] == -7).all() and not np.isnan(full["T"][:S2]).any()
    for name in ("C", "parent", "t0", "flags"):
        st, part = _raw(host, case, omit=(name,))
        assert st == 0
        assert all(np.array_equal(CR.bits(part[k]), CR.bits(full[k])) for k in full if k != name), name


def test_argument_errors(host, case):
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_UNSUPPORTED, TgmsError
    for mf in (-0.1, 1.0, np.nan, np.inf):
        st, o = _raw(host, case, mf=mf)
        assert st == ERR_INVALID_ARG and (o["so"] == -7).all()
    for name in ("so", "W", "T", "ED", "totals"):
        st, o = _raw(host, case, omit=(name,))
        assert st == ERR_INVALID_ARG, name
    c = case
    with pytest.raises(TgmsError) as e:  # the device entry needs a GPU handle
        host.cut_device(B0, c["so"], c["W"], c["T"], c["C"], c["tc"], 0.25, c["so"].copy(), c["W"].copy(),
                        c["T"].copy(), np.zeros((B0, 18)), np.zeros(1, np.int64))
    assert e.value.status == ERR_UNSUPPORTED
    st, o = _raw(host, case, B=0)
    assert st == 0 and o["so"][0] == 0 and o["totals"][0] == 0 and (o["so"][1:] == -7).all() and np.isnan(o["T"]).all()


def test_symbols_exported():
    from trajectory_generator_ros2_amd import _lib
    L = _lib.load()
    for name in ("tgms_cut_batch", "tgms_cut_batch_device"):
        assert name in _lib.EXPORTS and hasattr(L, name)
