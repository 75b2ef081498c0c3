"""Constructed minimum-snap problems for the solve kernels (TEST INFRASTRUCTURE ONLY).

The parity suites draw every solve input from synthetic.uniform_batch / ragged_batch: i.i.d.
waypoints in one room, compared with the fp64 oracle at the tolerance.  This module builds what
that distribution never contains -- a repeated waypoint inside a moving trajectory, an axis that
does not move, two identical axes, collinear back-and-forth legs with times 0.5 / 10, non-zero end
derivatives at every M, a trajectory 2^20 m from the origin -- with two references that do not
come from the hand that wrote the kernels:

* reference(problem): oracle/exact.py's rational solve of the very inputs, rounded once to fp64;
  for the `cubic` family also the closed form (waypoints and end derivatives sampled from one
  cubic per axis: that cubic has zero snap and is the unique optimum, so c4..c7 == 0 and c0..c3
  are its Taylor shift at each knot);
* symmetries that hold to the bit.  The solution is linear in the waypoints and end derivatives
  and every fp64 operation commutes with a power of two, so data scaled by 2^k gives the same
  bits scaled; two axes with the same data give the same bits; an axis that does not move gives
  exact zeros; permuted axes give permuted bits.

Every value is dyadic (waypoints multiples of 2^-10 with |w| <= 16, times multiples of 1/4 in
[0.5, 10], end derivatives multiples of 2^-6 or a dyadic cubic's), so each input is exact in fp64
and stays exact under the transforms.  A problem is built in Fractions and converted; the
conversion is asserted exact.  Every time ratio is <= 20, what the suite already covers.

End derivatives are the C ABI's [start|final][v,a,j][x,y,z], flattened to 18.

The check_* functions take a Run (one backend's results of one M) and are shared by
test_solve_zoo_host.py (host backend, CPU) and test_gpu_solve_zoo.py (every device method)."""
import functools
import itertools
import os
import sys
from fractions import Fraction as F

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import exact  # noqa: E402

TOL = 1e-9
B_TILED = 197               # three full wavefronts and a tail of five
OFFSET = (F(2) ** 20, -F(2) ** 20, F(2) ** 19)
PERMS = list(itertools.permutations(range(3)))
W_SCALES = (-20, 20)
T_SCALES = (-1, 1)
REST = ("repeat_first", "repeat_mid", "repeat_last", "one_axis_x", "one_axis_z", "zigzag", "plain")


# ---------------------------------------------------------------------------------- problems

class Problem:
    """One trajectory: Fractions (the construction) and their fp64 images (asserted exact)."""

    def __init__(self, Wq, Tq, EDq=None):
        self.Wq = [list(r) for r in Wq]
        self.Tq = list(Tq)
        self.EDq = None if EDq is None else list(EDq)
        self.M = len(self.Tq)
        assert len(self.Wq) == self.M + 1 and (self.EDq is None or len(self.EDq) == 18)
        self.W = np.array([[float(x) for x in r] for r in self.Wq], dtype=np.float64).reshape(-1, 3)
        self.T = np.array([float(t) for t in self.Tq], dtype=np.float64)
        self.ED = None if self.EDq is None else np.array([float(x) for x in self.EDq], dtype=np.float64)
        assert self.is_exact()
        for a in (self.W, self.T) + (() if self.ED is None else (self.ED,)):
            a.setflags(write=False)
        self.key = (self.W.tobytes(), self.T.tobytes(), None if self.ED is None else self.ED.tobytes())

    def is_exact(self):
        """Every fp64 input equals the Fraction it was built from."""
        ok = all(F(float(x)) == q for r, rq in zip(self.W, self.Wq) for x, q in zip(r, rq))
        ok = ok and all(F(float(x)) == q for x, q in zip(self.T, self.Tq))
        return ok and (self.ED is None or all(F(float(x)) == q for x, q in zip(self.ED, self.EDq)))

    def ed3(self):
        """End derivatives as exact.py takes them ([2][3][3]) or None."""
        return None if self.ED is None else self.ED.reshape(2, 3, 3)


def _dy(rng, lim, q, nonzero=False):
    """A random multiple of 1/q in [-lim, lim]."""
    while True:
        n = int(rng.integers(-lim * q, lim * q + 1))
        if n or not nonzero:
            return F(n, q)


def _times(rng, M):
    return [F(int(rng.integers(2, 41)), 4) for _ in range(M)]


def _waypoints(rng, M, lim=16):
    return [[_dy(rng, lim, 1024) for _ in range(3)] for _ in range(M + 1)]


def _end_derivs(rng):
    return [_dy(rng, 2, 64, nonzero=True) for _ in range(18)]


def _rng(family, M, seed):
    return np.random.default_rng([sum(map(ord, family)), M, seed])


def plain(M, seed=0):
    """Random dyadic waypoints, rest to rest: the base row of the transforms."""
    rng = _rng("plain", M, seed)
    return Problem(_waypoints(rng, M), _times(rng, M))


def _cubic_parts(M, seed):
    """Times (sum <= 8 s), the knots' offsets s_i from the middle of the flight (|s| <= 4) and the
    coefficients a[axis][0..3] of p(s) = a0 + a1 s + a2 s^2 + a3 s^3: a3 = +-1/16, a2 a multiple
    of 1/64 in +-1/4, a1 of 1/256 in +-1, a0 of 1/1024 in +-4, so that with s a multiple of 1/4
    every waypoint is a multiple of 2^-10 and |w| <= 4 + 4 + 4 + 4."""
    rng = _rng("cubic", M, seed)
    quarters = [2] * M
    for _ in range(int(rng.integers(0, 32 - 2 * M + 1))):
        quarters[int(rng.integers(0, M))] += 1
    Tq = [F(n, 4) for n in quarters]
    assert sum(Tq) <= 8
    tc = F(sum(quarters) // 2, 4)
    s = [sum(Tq[:i], F(0)) - tc for i in range(M + 1)]
    a = [[_dy(rng, 4, 1024), _dy(rng, 1, 256), F(int(rng.integers(-16, 17)), 64), F(int(rng.choice([-1, 1])), 16)]
         for _ in range(3)]
    return Tq, s, a


def _cubic_state(a, s):
    """p, p', p'', p''' of one axis' cubic at s."""
    return [a[0] + a[1] * s + a[2] * s * s + a[3] * s ** 3, a[1] + 2 * a[2] * s + 3 * a[3] * s * s,
            2 * a[2] + 6 * a[3] * s, 6 * a[3]]


def cubic(M, seed=0):
    """Waypoints and both ends' v, a, j sampled from one random dyadic cubic per axis."""
    Tq, s, a = _cubic_parts(M, seed)
    Wq = [[_cubic_state(a[ax], si)[0] for ax in range(3)] for si in s]
    assert all(abs(x) <= 16 for r in Wq for x in r)
    EDq = [_cubic_state(a[ax], s[e])[d] for e in (0, M) for d in (1, 2, 3) for ax in range(3)]
    return Problem(Wq, Tq, EDq)


def cubic_closed_form(M, seed=0):
    """The exact optimum of cubic(M, seed): coeffs[M][3][8] as Fractions."""
    _, s, a = _cubic_parts(M, seed)
    out = []
    for i in range(M):
        seg = []
        for ax in range(3):
            p = _cubic_state(a[ax], s[i])
            seg.append([p[0], p[1], p[2] / 2, p[3] / 6] + [F(0)] * 4)
        out.append(seg)
    return out


def repeat(M, leg, seed=0):
    """Random dyadic waypoints with waypoint leg + 1 equal to waypoint leg.  M = 1: the stationary
    row (the only leg is the repeated one)."""
    rng = _rng("repeat", M, 16 * seed + leg)
    Wq = _waypoints(rng, M)
    Wq[leg + 1] = list(Wq[leg])
    return Problem(Wq, _times(rng, M))


def one_axis(M, axis, seed=0):
    """Only `axis` moves, with plain(M, seed)'s column of that axis and plain's times; the other
    two axes hold a constant that is not zero."""
    base = plain(M, seed)
    rng = _rng("one_axis", M, 16 * seed + axis)
    const = [_dy(rng, 16, 1024, nonzero=True) for _ in range(3)]
    Wq = [[r[a] if a == axis else const[a] for a in range(3)] for r in base.Wq]
    return Problem(Wq, base.Tq)


def twin(M, seed=0):
    """The y column is a copy of the x column, waypoints and end derivatives (all non-zero)."""
    rng = _rng("twin", M, seed)
    Wq = [[r[0], r[0], r[2]] for r in _waypoints(rng, M)]
    EDq = _end_derivs(rng)
    for k in range(6):
        EDq[3 * k + 1] = EDq[3 * k]
    return Problem(Wq, _times(rng, M), EDq)


def zigzag(M, seed=0):
    """Collinear back and forth: base +- a (1, 1/2, -1/4) with alternating times 0.5 / 10."""
    rng = _rng("zigzag", M, seed)
    base = [_dy(rng, 4, 1024) for _ in range(3)]
    a = F(int(rng.integers(256, 8 * 256 + 1)), 256)
    d = (F(1), F(1, 2), F(-1, 4))
    Wq = [[base[ax] + (-1) ** i * a * d[ax] for ax in range(3)] for i in range(M + 1)]
    first = int(rng.integers(0, 2))
    return Problem(Wq, [F(1, 2) if (i + first) % 2 == 0 else F(10) for i in range(M)])


def hermite1(seed=0):
    """M = 1 with all six end derivatives non-zero on every axis."""
    rng = _rng("hermite1", 1, seed)
    return Problem(_waypoints(rng, 1), _times(rng, 1), _end_derivs(rng))


# -------------------------------------------------------------------------------- transforms
# Each returns (transformed problem, map of a base solution [..., 3, 8] to the transformed one).
# The maps are exact in fp64: powers of two, a permutation, or c0 + o where c0 is a waypoint.

def scale_w(p, k):
    s = F(2) ** k
    q = Problem([[x * s for x in r] for r in p.Wq], p.Tq, None if p.EDq is None else [x * s for x in p.EDq])
    return q, lambda C: np.ldexp(C, k)


def scale_t(p, k):
    ed = None if p.EDq is None else [x * F(2) ** (-k * (1 + (i // 3) % 3)) for i, x in enumerate(p.EDq)]
    q = Problem(p.Wq, [t * F(2) ** k for t in p.Tq], ed)
    return q, lambda C: np.ldexp(C, -k * np.arange(8))


def translate(p, o=OFFSET):
    q = Problem([[x + d for x, d in zip(r, o)] for r in p.Wq], p.Tq, p.EDq)
    of = np.array([float(d) for d in o])

    def fmap(C):
        out = np.array(C, dtype=np.float64)
        out[..., 0] += of
        return out
    return q, fmap


def swap_axes(p, perm):
    perm = list(perm)
    ed = None if p.EDq is None else [p.EDq[3 * (i // 3) + perm[i % 3]] for i in range(18)]
    q = Problem([[r[a] for a in perm] for r in p.Wq], p.Tq, ed)
    return q, lambda C: np.asarray(C)[..., perm, :]


# --------------------------------------------------------------------------------- reference

_exact_cache = {}


def exact_solution(p):
    """exact.reduced_solve of the problem's fp64 inputs: coeffs[M][3][8] as Fractions (cached)."""
    if p.key not in _exact_cache:
        _exact_cache[p.key] = exact.reduced_solve(p.W, p.T, p.ed3())
    return _exact_cache[p.key]


_ref_cache = {}


def reference(p):
    """The exact solution rounded once to fp64: [M, 3, 8], cached per problem, read-only."""
    if p.key not in _ref_cache:
        R = np.array([[[float(c) for c in ax] for ax in seg] for seg in exact_solution(p)], dtype=np.float64)
        R.setflags(write=False)
        _ref_cache[p.key] = R
    return _ref_cache[p.key]


# ----------------------------------------------------------------------------------- batches

def tiled_batch(rows, B=B_TILED):
    """The K rows of one M laid cyclically into a uniform batch of B trajectories:
    (seg_offsets, W [B(M+1),3], T [B M], ED [B,18] or None, source row per trajectory).  ED is
    None when no row has end derivatives; else rows without them get zeros."""
    M = rows[0].M
    assert all(r.M == M for r in rows)
    src = np.arange(B) % len(rows)
    return _pack([rows[k] for k in src]) + (src,)


def _pack(probs):
    so = np.concatenate([[0], np.cumsum([p.M for p in probs])]).astype(np.int32)
    W = np.concatenate([p.W for p in probs])
    T = np.concatenate([p.T for p in probs])
    ED = None
    if any(p.ED is not None for p in probs):
        ED = np.stack([np.zeros(18) if p.ED is None else p.ED for p in probs])
    return so, W, T, ED


def ragged_mix(rows_by_M, seed):
    """Rows of every M shuffled into one CSR batch: (seg_offsets, W, T, ED or None, order), where
    order[b] indexes the flat list of rows (rows_by_M's values concatenated in key order)."""
    flat = [r for M in sorted(rows_by_M) for r in rows_by_M[M]]
    order = np.random.default_rng(seed).permutation(len(flat))
    return _pack([flat[k] for k in order]) + (order, flat)


@functools.lru_cache(maxsize=None)
def families(M):
    """name -> Problem: the untransformed rows of one M."""
    legs = (0, M // 2, M - 1)
    rows = dict(repeat_first=repeat(M, legs[0], 0), repeat_mid=repeat(M, legs[1], 1), repeat_last=repeat(M, legs[2], 2),
                one_axis_x=one_axis(M, 0), one_axis_z=one_axis(M, 2), zigzag=zigzag(M), plain=plain(M),
                cubic=cubic(M), twin=twin(M))
    if M == 1:
        rows.update(hermite1=hermite1(0), hermite1_b=hermite1(1))
    return rows


def family_of(name):
    for f in ("repeat", "one_axis", "hermite1"):
        if name.startswith(f):
            return f
    return name


@functools.lru_cache(maxsize=None)
def transformed_rows(M):
    """label -> (base name, Problem, map) of the `plain` and `cubic` rows under every transform."""
    out = {}
    for base in ("plain", "cubic"):
        p = families(M)[base]
        out[base] = (base, p, lambda C: np.asarray(C))
        for k in W_SCALES:
            out["%s|scale_w%+d" % (base, k)] = (base,) + scale_w(p, k)
        for k in T_SCALES:
            out["%s|scale_t%+d" % (base, k)] = (base,) + scale_t(p, k)
        out["%s|translate" % base] = (base,) + translate(p)
        for perm in PERMS[1:]:
            out["%s|swap%d%d%d" % ((base,) + perm)] = (base,) + swap_axes(p, perm)
    return out


@functools.lru_cache(maxsize=None)
def cases(M):
    """The three uniform launches of one M: case -> (labels, problems, tiled batch).
    rest: the seven rows without end derivatives (ED NULL); ed: cubic, twin, plain (and hermite1 at
    M = 1) with the end-derivative array; xf: plain and cubic with all their transformed images."""
    fam = families(M)
    out = {}
    ed = ["cubic", "twin", "plain"] + [n for n in fam if n.startswith("hermite1")]
    for case, labels in (("rest", list(REST)), ("ed", ed)):
        probs = [fam[n] for n in labels]
        out[case] = (labels, probs, tiled_batch(probs))
    xf = transformed_rows(M)
    out["xf"] = (list(xf), [v[1] for v in xf.values()], tiled_batch([v[1] for v in xf.values()]))
    return out


def ragged_cases():
    """Two ragged mixes over every M in 1..16: `ed` holds every family row (the end-derivative array
    is passed: classes M <= 11 / M >= 12, end-derivative rows in both), `rest` the rows without end
    derivatives (ED NULL: classes M <= 13 / M >= 14).  One row of three M per mix comes 34 times: a
    ragged tile holds 32 trajectories of one M, so wherever the shuffle puts them, two copies lie
    in different tiles of that M's group."""
    out = {}
    for case, names, many in (("ed", None, {5: "plain", 11: "twin", 12: "cubic"}),
                              ("rest", REST, {4: "zigzag", 13: "repeat_mid", 14: "one_axis_x"})):
        rows = {}
        for M in range(1, 17):
            fam = families(M)
            rows[M] = [fam[n] for n in (names or fam)]
            if M in many:
                rows[M] += [fam[many[M]]] * 33
        out[case] = ragged_mix(rows, seed=len(case))
    return out


# ------------------------------------------------------------------------------- the checks

def rel_err_rows(C, R):
    """conftest.batch_rel_err's quantity per trajectory of a uniform batch: C, R [B, M, 3, 8] ->
    [B], max over axes of max|dC| / max|R| (denominator 1 where R is identically 0)."""
    d = np.abs(C - R).max(axis=(1, 3))
    r = np.abs(R).max(axis=(1, 3))
    return (d / np.where(r == 0.0, 1.0, r)).max(axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Run:
    """One backend's results on the three uniform launches of one M.  solve(so, W, T, ED) ->
    (coeffs [S,3,8], status [B])."""

    def __init__(self, solve, M, what):
        self.M, self.what, self.out = M, what, {}
        for case, (labels, probs, (so, W, T, ED, src)) in cases(M).items():
            C, st = solve(so, W, T, ED)
            self.out[case] = (np.asarray(C).reshape(len(src), M, 3, 8), np.asarray(st))

    def row(self, case, label):
        """The first copy of a row: [M, 3, 8]."""
        return self.out[case][0][cases(self.M)[case][0].index(label)]


def reference_batch(case, M):
    labels, probs, (so, W, T, ED, src) = cases(M)[case]
    return np.stack([reference(probs[k]) for k in src])


def worst_by_family(labels, src, err):
    out = {}
    for k, name in enumerate(labels):
        out[family_of(name)] = max(out.get(family_of(name), 0.0), float(err[src == k].max()))
    return out


def check_exact(run, batch_rel_err):
    """1. Every family against the exact reference at 1e-9, status 0; on `cubic` also
    max|c4..c7| <= 1e-9 max|c| per (trajectory, axis).  Returns the worst value per family."""
    worst = {}
    for case in ("rest", "ed"):
        labels, probs, (so, W, T, ED, src) = cases(run.M)[case]
        C, st = run.out[case]
        R = reference_batch(case, run.M)
        assert (st == 0).all(), (run.what, case, st)
        worst.update(worst_by_family(labels, src, rel_err_rows(C, R)))
        assert batch_rel_err(so, C, R) <= TOL, (run.what, case, worst)
        if "cubic" in labels:
            k = src == labels.index("cubic")
            hi = np.abs(C[k][:, :, :, 4:8]).max(axis=(1, 3)) / np.abs(R[k]).max(axis=(1, 3))
            worst["cubic c4..c7"] = float(hi.max())
            assert (hi <= TOL).all(), (run.what, hi.max())
    print("%s M=%d exact: %s" % (run.what, run.M, "  ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    return worst


def check_placement(run):
    """2. All copies of a source row in one launch are bit-identical, coefficients and status."""
    for case, (C, st) in run.out.items():
        src = cases(run.M)[case][2][4]
        for k in range(int(src.max()) + 1):
            c, s = C[src == k], st[src == k]
            assert same_bits(c, np.broadcast_to(c[0], c.shape)) and (s == s[0]).all(), (run.what, case, k)


def check_scale_w(run):
    """3. scale_w(+-20) of plain and cubic: the base row's bits times 2^+-20."""
    for base in ("plain", "cubic"):
        for k in W_SCALES:
            label = "%s|scale_w%+d" % (base, k)
            assert same_bits(np.ldexp(run.row("xf", label), -k), run.row("xf", base)), (run.what, label)


def check_twin(run, bitwise=True):
    """4. Two axes with the same data give the same bits.  bitwise False (a kernel variant whose
    axes legitimately round in different orders): each axis within 1e-9 of the exact reference, and
    whether the bits agreed is printed."""
    c = run.row("ed", "twin")
    if bitwise:
        assert same_bits(c[:, 0], c[:, 1]), run.what
        return
    R = reference(families(run.M)["twin"])
    err = [float(np.abs(c[:, a] - R[:, a]).max() / np.abs(R[:, a]).max()) for a in (0, 1)]
    print("%s M=%d twin: x %.2e, y %.2e of the exact reference, bit-equal: %s"
          % (run.what, run.M, err[0], err[1], same_bits(c[:, 0], c[:, 1])))
    assert max(err) <= TOL, (run.what, err)


def check_still(run):
    """5. A constant axis: c1..c7 == 0.0 and c0 the waypoint, exactly; the moving axis has the bits
    of the same column solved with the other two axes moving (plain)."""
    fam = families(run.M)
    for label, axis in (("one_axis_x", 0), ("one_axis_z", 2)):
        c = run.row("rest", label)
        for a in set(range(3)) - {axis}:
            assert (c[:, a, 1:] == 0.0).all() and (c[:, a, 0] == fam[label].W[0, a]).all(), (run.what, label, a)
        assert same_bits(c[:, axis], run.row("rest", "plain")[:, axis]), (run.what, label)


def check_swap(run, bitwise=True):
    """6. Permuted axes give the permuted result bit for bit, all six permutations.  bitwise False (a
    kernel variant whose axes legitimately round in different orders): the permuted solve and the
    base solve each within 1e-9 of the exact reference, and whether the bits agreed is printed."""
    xf = transformed_rows(run.M)
    worst, equal = 0.0, True
    for base in ("plain", "cubic"):
        worst = max(worst, _xf_err(run, base))
        for perm in PERMS[1:]:
            label = "%s|swap%d%d%d" % ((base,) + perm)
            eq = same_bits(run.row("xf", label), xf[label][2](run.row("xf", base)))
            assert eq or not bitwise, (run.what, label)
            equal = equal and eq
            worst = max(worst, _xf_err(run, label))
    if not bitwise:
        print("%s M=%d axis permutations: worst %.2e of the exact reference, bit-equal: %s" % (run.what, run.M, worst, equal))
    assert worst <= TOL, (run.what, worst)


def _xf_err(run, label):
    """Norm-wise error of a transformed row against the exactly transformed reference."""
    base, p, fmap = transformed_rows(run.M)[label]
    R = fmap(reference(families(run.M)[base]))
    return float(rel_err_rows(run.row("xf", label)[None], R[None])[0])


def check_scale_t(run, bitwise):
    """7. scale_t(+-1): within 1e-9 of the exactly transformed reference; `bitwise` (the reduced
    method and the host backend, whose block LDL^T is homogeneous in T): the scaled bits of the
    base row.  Returns (worst error, every row bit-equal)."""
    xf = transformed_rows(run.M)
    worst, equal = 0.0, True
    for base in ("plain", "cubic"):
        for k in T_SCALES:
            label = "%s|scale_t%+d" % (base, k)
            worst = max(worst, _xf_err(run, label))
            eq = same_bits(run.row("xf", label), xf[label][2](run.row("xf", base)))
            equal = equal and eq
            assert eq or not bitwise, (run.what, label)
    print("%s M=%d scale_t: worst %.2e, bit-equal to the scaled base: %s" % (run.what, run.M, worst, equal))
    assert worst <= TOL, (run.what, worst)
    return worst, equal


def check_translate(run, displacement):
    """8. translate(2^20, -2^20, 2^19).  `displacement` (the reduced method and the host backend,
    which couple through w1 - w0): c0 == w_i exactly, c1..c7 the untranslated bits, and the shape
    bound ||(C - o e0) - C_ref||_inf <= 1e-9 ||C_ref||_inf per axis.  Otherwise (band, dense: the
    absolute waypoints are the right-hand side) the header's contract, norm-wise 1e-9 with c0
    included; the shape error is measured and returned, not bounded."""
    xf = transformed_rows(run.M)
    worst, shape = 0.0, 0.0
    for base in ("plain", "cubic"):
        label = "%s|translate" % base
        _, p, fmap = xf[label]
        c, R0 = run.row("xf", label), reference(families(run.M)[base])
        worst = max(worst, _xf_err(run, label))
        back = np.array(c)
        back[..., 0] -= fmap(np.zeros((3, 8)))[..., 0]   # exact where c0 is a translated waypoint
        shape = max(shape, float(rel_err_rows(back[None], R0[None])[0]))
        if displacement:
            assert np.array_equal(c[:, :, 0], p.W[:-1]), (run.what, label)
            assert same_bits(c[:, :, 1:], run.row("xf", base)[:, :, 1:]), (run.what, label)
    print("%s M=%d translate: norm-wise with the offset %.2e, shape %.2e of the untranslated norm"
          % (run.what, run.M, worst, shape))
    assert worst <= TOL, (run.what, worst)
    assert shape <= TOL or not displacement, (run.what, shape)
    return worst, shape


def check_ragged(solve, batch_rel_err, what):
    """Both ragged mixes: every row against the exact reference at 1e-9, status 0, and all copies
    of a row (34 of some: at least two tiles of their M's group) bit-identical."""
    worst = {}
    for case, (so, W, T, ED, order, flat) in ragged_cases().items():
        C, st = solve(so, W, T, ED)
        C, st = np.asarray(C).reshape(-1, 3, 8), np.asarray(st)
        assert (st == 0).all(), (what, case)
        R = np.concatenate([reference(flat[k]) for k in order])
        worst[case] = batch_rel_err(so, C, R)
        seen = {}
        for b, k in enumerate(order):
            c = C[so[b]:so[b + 1]]
            first = seen.setdefault(flat[k].key, c)
            assert same_bits(c, first), (what, case, b)
        assert (ED is None) == (case == "rest") and len(seen) < len(order) - 90
    print("%s ragged: %s" % (what, "  ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= TOL, (what, worst)
    return worst
