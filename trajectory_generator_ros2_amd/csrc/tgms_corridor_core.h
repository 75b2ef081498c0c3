// tgms_corridor_core.h — corridor containment of one segment against one face, and the folds
// above it, shared by the gfx950 kernel (tgms_corridor.hip) and the host backend
// (tgms_host.cpp).  Plain C++17, as its siblings: the derivative ladder, the Horner chain and
// ffact are tgms_bounds_core.h's, the rule for a candidate's global time
// tgms_clearance_core.h's (written out here as in tgms_thrust_core.h).
//
// The quantity.  A face is n[3] d, a point inside it when n . p <= d.  On a segment, in
// normalised time u = t / T (a_ax,j = c_ax,j T^j),
//     q(u) = n . p(u) - d
// is a polynomial of degree 7 on [0, 1], and its maximum is the best of q(0), q(1) and q at the
// real roots of q' inside.
//   - Candidates.  q' has the coefficients f_k = (k + 1) sum_ax n_ax a_ax,k+1, k = 0..6: the
//     segment's normalised coefficients projected onto n.  bounds::Ladder<6, 6> on f gives six
//     slots: the located roots, and duplicates of breakpoints where an interval holds none.
//     The candidates are u = 0, the six slots and u = 1, taken in that order with a strict
//     comparison.
//   - Values.  Every value is evaluated from the three axis polynomials at the candidate:
//     three Horner chains p_x, p_y, p_z, then fma(n_z, p_z, fma(n_y, p_y, fma(n_x, p_x, -d))).
//     The projected coefficients only locate candidates.  A constant trajectory therefore
//     gives n . p0 - d with exactly that rounding at every candidate, and a waypoint lying on a
//     face gives what the end-point evaluation gives (at u = 0 the Horner chain returns c_0
//     itself).
//   - Error.  The argument of tgms_bounds_core.h carries over: q is stationary at its located
//     roots, so a slot off by 2^-41 moves the value by < 1.2e-20 max|q|; what remains is the
//     rounding of three degree-7 Horner chains and three FMAs, a few ulp of
//     L = sum_a |n_a| max|p_a| + |d|, against the 1e-9 L of tgms.h.
//   - Not a certificate, and a touch without a sign change may be skipped, as for the bounds.
// The folds.  (margin, segment, face) is a total order: the larger margin, then the lower
// segment, then the lower face index.  Both folds compare whole keys, so any order of taking
// the items gives the same winner; the kernel and the host take them in ascending order.
#pragma once

#include "tgms_bounds_core.h"

namespace tgms {
namespace corridor {

// A face that can be used: four finite entries and a normal that is not all zero.
TGMS_HD bool face_ok(double nx, double ny, double nz, double d) {
    const double chk = __builtin_fma(nx, 0.0, __builtin_fma(ny, 0.0, __builtin_fma(nz, 0.0, d * 0.0)));
    return chk == 0.0 && (nx != 0.0 || ny != 0.0 || nz != 0.0);
}

// A face span that can be used: faces a .. b-1 of F, at most TGMS_COR_MAX_FACES of them.
TGMS_HD bool span_ok(int64_t a, int64_t b, int64_t F) {
    return a >= 0 && b >= a && b <= F && b - a <= (int64_t)TGMS_COR_MAX_FACES;
}

// One (segment, face) item: the largest n . p(u) - d over the candidates and the u that
// attains it.  c [3][8] are the caller's coefficients on t in [0, T].  A candidate value that
// is not finite makes m NaN.
TGMS_HD void item(const double* c, double T, double nx, double ny, double nz, double d, double& m, double& um) {
    double a[3][8], f[7], s[6];
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double w = 1.0;
        a[ax][0] = c[ax * 8];
        TGMS_UNROLL
        for (int j = 1; j < 8; ++j) {
            w *= T;
            a[ax][j] = c[ax * 8 + j] * w;
        }
    }
    TGMS_UNROLL
    for (int j = 1; j < 8; ++j)
        f[j - 1] = (double)j * __builtin_fma(nz, a[2][j], __builtin_fma(ny, a[1][j], nx * a[0][j]));
    bounds::Ladder<6, 6>::run(f, s);
    auto value = [&](double u) {
        const double x = bounds::horner<7>(a[0], u), y = bounds::horner<7>(a[1], u), z = bounds::horner<7>(a[2], u);
        return __builtin_fma(nz, z, __builtin_fma(ny, y, __builtin_fma(nx, x, -d)));
    };
    m = value(0.0);
    um = 0.0;
    double chk = m * 0.0;
    TGMS_UNROLL
    for (int j = 0; j <= 6; ++j) {
        const double u = j < 6 ? s[j] : 1.0;
        const double v = value(u);
        chk = __builtin_fma(v, 0.0, chk);
        um = v > m ? u : um;
        m = v > m ? v : m;
    }
    if (chk != 0.0) m = __builtin_nan("");
}

// A segment's running best over its faces.  face: an index into faces, TGMS_NEAR_NONE before
// the first item.  A face that was left out is never offered.
struct SegBest {
    double m, u;
    int32_t face;
    bool bad;  // an item's result was not finite
};

TGMS_HD SegBest seg_init() { return SegBest{-__builtin_inf(), 0.0, TGMS_NEAR_NONE, false}; }

TGMS_HD void seg_take(SegBest& b, double m, double u, int32_t face) {
    b.bad = b.bad || !(m == m);
    const bool better = m > b.m || (m == b.m && (b.face < 0 || face < b.face));
    b.m = better ? m : b.m;
    b.u = better ? u : b.u;
    b.face = better ? face : b.face;
}

// The global time of a segment's stored value: the knot's prefix sum plus the local time,
// clamped to the duration; 0.0 for a segment with no face.
TGMS_HD double time_of(int32_t face, double knot, double T, double u, double D) {
    return face < 0 ? 0.0 : fmin(__builtin_fma(T, u, knot), D);
}

// A trajectory's running best over its segments, with what the time of the winner needs.
struct Fold {
    double m, knot, T, u;
    int32_t seg, face;
    double next;  // the left-to-right prefix sum of T: the next segment's knot, the duration at the end
    bool bad;
};

TGMS_HD Fold fold_init() { return Fold{-__builtin_inf(), 0.0, 0.0, 0.0, TGMS_NEAR_NONE, TGMS_NEAR_NONE, 0.0, false}; }

// Offers segment `seg` (its local index) to the fold, at the knot f.next.
TGMS_HD void fold(Fold& f, const SegBest& s, int32_t seg, double T) {
    f.bad = f.bad || s.bad || !(s.m == s.m);
    const bool better =
        s.face >= 0 && (s.m > f.m || (s.m == f.m && (f.face < 0 || seg < f.seg || (seg == f.seg && s.face < f.face))));
    f.m = better ? s.m : f.m;
    f.knot = better ? f.next : f.knot;
    f.T = better ? T : f.T;
    f.u = better ? s.u : f.u;
    f.seg = better ? seg : f.seg;
    f.face = better ? s.face : f.face;
    f.next += T;
}

// The record, the place and the flags of one trajectory from its fold.  bad: an input was
// not finite, a time not positive, a face span or the segment count unusable; bad_face: a
// face of the trajectory was left out.  A strict comparison on the very value stored.
TGMS_HD int finish(const Fold& f, bool bad, bool bad_face, double r, double (&rec)[TGMS_COR_STRIDE],
                   int32_t (&where)[2]) {
    const double D = f.next;
    rec[0] = f.m;
    rec[1] = time_of(f.face, f.knot, f.T, f.u, D);
    where[0] = f.seg;
    where[1] = f.face;
    const double fin = __builtin_fma(rec[1], 0.0, D * 0.0);  // m may be -inf: no face anywhere
    if (bad || f.bad || fin != 0.0 || !(rec[0] == rec[0])) {
        rec[0] = rec[1] = __builtin_nan("");
        where[0] = where[1] = TGMS_NEAR_NONE;
        return TGMS_FEAS_NONFINITE;
    }
    int fl = bad_face ? TGMS_COR_BAD_FACE : 0;
    fl |= rec[0] > -r ? TGMS_COR_OUTSIDE : 0;
    return fl;
}

// A segment's row: its margin, the global time and the face; NaN NaN TGMS_NEAR_NONE where the
// trajectory is unusable.
TGMS_HD void seg_row(const SegBest& s, double knot, double T, double D, bool bad, double& m, double& t,
                     int32_t& face) {
    m = bad ? __builtin_nan("") : s.m;
    t = bad ? __builtin_nan("") : time_of(s.face, knot, T, s.u, D);
    face = bad ? TGMS_NEAR_NONE : s.face;
}

}  // namespace corridor
}  // namespace tgms
