// tgms_separation_core.h — closest approach of a pair of trajectories, shared by the gfx950
// kernel (tgms_separation.hip) and the host backend (tgms_host.cpp).  Plain C++17, as
// tgms_bounds_core.h, whose derivative ladder and Horner chain it uses.
//
// Trajectory b lives on the global interval [t0_b, t0_b + D_b]; its knots are k_b[m] = t0_b +
// (left-to-right prefix sum of its first m times), and outside the interval it holds its
// nearest end point.  Between two consecutive entries a <= b of the merged knot list of a
// pair each side is one polynomial (its active segment) or one constant (a held end), so the
// squared scaled distance is a polynomial of degree <= 14 in u = (t - a) / (b - a):
//   - each side's axis polynomials are Taylor-shifted to the side's local time at a and
//     scaled by (b - a)^k (a held side keeps its constant only);
//   - e[3][8] is the scaled difference, f the 14 coefficients of the derivative of
//     sum_a e_a^2 (formed as bounds::norm_item forms its f);
//   - bounds::Ladder<13, 13> leaves 13 slots holding the stationary points found in [0, 1];
//   - the candidates 0, 1 and the 13 slots are evaluated FROM EACH SIDE'S OWN SEGMENT
//     POLYNOMIAL AT ITS OWN LOCAL TIME.  The shifted and convolved coefficients only locate
//     the candidates; the value's error is the rounding of two Horner chains, and two
//     identical trajectories with equal start times give exactly 0.0.
// The error argument of tgms_bounds_core.h carries over with n = 14: a root off by delta =
// 2^-41 moves the value at a stationary point by <= (2/3) 14^2 (14^2 - 1) delta^2 max|Q| <
// 5.3e-21 max|Q|.  The ladder's coefficients are f's times falling factorials up to 13!, all
// exact in fp64.
// A zero-length interval (coincident knots) has every coefficient of degree >= 1 equal to
// zero, so nothing is bisected; it contributes no candidate (its end point belongs to its
// neighbours) but still reports a non-finite coefficient of its segments, so that every
// segment of both trajectories is looked at by at least one interval.
#pragma once

#include <stdint.h>

#include "tgms_bounds_core.h"

namespace tgms {
namespace separation {

constexpr int MAX_KNOTS = TGMS_MAX_SEGMENTS + 1;  // of one trajectory
constexpr int MAX_MERGED = 2 * MAX_KNOTS;         // of a pair
constexpr int MAX_INTERVALS = MAX_MERGED - 1;     // 33

// Pair n of the all-pairs order (0,1), (0,2), ..., (0,B-1), (1,2), ... of B >= 2 trajectories,
// 0 <= n < P = B (B - 1) / 2.  Counted from the end the rows have 1, 2, 3, ... pairs, so the
// row is a triangular root: an fp64 estimate (8 r + 1 < 2^64, its root is off by far less
// than 1) and two exact integer corrections either way.
TGMS_HD void decode_pair(int64_t n, int32_t B, int64_t P, int32_t& i, int32_t& j) {
    const int64_t r = P - 1 - n;
    int64_t k = (int64_t)((sqrt(8.0 * (double)r + 1.0) - 1.0) * 0.5);
    TGMS_UNROLL
    for (int it = 0; it < 2; ++it) k -= (k * (k + 1) / 2 > r) ? 1 : 0;
    TGMS_UNROLL
    for (int it = 0; it < 2; ++it) k += ((k + 1) * (k + 2) / 2 <= r) ? 1 : 0;
    i = (int32_t)((int64_t)B - 2 - k);
    j = (int32_t)((int64_t)B - 1 - (r - k * (k + 1) / 2));
}

// Stable merge of the knots ki[0..Mi] and kj[0..Mj] (each ascending) into mk[0..Mi+Mj+1].
// seg[q] describes interval q = [mk[q], mk[q+1]], q = 0..Mi+Mj: (si + 1) | (sj + 1) << 8 with
// s the side's active segment, -1 before its first knot and M after its last.  The segment is
// counted from the entries taken, not compared by value, so every segment of either side
// owns at least one interval, whatever the rounding of the knots.
TGMS_HD void merge_knots(const double* ki, int Mi, const double* kj, int Mj, double* mk, int32_t* seg) {
    int mi = 0, mj = 0;
    const int n = Mi + Mj + 2;
    for (int q = 0; q < n; ++q) {
        const double a = ki[mi <= Mi ? mi : Mi], b = kj[mj <= Mj ? mj : Mj];
        const bool take_i = mj > Mj || (mi <= Mi && a <= b);
        mk[q] = take_i ? a : b;
        mi += take_i ? 1 : 0;
        mj += take_i ? 0 : 1;
        if (q < n - 1) seg[q] = mi | (mj << 8);
    }
}

// One side of one interval: the segment whose polynomial is read, the local time at u = 0
// and the local time per unit of u (0 for a held end).
struct Side {
    int seg;
    double la, hs;
};
// k: the side's knots [M + 1], T_last its last time; s in -1..M as merge_knots counts it.
TGMS_HD Side side_of(int s, int M, const double* k, double T_last, double a, double h) {
    Side r;
    const bool before = s < 0, after = s >= M;
    r.seg = before ? 0 : (after ? M - 1 : s);
    r.la = before ? 0.0 : (after ? T_last : a - k[r.seg]);
    r.hs = (before || after) ? 0.0 : h;
    return r;
}

// p(la + hs u) of one axis as coefficients in u.
TGMS_HD void shift_axis(const double (&c)[8], double la, double hs, double (&q)[8]) {
    TGMS_UNROLL
    for (int k = 0; k < 8; ++k) q[k] = c[k];
    TGMS_UNROLL
    for (int i = 0; i < 7; ++i) {
        TGMS_UNROLL
        for (int k = 6; k >= i; --k) q[k] = __builtin_fma(la, q[k + 1], q[k]);
    }
    double w = 1.0;
    TGMS_UNROLL
    for (int k = 1; k < 8; ++k) {
        w *= hs;
        q[k] *= w;
    }
}

// The minimum of the squared scaled distance over one interval of length h >= 0: ci, cj are
// the sides' segment coefficients [3][8].  d2 = +inf for a zero-length interval, NaN when a
// coefficient read is not finite; u in [0, 1] is where d2 is attained.
TGMS_HD void interval_item(const double* ci, const Side& si, const double* cj, const Side& sj,
                           const double (&scale)[3], double h, double& d2, double& u) {
    double pi[3][8], pj[3][8], e[3][8];
    double chk = 0.0;  // 0 while every coefficient is finite
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        TGMS_UNROLL
        for (int k = 0; k < 8; ++k) {
            pi[ax][k] = ci[ax * 8 + k];
            pj[ax][k] = cj[ax * 8 + k];
            chk = __builtin_fma(pi[ax][k], 0.0, chk);
            chk = __builtin_fma(pj[ax][k], 0.0, chk);
        }
        double qi[8], qj[8];
        shift_axis(pi[ax], si.la, si.hs, qi);
        shift_axis(pj[ax], sj.la, sj.hs, qj);
        TGMS_UNROLL
        for (int k = 0; k < 8; ++k) e[ax][k] = scale[ax] * (qi[k] - qj[k]);
    }
    double f[14], s[13];
    TGMS_UNROLL
    for (int m = 1; m <= 14; ++m) {  // f[m-1] = m * (coefficient m of sum_ax e_ax^2)
        double acc = 0.0;
        TGMS_UNROLL
        for (int i = 0; i <= 7; ++i) {
            const int k = m - i;
            if (k >= 0 && k <= 7) {
                TGMS_UNROLL
                for (int ax = 0; ax < 3; ++ax) acc = __builtin_fma(e[ax][i], e[ax][k], acc);
            }
        }
        f[m - 1] = (double)m * acc;
    }
    bounds::Ladder<13, 13>::run(f, s);
    auto dist2 = [&](double v) {
        const double ti = __builtin_fma(si.hs, v, si.la), tj = __builtin_fma(sj.hs, v, sj.la);
        double acc = 0.0;
        TGMS_UNROLL
        for (int ax = 0; ax < 3; ++ax) {
            const double d = scale[ax] * (bounds::horner<7>(pi[ax], ti) - bounds::horner<7>(pj[ax], tj));
            acc = __builtin_fma(d, d, acc);
        }
        return acc;
    };
    double best = dist2(0.0), at = 0.0;
    TGMS_UNROLL
    for (int j = 0; j <= 13; ++j) {
        const double v = j < 13 ? s[j] : 1.0;
        const double d = dist2(v);
        at = d < best ? v : at;
        best = d < best ? d : best;
    }
    d2 = chk != 0.0 ? __builtin_nan("") : (h > 0.0 ? best : __builtin_inf());
    u = at;
}

// Left-to-right fold of a pair's intervals: (d2, t) of interval q beats the running minimum
// only when strictly smaller; a NaN d2 marks the pair.
TGMS_HD void fold(double d2, double t, double& best, double& at, bool& bad) {
    bad = bad || !(d2 == d2);
    at = d2 < best ? t : at;
    best = d2 < best ? d2 : best;
}

// The record and the flag word of one pair from its folded minimum; bad: an index, a count,
// a time or a coefficient ruled the pair out.  The comparison is strict, on the stored value.
TGMS_HD int finish(double best, double at, bool bad, double r_min, double (&rec)[TGMS_SEP_STRIDE]) {
    rec[0] = sqrt(best);
    rec[1] = at;
    const double fin = __builtin_fma(rec[0], 0.0, rec[1] * 0.0);
    if (bad || fin != 0.0) {
        rec[0] = rec[1] = __builtin_nan("");
        return TGMS_SEP_NONFINITE;
    }
    return (r_min > 0.0 && rec[0] < r_min) ? TGMS_SEP_CLOSE : 0;
}

}  // namespace separation
}  // namespace tgms
