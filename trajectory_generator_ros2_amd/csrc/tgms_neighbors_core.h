// tgms_neighbors_core.h — the broad phase of the swarm neighbour search, shared by the gfx950
// kernels (tgms_neighbors.hip) and the host backend (tgms_host.cpp).  Plain C++17, as
// tgms_bounds_core.h and tgms_separation_core.h, whose merge rule and records it uses.
//
// The question is which ordered pairs (i, j) can have a closest approach below r_min; all
// others never reach the degree-13 ladder of separation::interval_item.  The answer is a
// lower bound of the distance from axis-aligned boxes.
//
// Boxes.  Vehicle b has M + 2 boxes of 6 doubles (lo[3], hi[3]), indexed as
// separation::merge_knots counts a side: 0 is the held start p(0) of the first segment, m + 1
// is segment m, M + 1 is the held end p(T_last) of the last segment.
//   - Segment box: with a_k = c_k Tb^k the Bernstein control values of degree 7 are
//     b_i = sum_{k<=i} C(i,k)/C(7,k) a_k, and p([0, Tb]) lies in [min_i b_i, max_i b_i]
//     (convex hull property; no root finding, 36 FMAs an axis).
//   - Tb is not always T.  The narrow phase evaluates a candidate at the local time
//     ti = fma(hs, v, la), v in [0, 1], la = fl(a - k_m) >= 0, hs = fl(b - a), a <= b <= k_{m+1}
//     two of the side's rounded global knots, so ti <= (k_{m+1} - k_m)(1 + eps)^2 (eps =
//     2^-53), and the knot difference is T only up to eps times the knots' magnitude, which a
//     late start time makes large against T.  Tb = max(T, fl(k_{m+1} - k_m)(1 + 2^-49)) covers
//     every local time that can be evaluated; the held end is evaluated at T <= Tb.
//   - Margin.  The box must hold the values the narrow phase COMPUTES, not the exact curve.
//     With S = sum_k |c_k| Tb^k (>= sum_k |c_k| t^k on [0, Tb]):
//       conversion:  Tb^k by repeated products (k - 1) eps, a_k one more, the weight's
//         rounding one, the sum of at most 8 FMA terms 8: |b_i computed - b_i| <= 17 eps S;
//       evaluation:  a degree-7 Horner chain of FMAs is within 2 * 7 eps S of p(t);
//       the subtraction / addition of the margin itself: eps S.
//     That is 32 eps S; every box is widened outward by MARGIN * S = 64 eps S on each side.
//   - Held ends: the point c_0 (Horner at 0 returns it exactly) and the point horner<7>(c,
//     T_last), the chain the narrow phase runs, each widened by the same MARGIN * S.
//   - The union box of a vehicle is the hull of all its boxes.
// Lower bound.  gap2 = sum_a (s_a max(0, lo_i - hi_j, lo_j - hi_i))^2.  The narrow phase's
// value is fl(sum_a fl(s_a fl(p_i - p_j))^2) >= (true gap)^2 (1 - 8 eps) and the computed gap2
// is <= (true gap)^2 (1 + 8 eps); sqrt and r_min^2 round once each, and the flag compares
// sqrt(best) < r_min.  A pair is culled only when gap2 >= r_min^2 (1 + R2_SLACK) on every
// interval, R2_SLACK = 64 eps > (8 + 8 + 4 + 1) eps: then the stored d_min is >= r_min.
// Walk.  The intervals of a pair are those of separation::merge_knots on the two rounded knot
// lists: the walk replays its take rule entry by entry (counted, not compared by value), so
// interval q pairs the same two box indices (mi, mj) that the narrow phase unpacks from
// seg[q].  It keeps no array: a lane holds two counters.  Zero-length intervals are walked
// too (the narrow phase gives them +inf, so that is conservative).
// Soundness is the contract (a pair with d_min < r_min is never culled); tightness is
// measured, not promised: a Bernstein hull is exact for straight lines and loose for a
// segment that turns.
#pragma once

#include <stdint.h>

#include "tgms_separation_core.h"

namespace tgms {
namespace neighbors {

constexpr int BOXES = TGMS_MAX_SEGMENTS + 2;       // held start, the segments, held end
constexpr int BOX_STRIDE = 6;                      // lo[3] hi[3]
constexpr int KNOT_STRIDE = TGMS_MAX_SEGMENTS + 2; // knots [0..M], T_last in the last slot
constexpr int TLAST = KNOT_STRIDE - 1;
constexpr double MARGIN = 0x1p-47;    // 64 eps, eps = 2^-53
constexpr double R2_SLACK = 0x1p-47;  // 64 eps
constexpr double T_SLACK = 0x1p-49;

constexpr double binom(int n, int k) {
    double r = 1.0;
    for (int i = 0; i < k; ++i) r = r * (double)(n - i) / (double)(i + 1);
    return r;
}

// r_min^2 with the slack of the cull test.
TGMS_HD double cull_r2(double r_min) { return r_min * r_min * (1.0 + R2_SLACK); }

// The box of one segment (c [3][8] on [0, T], kd the rounded difference of its two global
// knots) into box[6]; S[3] receives the margin's scale per axis.  chk stays 0 while every
// coefficient is finite.
TGMS_HD void segment_box(const double* c, double T, double kd, double* box, double (&S)[3], double& chk) {
    const double Tb = fmax(T, kd * (1.0 + T_SLACK));
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double a[8], w = 1.0, s = 0.0;
        TGMS_UNROLL
        for (int k = 0; k < 8; ++k) {
            a[k] = c[ax * 8 + k] * w;
            chk = __builtin_fma(c[ax * 8 + k], 0.0, chk);
            s += fabs(a[k]);
            w *= Tb;
        }
        double lo = a[0], hi = a[0];
        TGMS_UNROLL
        for (int i = 1; i < 8; ++i) {
            double b = a[0];
            TGMS_UNROLL
            for (int k = 1; k <= i; ++k) b = __builtin_fma(binom(i, k) / binom(7, k), a[k], b);
            lo = fmin(lo, b);
            hi = fmax(hi, b);
        }
        S[ax] = s;
        box[ax] = lo - MARGIN * s;
        box[3 + ax] = hi + MARGIN * s;
    }
}

// The box of a held point p[3].
TGMS_HD void point_box(const double (&p)[3], const double (&S)[3], double* box) {
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        box[ax] = p[ax] - MARGIN * S[ax];
        box[3 + ax] = p[ax] + MARGIN * S[ax];
    }
}

TGMS_HD void hull(const double* box, double (&u)[BOX_STRIDE]) {
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        u[ax] = fmin(u[ax], box[ax]);
        u[3 + ax] = fmax(u[3 + ax], box[3 + ax]);
    }
}

// Everything the broad phase keeps of one vehicle: its global knots (kn [KNOT_STRIDE], the last
// time in slot TLAST), its boxes (bx [M + 2][6]) and their hull (ub [6]).  The knots are formed
// as the narrow phase forms them: start + (left-to-right prefix sum).  Returns false, with
// unspecified contents, when the vehicle is unusable: a segment count outside
// 1..TGMS_MAX_SEGMENTS (nothing is read then), a time that is not > 0, a start time, knot or
// coefficient that is not finite.
TGMS_HD bool vehicle_boxes(int M, const double* C, const double* T, double start, double* kn, double* bx, double* ub) {
    if (M < 1 || M > TGMS_MAX_SEGMENTS) return false;
    double chk = start * 0.0, acc = 0.0, prev = start;
    bool neg = false;
    double u[BOX_STRIDE] = {HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    kn[0] = start;
    for (int m = 0; m < M; ++m) {
        const double t = T[m];
        neg = neg || !(t > 0.0);
        acc += t;  // the same order as the extrema record's duration
        const double k = start + acc;
        chk = __builtin_fma(k, 0.0, chk);
        kn[m + 1] = k;
        const double* c = C + m * 24;
        double S[3];
        double* box = bx + (m + 1) * BOX_STRIDE;
        segment_box(c, t, k - prev, box, S, chk);
        hull(box, u);
        if (m == 0) {
            const double p[3] = {c[0], c[8], c[16]};
            point_box(p, S, bx);
            hull(bx, u);
        }
        if (m == M - 1) {
            double p[3];
            TGMS_UNROLL
            for (int ax = 0; ax < 3; ++ax) {
                double q[8];
                TGMS_UNROLL
                for (int j = 0; j < 8; ++j) q[j] = c[ax * 8 + j];
                p[ax] = bounds::horner<7>(q, t);
            }
            point_box(p, S, bx + (M + 1) * BOX_STRIDE);
            hull(bx + (M + 1) * BOX_STRIDE, u);
            kn[TLAST] = t;
        }
        prev = k;
    }
    TGMS_UNROLL
    for (int q = 0; q < BOX_STRIDE; ++q) {
        ub[q] = u[q];
        chk = __builtin_fma(u[q], 0.0, chk);
    }
    return !neg && chk == 0.0;
}

// Squared scaled distance of two boxes, a lower bound of the squared scaled distance of any
// two points in them.
TGMS_HD double gap2(const double* bi, const double* bj, const double (&scale)[3]) {
    double acc = 0.0;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        const double g = scale[ax] * fmax(0.0, fmax(bi[ax] - bj[3 + ax], bj[ax] - bi[3 + ax]));
        acc = __builtin_fma(g, g, acc);
    }
    return acc;
}

// True when some interval of the pair's merged knot list has gap2 < r2: the pair goes to the
// narrow phase.  The loop is separation::merge_knots' (the same operands, the same take rule,
// the same clamped reads), with the box test in the place of its two stores.
TGMS_HD bool walk(const double* ki, int Mi, const double* bxi, const double* kj, int Mj, const double* bxj,
                  const double (&scale)[3], double r2) {
    int mi = 0, mj = 0;
    const int n = Mi + Mj + 2;
    bool hit = false;
    for (int q = 0; q < n - 1; ++q) {
        const double a = ki[mi <= Mi ? mi : Mi], b = kj[mj <= Mj ? mj : Mj];
        const bool take_i = mj > Mj || (mi <= Mi && a <= b);
        mi += take_i ? 1 : 0;
        mj += take_i ? 0 : 1;
        // interval q: side i is in box mi (0: before its first knot .. Mi + 1: after its last)
        hit = hit || gap2(bxi + mi * BOX_STRIDE, bxj + mj * BOX_STRIDE, scale) < r2;
    }
    return hit;
}

// The running result of one row and its order-free update.
struct Row {
    double d, t;  // the stored d_min, t_min of the nearest neighbour so far; d = +inf: none
    int32_t nbr, count, tested;
    bool bad;  // a result of this row was not finite
};
TGMS_HD Row row_init() { return Row{HUGE_VAL, 0.0, TGMS_NEAR_NONE, 0, 0, false}; }
// rec, fl: separation::finish of the ordered pair (row, j), run with the row's r_min.
TGMS_HD void row_update(Row& r, int32_t j, const double (&rec)[TGMS_SEP_STRIDE], int fl) {
    r.tested += 1;
    r.bad = r.bad || (fl & TGMS_SEP_NONFINITE) != 0;
    if (fl & TGMS_SEP_CLOSE) {
        r.count += 1;
        const bool better = rec[0] < r.d || (rec[0] == r.d && j < r.nbr) || r.nbr < 0;
        r.t = better ? rec[1] : r.t;
        r.nbr = better ? j : r.nbr;
        r.d = better ? rec[0] : r.d;
    }
}
// The outputs of a row; usable: the vehicle itself passed vehicle_boxes.
TGMS_HD int row_finish(const Row& r, bool usable, double (&rec)[TGMS_SEP_STRIDE], int32_t& nbr, int32_t& count) {
    if (!usable || r.bad) {
        rec[0] = rec[1] = __builtin_nan("");
        nbr = TGMS_NEAR_NONE;
        count = 0;
        return TGMS_SEP_NONFINITE;
    }
    rec[0] = r.d;
    rec[1] = r.t;
    nbr = r.nbr;
    count = r.count;
    return r.count > 0 ? TGMS_SEP_CLOSE : 0;
}

}  // namespace neighbors
}  // namespace tgms
