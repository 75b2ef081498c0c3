// tgms_clearance_core.h — distance of a trajectory to static axis-aligned boxes, shared by the
// gfx950 kernels (tgms_clearance.hip) and the host backend (tgms_host.cpp).  Plain C++17, as
// its siblings: the derivative ladder and the Horner chain are tgms_bounds_core.h's, the
// boxes, the cull test and the row record tgms_neighbors_core.h's, the pair's fold and finish
// tgms_separation_core.h's.
//
// The value.  Obstacle k is the box [lo, hi] (lo == hi allowed per axis).  At the local time t
// of a segment the squared scaled distance is
//     d2(t) = sum_a (s_a max(lo_a - p_a(t), 0, p_a(t) - hi_a))^2,
// which is C^1 on the segment but only piecewise polynomial: each axis is in one of three
// states, below lo (e_a = lo_a - p_a), inside (0) or above hi (e_a = p_a - hi_a).
//
// Exact phase.  The segment is NOT cut at the times an axis changes state.  For a combination
// A of states that is not all-inside, Q_A = sum_{a active} (s_a e_a)^2 is one polynomial of
// degree <= 14 in u = t / T on the whole of [0, 1].  Since d/dx max(0, x)^2 = 2 max(0, x) x',
// (d2)' = Q_A' wherever A is the active combination, also at a time where an axis sits exactly
// on a face (its term and its derivative both vanish there, for either neighbouring state).
// So every interior local minimum of d2 is a root of Q_A' for a combination active there, and
// every time an axis crosses a face is a root of the single-axis combination's Q' = 2 s^2 e e'
// (e changes sign, e' does not): this is how a penetration is found, as the time the
// trajectory enters the box.  The candidates of a (segment, obstacle) item are therefore
// u = 0, u = 1 and the 13 slots of bounds::Ladder<13, 13> on Q_A' for each admissible A, and
// the result is the least of the TRUE clamped d2 over them, evaluated by bounds::horner<7> on
// the segment's own coefficients at the local time fl(u T), never from the convolved
// coefficients (the rule separation::interval_item states): the polynomials only locate
// candidates, a candidate of a combination that is not active where it lies costs an
// evaluation and cannot lower the result below the true minimum.
//   - Admissible combinations come from the segment's Bernstein box (neighbors::segment_box,
//     which holds every value the Horner chain can return on [0, T]): an axis can be below
//     only if the box reaches below lo_a, above only if it reaches above hi_a, inside only if
//     it meets [lo_a, hi_a].  A far or one-sided obstacle leaves one to three combinations;
//     only a small obstacle inside a turning segment's box pays all 26.  When all-inside is
//     the only one (the segment's box lies in the obstacle) it is kept, so that the two end
//     points are still evaluated; Q is 0 then and nothing is bisected.
//   - Error.  The argument of tgms_bounds_core.h carries over with n = 14 as in the
//     separation core: a root off by delta = 2^-41 moves the value at a stationary point by
//     <= (2/3) 14^2 (14^2 - 1) delta^2 max|Q| < 5.3e-21 max|Q|; the value's error is the
//     rounding of three Horner chains.  At a face crossing d2 is not stationary in Q_A but is
//     0 beyond it: a root off by delta leaves d2 <= (s e' delta)^2, so a trajectory that
//     passes through a box reports a d_min of that size, not 0.0 to the bit, unless an end
//     point lies inside.  The ladder's coefficients are f's times falling factorials up to
//     13!, all exact in fp64.
//   - Settling.  A slot is the middle of a bracket of 2^-40 in u, so the chosen candidate may
//     lie on either side of a state change by half of that: just short of a face, where the
//     axis still adds a term that rounds away, instead of just beyond it, where the axis adds
//     exactly nothing.  The winner of a combination is therefore looked at once more at u -
//     2^-40 and u + 2^-40 (clamped to [0, 1]) and moved there when the value is smaller, or
//     equal with fewer axes outside the obstacle's extent: the place where the stored value
//     is attained exactly.  A flat minimum along a face is then reported inside the flat
//     stretch, and a penetration found as an entry time mostly reports 0.0 from inside.
//   - A touch without a sign change may be skipped, as tgms.h allows for the bounds: two roots
//     of Q_A' within O(delta) of each other (a face grazed tangentially) can hide behind a
//     breakpoint; the values there differ from a neighbouring candidate's by O(delta^3).
//
// Broad phase.  neighbors::vehicle_boxes with start 0 gives the trajectory's hull, knots and
// per-segment boxes (the two held-end point boxes lie on the curve and are harmless in the
// hull).  An obstacle is culled per trajectory when neighbors::gap2(hull, obstacle) >=
// neighbors::cull_r2(r_min), and per segment by the segment's box.  MARGIN and R2_SLACK still
// cover this narrow phase: the trajectory side evaluates the same Horner chain at a local
// time fl(u T) <= T <= Tb, which is what MARGIN was sized for; the obstacle side is exact
// data, so it needs no margin; the computed value is fl(sum_a fl(s_a fl(bound - p))^2), one
// subtraction, one product, one square and the sum per axis, the very operation count of
// fl(sum_a fl(s_a fl(p_i - p_j))^2) that R2_SLACK = 64 eps bounds with (8 + 8 + 4 + 1) eps.
// So an obstacle whose stored d_min would be < r_min is never culled.
#pragma once

#include <stdint.h>

#include "tgms_neighbors_core.h"

namespace tgms {
namespace clearance {

constexpr int OBS_STRIDE = 6;  // lo[3] hi[3]
constexpr int COMBOS = 27;     // 3 states on 3 axes; index sx * 9 + sy * 3 + sz, state 0 below, 1 inside, 2 above
constexpr int ALL_INSIDE = 13;
constexpr double SETTLE = 0x1p-40;  // the ladder's bracket: a root lies within half of it of its slot

// Usable: every entry finite and lo <= hi on every axis.
TGMS_HD bool obstacle_ok(const double* ob) {
    double chk = 0.0;
    bool ordered = true;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        chk = __builtin_fma(ob[ax], 0.0, __builtin_fma(ob[3 + ax], 0.0, chk));
        ordered = ordered && ob[ax] <= ob[3 + ax];
    }
    return ordered && chk == 0.0;
}

// The states each axis of a segment can take against an obstacle, from the segment's box:
// bit 3 * ax + state.  Every axis has at least one.
TGMS_HD int admissible(const double* box, const double* ob) {
    int mask = 0;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        const bool below = box[ax] < ob[ax], above = box[3 + ax] > ob[3 + ax];
        const bool inside = box[3 + ax] >= ob[ax] && box[ax] <= ob[3 + ax];
        mask |= ((below ? 1 : 0) | (inside ? 2 : 0) | (above ? 4 : 0)) << (3 * ax);
    }
    return mask;
}

TGMS_HD bool combo_in(int mask, int combo) {
    const int sx = combo / 9, sy = (combo / 3) % 3, sz = combo % 3;
    return ((mask >> sx) & 1) && ((mask >> (3 + sy)) & 1) && ((mask >> (6 + sz)) & 1);
}

// How many combinations an item runs: the admissible ones without all-inside, or all-inside
// alone when there is no other.  1..26.
TGMS_HD int combo_count(int mask) {
    const int n = __builtin_popcount(mask & 7) * __builtin_popcount((mask >> 3) & 7) * __builtin_popcount((mask >> 6) & 7);
    const int m = n - (combo_in(mask, ALL_INSIDE) ? 1 : 0);
    return m > 0 ? m : 1;
}

// The n-th of them in ascending index, 0 <= n < combo_count(mask).
TGMS_HD int nth_combo(int mask, int n) {
    const bool only_inside = (mask & 0x1ff) == ((2) | (2 << 3) | (2 << 6));
    int seen = 0, found = ALL_INSIDE;
    TGMS_UNROLL
    for (int combo = 0; combo < COMBOS; ++combo) {
        const bool in = combo_in(mask, combo) && (combo != ALL_INSIDE || only_inside);
        found = (in && seen == n) ? combo : found;
        seen += in ? 1 : 0;
    }
    return found;
}

// The true clamped squared scaled distance of the segment's point at the local time t; out:
// the number of axes on which the point lies outside the obstacle's extent.
TGMS_HD double dist2(const double (&p)[3][8], double t, const double* ob, const double (&scale)[3], int& out) {
    double acc = 0.0;
    out = 0;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        const double x = bounds::horner<7>(p[ax], t);
        const double g = scale[ax] * fmax(fmax(ob[ax] - x, x - ob[3 + ax]), 0.0);
        out += g > 0.0 ? 1 : 0;
        acc = __builtin_fma(g, g, acc);
    }
    return acc;
}

// One combination of one (segment, obstacle) item: c [3][8] on [0, T], ob lo[3] hi[3].  d2 is
// the least true clamped squared distance over u = 0, 1 and the 13 slots of the combination's
// ladder, settled (see above); u in [0, 1] is where it is attained.
TGMS_HD void combo_item(const double* c, double T, const double* ob, const double (&scale)[3], int combo, double& d2,
                        double& u) {
    double p[3][8], e[3][8];
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        const int st = ax == 0 ? combo / 9 : (ax == 1 ? (combo / 3) % 3 : combo % 3);
        const double sg = scale[ax] * (st == 0 ? -1.0 : (st == 2 ? 1.0 : 0.0));
        const double bound = st == 0 ? ob[ax] : ob[3 + ax];
        double w = 1.0;
        TGMS_UNROLL
        for (int k = 0; k < 8; ++k) {
            p[ax][k] = c[ax * 8 + k];
            const double a = p[ax][k] * w;
            e[ax][k] = sg * (k == 0 ? a - bound : a);
            w *= T;
        }
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
    int nb, n;
    double best = dist2(p, 0.0, ob, scale, nb), at = 0.0;
    TGMS_UNROLL
    for (int j = 0; j <= 13; ++j) {
        const double v = j < 13 ? s[j] : 1.0;
        const double d = dist2(p, v * T, ob, scale, n);
        const bool take = d < best;
        at = take ? v : at;
        nb = take ? n : nb;
        best = take ? d : best;
    }
    const double around[2] = {fmax(at - SETTLE, 0.0), fmin(at + SETTLE, 1.0)};
    TGMS_UNROLL
    for (int j = 0; j < 2; ++j) {
        const double d = dist2(p, around[j] * T, ob, scale, n);
        const bool take = d < best || (d == best && n < nb);
        at = take ? around[j] : at;
        nb = take ? n : nb;
        best = take ? d : best;
    }
    d2 = best;
    u = at;
}

// The global time of a candidate: the knot's prefix sum plus the local time, clamped to D.
TGMS_HD double time_of(double knot, double T, double u, double D) { return fmin(__builtin_fma(T, u, knot), D); }

// The flag word of a row: neighbors::row_finish's, and TGMS_CLR_BAD_OBSTACLE for a usable
// trajectory when an obstacle was left out.
TGMS_HD int row_flags(int fl, bool bad_obstacle) {
    return ((fl & TGMS_SEP_NONFINITE) == 0 && bad_obstacle) ? (fl | TGMS_CLR_BAD_OBSTACLE) : fl;
}

}  // namespace clearance
}  // namespace tgms
