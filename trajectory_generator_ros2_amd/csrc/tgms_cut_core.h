// tgms_cut_core.h — the decisions of the replan cut (tgms_cut_batch), shared by the gfx950
// kernels (tgms_cut.hip) and the host backend (tgms_host.cpp).  Plain C++17, as its siblings; the
// no-contraction macros and finite_chk are tgms_corridor_split_core.h's.
//
// The step.  A vehicle is at time t_cut of its trajectory and is replanned from there: the
// segments behind it go, the one it is in is shortened, and its state (p, v, a, j) becomes the
// start of the new batch.  Everything that decides the shape of the new batch is written once,
// here:
//   - clamp_cut: t_c = min(max(t_cut, 0), D), D the last knot of the left-to-right prefix sum of
//     T that the corridor call uses;
//   - in_or_after: knot k_m (m = 1..M-1) counts towards the segment index when k_m <= t_c, so a
//     cut exactly on an interior knot belongs to the later segment at local time 0;
//   - local_time: t_c back into segment s, min(max(t_c - k_s, 0), T_s);
//   - snaps: what is left of the segment, rem = T_s - t_loc, is too short when rem <= 0 or
//     rem < min_frac T_s; the cut then moves forward to knot s+1, or, off the last segment,
//     finishes the trajectory;
//   - resolve: the three rules above in their order, for one trajectory whose s, k_s, T_s and D
//     are known, into a Plan.  The kernel's lanes find s, k_s and T_s with a ballot and two
//     shuffles, the host with plan_row's loop; both then call resolve;
//   - first_time, start_clock: the shortened time T_s - t_loc and the old-clock time k_s + t_loc,
//     one rounded operation each.
// Every one of these is a comparison or a single rounded operation, so integers, flags, times
// and t0 are bit-equal between the two backends and any fp64 re-computation.  shift() is the
// Taylor shift of one axis by synthetic division: it gives the state and the shifted row to the
// accuracy of a Horner chain, not to the bit.
#pragma once

#include "tgms_corridor_split_core.h"

namespace tgms {
namespace cut {

// What a trajectory becomes.
enum Kind : int32_t {
    KEEP = 0,      // segments s.. are kept, the first one from t_loc on
    FINISHED = 1,  // one hold segment at the last waypoint
    THROUGH = 2,   // unusable: copied through unchanged
    PLACEHOLDER = 3  // device call only: a segment count outside 1..TGMS_MAX_SEGMENTS
};

struct Plan {
    int32_t kind;   // Kind
    int32_t s;      // first kept segment (KEEP), else 0
    int32_t flags;  // TGMS_CUT_* or TGMS_FEAS_NONFINITE alone
    int32_t M_out;  // segments afterwards
    double t_loc;   // local time of the cut in segment s; 0.0 unless KEEP
    double t0;      // the time on the old clock at which the new trajectory starts
};

TGMS_HD double clamp_cut(double t_cut, double D) { return fmin(fmax(t_cut, 0.0), D); }

TGMS_HD bool in_or_after(double knot, double t_c) { return knot <= t_c; }

TGMS_HD double local_time(double t_c, double knot, double T) { return fmin(fmax(t_c - knot, 0.0), T); }

TGMS_NO_CONTRACT_FN TGMS_HD bool snaps(double t_loc, double T, double min_frac) {
    TGMS_NO_CONTRACT
    const double rem = T - t_loc;
    const double least = min_frac * T;
    return rem <= 0.0 || rem < least;
}

TGMS_NO_CONTRACT_FN TGMS_HD double first_time(double T, double t_loc) {
    TGMS_NO_CONTRACT
    return t_loc > 0.0 ? T - t_loc : T;
}

TGMS_NO_CONTRACT_FN TGMS_HD double start_clock(double knot, double t_loc) {
    TGMS_NO_CONTRACT
    return knot + t_loc;
}

TGMS_HD Plan through(int M) { return Plan{THROUGH, 0, TGMS_FEAS_NONFINITE, M, 0.0, __builtin_nan("")}; }

// One usable trajectory: t_cut is not NaN, s counts the interior knots <= clamp_cut(t_cut, D),
// k_s and T_s are the knot and time of segment s, k_next the knot after it (D when s == M-1).
TGMS_HD Plan resolve(int M, double t_cut, double D, int s, double k_s, double T_s, double k_next, double min_frac) {
    const Plan done{FINISHED, 0, TGMS_CUT_FINISHED | TGMS_CUT_DONE, 1, 0.0, D};
    if (t_cut >= D) return done;  // at or beyond the end, +inf included
    const double t_c = clamp_cut(t_cut, D);
    double t_loc = local_time(t_c, k_s, T_s);
    int32_t flags = 0;
    if (snaps(t_loc, T_s, min_frac)) {
        if (s == M - 1) return done;
        s += 1;
        k_s = k_next;
        t_loc = 0.0;
        flags |= TGMS_CUT_SNAPPED;
    }
    if (s > 0 || t_loc > 0.0) flags |= TGMS_CUT_DONE;
    return Plan{KEEP, s, flags, M - s, t_loc, start_clock(k_s, t_loc)};
}

// One trajectory's plan on the host, knot after knot: what the kernel's lanes decide side by
// side.  bad: an input of the trajectory is not finite, a time is not positive or t_cut is NaN.
inline Plan plan_row(int M, const double* T, double t_cut, double min_frac, bool bad) {
    if (bad) return through(M);
    double knot[TGMS_MAX_SEGMENTS + 1];
    knot[0] = 0.0;
    for (int i = 0; i < M; ++i) knot[i + 1] = knot[i] + T[i];
    const double D = knot[M], t_c = clamp_cut(t_cut, D);
    int s = 0;
    for (int m = 1; m < M; ++m) s += in_or_after(knot[m], t_c) ? 1 : 0;
    return resolve(M, t_cut, D, s, knot[s], T[s], knot[s + 1], min_frac);
}

// The Taylor shift of one axis: c [8] on local time t becomes the coefficients on t - t0, by
// eight passes of synthetic division (each pass is a Horner chain that stops one place later).
// Afterwards c[k] = p^(k)(t0) / k!: c[0] is the Horner value of p(t0).
TGMS_HD void shift(double (&c)[8], double t0) {
    TGMS_UNROLL
    for (int k = 0; k < 7; ++k) {
        TGMS_UNROLL
        for (int j = 6; j >= k; --j) c[j] = __builtin_fma(c[j + 1], t0, c[j]);
    }
}

// The state of a shifted row c [3][8] (flat): p [3] and the v, a, j block [3][3] of end_derivs.
TGMS_HD void state_of(const double (&c)[24], double (&p)[3], double (&d)[9]) {
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        p[ax] = c[ax * 8];
        d[ax] = c[ax * 8 + 1];
        d[3 + ax] = 2.0 * c[ax * 8 + 2];
        d[6 + ax] = 6.0 * c[ax * 8 + 3];
    }
}

// Segment row c_in [24] shifted to t_loc into c [24], with its state.
TGMS_HD void shift_row(const double* c_in, double t_loc, double (&c)[24], double (&p)[3], double (&d)[9]) {
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double a[8];
        TGMS_UNROLL
        for (int j = 0; j < 8; ++j) a[j] = c_in[ax * 8 + j];
        shift(a, t_loc);
        TGMS_UNROLL
        for (int j = 0; j < 8; ++j) c[ax * 8 + j] = a[j];
    }
    state_of(c, p, d);
}

}  // namespace cut
}  // namespace tgms
