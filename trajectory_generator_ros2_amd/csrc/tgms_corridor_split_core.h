// tgms_corridor_split_core.h — the decisions of the corridor split (tgms_corridor_split_batch),
// shared by the gfx950 kernels (tgms_corridor_split.hip) and the host backend (tgms_host.cpp).
// Plain C++17, as its siblings; span_ok and the Horner chain are tgms_corridor_core.h's and
// tgms_bounds_core.h's.
//
// The step.  After a corridor call every segment s has a margin m_s, the global time t_s of it
// and the face that attains it.  A segment with m_s > -r (the corridor flag's comparison) is
// wanted: a waypoint is inserted at t_s, which splits it in two.  Everything that decides the
// shape of the new batch is written once, here:
//   - local_time: t_s back into the segment, against the knot that the corridor call used (the
//     left-to-right prefix sum of T);
//   - at_end: an excursion at a waypoint is not split (no inserted waypoint repairs a waypoint
//     that lies outside, and t_s - knot is not exact to the bit at u = 1): t_loc <= 2^-20 T or
//     t_loc >= (1 - 2^-20) T;
//   - before: the order in which wanted segments are taken while the trajectory has room, the
//     larger margin first, then the lower segment; a segment is taken when fewer than
//     TGMS_MAX_SEGMENTS - M wanted ones come before it;
//   - split_times: T_left = min(max(t_loc, lo), hi) with lo = min_frac T, hi = T - lo, and
//     T_right = T - T_left.  Every operation is rounded on its own: host, device and the numpy
//     reference agree to the bit, so nothing here may be contracted into an FMA;
//   - insert_pull / insert_chord: the inserted waypoint.  These agree between host and device
//     to the accuracy of a Horner chain, not to the bit.
// Integers and times are therefore bit-equal between the two backends, the inserted waypoints
// equal to a few ulp of max|p|.
#pragma once

#include "tgms_corridor_core.h"

#if defined(__clang__)
#define TGMS_NO_CONTRACT_FN
#define TGMS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TGMS_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off")))
#define TGMS_NO_CONTRACT
#endif

namespace tgms {
namespace split {

constexpr double END_FRAC = 1.0 / 1048576.0;  // 2^-20 of T from either waypoint: not split

// A trajectory's plan: which segments are split, and what the caller is told.
struct Row {
    int32_t mask;   // bit i: segment i is split
    int32_t flags;  // TGMS_SPLIT_* or TGMS_FEAS_NONFINITE alone
};

TGMS_HD bool wanted(double m, double r) { return m > -r; }

TGMS_HD double local_time(double t_s, double knot, double T) { return fmin(fmax(t_s - knot, 0.0), T); }

TGMS_HD bool at_end(double t_loc, double T) { return t_loc <= END_FRAC * T || t_loc >= (1.0 - END_FRAC) * T; }

// Segment j is taken before segment i.
TGMS_HD bool before(double mj, int j, double mi, int i) { return mj > mi || (mj == mi && j < i); }

TGMS_HD bool taken(int rank, int M) { return rank < TGMS_MAX_SEGMENTS - M; }

// 0.0 while every argument is finite, NaN afterwards.
TGMS_HD double finite_chk(double x, double chk) { return __builtin_fma(x, 0.0, chk); }

TGMS_NO_CONTRACT_FN TGMS_HD void split_times(double t_loc, double T, double min_frac, double& t_left,
                                             double& t_right) {
    TGMS_NO_CONTRACT
    const double lo = min_frac * T;
    const double hi = T - lo;
    t_left = fmin(fmax(t_loc, lo), hi);
    t_right = T - t_left;
}

// p(t_left) moved back along -n of face n d to margin -r where it is above it.  c [3][8] are the
// segment's coefficients on t in [0, T].  Nothing assumes a unit normal.
TGMS_HD void insert_pull(const double* c, double t_left, double nx, double ny, double nz, double d, double r,
                         double (&w)[3]) {
    double a[3][8];
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        TGMS_UNROLL
        for (int j = 0; j < 8; ++j) a[ax][j] = c[ax * 8 + j];
    }
    const double x = bounds::horner<7>(a[0], t_left), y = bounds::horner<7>(a[1], t_left),
                 z = bounds::horner<7>(a[2], t_left);
    const double q = __builtin_fma(nz, z, __builtin_fma(ny, y, __builtin_fma(nx, x, -d)));
    const double nn = __builtin_fma(nz, nz, __builtin_fma(ny, ny, nx * nx));
    const double s = q > -r ? (q + r) / nn : 0.0;
    w[0] = q > -r ? __builtin_fma(-s, nx, x) : x;
    w[1] = q > -r ? __builtin_fma(-s, ny, y) : y;
    w[2] = q > -r ? __builtin_fma(-s, nz, z) : z;
}

// The point of the straight line between the segment's two waypoints at the fraction t_left / T.
TGMS_HD void insert_chord(const double* w0, const double* w1, double t_left, double T, double (&w)[3]) {
    const double f = t_left / T;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) w[ax] = __builtin_fma(f, w1[ax] - w0[ax], w0[ax]);
}

// One trajectory's plan on the host, segment after segment: what the kernel's lanes decide
// side by side.  m, t_s: the corridor call's rows of the M segments; face: its seg_face;
// fb, cnt: each segment's face span (cnt < 0: not usable); bad: an input of the trajectory is
// not finite or a time not positive.
inline Row plan_row(int M, const double* T, const double* m, const double* t_s, const int32_t* face,
                    const int64_t* fb, const int* cnt, double r, bool bad) {
    bool want[TGMS_MAX_SEGMENTS], cand[TGMS_MAX_SEGMENTS];
    double knot = 0.0;
    int32_t flags = 0;
    for (int i = 0; i < M; ++i) {
        bad = bad || !(m[i] == m[i]) || !(t_s[i] == t_s[i]) || cnt[i] < 0;
        want[i] = cand[i] = false;
        if (bad) continue;
        want[i] = wanted(m[i], r);
        if (want[i] && !((int64_t)face[i] >= fb[i] && (int64_t)face[i] < fb[i] + cnt[i])) bad = true;
        const bool end = at_end(local_time(t_s[i], knot, T[i]), T[i]);
        cand[i] = want[i] && !end;
        if (want[i] && end) flags |= TGMS_SPLIT_AT_END;
        knot += T[i];
    }
    if (bad) return Row{0, TGMS_FEAS_NONFINITE};
    int32_t mask = 0;
    for (int i = 0; i < M; ++i) {
        if (!cand[i]) continue;
        int rank = 0;
        for (int j = 0; j < M; ++j) rank += cand[j] && before(m[j], j, m[i], i) ? 1 : 0;
        if (taken(rank, M))
            mask |= 1 << i;
        else
            flags |= TGMS_SPLIT_FULL;
    }
    if (mask) flags |= TGMS_SPLIT_DONE;
    return Row{mask, flags};
}

}  // namespace split
}  // namespace tgms
