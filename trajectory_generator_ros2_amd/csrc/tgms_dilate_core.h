// tgms_dilate_core.h — the least uniform time dilation of one trajectory that meets the dynamic
// limits, shared by the gfx950 kernel (tgms_dilate.hip) and the host backend (tgms_host.cpp).
// Plain C++17, as its siblings: the peaks are tgms_bounds_core.h's, the thrust and tilt
// extremes tgms_thrust_core.h's.
//
// The problem.  p_s(t) = p(t / s) on [0, s D] has the peaks v / s, a / s^2, j / s^3 and the
// thrust vector f_s = p''(t / s) / s^2 + g e_z.  With lambda = 1 / s^2,
//     f_s = lambda (p'' + (g / lambda) e_z),
// so the thrust record of the dilated trajectory is the record thrust::thrust_item /
// tilt_item return for the UNDILATED coefficients at g' = g / lambda, the norms times lambda,
// the tilt unchanged.  Nothing is rescaled inside the search; per evaluation only g' changes.
//   - Kinematic part, closed form: s_kin = max(v / v_max, sqrt(a / a_max), cbrt(j / j_max)).
//   - Thrust part: a root search in lambda on (0, 1 / max(s_lo, s_kin)^2] for the excess
//         h(lambda) = max(lambda sqrt(f2max') / f_hi - 1, 1 - lambda sqrt(f2min') / f_lo,
//                         tilt' - tilt_max),
//     feasible where h <= 0.  The first two terms are linear in lambda on a vertical
//     trajectory and convex / concave otherwise, the tilt condition is monotone for tilt_max <
//     pi / 2.  f_lo can be crossed several times near free fall: the search keeps a bracket
//     [lo feasible, hi infeasible] and returns lo, so the answer is feasible and minimal
//     locally.
//   - Order of evaluations.  (1) s0 = min(max(s_lo, s_kin), s_hi): feasible there ends the
//     search after one evaluation.  (2) A lambda that is feasible by the triangle inequality,
//     ||f_s|| within g -+ lambda a_peak and sin(tilt) <= lambda a_peak / g, pulled in by 2^-30:
//     it brackets the root from the feasible side within a small factor.  (3) Where that
//     guess does not exist or fails, s_hi itself; infeasible there is TGMS_DIL_CAPPED.  (4)
//     Illinois steps on the bracket, which close it from both sides in turns; where the width
//     is not below half of that three evaluations ago the step is a bisection (geometric while
//     hi > 4 lo), so the width halves every three evaluations at the worst and MAX_EVALS bounds
//     the loop.  A step is kept 2^-43 hi away from
//     both ends, which lets the bracket close to WIDTH = 2^-41 relative from both sides.
//   - Error.  The bracket leaves the active quantity within 2^-40 of its limit; what remains is
//     the evaluation's rounding (tgms_thrust_core.h) and that of c_k r^k in the output.
#pragma once

#include "tgms_thrust_core.h"

namespace tgms {
namespace dilate {

constexpr int MAX_EVALS = 160;       // of the thrust core per trajectory, the three opening ones apart
constexpr double WIDTH = 0x1p-41;    // relative width of the final bracket in lambda
constexpr double KEEP_OFF = 0x1p-43; // a step's least relative distance from both ends
constexpr double PULL_IN = 0x1p-30;  // of the triangle-inequality guess

// The six limits of a call, resolved: +inf (f_lo: <= 0) is unchecked.
struct Lim {
    double v_max, a_max, j_max, f_lo, f_hi, tilt;
};

struct Kin {
    double v, a, j;  // the continuous peaks of the undilated trajectory
};

enum { ST_FIRST = 0, ST_PROBE, ST_END, ST_ROOT, ST_DONE };

// One trajectory's search.  Plain data: the kernel keeps one per tile row in LDS.
struct Search {
    double lo, hi;   // lambda: the feasible and the infeasible end
    double hl, hh;   // the excess there, halved by the Illinois rule
    double x;        // the lambda to evaluate next
    double w1, w2, w3;  // the bracket's width one, two and three evaluations ago
    double s0, skin, kex, safe;
    double s;        // result
    int stage, act, side, evals;
    int kwhich, kexw;
    int active, flags;  // result
};

// peak / limit, with a limit <= 0 met by a zero peak only
TGMS_HD double ratio(double pk, double mx) { return mx > 0.0 ? pk / mx : (pk > mx ? __builtin_inf() : 0.0); }

// s_kin and the limit that sets it (TGMS_DIL_NONE for 0).
TGMS_HD double kin_scale(const Kin& k, const Lim& L, int& which) {
    const double sv = ratio(k.v, L.v_max), sa = sqrt(ratio(k.a, L.a_max)), sj = cbrt(ratio(k.j, L.j_max));
    double s = 0.0;
    which = TGMS_DIL_NONE;
    which = sv > s ? TGMS_DIL_SPEED : which;
    s = sv > s ? sv : s;
    which = sa > s ? TGMS_DIL_ACCEL : which;
    s = sa > s ? sa : s;
    which = sj > s ? TGMS_DIL_JERK : which;
    s = sj > s ? sj : s;
    return s;
}

// The largest relative excess of the three peaks at scale s, and which one.
TGMS_HD double kin_excess(const Kin& k, const Lim& L, double s, int& which) {
    const double r = 1.0 / s;
    const double ev = ratio(k.v * r, L.v_max) - 1.0, ea = ratio(k.a * r * r, L.a_max) - 1.0,
                 ej = ratio(k.j * r * r * r, L.j_max) - 1.0;
    double e = ev;
    which = TGMS_DIL_SPEED;
    which = ea > e ? TGMS_DIL_ACCEL : which;
    e = ea > e ? ea : e;
    which = ej > e ? TGMS_DIL_JERK : which;
    e = ej > e ? ej : e;
    return e;
}

// The thrust excess h at lambda from the fold of the core's items at g' = g / lambda; which:
// the limit that sets it.  fin != 0 when a value is not finite.
TGMS_HD double excess(const thrust::Fold& f, double lam, const Lim& L, int& which, double& fin) {
    const double fhi = lam * sqrt(f.hi.v), flo = lam * sqrt(f.lo.v), tilt = f.tilt.v;
    fin = __builtin_fma(fhi, 0.0, __builtin_fma(flo, 0.0, tilt * 0.0));
    const double eh = ratio(fhi, L.f_hi) - 1.0;
    const double el = L.f_lo > 0.0 ? 1.0 - flo / L.f_lo : -1.0;
    const double et = tilt - L.tilt;
    double e = eh;
    which = TGMS_DIL_THRUST_HIGH;
    which = el > e ? TGMS_DIL_THRUST_LOW : which;
    e = el > e ? el : e;
    which = et > e ? TGMS_DIL_TILT : which;
    e = et > e ? et : e;
    return e;
}

// A lambda at which the thrust limits hold by the triangle inequality; 0 when there is none.
TGMS_HD double safe_lambda(double a_pk, double g, const Lim& L) {
    double m = L.f_hi - g;
    m = L.f_lo > 0.0 ? fmin(m, g - L.f_lo) : m;
    m = L.tilt < __builtin_inf() ? fmin(m, g * sin(L.tilt)) : m;
    return (m > 0.0 && a_pk > 0.0) ? m / a_pk : 0.0;
}

TGMS_HD void finish(Search& q, double s, int active, int flags) {
    q.s = s;
    q.active = active;
    q.flags = flags | (q.evals << TGMS_DIL_EVALS_SHIFT);
    q.stage = ST_DONE;
}

TGMS_HD void nonfinite(Search& q) {
    q.s = __builtin_nan("");
    q.active = -1;
    q.flags = TGMS_FEAS_NONFINITE;
    q.stage = ST_DONE;
}

// Opens the search of one trajectory; bad: an input was not finite, a time not positive or the
// segment count unusable.  Leaves q.x, the first lambda to evaluate, unless the search is done.
TGMS_HD void init(Search& q, bool bad, const Kin& k, double g, const Lim& L, double s_lo, double s_hi) {
    const double inf = __builtin_inf();
    q.lo = q.hi = q.hl = q.hh = q.x = 0.0;
    q.w1 = q.w2 = q.w3 = inf;
    q.s0 = q.skin = q.kex = q.safe = q.s = 0.0;
    q.stage = ST_FIRST;
    q.act = q.kwhich = q.kexw = q.active = TGMS_DIL_NONE;
    q.side = q.evals = q.flags = 0;
    const double fin = __builtin_fma(k.v, 0.0, __builtin_fma(k.a, 0.0, k.j * 0.0));
    if (bad || fin != 0.0) {
        nonfinite(q);
        return;
    }
    q.skin = kin_scale(k, L, q.kwhich);
    q.s0 = fmin(fmax(s_lo, q.skin), s_hi);
    q.kex = kin_excess(k, L, s_hi, q.kexw);
    q.safe = safe_lambda(k.a, g, L);
    q.x = 1.0 / (q.s0 * q.s0);
}

// Takes the evaluation at q.x (the fold of the trajectory's items at g' = g / q.x) and either
// finishes or leaves the next q.x.
TGMS_HD void step(Search& q, const thrust::Fold& f, const Lim& L, double s_lo, double s_hi) {
    ++q.evals;
    int w;
    double fin;
    const double h = excess(f, q.x, L, w, fin);
    if (f.bad || fin != 0.0 || !(h == h)) {
        nonfinite(q);
        return;
    }
    const double lam_end = 1.0 / (s_hi * s_hi);
    if (q.stage == ST_FIRST) {
        if (q.skin > s_hi) {  // a peak is over its limit at s_hi whatever the thrust does
            finish(q, s_hi, q.kex >= h ? q.kexw : w, TGMS_DIL_CAPPED);
            return;
        }
        if (h <= 0.0) {
            finish(q, q.s0, q.skin > s_lo ? q.kwhich : TGMS_DIL_NONE, 0);
            return;
        }
        if (!(q.s0 < s_hi)) {
            finish(q, s_hi, w, TGMS_DIL_CAPPED);
            return;
        }
        q.hi = q.x;
        q.hh = h;
        q.act = w;
        const double x1 = q.safe * (1.0 - PULL_IN);
        const bool probe = x1 > lam_end && x1 < q.hi;
        q.x = probe ? x1 : lam_end;
        q.stage = probe ? ST_PROBE : ST_END;
        return;
    }
    if (q.stage == ST_PROBE && h > 0.0) {  // the guess failed: it is the new infeasible end
        q.hi = q.x;
        q.hh = h;
        q.act = w;
        q.x = lam_end;
        q.stage = ST_END;
        return;
    }
    if (q.stage == ST_END && h > 0.0) {
        finish(q, s_hi, w, TGMS_DIL_CAPPED);
        return;
    }
    if (q.stage != ST_ROOT) {  // the first feasible point closes the bracket
        q.lo = q.x;
        q.hl = h;
        q.side = 0;
        q.stage = ST_ROOT;
    } else if (h <= 0.0) {
        q.lo = q.x;
        q.hl = h;
        q.hh = q.side < 0 ? 0.5 * q.hh : q.hh;
        q.side = -1;
    } else {
        q.hi = q.x;
        q.hh = h;
        q.act = w;
        q.hl = q.side > 0 ? 0.5 * q.hl : q.hl;
        q.side = 1;
    }
    const double wd = q.hi - q.lo;
    if (wd <= WIDTH * q.hi || q.evals >= MAX_EVALS) {
        finish(q, fmin(fmax(1.0 / sqrt(q.lo), s_lo), s_hi), q.act, 0);
        return;
    }
    double xs = (q.lo * q.hh - q.hi * q.hl) / (q.hh - q.hl);
    if (wd > 0.5 * q.w3) xs = q.hi > 4.0 * q.lo ? sqrt(q.lo * q.hi) : 0.5 * (q.lo + q.hi);
    const double d = KEEP_OFF * q.hi;
    xs = fmin(fmax(xs, q.lo + d), q.hi - d);  // a NaN step becomes lo + d
    q.w3 = q.w2;
    q.w2 = q.w1;
    q.w1 = wd;
    q.x = xs;
}

// c_k r^k with the power formed by repeated multiplication (include/tgms.h fixes the rule).
TGMS_HD double scaled(double c, int k, double r) {
    double p = 1.0;
    TGMS_UNROLL
    for (int j = 0; j < 7; ++j) p = j < k ? p * r : p;
    return c * p;
}

}  // namespace dilate
}  // namespace tgms
