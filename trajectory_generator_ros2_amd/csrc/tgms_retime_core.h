// tgms_retime_core.h — segment re-timing: per segment the factor its own continuous peaks ask of
// its time, shared by the gfx950 kernel (tgms_retime.hip) and the host backend (tgms_host.cpp).
// Plain C++17, as its siblings; the squared peaks are bounds::norm_item's (tgms_bounds_core.h).
//
// A segment stretched by s keeps its shape and has the peaks v / s, a / s^2, j / s^3, so the least
// factor that brings the segment's own peaks under the limits is the dilation's s_kin
// (tgms_dilate_core.h) taken per segment,
//     r_i = max(v_i / v_max, sqrt(a_i / a_max), cbrt(j_i / j_max)),
// and the new time is s_i T_i with s_i = min(s_hi, max(s_lo, r_i)).  That is an allocation rule,
// not a solution: the re-solve with the new times moves every peak, which is why the caller
// iterates (Solver.retime_loop) and closes the rest with one uniform dilation.
//   - segment(): the row v a j r of one segment, s_i and the product s_i T_i (one rounding).  The
//     square roots are formed from the squared peaks exactly as bounds::finish forms the
//     trajectory's, so a row's peaks and the bounds record of that segment alone are the same
//     expressions.  A limit of +inf divides to 0 and contributes nothing; a peak whose ladder was
//     skipped arrives as 0.0.  A peak that is not finite makes r NaN (fmax would drop it).
//   - Fold / fold() / finish(): one trajectory, left to right.  r_max is a copy of one of the
//     r_i (ties to the lowest segment), D_in and D_out are the prefix sums of T and of the
//     products in segment order, and the flags are strict comparisons on the stored values.
#pragma once

#include "tgms_bounds_core.h"

namespace tgms {
namespace retime {

// v_max, a_max, j_max of a call: each > 0, +inf is unchecked.
struct Lim {
    double v_max, a_max, j_max;
};

struct Seg {
    double row[TGMS_RETIME_STRIDE];  // v a j r
    double s, T_out;
};

// n2: the segment's squared peaks (bounds::norm_item<1|2|3>, 0.0 for a skipped one); T: its time.
TGMS_HD Seg segment(const double (&n2)[3], double T, const Lim& L, double s_lo, double s_hi) {
    Seg g;
    const double v = sqrt(n2[0]), a = sqrt(n2[1]), j = sqrt(n2[2]);
    const double fin = __builtin_fma(v, 0.0, __builtin_fma(a, 0.0, j * 0.0));
    const double r = fmax(fmax(v / L.v_max, sqrt(a / L.a_max)), cbrt(j / L.j_max));
    g.row[0] = v;
    g.row[1] = a;
    g.row[2] = j;
    g.row[3] = fin != 0.0 ? __builtin_nan("") : r;
    g.s = fmin(s_hi, fmax(s_lo, g.row[3]));  // a NaN r gives s_lo; fold() sees the NaN
    g.T_out = g.s * T;
    return g;
}

struct Fold {
    double r_max, d_in, d_out, chk;  // chk: 0 while every folded value is finite, NaN afterwards
    int seg, changed;
};

TGMS_HD Fold fold_init() { return Fold{0.0, 0.0, 0.0, 0.0, 0, 0}; }

// Segment i (0, 1, ... in order) of the trajectory: its r, s, T and s T.
TGMS_HD void fold(Fold& f, int i, double r, double s, double T, double T_out) {
    f.seg = r > f.r_max ? i : f.seg;  // r >= 0: segment 0 holds a maximum of 0
    f.r_max = r > f.r_max ? r : f.r_max;
    f.d_in += T;
    f.d_out += T_out;
    f.chk = __builtin_fma(r, 0.0, f.chk);
    f.changed |= s != 1.0 ? 1 : 0;
}

// The record r_max D_in D_out and the flags of one trajectory; bad: an input was not finite, a
// time not positive or the segment count unusable.
TGMS_HD int finish(const Fold& f, bool bad, double s_hi, double (&rec)[TGMS_RETIME_REC]) {
    rec[0] = f.r_max;
    rec[1] = f.d_in;
    rec[2] = f.d_out;
    double fin = f.chk;
    TGMS_UNROLL
    for (int i = 0; i < TGMS_RETIME_REC; ++i) fin = __builtin_fma(rec[i], 0.0, fin);
    if (bad || fin != 0.0) {
        TGMS_UNROLL
        for (int i = 0; i < TGMS_RETIME_REC; ++i) rec[i] = __builtin_nan("");
        return TGMS_FEAS_NONFINITE;
    }
    int fl = f.seg << TGMS_RT_SEG_SHIFT;
    fl |= rec[0] > 1.0 ? TGMS_RT_OVER : 0;
    fl |= rec[0] > s_hi ? TGMS_RT_CAPPED : 0;  // some r_i > s_hi exactly when the largest is
    fl |= f.changed ? TGMS_RT_CHANGED : 0;
    return fl;
}

}  // namespace retime
}  // namespace tgms
