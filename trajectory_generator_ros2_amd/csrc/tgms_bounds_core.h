// tgms_bounds_core.h — the continuous feasibility bounds of one segment, shared by the gfx950
// kernel (tgms_bounds.hip) and the host backend (tgms_host.cpp).  Plain C++17: hipcc compiles
// it for host and device, g++ for the host.
//
// A segment's quantities are polynomials on the closed interval [0, T]; in normalised time
// u = t / T (coefficients a_j = c_j T^j) every one lives on [0, 1]:
//     p_x, p_y, p_z                degree 7, stationary points: roots of a degree-6 derivative
//     T^2 |p'|^2, T^4 |p''|^2, T^6 |p'''|^2   degrees 12, 10, 8, derivatives of degree 11, 9, 7
// The extremum over [0, 1] is the best of the values at 0, at 1 and at the real roots of the
// derivative f of degree D inside.  Those roots come from the derivative ladder: the roots
// of f^(k+1), with 0 and 1, cut [0, 1] into intervals on which f^(k) is monotone, so an
// interval holds one root of f^(k) exactly when f^(k) changes sign over it, and bisection
// finds it.  The ladder starts at the linear f^(D-1) and works down to f.
//   - Level d (the polynomial f^(D-d) of degree d) has d intervals and d slots.  An
//     interval with no sign change puts its left end into its slot: the list stays sorted and
//     of fixed length, the duplicate makes an empty interval one level down (which has no
//     sign change), and the control flow depends on no count of roots.  Every list index is
//     a compile-time constant, so the d slots are registers on the device.
//   - A level's coefficients are those of f times a falling factorial, formed when the
//     level is entered, so only f's D + 1 coefficients stay live across levels.
//   - BISECTIONS halvings leave a bracket of 2^-40 = 9.1e-13 in u.  At a stationary point of
//     a polynomial Q of degree n <= 12 a root off by delta moves the value by
//     Q'' delta^2 / 2 <= (2/3) n^2 (n^2 - 1) max|Q| delta^2 (Markov on [0, 1]) < 1.2e-20
//     max|Q|, far below the rounding of the evaluation itself; the 1e-9 contract of tgms.h
//     is met by the evaluation, not by the bracket.  A breakpoint off by delta can hide two
//     roots of the next level that lie within O(delta) of each other, the "touch without a
//     sign change" that tgms.h allows to skip: the values there differ from a neighbouring
//     candidate's by O(delta^3).
//   - Not an interval-arithmetic certificate: signs and values are fp64 evaluations (Horner
//     in FMAs).
// Values are evaluated from the axis polynomials (the squared norms as the sum of three
// squares, never from their convolved coefficients), so a constant trajectory gives exactly
// its point and exactly zero peaks.
#pragma once

#include <math.h>

#include "tgms.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TGMS_HD __host__ __device__ __forceinline__
#define TGMS_UNROLL _Pragma("unroll")
#else
#define TGMS_HD inline
#define TGMS_UNROLL _Pragma("GCC unroll 16")
#endif

namespace tgms {
namespace bounds {

constexpr int BISECTIONS = 40;

// n (n-1) ... (n-m+1); exact in fp64 for n <= 18 (18! < 2^53; the callers need n <= 13)
constexpr double ffact(int n, int m) {
    double r = 1.0;
    for (int i = 0; i < m; ++i) r *= (double)(n - i);
    return r;
}

template <int N>
TGMS_HD double horner(const double (&c)[N + 1], double u) {
    double s = c[N];
    TGMS_UNROLL
    for (int k = N - 1; k >= 0; --k) s = __builtin_fma(s, u, c[k]);
    return s;
}

// Levels 1..d of the ladder of f = sum_k c[k] u^k (degree D).  On return s[0..d-1] holds, in
// ascending order, the roots of f^(D-d) found in [0, 1] and duplicates of breakpoints.
template <int D, int d>
struct Ladder {
    static TGMS_HD void run(const double (&c)[D + 1], double (&s)[D]) {
        if constexpr (d > 1) Ladder<D, d - 1>::run(c, s);
        double g[d + 1];  // f^(D-d), up to a positive factor
        TGMS_UNROLL
        for (int k = 0; k <= d; ++k) g[k] = c[k + D - d] * ffact(k + D - d, D - d);
        double a = 0.0, fa = g[0];
        TGMS_UNROLL
        for (int j = 0; j < d; ++j) {  // interval [a, b]; s[j] still holds the level above's slot
            const double b = j < d - 1 ? s[j] : 1.0;
            const double fb = horner<d>(g, b);
            double r = a;
            if ((fa < 0.0 && fb > 0.0) || (fa > 0.0 && fb < 0.0)) {
                const bool neg = fa < 0.0;
                double lo = a, hi = b;
                for (int it = 0; it < BISECTIONS; ++it) {
                    const double m = 0.5 * (lo + hi);
                    const bool mneg = horner<d>(g, m) < 0.0;
                    lo = mneg == neg ? m : lo;
                    hi = mneg == neg ? hi : m;
                }
                r = 0.5 * (lo + hi);
            }
            s[j] = r;
            a = b;
            fa = fb;
        }
    }
};

// Extent of one axis of one segment: c[8] are the caller's coefficients on t in [0, T].
TGMS_HD void position_item(const double* c, double T, double& lo, double& hi) {
    double a[8], f[7], s[6];
    double w = 1.0;
    a[0] = c[0];
    TGMS_UNROLL
    for (int j = 1; j < 8; ++j) {
        w *= T;
        a[j] = c[j] * w;
        f[j - 1] = (double)j * a[j];
    }
    Ladder<6, 6>::run(f, s);
    const double p1 = horner<7>(a, 1.0);
    lo = fmin(a[0], p1);
    hi = fmax(a[0], p1);
    TGMS_UNROLL
    for (int j = 0; j < 6; ++j) {
        const double p = horner<7>(a, s[j]);
        lo = fmin(lo, p);
        hi = fmax(hi, p);
    }
}

// max over [0, T] of |p^(q)(t)|^2 of one segment, q = 1, 2, 3: c[3][8] as above.
template <int q>
TGMS_HD double norm_item(const double* c, double T) {
    constexpr int n = 7 - q;      // degree of an axis' q-th derivative
    constexpr int D = 2 * n - 1;  // degree of the squared norm's derivative
    double e[3][n + 1];           // T^q p^(q) in u
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double w = 1.0;
        TGMS_UNROLL
        for (int j = 1; j < 8; ++j) {
            w *= T;
            if (j >= q) e[ax][j - q] = ffact(j, q) * (c[ax * 8 + j] * w);
        }
    }
    double f[D + 1], s[D];
    TGMS_UNROLL
    for (int m = 1; m <= 2 * n; ++m) {  // f[m-1] = m * (coefficient m of sum_ax e_ax^2)
        double acc = 0.0;
        TGMS_UNROLL
        for (int i = 0; i <= n; ++i) {
            const int k = m - i;
            if (k >= 0 && k <= n) {
                TGMS_UNROLL
                for (int ax = 0; ax < 3; ++ax) acc = __builtin_fma(e[ax][i], e[ax][k], acc);
            }
        }
        f[m - 1] = (double)m * acc;
    }
    Ladder<D, D>::run(f, s);
    auto norm2 = [&e](double u) {
        const double x = horner<n>(e[0], u), y = horner<n>(e[1], u), z = horner<n>(e[2], u);
        return __builtin_fma(z, z, __builtin_fma(y, y, x * x));
    };
    double best = fmax(norm2(0.0), norm2(1.0));
    TGMS_UNROLL
    for (int j = 0; j < D; ++j) best = fmax(best, norm2(s[j]));
    double iw = 1.0 / T, sc = 1.0;
    TGMS_UNROLL
    for (int i = 0; i < q; ++i) sc *= iw;
    return best * sc * sc;
}

// The record and the flags of one trajectory from its reduced extents (lo, hi), squared peaks
// (n2) and duration; bad: an input was not finite or a time not positive.  Strict
// comparisons on the very values stored.
TGMS_HD int finish(const double (&lo)[3], const double (&hi)[3], const double (&n2)[3], double duration, bool bad,
                   const tgms_limits& lim, double (&rec)[TGMS_EXTREMA_STRIDE]) {
    double fin = 0.0;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        rec[a] = lo[a];
        rec[3 + a] = hi[a];
        rec[6 + a] = sqrt(n2[a]);
    }
    rec[9] = duration;
    TGMS_UNROLL
    for (int i = 0; i < TGMS_EXTREMA_STRIDE; ++i) fin = __builtin_fma(rec[i], 0.0, fin);
    if (bad || fin != 0.0) {
        TGMS_UNROLL
        for (int i = 0; i < TGMS_EXTREMA_STRIDE; ++i) rec[i] = __builtin_nan("");
        return TGMS_FEAS_NONFINITE;
    }
    int fl = 0;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) fl |= (rec[a] < lim.pmin[a] || rec[3 + a] > lim.pmax[a]) ? TGMS_FEAS_BOX : 0;
    fl |= rec[6] > lim.v_max ? TGMS_FEAS_SPEED : 0;
    fl |= rec[7] > lim.a_max ? TGMS_FEAS_ACCEL : 0;
    fl |= rec[8] > lim.j_max ? TGMS_FEAS_JERK : 0;
    return fl;
}

}  // namespace bounds
}  // namespace tgms
