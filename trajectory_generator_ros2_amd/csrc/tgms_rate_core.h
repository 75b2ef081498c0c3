// tgms_rate_core.h — continuous roll/pitch body-rate bound of one segment from differential
// flatness, shared by the gfx950 kernel (tgms_rate.hip) and the host backend (tgms_host.cpp).
// Plain C++17, as its siblings: the axis polynomials are tgms_thrust_core.h's, the derivative
// ladder and the Horner chain tgms_bounds_core.h's, the rule for a candidate's global time
// tgms_clearance_core.h's.
//
// The quantity.  With the mass-normalised thrust vector f(t) = p''(t) + g e_z the body z axis is
// f / ||f||, and its angular velocity perpendicular to itself, the roll/pitch rate, has the
// magnitude
//     omega(t) = ||f x p'''|| / ||f||^2        (rad/s; f' = p''' because g is constant).
// The yaw rate about the body axis depends on the yaw plan and is no part of it.
//   - Polynomials.  In normalised time u = t / T a segment's E = T^2 f is
//     thrust::accel_poly's three polynomials of degree 5 (g T^2 on the z constant), and E' = T^3
//     p'''.  The cross product Cr = E x E' would have degree 9, but its leading terms cancel
//     identically (5 a_5 b_5 - 5 b_5 a_5): per component
//         Cr_k = sum_{i < j, i + j = k + 1} (j - i) (a_i b_j - b_i a_j),  k = 0..8,
//     formed with 9 coefficients; the cancelling one is never computed.  With Nn = ||Cr||^2
//     (degree 16) and Dn = ||E||^2 (degree 10), omega = sqrt(Nn) / (T Dn), and the stationary
//     points of Nn / Dn^2 are the roots of
//         G = Nn' Dn - 2 Nn Dn',   G_k = sum_{i + m = k + 1} (i - 2 m) Nn_i Dn_m,  k = 0..25:
//     degree 25 (the leading coefficient is (16 - 20) Nn_16 Dn_10, which does not cancel).
//   - Candidates.  u = 0, u = 1 and the 25 slots of bounds::Ladder<25, 25> on G.  The ladder's
//     level factors bounds::ffact(n, m) are no longer exact in fp64 above n = 18; the rounded
//     factor is still positive, so no sign and no root moves.
//   - Polish.  G's 26 coefficients are convolved twice in fp64 in the monomial basis.  Where the
//     axis polynomials oscillate (Chebyshev-like input) they reach 1e34 while |G| near a root is
//     below 1e16: Horner's rounding then moves a located root by 1e-3 in u, and where omega is
//     sharply peaked the value there is 2e-3 short.  So every slot is the start of a
//     golden-section ascent of omega^2 itself, evaluated from the axis polynomials, on the
//     bracket that reaches half way to the neighbouring slots (POLISH steps: 0.618^40 = 4e-9 of
//     the bracket, and omega^2 is stationary at the maximum).  A polished point replaces nothing:
//     it is one more candidate, so the result can only rise towards the true maximum, and a slot
//     that was exact already stays the winner unless a polished value is strictly larger.
//   - Values.  Every value is evaluated from the axis polynomials at the candidate: f = E(u) /
//     T^2 with g added to z after the Horner chain, p''' = E'(u) / T^3 by a Horner chain on the
//     same coefficients, the cross product, the two sums of squares and the quotient; never from
//     convolved coefficients, which only locate candidates.  Where the cross product is exactly
//     0.0, omega is 0.0 whatever the denominator: a constant trajectory and a purely vertical
//     one give omega_max == 0.0 for every g, 0 included (f x p''' has only products with an
//     exact zero factor there).
//   - Error.  omega^2 is stationary at the located roots, so a slot off by delta moves it by
//     O(delta^2); what remains is the rounding of six degree-5 and degree-4 Horner chains:
//     that of f relative to F = f_max, that of p''' relative to J = j_peak.  omega <= J / m
//     with m = f_min, and the quotient amplifies a relative error of f by F / m: |omega - true|
//     = O(eps F J / m^2), against the 1e-9 F J / m^2 of tgms.h.  Measured: DESIGN.md, k_rate.
//     The roots of G come from coefficients convolved in fp64; where their rounding moves a
//     root by eps, the value moves by O(eps^2).
//   - Where thrust vanishes on the trajectory omega is unbounded and carries no accuracy claim;
//     the thrust call's f_min says so.
//   - Not a certificate, and a touch without a sign change may be skipped, as for the bounds.
#pragma once

#include "tgms_thrust_core.h"

namespace tgms {
namespace rate {

constexpr int N = thrust::N;  // 5: degree of an axis of E
constexpr int DC = 2 * N - 2;  // 8: degree of a component of E x E'
constexpr int DG = 25;         // degree of G
constexpr int POLISH = 40;     // golden-section steps per slot

// E'(u) of one axis: the Horner chain on k e_k.
TGMS_HD double dhorner(const double (&e)[N + 1], double u) {
    double s = (double)N * e[N];
    TGMS_UNROLL
    for (int k = N - 1; k >= 1; --k) s = __builtin_fma(s, u, (double)k * e[k]);
    return s;
}

// omega^2 at u: f and p''' from the axis polynomials, then the cross product and the quotient.
TGMS_HD double omega2_at(const double (&e)[3][N + 1], double iT2, double iT3, double g, double u) {
    const double x = bounds::horner<N>(e[0], u) * iT2, y = bounds::horner<N>(e[1], u) * iT2;
    const double z = __builtin_fma(bounds::horner<N>(e[2], u), iT2, g);
    const double jx = dhorner(e[0], u) * iT3, jy = dhorner(e[1], u) * iT3, jz = dhorner(e[2], u) * iT3;
    const double cx = __builtin_fma(y, jz, -(z * jy)), cy = __builtin_fma(z, jx, -(x * jz));
    const double cz = __builtin_fma(x, jy, -(y * jx));
    const double n2 = __builtin_fma(cz, cz, __builtin_fma(cy, cy, cx * cx));
    const double d = __builtin_fma(z, z, __builtin_fma(y, y, x * x));
    return n2 == 0.0 ? 0.0 : n2 / (d * d);
}

// Golden-section ascent of omega^2 on [lo, hi]: the larger of the two interior points left after
// POLISH steps, one evaluation per step.  lo >= hi (a duplicate slot) returns at once with v < 0.
TGMS_HD void polish(const double (&e)[3][N + 1], double iT2, double iT3, double g, double lo, double hi, double& u,
                    double& v) {
    constexpr double PHI = 0.6180339887498949;
    u = lo;
    v = -1.0;
    if (!(hi > lo)) return;
    double a = lo, b = hi;
    double c = b - PHI * (b - a), d = a + PHI * (b - a);
    double fc = omega2_at(e, iT2, iT3, g, c), fd = omega2_at(e, iT2, iT3, g, d);
    for (int it = 0; it < POLISH; ++it) {
        const bool left = fc > fd;  // the maximum is in [a, d]; else in [c, b]
        b = left ? d : b;
        a = left ? a : c;
        const double x = left ? b - PHI * (b - a) : a + PHI * (b - a);
        const double fx = omega2_at(e, iT2, iT3, g, x);
        const double oc = c, ofc = fc;
        c = left ? x : d;
        fc = left ? fx : fd;
        d = left ? oc : x;
        fd = left ? ofc : fx;
    }
    u = fc > fd ? c : d;
    v = fc > fd ? fc : fd;
}

// The 26 coefficients of G of one segment: c [3][8] on t in [0, T].
TGMS_HD void rate_poly(const double* c, double T, double g, double (&G)[DG + 1]) {
    double e[3][N + 1], iT2;
    thrust::accel_poly(c, T, e, iT2);
    e[2][0] = __builtin_fma(g, T * T, e[2][0]);
    double Nn[2 * DC + 1], Dn[2 * N + 1];
    {
        double cr[3][DC + 1];
        TGMS_UNROLL
        for (int ax = 0; ax < 3; ++ax) {  // component ax of a x a', from the axes ax + 1 and ax + 2
            const int p = (ax + 1) % 3, q = (ax + 2) % 3;
            TGMS_UNROLL
            for (int k = 0; k <= DC; ++k) {
                double acc = 0.0;
                TGMS_UNROLL
                for (int i = 0; i <= N; ++i) {
                    const int j = k + 1 - i;
                    if (j > i && j <= N)
                        acc = __builtin_fma((double)(j - i), __builtin_fma(e[p][i], e[q][j], -(e[q][i] * e[p][j])), acc);
                }
                cr[ax][k] = acc;
            }
        }
        TGMS_UNROLL
        for (int m = 0; m <= 2 * DC; ++m) {
            double acc = 0.0;
            TGMS_UNROLL
            for (int i = 0; i <= DC; ++i) {
                const int k = m - i;
                if (k >= 0 && k <= DC) {
                    TGMS_UNROLL
                    for (int ax = 0; ax < 3; ++ax) acc = __builtin_fma(cr[ax][i], cr[ax][k], acc);
                }
            }
            Nn[m] = acc;
        }
    }
    TGMS_UNROLL
    for (int m = 0; m <= 2 * N; ++m) {
        double acc = 0.0;
        TGMS_UNROLL
        for (int i = 0; i <= N; ++i) {
            const int k = m - i;
            if (k >= 0 && k <= N) {
                TGMS_UNROLL
                for (int ax = 0; ax < 3; ++ax) acc = __builtin_fma(e[ax][i], e[ax][k], acc);
            }
        }
        Dn[m] = acc;
    }
    TGMS_UNROLL
    for (int k = 0; k <= DG; ++k) {
        double acc = 0.0;
        TGMS_UNROLL
        for (int i = 0; i <= 2 * DC; ++i) {
            const int m = k + 1 - i;
            if (m >= 0 && m <= 2 * N && i != 2 * m) acc = __builtin_fma((double)(i - 2 * m) * Nn[i], Dn[m], acc);
        }
        G[k] = acc;
    }
}

// What a segment leaves for the fold: the largest omega^2 over its candidates and the u where it
// is attained.  A candidate value that is not finite makes w2 NaN.
struct Item {
    double w2, u;
};

TGMS_HD void rate_item(const double* c, double T, double g, Item& it) {
    double s[DG];
    {
        double G[DG + 1];
        rate_poly(c, T, g, G);
        bounds::Ladder<DG, DG>::run(G, s);
    }
    double e[3][N + 1], iT2;
    thrust::accel_poly(c, T, e, iT2);
    const double iT3 = iT2 * (1.0 / T);
    double v = omega2_at(e, iT2, iT3, g, 0.0);
    double chk = v * 0.0;
    it.w2 = v;
    it.u = 0.0;
    TGMS_UNROLL
    for (int j = 0; j <= DG; ++j) {
        const double u = j < DG ? s[j] : 1.0;
        v = omega2_at(e, iT2, iT3, g, u);
        chk = __builtin_fma(v, 0.0, chk);
        it.u = v > it.w2 ? u : it.u;
        it.w2 = v > it.w2 ? v : it.w2;
    }
    TGMS_UNROLL
    for (int j = 0; j < DG; ++j) {  // the slots polished: candidates added, none replaced
        const double lo = 0.5 * ((j > 0 ? s[j - 1] : 0.0) + s[j]), hi = 0.5 * (s[j] + (j < DG - 1 ? s[j + 1] : 1.0));
        double u;
        polish(e, iT2, iT3, g, lo, hi, u, v);
        chk = __builtin_fma(v, 0.0, chk);
        it.u = v > it.w2 ? u : it.u;
        it.w2 = v > it.w2 ? v : it.w2;
    }
    if (chk != 0.0) it.w2 = __builtin_nan("");
}

// A trajectory's running maximum with the knot, the time and the u of the segment that holds
// it (thrust::Best: strict comparisons, so the earliest segment wins a tie).
struct Fold {
    thrust::Best hi;
    double knot;  // the left-to-right prefix sum of T: the next segment's knot, the duration at the end
    bool bad;
};

TGMS_HD Fold fold_init() { return Fold{{-__builtin_inf(), 0.0, 0.0, 0.0}, 0.0, false}; }

TGMS_HD void fold(Fold& f, const Item& it, double T) {
    f.bad = f.bad || !(it.w2 == it.w2);
    thrust::take(f.hi, it.w2 > f.hi.v, it.w2, f.knot, T, it.u);
    f.knot += T;
}

// The record and the flags of one trajectory from its fold; bad: an input was not finite, a
// time not positive or the segment count unusable.  The time by clearance::time_of's rule.  A
// strict comparison on the very value stored.
TGMS_HD int finish(const Fold& f, bool bad, double omega_limit, double (&rec)[TGMS_RATE_STRIDE]) {
    const double D = f.knot;
    rec[0] = sqrt(f.hi.v);
    rec[1] = fmin(__builtin_fma(f.hi.T, f.hi.u, f.hi.knot), D);
    const double fin = __builtin_fma(rec[1], 0.0, __builtin_fma(rec[0], 0.0, D * 0.0));
    if (bad || f.bad || fin != 0.0) {
        rec[0] = rec[1] = __builtin_nan("");
        return TGMS_FEAS_NONFINITE;
    }
    return rec[0] > omega_limit ? TGMS_RATE_HIGH : 0;
}

// A segment's own row: its maximum and the local time u T; NaN when its trajectory is unusable.
TGMS_HD void seg_row(const Item& it, double T, bool bad, double& w, double& t) {
    const double nan = __builtin_nan("");
    w = bad ? nan : sqrt(it.w2);
    t = bad ? nan : it.u * T;
}

}  // namespace rate
}  // namespace tgms
