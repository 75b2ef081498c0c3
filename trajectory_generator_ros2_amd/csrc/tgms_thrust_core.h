// tgms_thrust_core.h — continuous thrust and tilt bounds of one segment from differential
// flatness, shared by the gfx950 kernel (tgms_thrust.hip) and the host backend
// (tgms_host.cpp).  Plain C++17, as its siblings: the derivative ladder and the Horner chain are
// tgms_bounds_core.h's, the rule for a candidate's global time tgms_clearance_core.h's.
//
// The quantities.  A multirotor's mass-normalised thrust vector is f(t) = p''(t) + g e_z.  What
// saturates a motor is ||f||, what tips the vehicle is the angle between f and +z,
//     theta = atan2(sqrt(h), f_z),  h = f_x^2 + f_y^2,  theta in [0, pi].
// In normalised time u = t / T (a_j = c_j T^j) a segment's E = T^2 f has the coefficients
// e_j = (j + 2)(j + 1) a_{j+2}, j = 0..5, with g T^2 added to the z constant: three polynomials
// of degree 5 on [0, 1].
//   - Thrust.  ||E||^2 has degree 10, its derivative degree 9: bounds::norm_item<2> with the
//     gravity term.  One bounds::Ladder<9, 9> on the derivative gives the stationary points of
//     the minimum and of the maximum together.
//   - Tilt.  Where f != 0, theta' = (f_z h' - 2 h f_z') / (2 sqrt(h) ||f||^2), so the
//     stationary points are the roots of G = E_z H' - 2 H E_z' with H = E_x^2 + E_y^2 (the
//     common factor T^2 of E moves no root).  Both products have degree 14, and their leading
//     coefficients cancel identically (10 z_5 H_10 - 2 * 5 z_5 H_10), so G has degree <= 13:
//         G_k = sum_{i + m = k + 1} (m - 2 i) z_i H_m,  i = 0..5, m = 0..10, k = 0..13,
//     formed with 14 coefficients; the cancelling one is never computed.  bounds::Ladder<13, 13>
//     serves, the ladder of the separation and clearance kernels.  A point where h touches 0 is
//     a double root of H and a simple root of G, so it is found.
//   - Candidates.  u = 0, u = 1 and the slots of the two ladders.  The thrust ladder's slots
//     are candidates of the tilt as well: on a purely vertical trajectory H and G vanish
//     identically and the tilt ladder has nothing to find, but where f_z dips below zero theta
//     is pi, and the lowest f_z is a stationary point of ||f||^2.
//   - Values.  Every value is evaluated from the axis polynomials at the candidate: x, y, z =
//     E_ax(u) / T^2 with g added to z after the Horner chain, then the sum of squares, sqrt and
//     atan2; never from convolved coefficients, which only locate candidates.  A constant
//     trajectory therefore gives f = (0, 0, g) at every candidate: ||f|| == g to the bit
//     (sqrt(fl(g^2)) == g) and theta == 0.0; a purely vertical one has h == 0.0 and theta == 0.0
//     while f_z > 0.
//   - Error.  The argument of tgms_bounds_core.h carries over.  ||f||^2 is stationary at its
//     located roots: a slot off by delta = 2^-41 moves the value by <= (2/3) 10^2 (10^2 - 1)
//     delta^2 max < 1.4e-21 max||f||^2.  theta is stationary at the roots of G: with theta''
//     bounded by Markov on E and 1 / f_min, the same delta moves it by O(delta^2 (F / f_min)^2)
//     < 1e-20 for every ratio below 1e2.  What remains is the rounding of three degree-5
//     Horner chains in u (coefficients a_j = c_j T^j formed by repeated products, <= 8 ulp
//     each): about 20 ulp of sum_j |e_j| / T^2 per axis, which can exceed F where the terms of
//     a segment cancel.  Measured (k_thrust): 2e-15 F^2 on the squares and 1.6e-15 F
//     / f_min rad on the tilt on solved ragged batches, 1.7e-14 F^2 at worst (a trajectory
//     mixing T = 0.05 and T = 20), against the 1e-9 of tgms.h.  The roots of G themselves come
//     from convolved fp64 coefficients; where their rounding moves a root by eps, the value
//     moves by O(eps^2).
//   - Where thrust vanishes, theta jumps (by pi on a vertical trajectory): the stored tilt is
//     the maximum over the candidates and carries no accuracy claim there; f_min says so.
//   - Not a certificate, and a touch without a sign change may be skipped, as for the bounds.
// Body rate |f x p'''| / ||f||^2 is tgms_rate_core.h's: its stationary points are the roots of
// a polynomial of degree 25, a ladder of its own at one wave per SIMD.  j_peak / f_min from the
// bounds and thrust records is a sound but loose upper bound of it.
#pragma once

#include "tgms_bounds_core.h"

namespace tgms {
namespace thrust {

constexpr int N = 5;  // degree of an axis of E = T^2 (p'' + g e_z) in u

// One segment's E without the gravity term (e [3][6]) and 1 / T^2: c [3][8] on t in [0, T].
TGMS_HD void accel_poly(const double* c, double T, double (&e)[3][N + 1], double& iT2) {
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double w = 1.0;
        TGMS_UNROLL
        for (int j = 1; j < 8; ++j) {
            w *= T;
            if (j >= 2) e[ax][j - 2] = bounds::ffact(j, 2) * (c[ax * 8 + j] * w);
        }
    }
    const double iw = 1.0 / T;
    iT2 = iw * iw;
}

// f at u: the three Horner chains, 1 / T^2, and g added last.  h = f_x^2 + f_y^2.
TGMS_HD void force_at(const double (&e)[3][N + 1], double iT2, double g, double u, double& h, double& z) {
    const double x = bounds::horner<N>(e[0], u) * iT2, y = bounds::horner<N>(e[1], u) * iT2;
    z = __builtin_fma(bounds::horner<N>(e[2], u), iT2, g);
    h = __builtin_fma(y, y, x * x);
}

// What a segment leaves for the fold: the extremes over its candidates and the u where each
// is attained.  A candidate value that is not finite makes f2max NaN.
struct Item {
    double f2min, umin, f2max, umax, tilt, utilt;
};

TGMS_HD void tilt_take(double h, double z, double u, double& tilt, double& utilt, double& chk) {
    const double th = atan2(sqrt(h), z);
    chk = __builtin_fma(th, 0.0, chk);
    utilt = th > tilt ? u : utilt;
    tilt = th > tilt ? th : tilt;
}

// Thrust of one segment: ||f||^2 and theta at u = 0, 1 and the 9 slots of the ladder on
// (||E||^2)'.  Sets every field of it.
TGMS_HD void thrust_item(const double* c, double T, double g, Item& it) {
    constexpr int D = 2 * N - 1;
    double e[3][N + 1], iT2;
    accel_poly(c, T, e, iT2);
    double f[D + 1], s[D];
    {
        const double z0 = __builtin_fma(g, T * T, e[2][0]);  // the ladder's E_z constant
        TGMS_UNROLL
        for (int m = 1; m <= 2 * N; ++m) {  // f[m-1] = m * (coefficient m of sum_ax E_ax^2)
            double acc = 0.0;
            TGMS_UNROLL
            for (int i = 0; i <= N; ++i) {
                const int k = m - i;
                if (k >= 0 && k <= N) {
                    TGMS_UNROLL
                    for (int ax = 0; ax < 3; ++ax) {
                        const double a = (ax == 2 && i == 0) ? z0 : e[ax][i];
                        const double b = (ax == 2 && k == 0) ? z0 : e[ax][k];
                        acc = __builtin_fma(a, b, acc);
                    }
                }
            }
            f[m - 1] = (double)m * acc;
        }
    }
    bounds::Ladder<D, D>::run(f, s);
    double h, z, chk = 0.0;
    force_at(e, iT2, g, 0.0, h, z);
    double v = __builtin_fma(z, z, h);
    chk = __builtin_fma(v, 0.0, chk);
    it.f2min = it.f2max = v;
    it.umin = it.umax = it.utilt = 0.0;
    it.tilt = -1.0;
    tilt_take(h, z, 0.0, it.tilt, it.utilt, chk);
    TGMS_UNROLL
    for (int j = 0; j <= D; ++j) {
        const double u = j < D ? s[j] : 1.0;
        force_at(e, iT2, g, u, h, z);
        v = __builtin_fma(z, z, h);
        chk = __builtin_fma(v, 0.0, chk);
        it.umin = v < it.f2min ? u : it.umin;
        it.f2min = v < it.f2min ? v : it.f2min;
        it.umax = v > it.f2max ? u : it.umax;
        it.f2max = v > it.f2max ? v : it.f2max;
        tilt_take(h, z, u, it.tilt, it.utilt, chk);
    }
    if (chk != 0.0) it.f2max = __builtin_nan("");
}

// Tilt of one segment: theta at the 13 slots of the ladder on G, folded into it.tilt /
// it.utilt, which thrust_item has set (u = 0 and u = 1 are its candidates already).
TGMS_HD void tilt_item(const double* c, double T, double g, Item& it) {
    double e[3][N + 1], iT2;
    accel_poly(c, T, e, iT2);
    double G[14], s[13];
    {
        double H[2 * N + 1], zz[N + 1];
        TGMS_UNROLL
        for (int m = 0; m <= 2 * N; ++m) {  // H = E_x^2 + E_y^2
            double acc = 0.0;
            TGMS_UNROLL
            for (int i = 0; i <= N; ++i) {
                const int k = m - i;
                if (k >= 0 && k <= N) acc = __builtin_fma(e[0][i], e[0][k], __builtin_fma(e[1][i], e[1][k], acc));
            }
            H[m] = acc;
        }
        TGMS_UNROLL
        for (int i = 0; i <= N; ++i) zz[i] = e[2][i];
        zz[0] = __builtin_fma(g, T * T, zz[0]);
        TGMS_UNROLL
        for (int k = 0; k <= 13; ++k) {  // G_k = sum_{i + m = k + 1} (m - 2 i) z_i H_m
            double acc = 0.0;
            TGMS_UNROLL
            for (int i = 0; i <= N; ++i) {
                const int m = k + 1 - i;
                if (m >= 0 && m <= 2 * N && m != 2 * i) acc = __builtin_fma((double)(m - 2 * i) * zz[i], H[m], acc);
            }
            G[k] = acc;
        }
    }
    bounds::Ladder<13, 13>::run(G, s);
    double h, z, chk = 0.0;
    TGMS_UNROLL
    for (int j = 0; j < 13; ++j) {
        force_at(e, iT2, g, s[j], h, z);
        tilt_take(h, z, s[j], it.tilt, it.utilt, chk);
    }
    if (chk != 0.0) it.f2max = __builtin_nan("");
}

// A trajectory's running extremes: each value with the knot, the time and the u of the
// segment that holds it.  Strict comparisons, so the earliest segment wins a tie.
struct Best {
    double v, knot, T, u;
};

TGMS_HD void take(Best& b, bool better, double v, double knot, double T, double u) {
    b.v = better ? v : b.v;
    b.knot = better ? knot : b.knot;
    b.T = better ? T : b.T;
    b.u = better ? u : b.u;
}

struct Fold {
    Best lo, hi, tilt;
    double knot;  // the left-to-right prefix sum of T: the next segment's knot, the duration at the end
    bool bad;
};

TGMS_HD Fold fold_init() {
    const double inf = __builtin_inf();
    return Fold{{inf, 0.0, 0.0, 0.0}, {-inf, 0.0, 0.0, 0.0}, {-inf, 0.0, 0.0, 0.0}, 0.0, false};
}

TGMS_HD void fold(Fold& f, const Item& it, double T) {
    f.bad = f.bad || !(it.f2min == it.f2min) || !(it.f2max == it.f2max) || !(it.tilt == it.tilt);
    take(f.lo, it.f2min < f.lo.v, it.f2min, f.knot, T, it.umin);
    take(f.hi, it.f2max > f.hi.v, it.f2max, f.knot, T, it.umax);
    take(f.tilt, it.tilt > f.tilt.v, it.tilt, f.knot, T, it.utilt);
    f.knot += T;
}

// The record and the flags of one trajectory from its fold; bad: an input was not finite, a
// time not positive or the segment count unusable.  Times by clearance::time_of's rule (the
// knot's prefix sum plus the local time, clamped to the duration).  Strict comparisons on the
// very values stored.
TGMS_HD int finish(const Fold& f, bool bad, const tgms_thrust_limits& lim, double (&rec)[TGMS_THRUST_STRIDE]) {
    const double D = f.knot;
    rec[0] = sqrt(f.lo.v);
    rec[1] = fmin(__builtin_fma(f.lo.T, f.lo.u, f.lo.knot), D);
    rec[2] = sqrt(f.hi.v);
    rec[3] = fmin(__builtin_fma(f.hi.T, f.hi.u, f.hi.knot), D);
    rec[4] = f.tilt.v;
    rec[5] = fmin(__builtin_fma(f.tilt.T, f.tilt.u, f.tilt.knot), D);
    double fin = D * 0.0;
    TGMS_UNROLL
    for (int i = 0; i < TGMS_THRUST_STRIDE; ++i) fin = __builtin_fma(rec[i], 0.0, fin);
    if (bad || f.bad || fin != 0.0) {
        TGMS_UNROLL
        for (int i = 0; i < TGMS_THRUST_STRIDE; ++i) rec[i] = __builtin_nan("");
        return TGMS_FEAS_NONFINITE;
    }
    int fl = 0;
    fl |= rec[0] < lim.f_min ? TGMS_THRUST_LOW : 0;
    fl |= rec[2] > lim.f_max ? TGMS_THRUST_HIGH : 0;
    fl |= rec[4] > lim.tilt_max ? TGMS_THRUST_TILT : 0;
    return fl;
}

}  // namespace thrust
}  // namespace tgms
