// tgms_host.cpp — the explicit host backend of the C ABI (tgms_create_host, include/tgms.h)
// for BASELINE config 1: "single goal, 3-segment order-7 min-snap via the CPU
// TrajectoryGenerator (ROS2 node up, no GPU)".  The reference generates its goals on the
// rclcpp executor thread's CPU (src/TrajectoryGenerator.cpp:54-57, :71); a node with no GPU
// gets the same MinSnap primitive from this file when its YAML asks for
// `minsnap_backend: host`.  It is never a fallback: tgms_create still fails with
// TGMS_ERR_NO_DEVICE when no GPU exists, and a host handle accepts only the host-pointer
// solve / sample entry points (B = 1 at config 1; any B works).
//
// The solve is the reduced formulation of DESIGN.md §2 (the product's own math, written
// from the Hermite elimination, not from oracle/): per axis the SPD block-tridiagonal
// system over the free knot derivatives u_k = (v, a, j), k = 1..M-1, with 3x3 blocks
//     H_kk    = KEE o r_{k-1}^(5-d-e) + KSS o r_k^(5-d-e),   H_k,k+1 = KSE o r_k^(5-d-e)
//     rhs_k   = -KEP r_{k-1}^(6-d) (w_k - w_{k-1}) - KSP r_k^(6-d) (w_{k+1} - w_k)
// (r_i = 1/T_i; the same integer matrices as the kernels, tgms_device.h), shared by the
// three axes, solved by a one-sided block LDL^T (block Thomas: S_k = H_kk - C^T S^-1 C),
// then each segment's septic Hermite data converted to monomial coefficients.  The sampler
// evaluates p/v/a/j by Horner in local time with the GPU sampler's conventions (segment
// scan, pinned last sample, yaw).  tests/test_host_backend.py holds both to the oracle and
// the exact goldens at 1e-9.
#include "tgms_host.h"

#include <cfloat>
#include <cmath>
#include <vector>
#include <algorithm>

#include "tgms_bounds_core.h"
#include "tgms_clearance_core.h"
#include "tgms_corridor_core.h"
#include "tgms_corridor_split_core.h"
#include "tgms_cut_core.h"
#include "tgms_dilate_core.h"
#include "tgms_edt_core.h"
#include "tgms_field_core.h"
#include "tgms_inflate_core.h"
#include "tgms_neighbors_core.h"
#include "tgms_separation_core.h"
#include "tgms_repair_core.h"
#include "tgms_retime_core.h"
#include "tgms_reroute_core.h"
#include "tgms_subdivide_core.h"
#include "tgms_rate_core.h"
#include "tgms_thrust_core.h"

namespace tgms {
namespace host {
namespace {

constexpr double KSS[3][3] = {{25920, 5400, 480}, {5400, 1200, 120}, {480, 120, 16}};
constexpr double KEE[3][3] = {{25920, -5400, 480}, {-5400, 1200, -120}, {480, -120, 16}};
constexpr double KSE[3][3] = {{24480, -4680, 360}, {4680, -840, 60}, {360, -60, 4}};
constexpr double KSP[3] = {-50400, -10080, -840};
constexpr double KEP[3] = {-50400, 10080, -840};

bool finite(double v) { return v * 0.0 == 0.0; }

// r^0 .. r^7
void powers(double r, double (&p)[8]) {
    p[0] = 1.0;
    for (int k = 1; k < 8; ++k) p[k] = p[k - 1] * r;
}

struct Ldl {  // LDL^T of an SPD 3x3 block: reciprocal pivots, unit-lower multipliers
    double i0, i1, i2, l10, l20, l21;
};

bool factor(const double (&D)[3][3], Ldl& f) {
    const double p0 = D[0][0];
    f.i0 = 1.0 / p0;
    f.l10 = D[0][1] * f.i0;
    f.l20 = D[0][2] * f.i0;
    const double p1 = D[1][1] - f.l10 * D[0][1];
    f.i1 = 1.0 / p1;
    const double t12 = D[1][2] - f.l20 * D[0][1];
    f.l21 = t12 * f.i1;
    const double p2 = D[2][2] - f.l20 * D[0][2] - f.l21 * t12;
    f.i2 = 1.0 / p2;
    return p0 > 0.0 && p1 > 0.0 && p2 > 0.0;
}

void solve3(const Ldl& f, const double (&b)[3], double (&x)[3]) {
    const double y1 = b[1] - f.l10 * b[0];
    const double y2 = b[2] - f.l20 * b[0] - f.l21 * y1;
    x[2] = y2 * f.i2;
    x[1] = y1 * f.i1 - f.l21 * x[2];
    x[0] = b[0] * f.i0 - f.l10 * x[1] - f.l20 * x[2];
}

// Septic Hermite data of one axis of a segment (positions w0, w1; derivatives (v, a, j) at
// both ends) -> ascending monomial coefficients in local time, in r = 1/T scaled
// variables: c_k = r^(k-3) P_k for k >= 4, P linear in ((w1 - w0) r^3, v r^2, a r, j).
void hermite(double w0, double w1, const double (&s)[3], const double (&e)[3], double r, double* c) {
    const double r2 = r * r, r3 = r2 * r, r4 = r2 * r2;
    const double D = (w1 - w0) * r3;
    const double V0 = s[0] * r2, A0 = s[1] * r, J0 = s[2], V1 = e[0] * r2, A1 = e[1] * r, J1 = e[2];
    const double P4 = 35.0 * D - 20.0 * V0 - 5.0 * A0 - (2.0 / 3.0) * J0 - 15.0 * V1 + 2.5 * A1 - (1.0 / 6.0) * J1;
    const double P5 = -84.0 * D + 45.0 * V0 + 10.0 * A0 + J0 + 39.0 * V1 - 7.0 * A1 + 0.5 * J1;
    const double P6 = 70.0 * D - 36.0 * V0 - 7.5 * A0 - (2.0 / 3.0) * J0 - 34.0 * V1 + 6.5 * A1 - 0.5 * J1;
    const double P7 = -20.0 * D + 10.0 * V0 + 2.0 * A0 + (1.0 / 6.0) * J0 + 10.0 * V1 - 2.0 * A1 + (1.0 / 6.0) * J1;
    c[0] = w0;
    c[1] = s[0];
    c[2] = 0.5 * s[1];
    c[3] = s[2] * (1.0 / 6.0);
    c[4] = P4 * r;
    c[5] = P5 * r2;
    c[6] = P6 * r3;
    c[7] = P7 * r4;
}

// p, v, a, j of one segment (c [3][8]) at local time lt into o[q*3 + axis]: d^q/dt^q by
// Horner on j!/(j-q)! c_j, the GPU sampler's four FMA chains.
void pvaj(const double* c3, double lt, double* o) {
    for (int a = 0; a < 3; ++a) {
        const double* c = c3 + a * 8;
        for (int q = 0; q < 4; ++q) {
            auto coef = [&](int j) {
                double f = 1.0;
                for (int m = 0; m < q; ++m) f *= (double)(j - m);
                return f * c[j];
            };
            double s = coef(7);
            for (int j = 6; j >= q; --j) s = std::fma(s, lt, coef(j));
            o[q * 3 + a] = s;
        }
    }
}

}  // namespace

int solve(int M, const double* W, const double* T, const double* ED, double* C) {
    const int n = M * 24;
    for (int q = 0; q < n; ++q) C[q] = 0.0;
    if (M < 1 || M > TGMS_MAX_SEGMENTS) return TGMS_ERR_INVALID_ARG;
    bool ok = true;
    for (int i = 0; i < M; ++i) ok = ok && T[i] > 0.0 && T[i] <= DBL_MAX;
    for (int q = 0; q < (M + 1) * 3; ++q) ok = ok && finite(W[q]);
    if (ED)
        for (int q = 0; q < 18; ++q) ok = ok && finite(ED[q]);
    if (!ok) return TGMS_ERR_INVALID_ARG;

    double rp[TGMS_MAX_SEGMENTS][8];
    for (int i = 0; i < M; ++i) powers(1.0 / T[i], rp[i]);
    // knot derivatives [knot][derivative][axis]: knot 0 and M from the end derivatives
    double x[TGMS_MAX_SEGMENTS + 1][3][3] = {};
    for (int d = 0; d < 3; ++d)
        for (int a = 0; a < 3; ++a) {
            x[0][d][a] = ED ? ED[d * 3 + a] : 0.0;
            x[M][d][a] = ED ? ED[9 + d * 3 + a] : 0.0;
        }
    const int NK = M - 1;  // interior knots 1..M-1, index k
    Ldl F[TGMS_MAX_SEGMENTS];
    double G[TGMS_MAX_SEGMENTS][3][3];  // G_k = S_k^-1 C_k (C_k couples knots k and k+1)
    bool spd = true;
    for (int k = 1; k <= NK; ++k) {
        const double(&pp)[8] = rp[k - 1];
        const double(&pn)[8] = rp[k];
        double S[3][3];
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) S[d][e] = KEE[d][e] * pp[5 - d - e] + KSS[d][e] * pn[5 - d - e];
        if (k >= 2) {  // S_k = H_kk - C_{k-1}^T G_{k-1}
            const double(&pc)[8] = rp[k - 1];
            for (int d = 0; d < 3; ++d)
                for (int e = 0; e < 3; ++e) {
                    double acc = 0.0;
                    for (int f = 0; f < 3; ++f) acc += KSE[f][d] * pc[5 - f - d] * G[k - 1][f][e];
                    S[d][e] -= acc;
                }
        }
        spd = factor(S, F[k]) && spd;
        if (k < NK) {  // G_k = S_k^-1 C_k, C_k[d][e] = KSE[d][e] r_k^(5-d-e)
            for (int e = 0; e < 3; ++e) {
                const double col[3] = {KSE[0][e] * pn[5 - e], KSE[1][e] * pn[4 - e], KSE[2][e] * pn[3 - e]};
                double g[3];
                solve3(F[k], col, g);
                for (int d = 0; d < 3; ++d) G[k][d][e] = g[d];
            }
        }
    }
    if (!spd) return TGMS_ERR_SINGULAR;
    // forward: z_k = y_k - G_{k-1}^T z_{k-1} (C^T S^-1 = G^T: S symmetric), g_k = S_k^-1 z_k,
    // then back: x_k = g_k - G_k x_{k+1}, per axis
    for (int a = 0; a < 3; ++a) {
        double z[TGMS_MAX_SEGMENTS][3];
        for (int k = 1; k <= NK; ++k) {
            const double(&pp)[8] = rp[k - 1];
            const double(&pn)[8] = rp[k];
            const double wp = W[(k - 1) * 3 + a], wk = W[k * 3 + a], wn = W[(k + 1) * 3 + a];
            double y[3];
            for (int d = 0; d < 3; ++d)
                y[d] = -KEP[d] * pp[6 - d] * (wk - wp) - KSP[d] * pn[6 - d] * (wn - wk);
            if (k == 1)  // start derivatives through C_0
                for (int d = 0; d < 3; ++d)
                    for (int e = 0; e < 3; ++e) y[d] -= KSE[e][d] * pp[5 - d - e] * x[0][e][a];
            if (k == NK)  // final derivatives through C_{M-1}
                for (int d = 0; d < 3; ++d)
                    for (int e = 0; e < 3; ++e) y[d] -= KSE[d][e] * pn[5 - d - e] * x[M][e][a];
            if (k >= 2)
                for (int d = 0; d < 3; ++d)
                    for (int f = 0; f < 3; ++f) y[d] -= G[k - 1][f][d] * z[k - 1][f];
            for (int d = 0; d < 3; ++d) z[k][d] = y[d];
        }
        for (int k = NK; k >= 1; --k) {
            double g[3];
            solve3(F[k], z[k], g);
            if (k < NK)
                for (int d = 0; d < 3; ++d)
                    for (int e = 0; e < 3; ++e) g[d] -= G[k][d][e] * x[k + 1][e][a];
            for (int d = 0; d < 3; ++d) x[k][d][a] = g[d];
        }
    }
    double fin = 0.0;
    for (int i = 0; i < M; ++i)
        for (int a = 0; a < 3; ++a) {
            const double s[3] = {x[i][0][a], x[i][1][a], x[i][2][a]};
            const double e[3] = {x[i + 1][0][a], x[i + 1][1][a], x[i + 1][2][a]};
            double* c = C + (i * 3 + a) * 8;
            hermite(W[i * 3 + a], W[(i + 1) * 3 + a], s, e, rp[i][1], c);
            for (int j = 0; j < 8; ++j) fin += c[j] * 0.0;
        }
    if (!finite(fin)) {
        for (int q = 0; q < n; ++q) C[q] = 0.0;
        return TGMS_ERR_NONFINITE;
    }
    return TGMS_OK;
}

void sample(int M, const double* C, const double* T, const double* W, const double* ED, double dt, int yaw_mode,
            double yaw_const, int64_t ns, double* out) {
    double tau[TGMS_MAX_SEGMENTS + 1];
    tau[0] = 0.0;
    double acc = 0.0;
    for (int i = 0; i < M; ++i) tau[i + 1] = (acc += T[i]);  // the same order as tgms_sample_offsets
    int i = 0;
    double t_cur = 0.0, t_next = M > 1 ? tau[1] : 0.0;
    for (int64_t k = 0; k < ns; ++k) {
        double* o = out + k * TGMS_GOAL_STRIDE;
        if (k < ns - 1) {
            const double t = (double)k * dt;
            while (i + 1 < M && t_next <= t) {  // segment scan, as the GPU sampler's
                ++i;
                t_cur = t_next;
                t_next = tau[i + 1 < M ? i + 1 : M];
            }
            pvaj(C + i * 24, t - t_cur, o);
        } else {  // the last sample, pinned to the final waypoint and end derivatives
            for (int a = 0; a < 3; ++a) {
                o[a] = W[M * 3 + a];
                o[3 + a] = ED ? ED[9 + a] : 0.0;
                o[6 + a] = ED ? ED[12 + a] : 0.0;
                o[9 + a] = ED ? ED[15 + a] : 0.0;
            }
        }
        const double vx = o[3], vy = o[4], ax = o[6], ay = o[7];
        const double s2 = vx * vx + vy * vy;
        const bool yv = yaw_mode == TGMS_YAW_VELOCITY && s2 > 1e-6;
        o[12] = yv ? std::atan2(vy, vx) : yaw_const;
        o[13] = yv ? (vx * ay - vy * ax) / s2 : 0.0;
    }
}

int extrema(int M, const double* C, const double* T, const double* W, const double* ED, double dt,
            const tgms_limits* lim, double* rec) {
    double tau[TGMS_MAX_SEGMENTS + 1];
    tau[0] = 0.0;
    double acc = 0.0, chk = 0.0;  // chk: 0 while everything read is finite
    for (int i = 0; i < M; ++i) tau[i + 1] = (acc += T[i]);  // the same order as tgms_sample_offsets
    for (int q = 0; q < M * 24; ++q) chk += C[q] * 0.0;
    for (int a = 0; a < 3; ++a) chk += W[M * 3 + a] * 0.0;
    for (int q = 9; ED && q < 18; ++q) chk += ED[q] * 0.0;
    const int64_t ns = tgms_sample_count(acc, dt);  // 0: the sum is negative or not finite
    double lo[3], hi[3], n2[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 3; ++a) lo[a] = HUGE_VAL, hi[a] = -HUGE_VAL;
    bool bad = !finite(chk) || ns < 2 || !(std::ceil(acc / dt - 1e-9) < 9007199254740992.0);
    int i = 0;
    double t_cur = 0.0, t_next = M > 1 ? tau[1] : 0.0;
    for (int64_t k = 0; !bad && k < ns; ++k) {
        double o[12];
        if (k < ns - 1) {
            const double t = (double)k * dt;
            while (i + 1 < M && t_next <= t) {  // segment scan, as sample()'s
                ++i;
                t_cur = t_next;
                t_next = tau[i + 1 < M ? i + 1 : M];
            }
            pvaj(C + i * 24, t - t_cur, o);
        } else {  // the pinned last sample
            for (int a = 0; a < 3; ++a) {
                o[a] = W[M * 3 + a];
                for (int q = 1; q < 4; ++q) o[q * 3 + a] = ED ? ED[9 + (q - 1) * 3 + a] : 0.0;
            }
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::fmin(lo[a], o[a]);
            hi[a] = std::fmax(hi[a], o[a]);
        }
        for (int q = 0; q < 3; ++q) {
            const double* d = o + 3 + q * 3;
            n2[q] = std::fmax(n2[q], d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        }
    }
    for (int a = 0; a < 3; ++a) {
        rec[a] = lo[a];
        rec[3 + a] = hi[a];
        rec[6 + a] = std::sqrt(n2[a]);
    }
    rec[9] = acc;
    for (int q = 0; q < TGMS_EXTREMA_STRIDE; ++q) bad = bad || !finite(rec[q]);
    if (bad) {
        for (int q = 0; q < TGMS_EXTREMA_STRIDE; ++q) rec[q] = NAN;
        return TGMS_FEAS_NONFINITE;
    }
    int fl = 0;
    if (lim) {  // strict comparisons on the stored values
        for (int a = 0; a < 3; ++a)
            if (rec[a] < lim->pmin[a] || rec[3 + a] > lim->pmax[a]) fl |= TGMS_FEAS_BOX;
        if (rec[6] > lim->v_max) fl |= TGMS_FEAS_SPEED;
        if (rec[7] > lim->a_max) fl |= TGMS_FEAS_ACCEL;
        if (rec[8] > lim->j_max) fl |= TGMS_FEAS_JERK;
    }
    return fl;
}

int bounds(int M, const double* C, const double* T, const tgms_limits* lim, double* rec) {
    const double inf = HUGE_VAL;
    const tgms_limits none{{-inf, -inf, -inf}, {inf, inf, inf}, inf, inf, inf};
    double lo[3], hi[3], n2[3] = {0.0, 0.0, 0.0}, acc = 0.0, chk = 0.0;
    for (int a = 0; a < 3; ++a) lo[a] = inf, hi[a] = -inf;
    bool bad = false;
    for (int i = 0; i < M; ++i) {
        acc += T[i];  // the same order as tgms_sample_offsets
        chk += T[i] * 0.0;
        bad = bad || !(T[i] > 0.0);
    }
    for (int q = 0; q < M * 24; ++q) chk += C[q] * 0.0;
    bad = bad || !finite(chk);
    for (int i = 0; !bad && i < M; ++i) {  // tgms_bounds_core.h: the kernel's items, one after the other
        const double* c = C + i * 24;
        for (int a = 0; a < 3; ++a) {
            double l, h;
            tgms::bounds::position_item(c + a * 8, T[i], l, h);
            lo[a] = std::fmin(lo[a], l);
            hi[a] = std::fmax(hi[a], h);
        }
        n2[0] = std::fmax(n2[0], tgms::bounds::norm_item<1>(c, T[i]));
        n2[1] = std::fmax(n2[1], tgms::bounds::norm_item<2>(c, T[i]));
        n2[2] = std::fmax(n2[2], tgms::bounds::norm_item<3>(c, T[i]));
    }
    double r[TGMS_EXTREMA_STRIDE];
    const int fl = tgms::bounds::finish(lo, hi, n2, acc, bad, lim ? *lim : none, r);
    for (int q = 0; q < TGMS_EXTREMA_STRIDE; ++q) rec[q] = r[q];
    return fl;
}

int thrust(int M, const double* C, const double* T, double g, const tgms_thrust_limits* lim, double* rec) {
    namespace th = tgms::thrust;
    const tgms_thrust_limits none{-HUGE_VAL, HUGE_VAL, HUGE_VAL};
    double chk = 0.0;
    bool bad = M < 1 || M > TGMS_MAX_SEGMENTS;
    for (int i = 0; !bad && i < M; ++i) {
        chk += T[i] * 0.0;
        bad = bad || !(T[i] > 0.0);
    }
    for (int q = 0; !bad && q < M * 24; ++q) chk += C[q] * 0.0;
    bad = bad || !finite(chk);
    th::Fold f = th::fold_init();
    for (int i = 0; !bad && i < M; ++i) {  // tgms_thrust_core.h: the kernel's items, one after the other
        th::Item it;
        th::thrust_item(C + i * 24, T[i], g, it);
        th::tilt_item(C + i * 24, T[i], g, it);
        th::fold(f, it, T[i]);
    }
    double r[TGMS_THRUST_STRIDE];
    const int fl = th::finish(f, bad, lim ? *lim : none, r);
    for (int q = 0; q < TGMS_THRUST_STRIDE; ++q) rec[q] = r[q];
    return fl;
}

int rate(int M, const double* C, const double* T, double g, double omega_limit, double* rec, double* seg_rec) {
    namespace rt = tgms::rate;
    const bool count_ok = M >= 1 && M <= TGMS_MAX_SEGMENTS;
    double chk = 0.0;
    bool bad = !count_ok;
    for (int i = 0; !bad && i < M; ++i) {
        chk += T[i] * 0.0;
        bad = bad || !(T[i] > 0.0);
    }
    for (int q = 0; !bad && q < M * 24; ++q) chk += C[q] * 0.0;
    bad = bad || !finite(chk);
    rt::Item items[TGMS_MAX_SEGMENTS];
    rt::Fold f = rt::fold_init();
    for (int i = 0; !bad && i < M; ++i) {  // tgms_rate_core.h: the kernel's items, one after the other
        rt::rate_item(C + i * 24, T[i], g, items[i]);
        rt::fold(f, items[i], T[i]);
    }
    double r[TGMS_RATE_STRIDE];
    const int fl = rt::finish(f, bad, omega_limit, r);
    if (rec)
        for (int q = 0; q < TGMS_RATE_STRIDE; ++q) rec[q] = r[q];
    for (int i = 0; seg_rec && count_ok && i < M; ++i) {
        const rt::Item none{0.0, 0.0};
        const bool nan = (fl & TGMS_FEAS_NONFINITE) != 0;
        rt::seg_row(nan ? none : items[i], nan ? 0.0 : T[i], nan, seg_rec[i * TGMS_RATE_STRIDE],
                    seg_rec[i * TGMS_RATE_STRIDE + 1]);
    }
    return fl;
}

int dilate(int M, const double* C, const double* T, double g, const tgms::dilate::Lim& lim, double s_lo, double s_hi,
           double* scale, int* active, double* T_out, double* C_out) {
    namespace th = tgms::thrust;
    namespace dl = tgms::dilate;
    double chk = 0.0;
    const bool badM = M < 1 || M > TGMS_MAX_SEGMENTS;
    bool bad = badM;
    for (int i = 0; !bad && i < M; ++i) {
        chk += T[i] * 0.0;
        bad = bad || !(T[i] > 0.0);
    }
    for (int q = 0; !bad && q < M * 24; ++q) chk += C[q] * 0.0;
    bad = bad || !finite(chk);
    const double inf = HUGE_VAL;
    double n2[3] = {0.0, 0.0, 0.0};
    for (int i = 0; !bad && i < M; ++i) {  // phase 1 of the kernel: the peaks, unchecked ones skipped
        const double r[3] = {lim.v_max < inf ? tgms::bounds::norm_item<1>(C + i * 24, T[i]) : 0.0,
                             tgms::bounds::norm_item<2>(C + i * 24, T[i]),
                             lim.j_max < inf ? tgms::bounds::norm_item<3>(C + i * 24, T[i]) : 0.0};
        for (int a = 0; a < 3; ++a) n2[a] = std::fmax(n2[a], r[a] == r[a] ? r[a] : inf);
    }
    dl::Search q;
    dl::init(q, bad, dl::Kin{std::sqrt(n2[0]), std::sqrt(n2[1]), std::sqrt(n2[2])}, g, lim, s_lo, s_hi);
    for (int round = 0; q.stage != dl::ST_DONE && round < dl::MAX_EVALS + 3; ++round) {  // phase 2: the search
        const double gp = g / q.x;
        th::Fold f = th::fold_init();
        for (int i = 0; i < M; ++i) {
            th::Item it;
            th::thrust_item(C + i * 24, T[i], gp, it);
            if (lim.tilt < inf) th::tilt_item(C + i * 24, T[i], gp, it);
            th::fold(f, it, T[i]);
        }
        dl::step(q, f, lim, s_lo, s_hi);
    }
    const bool keep = !(q.s == q.s);  // unusable: the rows are copied unchanged
    const double r = keep ? 1.0 : 1.0 / q.s;
    if (!badM) {  // phase 3; the inputs may be the outputs, each element is read before it is written
        for (int e = 0; C_out && e < M * 24; ++e) C_out[e] = keep ? C[e] : dl::scaled(C[e], e & 7, r);
        for (int i = 0; T_out && i < M; ++i) T_out[i] = keep ? T[i] : q.s * T[i];
    }
    if (scale) *scale = q.s;
    if (active) *active = q.active;
    return q.flags;
}

int retime(int M, const double* C, const double* T, const tgms::retime::Lim& lim, double s_lo, double s_hi,
           double* T_out, double* seg_rec, double* rec) {
    namespace rt = tgms::retime;
    double chk = 0.0;
    bool bad = false;
    for (int i = 0; i < M; ++i) {
        chk += T[i] * 0.0;
        bad = bad || !(T[i] > 0.0);
    }
    for (int q = 0; q < M * 24; ++q) chk += C[q] * 0.0;
    bad = bad || !finite(chk);
    const double inf = HUGE_VAL;
    const bool run[3] = {seg_rec || lim.v_max < inf, seg_rec || lim.a_max < inf, seg_rec || lim.j_max < inf};
    rt::Seg g[TGMS_MAX_SEGMENTS];
    rt::Fold f = rt::fold_init();
    for (int i = 0; !bad && i < M; ++i) {  // the kernel's phases, unchecked ones skipped when no row is asked for
        const double* c = C + i * 24;
        const double n2[3] = {run[0] ? tgms::bounds::norm_item<1>(c, T[i]) : 0.0,
                              run[1] ? tgms::bounds::norm_item<2>(c, T[i]) : 0.0,
                              run[2] ? tgms::bounds::norm_item<3>(c, T[i]) : 0.0};
        g[i] = rt::segment(n2, T[i], lim, s_lo, s_hi);
        rt::fold(f, i, g[i].row[3], g[i].s, T[i], g[i].T_out);
    }
    double r[TGMS_RETIME_REC];
    const int fl = rt::finish(f, bad, s_hi, r);
    const bool nan = (fl & TGMS_FEAS_NONFINITE) != 0;
    for (int q = 0; rec && q < TGMS_RETIME_REC; ++q) rec[q] = r[q];
    for (int i = 0; i < M; ++i) {  // T_out may be T: every product was formed above
        for (int q = 0; seg_rec && q < TGMS_RETIME_STRIDE; ++q) seg_rec[i * TGMS_RETIME_STRIDE + q] = nan ? NAN : g[i].row[q];
        if (T_out) T_out[i] = nan ? T[i] : g[i].T_out;
    }
    return fl;
}

int separation(int Mi, const double* ci, const double* Ti, double t0i, int Mj, const double* cj, const double* Tj,
               double t0j, const double* scale, double r_min, double* rec) {
    namespace sp = tgms::separation;
    const int M[2] = {Mi, Mj};
    const double* T[2] = {Ti, Tj};
    const double* C[2] = {ci, cj};
    const double t0[2] = {t0i, t0j};
    const double sc[3] = {scale[0], scale[1], scale[2]};
    double kn[2][sp::MAX_KNOTS], tl[2] = {0.0, 0.0};
    bool bad = false;
    for (int s = 0; s < 2; ++s) {
        bad = bad || M[s] < 1 || M[s] > TGMS_MAX_SEGMENTS || !finite(t0[s]);
        if (bad) break;
        double acc = 0.0;
        kn[s][0] = t0[s];
        for (int m = 0; m < M[s]; ++m) {
            tl[s] = T[s][m];
            bad = bad || !(tl[s] > 0.0);
            acc += tl[s];  // the same order as the extrema record's duration
            kn[s][m + 1] = t0[s] + acc;
            bad = bad || !finite(kn[s][m + 1]);
        }
    }
    double best = HUGE_VAL, at = 0.0;
    if (!bad) {
        double mk[sp::MAX_MERGED];
        int32_t sg[sp::MAX_INTERVALS];
        sp::merge_knots(kn[0], Mi, kn[1], Mj, mk, sg);
        for (int q = 0; q < Mi + Mj + 1; ++q) {
            const double a = mk[q], b = mk[q + 1], h = b - a;
            const sp::Side si = sp::side_of((sg[q] & 255) - 1, Mi, kn[0], tl[0], a, h);
            const sp::Side sj = sp::side_of((sg[q] >> 8) - 1, Mj, kn[1], tl[1], a, h);
            double d2, u;
            sp::interval_item(C[0] + si.seg * 24, si, C[1] + sj.seg * 24, sj, sc, h, d2, u);
            sp::fold(d2, std::fmin(std::fma(h, u, a), b), best, at, bad);
        }
    }
    double r[TGMS_SEP_STRIDE];
    const int fl = sp::finish(best, at, bad, r_min, r);
    for (int q = 0; q < TGMS_SEP_STRIDE; ++q) rec[q] = r[q];
    return fl;
}

void neighbors(int32_t B, const int32_t* so, const double* T, const double* C, const double* t0, const double* scale,
               double r_min, double* near, int32_t* nbr, int32_t* count, int32_t* tested, int32_t* flags) {
    namespace nb = tgms::neighbors;
    const double sc[3] = {scale[0], scale[1], scale[2]};
    const double r2 = nb::cull_r2(r_min);
    constexpr int BX = nb::BOXES * nb::BOX_STRIDE;
    std::vector<int32_t> M((size_t)B);
    std::vector<double> ub((size_t)B * nb::BOX_STRIDE), kn((size_t)B * nb::KNOT_STRIDE), bx((size_t)B * BX);
    for (int32_t b = 0; b < B; ++b) {
        const int m = so[b + 1] - so[b];
        const bool ok = nb::vehicle_boxes(m, C + (int64_t)so[b] * 24, T + so[b], t0 ? t0[b] : 0.0,
                                          &kn[(size_t)b * nb::KNOT_STRIDE], &bx[(size_t)b * BX],
                                          &ub[(size_t)b * nb::BOX_STRIDE]);
        M[b] = ok ? m : 0;
    }
    for (int32_t i = 0; i < B; ++i) {
        nb::Row row = nb::row_init();
        for (int32_t j = 0; j < B && M[i] > 0; ++j) {
            if (j == i || M[j] == 0) continue;
            if (!(nb::gap2(&ub[(size_t)i * nb::BOX_STRIDE], &ub[(size_t)j * nb::BOX_STRIDE], sc) < r2)) continue;
            if (!nb::walk(&kn[(size_t)i * nb::KNOT_STRIDE], M[i], &bx[(size_t)i * BX], &kn[(size_t)j * nb::KNOT_STRIDE],
                          M[j], &bx[(size_t)j * BX], sc, r2))
                continue;
            double rec[TGMS_SEP_STRIDE];
            const int fl = separation(M[i], C + (int64_t)so[i] * 24, T + so[i], t0 ? t0[i] : 0.0, M[j],
                                      C + (int64_t)so[j] * 24, T + so[j], t0 ? t0[j] : 0.0, sc, r_min, rec);
            nb::row_update(row, j, rec, fl);
        }
        double rec[TGMS_SEP_STRIDE];
        int32_t nb_i, ct;
        const int fl = nb::row_finish(row, M[i] > 0, rec, nb_i, ct);
        if (near) std::copy(rec, rec + TGMS_SEP_STRIDE, near + (int64_t)i * TGMS_SEP_STRIDE);
        if (nbr) nbr[i] = nb_i;
        if (count) count[i] = ct;
        if (tested) tested[i] = (fl & TGMS_SEP_NONFINITE) ? 0 : row.tested;
        if (flags) flags[i] = fl;
    }
}

void clearance(int32_t B, const int32_t* so, const double* T, const double* C, int32_t K, const double* obstacles,
               const double* scale, double r_min, double* near, int32_t* obs, int32_t* count, int32_t* tested,
               int32_t* flags) {
    namespace nb = tgms::neighbors;
    namespace cl = tgms::clearance;
    namespace sp = tgms::separation;
    const double sc[3] = {scale[0], scale[1], scale[2]};
    const double r2 = nb::cull_r2(r_min);
    std::vector<char> ok((size_t)K);
    bool bad_obstacle = false;
    for (int32_t k = 0; k < K; ++k) {
        ok[k] = cl::obstacle_ok(obstacles + (int64_t)k * cl::OBS_STRIDE);
        bad_obstacle = bad_obstacle || !ok[k];
    }
    for (int32_t i = 0; i < B; ++i) {
        const int M = so[i + 1] - so[i];
        const double* Ti = T + so[i];
        const double* Ci = C + (int64_t)so[i] * 24;
        double kn[nb::KNOT_STRIDE], bx[nb::BOXES * nb::BOX_STRIDE], ub[nb::BOX_STRIDE];
        const bool usable = nb::vehicle_boxes(M, Ci, Ti, 0.0, kn, bx, ub);
        nb::Row row = nb::row_init();
        for (int32_t k = 0; k < K && usable; ++k) {
            const double* ob = obstacles + (int64_t)k * cl::OBS_STRIDE;
            if (!ok[k] || !(nb::gap2(ub, ob, sc) < r2)) continue;
            double best = HUGE_VAL, at = 0.0;
            bool bad = false, any = false;
            for (int m = 0; m < M; ++m) {  // the kernel's items of the pair, in its order
                const double* box = bx + (m + 1) * nb::BOX_STRIDE;
                if (!(nb::gap2(box, ob, sc) < r2)) continue;
                any = true;
                const int mask = cl::admissible(box, ob);
                const int n = cl::combo_count(mask);
                for (int q = 0; q < n; ++q) {
                    double d2, u;
                    cl::combo_item(Ci + m * 24, Ti[m], ob, sc, cl::nth_combo(mask, q), d2, u);
                    sp::fold(d2, cl::time_of(kn[m], Ti[m], u, kn[M]), best, at, bad);
                }
            }
            if (!any) continue;
            double rec[TGMS_SEP_STRIDE];
            const int fl = sp::finish(best, at, bad, r_min, rec);
            nb::row_update(row, k, rec, fl);
        }
        double rec[TGMS_SEP_STRIDE];
        int32_t ob_i, ct;
        const int fl = nb::row_finish(row, usable, rec, ob_i, ct);
        if (near) std::copy(rec, rec + TGMS_SEP_STRIDE, near + (int64_t)i * TGMS_SEP_STRIDE);
        if (obs) obs[i] = ob_i;
        if (count) count[i] = ct;
        if (tested) tested[i] = (fl & TGMS_SEP_NONFINITE) ? 0 : row.tested;
        if (flags) flags[i] = cl::row_flags(fl, bad_obstacle);
    }
}

void field_clearance(int32_t B, const int32_t* so, const double* T, const double* C, const tgms_field& fld,
                     const float* values, double lip, double r_min, double tol, int32_t max_evals, double* near,
                     int32_t* evals, int32_t* flags) {
    namespace fd = tgms::field;
    const fd::Grid world = fd::make_grid(fld), g = fd::grid_frame(world);
    double L = lip;
    if (lip == 0.0) {
        double m[3] = {0.0, 0.0, 0.0};
        const int64_t total = (int64_t)fld.n[0] * fld.n[1] * fld.n[2];
        for (int64_t e = 0; e < total; ++e) fd::edge_max(values, fld.n, e, m);
        L = fd::lipschitz(m, g.ih);
    }
    for (int32_t b = 0; b < B; ++b) {
        const int M = so[b + 1] - so[b];
        const double* Tb = T + so[b];
        bool bad = M < 1 || M > TGMS_MAX_SEGMENTS, unresolved = false;
        double c[TGMS_MAX_SEGMENTS][3][8], V[TGMS_MAX_SEGMENTS], A[TGMS_MAX_SEGMENTS], kn[TGMS_MAX_SEGMENTS + 1];
        double fk[TGMS_MAX_SEGMENTS + 1], jump[TGMS_MAX_SEGMENTS], chk = 0.0, best = HUGE_VAL, at = 0.0, D = 0.0;
        int32_t n = 0;
        for (int m = 0; !bad && m < M; ++m) {
            bad = bad || !(Tb[m] > 0.0);
            chk = __builtin_fma(Tb[m], 0.0, chk);
            kn[m] = D;
            D += Tb[m];
            const double* cm = C + ((int64_t)so[b] + m) * 24;
            for (int q = 0; q < 24; ++q) c[m][q / 8][q % 8] = cm[q];
            fd::to_grid_frame(world, c[m]);
            fd::speed_bounds(c[m], Tb[m], V[m], A[m], chk);
        }
        bad = bad || !finite(chk) || !finite(D);
        if (!bad) {
            // the knots: every segment's left end, the last one's right end; the jumps between them
            for (int m = 0; m <= M; ++m) {
                double p[3];
                if (m < M) {
                    p[0] = c[m][0][0], p[1] = c[m][1][0], p[2] = c[m][2][0];
                } else {
                    fd::position(c[M - 1], Tb[M - 1], p);
                }
                if (m > 0 && m < M) {
                    double e[3];
                    fd::position(c[m - 1], Tb[m - 1], e);
                    jump[m - 1] = sqrt((p[0] - e[0]) * (p[0] - e[0]) + (p[1] - e[1]) * (p[1] - e[1]) +
                                       (p[2] - e[2]) * (p[2] - e[2]));
                }
                fk[m] = fd::phi(g, values, p);
                bad = bad || !finite(fk[m]);
                if (fk[m] < best) {
                    best = fk[m];
                    at = m < M ? kn[m] : kn[M - 1] + Tb[M - 1];
                }
            }
            jump[M - 1] = 0.0;
            n = M + 1;
            unresolved = n > max_evals;
        }
        for (int m = 0; !bad && !unresolved && m < M; ++m) {
            if (fd::ends_rule_out(fk[m], fk[m + 1] - L * jump[m], L, V[m], Tb[m], fd::threshold(best, tol, r_min)))
                continue;
            int level = 0;
            uint64_t index = 0;
            for (bool more = true; more;) {
                if (n >= max_evals) {
                    unresolved = true;
                    break;
                }
                double hwu, speed;
                const double u = fd::centre(level, index, hwu);
                const double f = fd::eval(g, values, c[m], u * Tb[m], speed);
                ++n;
                if (!finite(f)) {
                    bad = true;
                    break;
                }
                if (f < best) {
                    best = f;
                    at = kn[m] + u * Tb[m];
                }
                if (f - L * fd::reach(V[m], A[m], speed, hwu * Tb[m]) >= fd::threshold(best, tol, r_min)) {
                    more = fd::advance(level, index);
                } else if (level < fd::MAX_LEVEL) {
                    fd::descend(level, index);
                } else {
                    unresolved = true;
                    break;
                }
            }
        }
        double rec[TGMS_SEP_STRIDE];
        const int fl = fd::finish(best, at, D, bad, unresolved, r_min, rec);
        if (near) std::copy(rec, rec + TGMS_SEP_STRIDE, near + (int64_t)b * TGMS_SEP_STRIDE);
        if (evals) evals[b] = (fl & TGMS_SEP_NONFINITE) ? 0 : n;
        if (flags) flags[b] = fl;
    }
}

void field_occupancy(const tgms_field& fld, const float* values, double r_free, int32_t* table) {
    namespace inf = tgms::inflate;
    const inf::Grid g = inf::make_grid(fld);
    const float rf = (float)r_free;
    const int32_t nx = fld.n[0], ny = fld.n[1], nz = fld.n[2];
    for (int32_t k = 0; k <= nz; ++k) {
        for (int32_t j = 0; j <= ny; ++j) {
            int32_t* row = table + inf::table_index(g, 0, j, k);
            if (j == 0 || k == 0) {
                std::fill(row, row + nx + 1, 0);
                continue;
            }
            // along x the row's own count, plus the rectangle below it in y, plus the plane below in z
            const float* in = values + ((int64_t)(k - 1) * ny + (j - 1)) * nx;
            const int32_t* py = table + inf::table_index(g, 0, j - 1, k);
            const int32_t* pz = table + inf::table_index(g, 0, j, k - 1);
            const int32_t* pyz = table + inf::table_index(g, 0, j - 1, k - 1);
            int32_t run = 0;
            row[0] = 0;
            for (int32_t i = 0; i < nx; ++i) {
                run += inf::node_free(in[i], rf) ? 0 : 1;
                row[i + 1] = run + py[i + 1] + pz[i + 1] - pyz[i + 1];
            }
        }
    }
}

void corridor_inflate(int32_t B, const int32_t* so, const double* W, const tgms_field& fld, const float* values,
                      double r_free, int32_t max_grow, int32_t* box, double* faces, int64_t* fo, int32_t* seg_flags,
                      int32_t* flags) {
    namespace inf = tgms::inflate;
    const inf::Grid g = inf::make_grid(fld);
    std::vector<int32_t> table((size_t)(fld.n[0] + 1) * (fld.n[1] + 1) * (fld.n[2] + 1));
    field_occupancy(fld, values, r_free, table.data());
    for (int32_t b = 0; b < B; ++b) {
        int32_t all = 0;
        for (int64_t s = so[b]; s < so[b + 1]; ++s) {
            const double* w = W + (s + b) * 3;
            const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
            int32_t bx[6];
            double fc[6];
            const int32_t fl = inf::segment(g, table.data(), w0, w1, max_grow, bx, fc);
            all |= fl;
            if (box) std::copy(bx, bx + 6, box + s * 6);
            for (int d = 0; faces && d < 6; ++d) {
                double row[4];
                inf::face_row(d, fc[d], row);
                std::copy(row, row + 4, faces + (s * 6 + d) * 4);
            }
            if (fo) fo[s] = 6 * s;
            if (seg_flags) seg_flags[s] = fl;
        }
        if (flags) flags[b] = all;
    }
    if (fo && B > 0) fo[so[B]] = 6 * (int64_t)so[B];
}

void field_edt(const tgms_field& fld, const uint8_t* occ, double max_dist, int32_t mode, float* values, int32_t* d2) {
    namespace e = tgms::edt;
    const int64_t nx = fld.n[0], ny = fld.n[1], nz = fld.n[2], N = nx * ny * nz;
    const bool is_signed = (mode & TGMS_EDT_SIGNED) != 0;
    const e::Cap cap = e::make_cap(fld.h, max_dist);
    const e::Conv cv = e::make_conv(fld.h, max_dist, cap, is_signed);
    std::vector<int32_t> a((size_t)N), b((size_t)N), s((size_t)std::max(ny, nz)), t((size_t)std::max(ny, nz));
    for (int complement = 0; complement < (is_signed ? 2 : 1); ++complement) {
        for (int64_t r = 0; r < ny * nz; ++r) e::row_pass(occ + r * nx, (int32_t)nx, complement != 0, cap, a.data() + r * nx);
        for (int64_t k = 0; k < nz; ++k)
            for (int64_t i = 0; i < nx; ++i)
                e::line_pass(a.data() + k * nx * ny + i, b.data() + k * nx * ny + i, nx, (int32_t)ny, cap.K, s.data(), t.data());
        for (int64_t q = 0; q < nx * ny; ++q)
            e::line_pass(b.data() + q, a.data() + q, nx * ny, (int32_t)nz, cap.K, s.data(), t.data());
        // in the signed mode this transform is for the free nodes, the one on the complement for the occupied
        for (int64_t node = 0; node < N; ++node) {
            if (is_signed && (occ[node] != 0) != (complement != 0)) continue;
            const float val = e::value(cv, a[(size_t)node]);
            const int32_t sq = e::squared(cv, a[(size_t)node]);
            if (values) values[node] = complement ? -val : val;
            if (d2) d2[node] = complement ? -sq : sq;
        }
    }
}

void subdivide(int32_t B, const int32_t* so, const double* W, const double* T, const tgms_field& fld, const float* values,
               double r_free, int32_t max_depth, int32_t* so_out, double* W_out, double* T_out, int32_t* parent,
               int32_t* seg_flags, int64_t* totals, int32_t* flags) {
    namespace inf = tgms::inflate;
    namespace sub = tgms::subdivide;
    const inf::Grid g = inf::make_grid(fld);
    std::vector<int32_t> table((size_t)(fld.n[0] + 1) * (fld.n[1] + 1) * (fld.n[2] + 1));
    field_occupancy(fld, values, r_free, table.data());
    int64_t out = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t s0 = so[b];
        const int M = so[b + 1] - so[b];
        int32_t status[TGMS_MAX_SEGMENTS];
        uint32_t reached[TGMS_MAX_SEGMENTS], clr[TGMS_MAX_SEGMENTS];
        int sum[sub::MAX_DEPTH + 1] = {M, 0, 0, 0, 0};
        for (int i = 0; i < M; ++i) {
            const double* w = W + (s0 + i + b) * 3;
            const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
            status[i] = sub::leg_status(g, w0, w1);
            reached[i] = clr[i] = 1u;  // never subdivided: one leaf at every depth
            if (status[i] == sub::LEG_OK) sub::traverse(g, table.data(), w0, w1, max_depth, reached[i], clr[i]);
            for (int d = 1; d <= max_depth; ++d) sum[d] += sub::need(reached[i], clr[i], d);
        }
        const int D = sub::pick_depth(sum, max_depth);
        int32_t all = (sum[D] > M ? TGMS_SUB_DONE : 0) | (D < max_depth ? TGMS_SUB_FULL : 0);
        so_out[b] = (int32_t)out;
        for (int i = 0; i < M; ++i) {
            const double* w = W + (s0 + i + b) * 3;
            const uint32_t leaf = sub::leaves(reached[i], D);
            const int32_t word = sub::pack_leg(status[i], leaf, sub::blocked(reached[i], clr[i], D));
            all |= sub::word_flags(word);
            const int n = __builtin_popcount(word & 0xFFFF);
            for (int q = 0; q < n; ++q, ++out) {
                int i0, i1;
                sub::leaf_span((uint32_t)word, q, i0, i1);
                for (int a = 0; a < 3; ++a) W_out[(out + b) * 3 + a] = sub::point(w[a], w[3 + a], i0);
                if (T_out) T_out[out] = sub::leaf_time(T[s0 + i], i1 - i0);
                if (parent) parent[out] = (int32_t)(s0 + i);
                if (seg_flags) seg_flags[out] = sub::leaf_flag(word, i0);
            }
            if (i == M - 1) std::copy(w + 3, w + 6, W_out + (out + b) * 3);
        }
        if (flags) flags[b] = all;
    }
    so_out[B] = (int32_t)out;
    totals[0] = out;
}

namespace {

// One leg of the re-route: its record and its hop count.  dist and queue are the caller's, reused.
void reroute_leg(const tgms::inflate::Grid& g, const int32_t* table, const double (&w0)[3], const double (&w1)[3],
                 int32_t margin, int max_pieces, tgms::reroute::Record& rec, int32_t& hops, std::vector<uint16_t>& dist,
                 std::vector<int32_t>& queue) {
    namespace rr = tgms::reroute;
    hops = TGMS_NEAR_NONE;
    int32_t lo[3], hi[3];
    const int32_t fl = rr::classify(g, table, w0, w1, lo, hi);
    rec.head = rr::pack_head(1, fl < 0 ? TGMS_RRT_BLOCKED : fl);
    if (fl >= 0) return;
    auto keep = [&](int32_t why) { rec.head = rr::pack_head(1, TGMS_RRT_BLOCKED | why); };
    const rr::Window w = rr::window(g, lo, hi, margin);
    if (w.nodes > rr::WINDOW_NODES) return keep(TGMS_RRT_WINDOW);
    int32_t A[3], Z[3];
    for (int a = 0; a < 3; ++a) {
        A[a] = rr::nearest(g.o[a], g.h, w0[a], lo[a], hi[a]);
        Z[a] = rr::nearest(g.o[a], g.h, w1[a], lo[a], hi[a]);
    }
    if (!rr::node_free(g, table, A[0], A[1], A[2]) || !rr::node_free(g, table, Z[0], Z[1], Z[2]))
        return keep(TGMS_RRT_ENDS);
    // the search: a queue from Z, until A has its distance
    dist.assign((size_t)w.nodes, rr::D_UNREACHED);
    for (int32_t z = 0; z < w.n[2]; ++z)
        for (int32_t y = 0; y < w.n[1]; ++y)
            for (int32_t x = 0; x < w.n[0]; ++x)
                if (!rr::node_free(g, table, w.lo[0] + x, w.lo[1] + y, w.lo[2] + z))
                    dist[(size_t)rr::window_index(w, x, y, z)] = rr::D_NOT_FREE;
    const int32_t qa = rr::window_index(w, A[0] - w.lo[0], A[1] - w.lo[1], A[2] - w.lo[2]);
    const int32_t qz = rr::window_index(w, Z[0] - w.lo[0], Z[1] - w.lo[1], Z[2] - w.lo[2]);
    queue.clear();
    queue.push_back(qz);
    dist[(size_t)qz] = 0;
    for (size_t head = 0; head < queue.size() && dist[(size_t)qa] == rr::D_UNREACHED; ++head) {
        const int32_t q = queue[head], x = q % w.n[0], y = (q / w.n[0]) % w.n[1], z = q / (w.n[0] * w.n[1]);
        for (int d = 0; d < 6; ++d) {
            int32_t nx, ny, nz;
            if (!rr::neighbour(w, x, y, z, d, nx, ny, nz)) continue;
            const int32_t qi = rr::window_index(w, nx, ny, nz);
            if (dist[(size_t)qi] != rr::D_UNREACHED) continue;
            dist[(size_t)qi] = (uint16_t)(dist[(size_t)q] + 1);
            queue.push_back(qi);
        }
    }
    if (dist[(size_t)qa] == rr::D_UNREACHED) return keep(TGMS_RRT_NOPATH);
    hops = dist[(size_t)qa];
    // the targets: the path nodes first .. last, then w1; the descent runs beside the greedy
    double pt[3];
    rr::node_point(g, rr::node_id(g, A[0], A[1], A[2]), pt);
    const int first = rr::same_point(pt, w0) ? 1 : 0;
    rr::node_point(g, rr::node_id(g, Z[0], Z[1], Z[2]), pt);
    const int last = hops - (rr::same_point(pt, w1) ? 1 : 0);
    const int n = std::max(0, last - first + 1) + 1;
    int32_t cur[3] = {A[0] - w.lo[0], A[1] - w.lo[1], A[2] - w.lo[2]};
    int pos = 0, anchor = -1, anchors = 0;
    double qanchor[3] = {w0[0], w0[1], w0[2]}, prev[3] = {w0[0], w0[1], w0[2]};
    int32_t prev_id = TGMS_NEAR_NONE;
    for (int t = 0; t < n; ++t) {
        int32_t id = TGMS_NEAR_NONE;
        if (t < n - 1) {
            while (pos < first + t) {  // one step of the descent
                const int want = (int)dist[(size_t)rr::window_index(w, cur[0], cur[1], cur[2])] - 1;
                for (int d = 0; d < 6; ++d) {
                    int32_t nx, ny, nz;
                    if (!rr::neighbour(w, cur[0], cur[1], cur[2], d, nx, ny, nz)) continue;
                    if ((int)dist[(size_t)rr::window_index(w, nx, ny, nz)] != want) continue;
                    cur[0] = nx, cur[1] = ny, cur[2] = nz;
                    break;
                }
                ++pos;
            }
            id = rr::node_id(g, w.lo[0] + cur[0], w.lo[1] + cur[1], w.lo[2] + cur[2]);
            rr::node_point(g, id, pt);
        } else {
            std::copy(w1, w1 + 3, pt);
        }
        while (!rr::clear_points(g, table, qanchor, pt)) {
            if (const int32_t why = rr::on_fail(anchor, t, anchors, max_pieces)) return keep(why);
            rec.anchor[anchors++] = prev_id;
            anchor = t - 1;
            std::copy(prev, prev + 3, qanchor);
        }
        std::copy(pt, pt + 3, prev);
        prev_id = id;
    }
    rec.head = rr::pack_head(anchors + 1, 0);
}

}  // namespace

void reroute(int32_t B, const int32_t* so, const double* W, const double* T, const tgms_field& fld, const float* values,
             double r_free, int32_t margin, int32_t max_pieces, int32_t* so_out, double* W_out, double* T_out,
             int32_t* parent, int32_t* seg_flags, int32_t* hops, int64_t* totals, int32_t* flags) {
    namespace inf = tgms::inflate;
    namespace rr = tgms::reroute;
    const inf::Grid g = inf::make_grid(fld);
    std::vector<int32_t> table((size_t)(fld.n[0] + 1) * (fld.n[1] + 1) * (fld.n[2] + 1));
    field_occupancy(fld, values, r_free, table.data());
    std::vector<uint16_t> dist;
    std::vector<int32_t> queue;
    int64_t out = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t s0 = so[b];
        const int M = so[b + 1] - so[b];
        rr::Record rec[TGMS_MAX_SEGMENTS];
        int sum = 0;
        for (int i = 0; i < M; ++i) {
            const double* w = W + (s0 + i + b) * 3;
            const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
            int32_t hp;
            reroute_leg(g, table.data(), w0, w1, margin, max_pieces, rec[i], hp, dist, queue);
            if (hops) hops[s0 + i] = hp;
            sum += rr::head_pieces(rec[i].head);
        }
        const bool full = sum > TGMS_MAX_SEGMENTS;
        int32_t all = full ? TGMS_RRT_FULL : (sum > M ? TGMS_RRT_DONE : 0);
        so_out[b] = (int32_t)out;
        for (int i = 0; i < M; ++i) {
            const double* w = W + (s0 + i + b) * 3;
            const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
            const int p = full ? 1 : rr::head_pieces(rec[i].head);
            const double leg = p > 1 ? rr::length(w0, w1) : 0.0;
            for (int q = 0; q < p; ++q, ++out) {
                double a[3] = {w0[0], w0[1], w0[2]}, e[3] = {w1[0], w1[1], w1[2]};
                if (q > 0) rr::node_point(g, rec[i].anchor[q - 1], a);
                if (q < p - 1) rr::node_point(g, rec[i].anchor[q], e);
                std::copy(a, a + 3, W_out + (out + b) * 3);
                if (T_out) T_out[out] = p > 1 ? rr::piece_time(T[s0 + i], rr::length(a, e), leg) : T[s0 + i];
                if (parent) parent[out] = (int32_t)(s0 + i);
                const int32_t fl = p > 1 ? 0 : rr::kept_flag(rec[i].head, full);
                all |= fl;
                if (seg_flags) seg_flags[out] = fl;
            }
            if (i == M - 1) std::copy(w + 3, w + 6, W_out + (out + b) * 3);
        }
        if (flags) flags[b] = all;
    }
    so_out[B] = (int32_t)out;
    totals[0] = out;
}

void nearest_free(const tgms_field& fld, const float* values, double r_free, int32_t max_shift, int32_t* nearest,
                  int32_t* dsq) {
    namespace rp = tgms::repair;
    const int64_t nx = fld.n[0], ny = fld.n[1], nz = fld.n[2], N = nx * ny * nz;
    const int32_t K = rp::limit(max_shift);
    const float rf = (float)r_free;
    const size_t len = (size_t)std::max(ny, nz);
    std::vector<int32_t> a((size_t)N), b((size_t)N), f(len), arg(len), val(len), s(len), t(len);
    for (int64_t r = 0; r < ny * nz; ++r) rp::row_pass(values + r * nx, rf, (int32_t)nx, max_shift, a.data() + r * nx);
    for (int64_t k = 0; k < nz; ++k)
        for (int64_t i = 0; i < nx; ++i) {
            const int32_t* const in = a.data() + k * nx * ny + i;
            for (int64_t j = 0; j < ny; ++j) f[(size_t)j] = rp::f_row(in[j * nx], (int32_t)i, K);
            rp::line_pass(f.data(), (int32_t)ny, K, arg.data(), val.data(), s.data(), t.data());
            for (int64_t j = 0; j < ny; ++j) {
                const int32_t w = arg[(size_t)j];
                b[(size_t)(k * nx * ny + j * nx + i)] = w < 0 ? rp::NONE : rp::pack_yx(w, in[(int64_t)w * nx]);
            }
        }
    for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
            const int32_t* const in = b.data() + j * nx + i;
            for (int64_t k = 0; k < nz; ++k) f[(size_t)k] = rp::f_plane(in[k * nx * ny], (int32_t)i, (int32_t)j, K);
            rp::line_pass(f.data(), (int32_t)nz, K, arg.data(), val.data(), s.data(), t.data());
            for (int64_t k = 0; k < nz; ++k) {
                const int32_t w = arg[(size_t)k];
                const int64_t node = k * nx * ny + j * nx + i;
                const int32_t yx = w < 0 ? 0 : in[(int64_t)w * nx * ny];
                nearest[node] = w < 0 ? rp::NONE : (int32_t)(((int64_t)w * ny + rp::site_y(yx)) * nx + rp::site_x(yx));
                if (dsq) dsq[node] = w < 0 ? rp::NONE : val[(size_t)k];
            }
        }
}

void waypoints_repair(int32_t B, const int32_t* so, const double* W, const double* T, const tgms_field& fld,
                      const float* values, double r_free, int32_t max_shift, int32_t mode, double* W_out, double* T_out,
                      int32_t* wp_flags, int32_t* shift, int32_t* flags) {
    namespace rp = tgms::repair;
    const tgms::inflate::Grid g = tgms::inflate::make_grid(fld);
    std::vector<int32_t> map((size_t)fld.n[0] * fld.n[1] * fld.n[2]);
    nearest_free(fld, values, r_free, max_shift, map.data(), nullptr);
    for (int32_t b = 0; b < B; ++b) {
        const int64_t s0 = so[b];
        const int M = so[b + 1] - so[b];
        int32_t fl[TGMS_MAX_SEGMENTS + 1], all = 0;
        for (int i = 0; i <= M; ++i) {
            const int64_t row = s0 + i + b;
            const double* w = W + row * 3;
            const double p[3] = {w[0], w[1], w[2]};
            const bool protect = (i == 0 && (mode & TGMS_RPR_KEEP_FIRST)) || (i == M && (mode & TGMS_RPR_KEEP_LAST));
            double o[3];
            int32_t sh;
            fl[i] = rp::waypoint(g, map.data(), p, protect, o, sh);
            std::copy(o, o + 3, W_out + row * 3);
            if (wp_flags) wp_flags[row] = fl[i];
            if (shift) shift[row] = sh;
            all |= fl[i];
        }
        for (int i = 0; T_out && i < M; ++i) {
            const double *w = W + (s0 + i + b) * 3, *o = W_out + (s0 + i + b) * 3;
            const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
            const double p0[3] = {o[0], o[1], o[2]}, p1[3] = {o[3], o[4], o[5]};
            const double t = T[s0 + i];
            T_out[s0 + i] = ((fl[i] | fl[i + 1]) & TGMS_RPR_MOVED) ? rp::leg_time(t, w0, w1, p0, p1) : t;
        }
        if (flags) flags[b] = all;
    }
}

void corridor(int32_t B, const int32_t* so, const double* T, const double* C, int64_t F, const double* faces,
              const int64_t* fo, double r, double* rec, int32_t* where, double* seg_rec, int32_t* seg_face,
              int32_t* flags) {
    namespace co = tgms::corridor;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t s0 = so[b];
        const int M = so[b + 1] - so[b];
        const double* Tb = T + s0;
        const double* Cb = C + s0 * 24;
        double chk = 0.0;
        bool bad = M < 1 || M > TGMS_MAX_SEGMENTS;
        for (int i = 0; !bad && i < M; ++i) {
            chk += Tb[i] * 0.0;
            bad = bad || !(Tb[i] > 0.0);
        }
        for (int q = 0; !bad && q < M * 24; ++q) chk += Cb[q] * 0.0;
        bad = bad || !finite(chk);
        for (int i = 0; !bad && i < M; ++i) bad = !co::span_ok(fo ? fo[s0 + i] : 0, fo ? fo[s0 + i + 1] : F, F);
        if (M < 1 || M > TGMS_MAX_SEGMENTS) {  // nothing is read, and no segment row is written
            if (rec) rec[(int64_t)b * 2] = rec[(int64_t)b * 2 + 1] = __builtin_nan("");
            if (where) where[(int64_t)b * 2] = where[(int64_t)b * 2 + 1] = TGMS_NEAR_NONE;
            if (flags) flags[b] = TGMS_FEAS_NONFINITE;
            continue;
        }
        // tgms_corridor_core.h: the kernel's items, one after the other
        co::SegBest best[TGMS_MAX_SEGMENTS];
        double kn[TGMS_MAX_SEGMENTS];
        co::Fold f = co::fold_init();
        bool bad_face = false;
        for (int i = 0; i < M; ++i) {
            best[i] = co::seg_init();
            const int64_t fb = fo ? fo[s0 + i] : 0, fe = fo ? fo[s0 + i + 1] : F;
            for (int64_t h = fb; !bad && h < fe; ++h) {
                const double* n = faces + h * 4;
                if (!co::face_ok(n[0], n[1], n[2], n[3])) {
                    bad_face = true;
                    continue;
                }
                double m, u;
                co::item(Cb + i * 24, Tb[i], n[0], n[1], n[2], n[3], m, u);
                co::seg_take(best[i], m, u, (int32_t)h);
            }
            kn[i] = f.next;
            co::fold(f, best[i], i, Tb[i]);
        }
        double out[TGMS_COR_STRIDE];
        int32_t wh[2];
        const int fl = co::finish(f, bad, bad_face, r, out, wh);
        bad = (fl & TGMS_FEAS_NONFINITE) != 0;
        if (rec) std::copy(out, out + TGMS_COR_STRIDE, rec + (int64_t)b * TGMS_COR_STRIDE);
        if (where) std::copy(wh, wh + 2, where + (int64_t)b * 2);
        if (flags) flags[b] = fl;
        for (int i = 0; i < M && (seg_rec || seg_face); ++i) {
            double m, t;
            int32_t face;
            co::seg_row(best[i], kn[i], Tb[i], f.next, bad, m, t, face);
            if (seg_rec) {
                seg_rec[(s0 + i) * TGMS_COR_STRIDE] = m;
                seg_rec[(s0 + i) * TGMS_COR_STRIDE + 1] = t;
            }
            if (seg_face) seg_face[s0 + i] = face;
        }
    }
}

void corridor_split(int32_t B, const int32_t* so, const double* W, const double* T, const double* C, int64_t F,
                    const double* faces, const int64_t* fo, const double* seg_rec, const int32_t* seg_face, double r,
                    int mode, double min_frac, int32_t* so_out, double* W_out, double* T_out, double* faces_out,
                    int64_t* fo_out, int32_t* parent, int64_t* totals, int32_t* flags) {
    namespace sp = tgms::split;
    int64_t s_out = 0, f_out = 0;  // the next segment row and face row
    so_out[0] = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t s0 = so[b];
        const int M = so[b + 1] - so[b];
        const double* Tb = T + s0;
        const double* Wb = W + (s0 + b) * 3;
        double chk = 0.0;
        bool bad = false;
        for (int i = 0; i < M; ++i) {
            chk = sp::finite_chk(Tb[i], chk);
            bad = bad || !(Tb[i] > 0.0);
        }
        for (int q = 0; q < M * 24; ++q) chk = sp::finite_chk(C[s0 * 24 + q], chk);
        for (int q = 0; q < (M + 1) * 3; ++q) chk = sp::finite_chk(Wb[q], chk);
        bad = bad || chk != 0.0;
        double m[TGMS_MAX_SEGMENTS], ts[TGMS_MAX_SEGMENTS];
        int64_t fb[TGMS_MAX_SEGMENTS];
        int cnt[TGMS_MAX_SEGMENTS];
        for (int i = 0; i < M; ++i) {
            m[i] = seg_rec[(s0 + i) * TGMS_COR_STRIDE];
            ts[i] = seg_rec[(s0 + i) * TGMS_COR_STRIDE + 1];
            fb[i] = fo ? fo[s0 + i] : 0;
            const int64_t fe = fo ? fo[s0 + i + 1] : F;
            cnt[i] = tgms::corridor::span_ok(fb[i], fe, F) ? (int)(fe - fb[i]) : -1;
        }
        const sp::Row row = sp::plan_row(M, Tb, m, ts, seg_face + s0, fb, cnt, r, bad);
        if (flags) flags[b] = row.flags;
        double knot = 0.0;
        for (int i = 0; i < M; ++i) {
            const bool cut = ((row.mask >> i) & 1) != 0;
            const int64_t w_out = s_out + b;  // the row of this segment's start waypoint
            std::copy(Wb + i * 3, Wb + i * 3 + 3, W_out + w_out * 3);
            if (cut) {
                double tl, tr, w[3];
                sp::split_times(sp::local_time(ts[i], knot, Tb[i]), Tb[i], min_frac, tl, tr);
                if (mode == TGMS_SPLIT_PULL) {
                    const double* n = faces + (int64_t)seg_face[s0 + i] * 4;
                    sp::insert_pull(C + (s0 + i) * 24, tl, n[0], n[1], n[2], n[3], r, w);
                } else {
                    sp::insert_chord(Wb + i * 3, Wb + i * 3 + 3, tl, Tb[i], w);
                }
                T_out[s_out] = tl;
                T_out[s_out + 1] = tr;
                std::copy(w, w + 3, W_out + (w_out + 1) * 3);
            } else {
                T_out[s_out] = Tb[i];
            }
            for (int k = 0; k < (cut ? 2 : 1); ++k) {  // each child owns a copy of the parent's span
                if (parent) parent[s_out] = (int32_t)(s0 + i);
                if (fo) {
                    fo_out[s_out] = f_out;
                    if (cnt[i] > 0) std::copy(faces + fb[i] * 4, faces + (fb[i] + cnt[i]) * 4, faces_out + f_out * 4);
                    f_out += cnt[i] > 0 ? cnt[i] : 0;
                }
                ++s_out;
            }
            knot += Tb[i];
        }
        std::copy(Wb + M * 3, Wb + M * 3 + 3, W_out + (s_out + b) * 3);
        so_out[b + 1] = (int32_t)s_out;
    }
    if (fo) fo_out[s_out] = f_out;
    totals[0] = s_out;
    totals[1] = fo ? f_out : F;
}

void cut(int32_t B, const int32_t* so, const double* W, const double* T, const double* ED, const double* C,
         const double* t_cut, double min_frac, int32_t* so_out, double* W_out, double* T_out, double* ED_out,
         double* C_out, int32_t* parent, double* t0_out, int64_t* totals, int32_t* flags) {
    namespace ct = tgms::cut;
    int64_t s_out = 0;  // the next segment row
    so_out[0] = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t s0 = so[b];
        const int M = so[b + 1] - so[b];
        const double* Tb = T + s0;
        const double* Wb = W + (s0 + b) * 3;
        const double* Eb = ED ? ED + (int64_t)b * 18 : nullptr;
        double chk = 0.0;
        bool bad = !(t_cut[b] == t_cut[b]);
        for (int i = 0; i < M; ++i) {
            chk = tgms::split::finite_chk(Tb[i], chk);
            bad = bad || !(Tb[i] > 0.0);
        }
        for (int q = 0; q < M * 24; ++q) chk = tgms::split::finite_chk(C[s0 * 24 + q], chk);
        for (int q = 0; q < (M + 1) * 3; ++q) chk = tgms::split::finite_chk(Wb[q], chk);
        for (int q = 0; Eb && q < 18; ++q) chk = tgms::split::finite_chk(Eb[q], chk);
        bad = bad || chk != 0.0;
        const ct::Plan p = ct::plan_row(M, Tb, t_cut[b], min_frac, bad);
        if (flags) flags[b] = p.flags;
        if (t0_out) t0_out[b] = p.t0;
        double* Eo = ED_out + (int64_t)b * 18;
        std::fill(Eo, Eo + 18, 0.0);
        const int64_t w_out = s_out + b;  // the row of the first waypoint
        if (p.kind == ct::FINISHED) {
            const double* wM = Wb + M * 3;
            T_out[s_out] = Tb[M - 1];
            if (parent) parent[s_out] = (int32_t)(s0 + M - 1);
            std::copy(wM, wM + 3, W_out + w_out * 3);
            std::copy(wM, wM + 3, W_out + (w_out + 1) * 3);
            if (C_out) {
                std::fill(C_out + s_out * 24, C_out + (s_out + 1) * 24, 0.0);
                for (int ax = 0; ax < 3; ++ax) C_out[s_out * 24 + ax * 8] = wM[ax];
            }
        } else {
            const int s = p.s;
            const bool inside = p.t_loc > 0.0;
            if (Eb) std::copy(Eb + 9, Eb + 18, Eo + 9);
            if (s == 0 && !inside) {
                if (Eb) std::copy(Eb, Eb + 9, Eo);
            } else {
                double c[24], x[3], d[9];
                ct::shift_row(C + (s0 + s) * 24, p.t_loc, c, x, d);
                std::copy(d, d + 9, Eo);
                if (inside) {
                    std::copy(x, x + 3, W_out + w_out * 3);
                    if (C_out) std::copy(c, c + 24, C_out + s_out * 24);
                }
            }
            if (!inside) std::copy(Wb + s * 3, Wb + s * 3 + 3, W_out + w_out * 3);
            std::copy(Wb + (s + 1) * 3, Wb + (M + 1) * 3, W_out + (w_out + 1) * 3);
            T_out[s_out] = ct::first_time(Tb[s], p.t_loc);
            std::copy(Tb + s + 1, Tb + M, T_out + s_out + 1);
            if (C_out) std::copy(C + (s0 + s + (inside ? 1 : 0)) * 24, C + (s0 + M) * 24,
                                 C_out + (s_out + (inside ? 1 : 0)) * 24);
            for (int i = s; parent && i < M; ++i) parent[s_out + i - s] = (int32_t)(s0 + i);
        }
        s_out += p.M_out;
        so_out[b + 1] = (int32_t)s_out;
    }
    totals[0] = s_out;
}

}  // namespace host
}  // namespace tgms
