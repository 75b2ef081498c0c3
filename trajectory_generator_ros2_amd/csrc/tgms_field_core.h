// tgms_field_core.h — closest approach of a trajectory to a voxel distance field, shared by
// the gfx950 kernels (tgms_field.hip) and the host backend (tgms_host.cpp).  Plain C++17, as
// its siblings: the Horner chain is tgms_bounds_core.h's, the Bernstein weights
// tgms_neighbors_core.h's, the rule for a candidate's global time tgms_clearance_core.h's.
//
// The value.  phi(p) is the trilinear interpolant of float nodes on a regular grid, taken at
// the point clamped to the grid (include/tgms.h has the formula).  It is Lipschitz with
//     L = sqrt(G_x^2 + G_y^2 + G_z^2),   G_a = max over edges along a of |v(node + e_a) - v(node)| / h:
// inside a cell d phi / d a is a bilinear blend of the four edge differences along a, hence at
// most G_a in magnitude; phi is continuous across cells; clamping moves two points no further
// apart.  So for any two points |phi(p) - phi(q)| <= L ||p - q||.
//
// The search.  Per segment a binary interval tree over u = t / T in [0, 1]: node (level, index)
// is [index 2^-level, (index + 1) 2^-level], evaluated at its centre t_c.  With hw the half
// width in seconds every point of the node is within
//     reach(hw) = min(V hw, ||p'(t_c)|| hw + A hw^2 / 2)
// of p(t_c): V and A bound ||p'|| and ||p''|| on the whole segment (the Bernstein control
// values of the two derivative polynomials, per axis, then the Euclidean norm), and the second
// form is Taylor's bound around the centre, far tighter where the vehicle is slow.  Hence
//     phi(p(t)) >= phi(p(t_c)) - L reach(hw)      on the node,
// and the node is discarded when that is >= min(best - tol, r_min), best the least value
// evaluated so far for the trajectory; otherwise its two halves follow, the left one first.
// Since best <= phi(p(t_c)), a node is discarded at the latest when L reach(hw) <= tol: the
// depth is bounded by log2(L V T / tol), and the cost follows how close the trajectory comes.
// A discarded node satisfied the test against a best that only falls afterwards, so at the end
// every point of every segment has phi >= min(d_min - tol, r_min): the certificate.
//   - The walk keeps no stack: after a node is discarded, "while index odd: index >>= 1,
//     level -= 1; then index += 1" is its successor in depth-first order; level 0 ends it.
//   - Knots.  Every segment's left end (local time 0) and the last segment's right end are
//     evaluated before any tree, so M + 1 evaluations seed best.  A segment whose two end values
//     already rule it out is never entered: every point is within hw = T / 2 of an end, so
//     min(phi_left, phi_right) - L V T / 2 bounds it.  The right end's value is the next
//     segment's left end; where the coefficients jump at the knot by `jump`, L jump is taken off
//     that value first, so the bound holds for any input.  A constant field (L = 0) and a
//     hovering vehicle (V = 0) therefore cost M + 1 evaluations.
//   - Depth.  MAX_LEVEL = 48 halvings leave the centre's local time exact in fp64; a node
//     there that still cannot be discarded ends the row as unresolved (only with a Lipschitz
//     bound or a speed that overflowed; the evaluation budget ends every real search first).
//   - Rounding.  The Horner chains, the blend and the bound are plain fp64; their error is
//     some 1e-15 of F + L (P + h), against the 1e-9 of it that the contract allows.
#pragma once

#include <stdint.h>

#include "tgms_neighbors_core.h"

namespace tgms {
namespace field {

constexpr int MAX_LEVEL = 48;
constexpr int LIP_BLOCK = 256;   // threads of a block of the Lipschitz reduction
constexpr int LIP_BLOCKS = 256;  // its blocks: [LIP_BLOCKS][3] partial maxima

// The grid as the evaluation wants it: 1 / h, and the extents as doubles for the clamp.
struct Grid {
    double o[3];
    double ih;
    int32_t n[3];
};

TGMS_HD Grid make_grid(const tgms_field& f) {
    Grid g;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        g.o[a] = f.origin[a];
        g.n[a] = f.n[a];
    }
    g.ih = 1.0 / f.h;
    return g;
}

// The grid's frame.  A map far from the world's origin (2^14 m, say) would leave p(t) an ulp of
// 1.8e-12 and p - origin no better.  So both backends take the origin off each segment's constant
// coefficient once, c_0 - origin, and evaluate in a grid whose origin is 0: the Horner chain
// then rounds at the size of the position within the map, and a map and a trajectory moved by
// the same exactly representable shift give the same bits.
TGMS_HD void to_grid_frame(const Grid& g, double (&c)[3][8]) {
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) c[a][0] -= g.o[a];
}

TGMS_HD Grid grid_frame(Grid g) {
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) g.o[a] = 0.0;
    return g;
}

TGMS_HD double lerp(double a, double b, double f) { return __builtin_fma(f, b - a, a); }  // a == b: a to the bit

// phi at the point p: eight nodes, converted to fp64, blended in fp64.  A NaN coordinate
// clamps to 0 (fmax / fmin drop it); the callers rule such rows out by their coefficients.
TGMS_HD double phi(const Grid& g, const float* __restrict__ v, const double (&p)[3]) {
    int32_t i[3];
    double f[3];
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        const double q = fmin(fmax((p[a] - g.o[a]) * g.ih, 0.0), (double)(g.n[a] - 1));
        const int32_t c = (int32_t)q;
        i[a] = c < g.n[a] - 2 ? c : g.n[a] - 2;
        f[a] = q - (double)i[a];
    }
    const int32_t nx = g.n[0], sl = g.n[0] * g.n[1];      // n_x n_y n_z <= 2^31 - 1: no overflow
    const int32_t at = (i[2] * g.n[1] + i[1]) * nx + i[0];
    const double v000 = v[at], v100 = v[at + 1], v010 = v[at + nx], v110 = v[at + nx + 1];
    const double v001 = v[at + sl], v101 = v[at + sl + 1], v011 = v[at + sl + nx], v111 = v[at + sl + nx + 1];
    const double x00 = lerp(v000, v100, f[0]), x10 = lerp(v010, v110, f[0]);
    const double x01 = lerp(v001, v101, f[0]), x11 = lerp(v011, v111, f[0]);
    return lerp(lerp(x00, x10, f[1]), lerp(x01, x11, f[1]), f[2]);
}

// The largest |Bernstein control value| of sum_k a[k] u^k on [0, 1]: a bound of its magnitude there.
template <int N>
TGMS_HD double bern_absmax(const double (&a)[N + 1]) {
    double m = fabs(a[0]);
    TGMS_UNROLL
    for (int i = 1; i <= N; ++i) {
        double b = a[0];
        TGMS_UNROLL
        for (int k = 1; k <= i; ++k) b = __builtin_fma(neighbors::binom(i, k) / neighbors::binom(N, k), a[k], b);
        m = fmax(m, fabs(b));
    }
    return m;
}

// V >= ||p'|| and A >= ||p''|| on [0, T] of the segment c [3][8]; chk stays 0 while every
// coefficient is finite.
TGMS_HD void speed_bounds(const double (&c)[3][8], double T, double& V, double& A, double& chk) {
    double v2 = 0.0, a2 = 0.0;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double dv[7], da[6], w = 1.0;
        chk = __builtin_fma(c[ax][0], 0.0, chk);
        TGMS_UNROLL
        for (int k = 1; k < 8; ++k) {  // w = T^(k-1)
            chk = __builtin_fma(c[ax][k], 0.0, chk);
            dv[k - 1] = (double)k * c[ax][k] * w;
            w *= T;
        }
        w = 1.0;
        TGMS_UNROLL
        for (int k = 2; k < 8; ++k) {  // w = T^(k-2)
            da[k - 2] = (double)(k * (k - 1)) * c[ax][k] * w;
            w *= T;
        }
        const double mv = bern_absmax<6>(dv), ma = bern_absmax<5>(da);
        v2 = __builtin_fma(mv, mv, v2);
        a2 = __builtin_fma(ma, ma, a2);
    }
    V = sqrt(v2);
    A = sqrt(a2);
}

TGMS_HD void position(const double (&c)[3][8], double t, double (&p)[3]) {
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) p[ax] = bounds::horner<7>(c[ax], t);
}

// phi(p(t)) at the local time t and the speed ||p'(t)|| there.  The derivative rides along the
// position's Horner chain (d = d t + s before s = s t + c_k), which needs no product k c_k: a
// kernel would keep those 21 loop invariants in registers.  The position is horner<7>'s to the bit.
TGMS_HD double eval(const Grid& g, const float* __restrict__ v, const double (&c)[3][8], double t, double& speed) {
    double p[3], s2 = 0.0;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double s = c[ax][7], d = 0.0;
        TGMS_UNROLL
        for (int k = 6; k >= 0; --k) {
            d = __builtin_fma(d, t, s);
            s = __builtin_fma(s, t, c[ax][k]);
        }
        p[ax] = s;
        s2 = __builtin_fma(d, d, s2);
    }
    speed = sqrt(s2);
    return phi(g, v, p);
}

// How far the vehicle can be from p(t_c) within hw seconds of t_c.
TGMS_HD double reach(double V, double A, double speed, double hw) {
    return fmin(V * hw, __builtin_fma(0.5 * A * hw, hw, speed * hw));
}

// What a node must reach to be discarded.
TGMS_HD double threshold(double best, double tol, double r_min) { return fmin(best - tol, r_min); }

// The centre of node (level, index) as u in (0, 1), and its half width in u.
TGMS_HD double centre(int level, uint64_t index, double& hwu) {
    hwu = __builtin_ldexp(1.0, -(level + 1));
    return (double)(2 * index + 1) * hwu;  // exact: index < 2^MAX_LEVEL
}

// The depth-first successor of a node that is done with; false when the tree is.
TGMS_HD bool advance(int& level, uint64_t& index) {
    while (index & 1) {
        index >>= 1;
        --level;
    }
    ++index;
    return level > 0;
}

// The left child.
TGMS_HD void descend(int& level, uint64_t& index) {
    ++level;
    index <<= 1;
}

// Whether the end values rule a whole segment out (see above); fr is the right end's value
// less L times the jump of the coefficients at that knot.
TGMS_HD bool ends_rule_out(double fl, double fr, double L, double V, double T, double thr) {
    return fmin(fl, fr) - L * (V * (0.5 * T)) >= thr;
}

// The record and the flag word of a row.  bad: an input of the row was unusable or a value
// was not finite.  The comparison is strict, on the stored value.
TGMS_HD int finish(double best, double at, double D, bool bad, bool unresolved, double r_min,
                   double (&rec)[TGMS_SEP_STRIDE]) {
    rec[0] = best;
    rec[1] = fmin(at, D);
    const double fin = __builtin_fma(rec[0], 0.0, rec[1] * 0.0);
    if (bad || fin != 0.0) {
        rec[0] = rec[1] = __builtin_nan("");
        return TGMS_SEP_NONFINITE;
    }
    return (rec[0] < r_min ? TGMS_SEP_CLOSE : 0) | (unresolved ? TGMS_FLD_UNRESOLVED : 0);
}

// One node's part of the three per-axis edge maxima |v(node + e_a) - v(node)| (not yet over h).
TGMS_HD void edge_max(const float* __restrict__ v, const int32_t (&n)[3], int64_t e, double (&g)[3]) {
    const int32_t i = (int32_t)(e % n[0]);
    const int64_t r = e / n[0];
    const int32_t j = (int32_t)(r % n[1]), k = (int32_t)(r / n[1]);
    const double c = v[e];
    if (i + 1 < n[0]) g[0] = fmax(g[0], fabs((double)v[e + 1] - c));
    if (j + 1 < n[1]) g[1] = fmax(g[1], fabs((double)v[e + n[0]] - c));
    if (k + 1 < n[2]) g[2] = fmax(g[2], fabs((double)v[e + (int64_t)n[0] * n[1]] - c));
}

// L from the three maxima.
TGMS_HD double lipschitz(const double (&g)[3], double ih) {
    const double x = g[0] * ih, y = g[1] * ih, z = g[2] * ih;
    return sqrt(__builtin_fma(z, z, __builtin_fma(y, y, x * x)));
}

}  // namespace field
}  // namespace tgms
