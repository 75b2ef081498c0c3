// tgms_repair_core.h — waypoint repair: the nearest free node of every node of a voxel map
// (a feature transform: the argument of the distance transform, not only its value), and the
// move of a map-blocked waypoint onto it.  Shared by the gfx950 kernels (tgms_repair.hip) and
// the host backend (tgms_host.cpp).  Plain C++17, as its siblings.  include/tgms.h states the
// result to the bit; this file holds what both backends must take from one place:
//   - the cap (limit): a site counts when its squared lattice distance is at most max_shift^2;
//     K = max_shift^2 + 1 stands for "no site", also between the passes;
//   - what a pass leaves for the next one (pack_yx / site_x / site_y) and the squares a pass
//     reads back from it (f_row, f_plane);
//   - the host backend's passes (row_pass, line_pass), the argument-carrying variants of
//     edt::row_pass and edt::line_pass;
//   - the decision for one waypoint (waypoint) and the time of a leg with a moved end (leg_time).
//
// The tie rule.  The site of p is the free node q with the least D = sum_a (p_a - q_a)^2; among
// equal D the lowest k', then the lowest j', then the lowest i'.  The transform is separable and
// so is this order:
//   - the x pass gives node (i, j, k) the nearest free node of its own row, X(i, j, k) = i',
//     the lower i' when two are equally far;
//   - the y pass gives it the row j' of its plane with the least (i - X(i, j', k))^2 + (j - j')^2,
//     the lowest such j', and keeps (j', X(i, j', k));
//   - the z pass gives it the plane k' with the least in-plane square + (k - k')^2, the lowest
//     such k', and keeps that plane's (j', i').
// Let M be the set of global minimisers of p = (i, j, k) and (k*, j*, i*) its lexicographic
// minimum.  A plane that holds a member of M has the in-plane minimum D_min - (k - k')^2 (a
// smaller one would beat D_min), and no plane has a smaller sum, so the z pass, which takes the
// lowest k' among the planes with the least sum, takes k*.  Inside plane k* the members of M are
// exactly the in-plane minimisers of (i, j); the same argument one dimension down makes the y
// pass take j*, and the x pass takes the lowest nearest free i' of row (j*, k*), which is i*.
// A partial sum above max_shift^2 cannot come back under it, so a pass may drop it (K) at once,
// and it may look max_shift entries to either side or along the whole line: the integers are
// the same.  Sums stay below 2^30 + 1 + 2^28, inside int32.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tgms_edt_core.h"      // MAX_NODES_PER_AXIS, MAX_R
#include "tgms_reroute_core.h"  // nearest, node_id, node_point, length, piece_time; the inflation's and the subdivision's cores

namespace tgms {
namespace repair {

constexpr int32_t MAX_SHIFT = edt::MAX_R;
constexpr int AXIS_BITS = 14;  // an index below MAX_NODES_PER_AXIS
static_assert((1 << AXIS_BITS) == edt::MAX_NODES_PER_AXIS, "two indices of a plane are packed into one int32");
constexpr int32_t NONE = TGMS_NEAR_NONE;

// "No site": one more than the largest square that counts.  max_shift in 1..MAX_SHIFT.
TGMS_HD int32_t limit(int32_t max_shift) { return max_shift * max_shift + 1; }

// What the y pass leaves per node: (j', i') of the site in the node's plane.
TGMS_HD int32_t pack_yx(int32_t j, int32_t i) { return (j << AXIS_BITS) | i; }
TGMS_HD int32_t site_x(int32_t yx) { return yx & ((1 << AXIS_BITS) - 1); }
TGMS_HD int32_t site_y(int32_t yx) { return yx >> AXIS_BITS; }

// The square the y pass starts from at an entry of the line x = i: from the x pass' i' (or NONE).
TGMS_HD int32_t f_row(int32_t xsite, int32_t i, int32_t K) {
    const int32_t d = i - xsite;
    return xsite < 0 ? K : d * d;  // |d| <= max_shift by the x pass
}
// The square the z pass starts from at an entry of the line (i, j): from the y pass' pair.
TGMS_HD int32_t f_plane(int32_t yx, int32_t i, int32_t j, int32_t K) {
    const int32_t dx = i - site_x(yx), dy = j - site_y(yx);
    return yx < 0 ? K : dx * dx + dy * dy;  // <= max_shift^2 by the y pass
}

// ---- the host backend's passes ----

// One row along x: out[i] = the nearest free i' with |i - i'| <= max_shift, the lower of two
// equally far, or NONE.
inline void row_pass(const float* values, float r_free, int32_t n, int32_t max_shift, int32_t* out) {
    const int32_t far = 1 << 20;  // beyond any max_shift
    int32_t last = -far;
    for (int32_t i = 0; i < n; ++i) {
        if (inflate::node_free(values[i], r_free)) last = i;
        out[i] = last;
    }
    int32_t next = 2 * far;
    for (int32_t i = n - 1; i >= 0; --i) {
        if (inflate::node_free(values[i], r_free)) next = i;
        const int32_t dl = i - out[i], dr = next - i;
        const int32_t g = dl <= dr ? dl : dr;
        out[i] = g > max_shift ? NONE : (dl <= dr ? i - dl : i + dr);
    }
}

// One line of n entries: arg[u] = the lowest u' with the least f[u'] + (u - u')^2, and val[u] that
// least sum; arg NONE and val K where it is K or more.  The lower envelope of the parabolas in
// exact integers, as edt::line_pass: parabola u replaces s[q] only from the first x at which it
// is strictly lower, so of two equal sums the lower index stays.  s and t hold n entries each.
inline void line_pass(const int32_t* f, int32_t n, int32_t K, int32_t* arg, int32_t* val, int32_t* s, int32_t* t) {
    const auto F = [&](int64_t x, int64_t i) { return (x - i) * (x - i) + (int64_t)f[i]; };
    int32_t q = 0;
    s[0] = 0;
    t[0] = 0;
    for (int32_t u = 1; u < n; ++u) {
        while (q >= 0 && F(t[q], s[q]) > F(t[q], u)) --q;
        if (q < 0) {
            q = 0;
            s[0] = u;
        } else {
            // the first x at which parabola u is strictly lower than parabola s[q]: 1 + floor(num / den)
            const int64_t i = s[q];
            const int64_t num = (int64_t)u * u - i * i + (int64_t)f[u] - (int64_t)f[i];
            const int64_t den = 2 * ((int64_t)u - i);
            int64_t fl = num / den;
            if (num % den != 0 && num < 0) --fl;
            const int64_t w = 1 + fl;
            if (w < n) {
                ++q;
                s[q] = u;
                t[q] = (int32_t)(w < 0 ? 0 : w);
            }
        }
    }
    for (int32_t u = n - 1; u >= 0; --u) {
        const int64_t v = F(u, s[q]);
        arg[u] = v < K ? s[q] : NONE;
        val[u] = (int32_t)(v < K ? v : K);
        if (u == t[q]) --q;
    }
}

// ---- one waypoint ----

// The flag of waypoint w, its row `out` and its shift.  `nearest` is the map of the nearest-free
// call for the grid g; `protect`: the mode keeps this waypoint where it is.
TGMS_HD int32_t waypoint(const inflate::Grid& g, const int32_t* __restrict__ nearest, const double (&w)[3], bool protect,
                         double (&out)[3], int32_t& shift) {
    shift = NONE;
    double chk = 0.0;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        out[a] = w[a];
        chk = __builtin_fma(w[a], 0.0, chk);
    }
    if (!(chk == 0.0)) return TGMS_FEAS_NONFINITE;
    int32_t lo[3], hi[3];
    if (!subdivide::seed(g, w, w, lo, hi)) return TGMS_RPR_OUTSIDE;
    // the seed of a point: one or two nodes an axis, every one its own site when the waypoint is clear
    bool clear = true;
    for (int32_t k = lo[2]; k <= hi[2]; ++k)
        for (int32_t j = lo[1]; j <= hi[1]; ++j)
            for (int32_t i = lo[0]; i <= hi[0]; ++i) {
                const int32_t node = reroute::node_id(g, i, j, k);
                clear = clear && nearest[node] == node;
            }
    if (clear) return 0;
    if (protect) return TGMS_RPR_KEPT;
    int32_t nn[3];
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) nn[a] = reroute::nearest(g.o[a], g.h, w[a], 0, g.n[a] - 1);
    const int32_t q = nearest[reroute::node_id(g, nn[0], nn[1], nn[2])];
    if (q < 0) return TGMS_RPR_STUCK;
    reroute::node_point(g, q, out);
    const int32_t qi = q % g.n[0], r = q / g.n[0];
    const int32_t dx = nn[0] - qi, dy = nn[1] - r % g.n[1], dz = nn[2] - r / g.n[1];
    shift = dx * dx + dy * dy + dz * dz;
    return TGMS_RPR_MOVED;
}

// The time of a leg of which at least one end moved: T len(new) / len(old) when both lengths are
// finite and positive, else T bit for bit.
TGMS_HD double leg_time(double T, const double (&a0)[3], const double (&a1)[3], const double (&b0)[3],
                        const double (&b1)[3]) {
    const double was = reroute::length(a0, a1), is = reroute::length(b0, b1);
    const bool usable = was > 0.0 && is > 0.0 && was - was == 0.0 && is - is == 0.0;
    return usable ? reroute::piece_time(T, is, was) : T;
}

}  // namespace repair
}  // namespace tgms
