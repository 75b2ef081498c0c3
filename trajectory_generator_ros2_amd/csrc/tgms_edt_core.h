// tgms_edt_core.h — distance-field build: the exact Euclidean transform of an occupancy grid,
// shared by the gfx950 kernels (tgms_edt.hip) and the host backend (tgms_host.cpp).  Plain
// C++17, as its siblings.  include/tgms.h states the result to the bit; this file holds what
// both backends must take from one place:
//   - the cap (make_cap): R from max_dist / h with its one corrected step, and the two squares
//     the passes and the outputs saturate at;
//   - the conversion of a squared lattice distance into the value and the reported square
//     (value, squared): one correctly rounded square root, one product, in signed mode one
//     difference, each rounded on its own (mul_rn / add_rn of tgms_inflate_core.h: the device
//     compiler must not contract h sqrt(D) - h/2 into an fma);
//   - the passes of the host backend (row_pass, line_pass), which produce the integers the
//     kernels produce.
// Every pass works on int32 squares saturated at K = (R + 1)^2.  A square of K or more cannot
// change an output: the reported square is min(D, R^2), and a node (R + 1) spacings away has
// h (R + 1) - h/2 >= h R + h/2 - (roundings of a few 2^-53 h R) > max_dist, because h R >=
// max_dist as rounded and R <= 32,768.  The signed mode is why K is not R^2: there a node
// between R and R + 1/2 spacings away still has a value below max_dist.  A term f + d^2 with
// |d| > R is at least K, so a pass may look R entries to either side or along the whole line
// and gets the same integers.  f <= K < 2^30 + 2^17 and d^2 < 2^28, so no sum leaves int32.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tgms_inflate_core.h"  // TGMS_HD, mul_rn, add_rn

namespace tgms {
namespace edt {

constexpr int32_t MAX_NODES_PER_AXIS = 16384;  // 3 (n - 1)^2 stays inside int32
constexpr int32_t MAX_R = 32768;

struct Cap {
    int32_t R;   // nodes: ceil(max_dist / h), corrected, clipped to MAX_R
    int32_t R2;  // what the reported squares saturate at
    int32_t K;   // (R + 1)^2: what the passes saturate at
};

// h > 0 and max_dist > 0, both finite (the caller's check).
inline Cap make_cap(double h, double max_dist) {
    double r = ceil(max_dist / h);
    if (inflate::mul_rn(h, r) < max_dist) r += 1.0;
    if (!(r <= (double)MAX_R)) r = (double)MAX_R;
    Cap c;
    c.R = (int32_t)r;
    c.R2 = c.R * c.R;
    c.K = (c.R + 1) * (c.R + 1);
    return c;
}

// What the last pass needs to turn a square into the outputs.
struct Conv {
    double h, half_h, max_dist;
    int32_t R2, K;
    int32_t is_signed;
};

inline Conv make_conv(double h, double max_dist, const Cap& c, bool is_signed) {
    return Conv{h, 0.5 * h, max_dist, c.R2, c.K, is_signed ? 1 : 0};
}

// The magnitude of the value of a node whose nearest node of the other kind is D away, squared;
// D >= K stands for every square that cannot matter, the empty set among them.
TGMS_HD float value(const Conv& c, int32_t D) {
    double m = c.max_dist;
    if (D < c.K) {
        double d = inflate::mul_rn(c.h, sqrt((double)D));
        if (c.is_signed) d = inflate::add_rn(d, -c.half_h);
        m = d < m ? d : m;
    }
    return (float)m;
}
TGMS_HD int32_t squared(const Conv& c, int32_t D) { return D < c.R2 ? D : c.R2; }

// ---- the host backend's passes ----

// One row along x: out[i] = min((i - i')^2, K) over the targets i' of the row; a node is a
// target when (occ != 0) != complement.
inline void row_pass(const uint8_t* occ, int32_t n, bool complement, const Cap& c, int32_t* out) {
    const int32_t far = 1 << 20;  // beyond any R
    int32_t last = -far;
    for (int32_t i = 0; i < n; ++i) {
        if ((occ[i] != 0) != complement) last = i;
        out[i] = i - last;
    }
    int32_t next = 2 * far;
    for (int32_t i = n - 1; i >= 0; --i) {
        if ((occ[i] != 0) != complement) next = i;
        const int32_t g = out[i] < next - i ? out[i] : next - i;
        out[i] = g > c.R ? c.K : g * g;
    }
}

// One line of n entries `step` apart: out[j] = min(min over j' of f[j'] + (j - j')^2, K), by the
// lower envelope of the parabolas in exact integers (Meijster, Roerdink and Hesselink).  s and t
// hold n entries each.
inline void line_pass(const int32_t* f, int32_t* out, int64_t step, int32_t n, int32_t K, int32_t* s, int32_t* t) {
    const auto F = [&](int64_t x, int64_t i) { return (x - i) * (x - i) + (int64_t)f[i * step]; };
    int32_t q = 0;
    s[0] = 0;
    t[0] = 0;
    for (int32_t u = 1; u < n; ++u) {
        while (q >= 0 && F(t[q], s[q]) > F(t[q], u)) --q;
        if (q < 0) {
            q = 0;
            s[0] = u;
        } else {
            // the first x at which parabola u is no higher than parabola s[q]: 1 + floor(num / den)
            const int64_t i = s[q];
            const int64_t num = (int64_t)u * u - i * i + (int64_t)f[u * step] - (int64_t)f[i * step];
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
        out[u * step] = (int32_t)(v < K ? v : K);
        if (u == t[q]) --q;
    }
}

}  // namespace edt
}  // namespace tgms
