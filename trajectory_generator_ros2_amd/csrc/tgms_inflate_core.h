// tgms_inflate_core.h — corridor inflation: the largest free lattice box around a segment of a
// waypoint path, shared by the gfx950 kernels (tgms_inflate.hip) and the host backend
// (tgms_host.cpp).  Plain C++17, as its siblings.  include/tgms.h states the result to the bit;
// this file holds the three pieces both backends must take from one place:
//   - the seed (seed_axis): the least lattice interval [lo, hi] per axis with
//     origin + h lo <= mn and origin + h hi >= mx, decided on the very products the faces are
//     made of.  floor / ceil of the quotient may be off by one after rounding, so one corrected
//     step follows; every operation is rounded on its own (mul_rn / add_rn: the compiler must
//     not contract origin + h i into an fma, which would make the two backends differ);
//   - the count of non-free nodes in a lattice box from the summed-volume table (box_count):
//     eight loads, issued together, signs by inclusion and exclusion;
//   - the growth (grow): up to max_grow rounds over +x -x +y -y +z -z, each direction testing
//     the one-layer slab beyond its face across the box as the earlier directions left it.  A
//     direction that meets the grid's edge or a non-free node closes for good.
// The table (table_index) is [(nz+1)][(ny+1)][(nx+1)] int32, x fastest: entry (i, j, k) counts
// the non-free nodes with index below (i, j, k) on every axis, so the planes i = 0, j = 0 and
// k = 0 are zero.  (nx+1)(ny+1)(nz+1) <= 2^31 - 1 is the caller's check; indices are formed in
// 64 bits all the same.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tgms_bounds_core.h"  // TGMS_HD, TGMS_UNROLL

namespace tgms {
namespace inflate {

// One rounding each, never an fma.  On the device the compiler contracts a * b + c by default, also
// through an inlined call, so contraction is switched off where the operations are written; on
// the host the result passes through a volatile.
TGMS_HD double mul_rn(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
    return a * b;
#else
    volatile double p = a * b;
    return p;
#endif
}
TGMS_HD double add_rn(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
    return a + b;
#else
    volatile double s = a + b;
    return s;
#endif
}

// The position of lattice plane i on an axis: the two roundings of the faces.
TGMS_HD double plane(double origin, double h, double i) { return add_rn(origin, mul_rn(h, i)); }

// A node is free when its value is at least the threshold, in fp32; NaN is not free.
TGMS_HD bool node_free(float v, float r_free) { return v >= r_free; }

struct Grid {
    double o[3];
    double h;
    int32_t n[3];
};

TGMS_HD Grid make_grid(const tgms_field& f) {
    Grid g;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        g.o[a] = f.origin[a];
        g.n[a] = f.n[a];
    }
    g.h = f.h;
    return g;
}

TGMS_HD int64_t table_index(const Grid& g, int32_t i, int32_t j, int32_t k) {
    return ((int64_t)k * (g.n[1] + 1) + j) * (int64_t)(g.n[0] + 1) + i;
}

// The seed on one axis, as doubles (a far waypoint must not overflow an integer): lo and hi
// hold integers.  w0, w1 finite.
TGMS_HD void seed_axis(double origin, double h, double w0, double w1, double& mn, double& mx, double& lo, double& hi) {
    mn = w1 < w0 ? w1 : w0;
    mx = w1 > w0 ? w1 : w0;
    lo = floor((mn - origin) / h);
    if (plane(origin, h, lo) > mn) lo -= 1.0;
    hi = ceil((mx - origin) / h);
    if (plane(origin, h, hi) < mx) hi += 1.0;
}

// The non-free nodes of the lattice box lo..hi (inclusive, inside the grid).
TGMS_HD int32_t box_count(const Grid& g, const int32_t* __restrict__ t, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                          int32_t z0, int32_t z1) {
    const int64_t sx = (int64_t)(x1 + 1 - x0), sy = (int64_t)(y1 + 1 - y0) * (g.n[0] + 1);
    const int64_t a = table_index(g, x0, y0, z0), b = table_index(g, x0, y0, z1 + 1);
    const int32_t a00 = t[a], a10 = t[a + sx], a01 = t[a + sy], a11 = t[a + sy + sx];
    const int32_t b00 = t[b], b10 = t[b + sx], b01 = t[b + sy], b11 = t[b + sy + sx];
    return ((b11 - b10) - (b01 - b00)) - ((a11 - a10) - (a01 - a00));
}

// One segment.  Returns its flags; box = lo[3] hi[3]; face[d] = the offset of face d in the
// order +x -x +y -y +z -z (the normal is +-e_a).
TGMS_HD int32_t segment(const Grid& g, const int32_t* __restrict__ table, const double (&w0)[3], const double (&w1)[3],
                        int32_t max_grow, int32_t (&box)[6], double (&face)[6]) {
    double chk = 0.0;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) chk = __builtin_fma(w0[a], 0.0, __builtin_fma(w1[a], 0.0, chk));
    if (!(chk == 0.0)) {
        TGMS_UNROLL
        for (int d = 0; d < 6; ++d) {
            box[d] = TGMS_NEAR_NONE;
            face[d] = __builtin_nan("");
        }
        return TGMS_FEAS_NONFINITE;
    }
    double mn[3], mx[3], flo[3], fhi[3];
    bool outside = false;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        seed_axis(g.o[a], g.h, w0[a], w1[a], mn[a], mx[a], flo[a], fhi[a]);
        outside = outside || !(flo[a] >= 0.0) || !(fhi[a] <= (double)(g.n[a] - 1));
    }
    if (outside) {
        TGMS_UNROLL
        for (int a = 0; a < 3; ++a) {
            box[a] = box[3 + a] = TGMS_NEAR_NONE;
            face[2 * a] = mx[a];
            face[2 * a + 1] = -mn[a];
        }
        return TGMS_INF_OUTSIDE;
    }
    int32_t lo[3], hi[3];
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int32_t)flo[a];
        hi[a] = (int32_t)fhi[a];
    }
    int32_t flags = 0;
    if (box_count(g, table, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]) != 0) {
        flags = TGMS_INF_BLOCKED;
    } else {
        unsigned open = 0x3fu;
        for (int32_t round = 0; round < max_grow && open != 0u; ++round) {
            TGMS_UNROLL
            for (int d = 0; d < 6; ++d) {
                if (!(open & (1u << d))) continue;
                const int a = d >> 1;
                const bool up = (d & 1) == 0;
                const int32_t layer = up ? hi[a] + 1 : lo[a] - 1;
                bool take = up ? layer <= g.n[a] - 1 : layer >= 0;
                if (take) {
                    const int32_t x0 = a == 0 ? layer : lo[0], x1 = a == 0 ? layer : hi[0];
                    const int32_t y0 = a == 1 ? layer : lo[1], y1 = a == 1 ? layer : hi[1];
                    const int32_t z0 = a == 2 ? layer : lo[2], z1 = a == 2 ? layer : hi[2];
                    take = box_count(g, table, x0, x1, y0, y1, z0, z1) == 0;
                }
                if (!take)
                    open &= ~(1u << d);
                else if (up)
                    hi[a] = layer;
                else
                    lo[a] = layer;
            }
        }
        if (open != 0u) flags = TGMS_INF_CAPPED;
    }
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        box[a] = lo[a];
        box[3 + a] = hi[a];
        face[2 * a] = plane(g.o[a], g.h, (double)hi[a]);
        face[2 * a + 1] = -plane(g.o[a], g.h, (double)lo[a]);
    }
    return flags;
}

// Row d of a segment's six faces: n[3] d; all four NaN for a segment that is not finite.
TGMS_HD void face_row(int d, double off, double (&row)[4]) {
    const double zero = off != off ? off : 0.0, one = off != off ? off : ((d & 1) ? -1.0 : 1.0);
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) row[a] = a == (d >> 1) ? one : zero;
    row[3] = off;
}

}  // namespace inflate
}  // namespace tgms
