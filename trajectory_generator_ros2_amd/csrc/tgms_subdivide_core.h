// tgms_subdivide_core.h — corridor subdivision: the legs of a waypoint path whose own lattice
// bounding box holds a non-free node are halved, down to sixteenths, until every piece has a free
// box or the depth runs out.  Shared by the gfx950 kernels (tgms_subdivide.hip) and the host
// backend (tgms_host.cpp).  Plain C++17, as its siblings.  include/tgms.h states the result to
// the bit; this file holds the pieces both backends must take from one place:
//   - the points (point): P(i), i = 0..16, on the leg w0 -> w1.  P(0) and P(16) are the waypoints
//     themselves; in between w0 + (i / 16) (w1 - w0) with the difference, the product and the sum
//     each rounded on its own (mul_rn / add_rn of tgms_inflate_core.h).  A point depends on i alone;
//   - whether a piece P(i0) -> P(i1) is clear (clear): the inflate call's seed of the two points
//     lies inside the grid and its eight-corner count is zero;
//   - the traversal (traverse): piece (k, j), 0 <= j < 2^k, joins P(j 2^(4-k)) and
//     P((j+1) 2^(4-k)) and has the index 2^k - 1 + j, so its children are 2 p + 1 and 2 p + 2.  A
//     piece is reached when every piece above it is not clear; only reached pieces are tested, at
//     most 2^(max_depth+1) - 1 of them.  From the two bit sets (reached, clear) come the demand
//     need(D) for every depth (need), the leaf starts of the leg at a depth on the 1/16 grid
//     (leaves) and which of those leaves are not clear (blocked);
//   - the word a leg leaves for the write stage (pack_leg) and the flag of a leaf (leaf_flag).
#pragma once

#include <stdint.h>

#include "tgms_inflate_core.h"

namespace tgms {
namespace subdivide {

constexpr int MAX_DEPTH = 4;            // sixteenths
constexpr int GRID = 1 << MAX_DEPTH;    // P(0) .. P(GRID)

// A leg that is never subdivided: one leaf at every depth.
constexpr int32_t LEG_OK = 0, LEG_OUTSIDE = 1, LEG_NONFINITE = 2;

TGMS_HD double point(double w0, double w1, int i) {
    if (i <= 0) return w0;
    if (i >= GRID) return w1;
    return inflate::add_rn(w0, inflate::mul_rn((double)i * (1.0 / GRID), inflate::add_rn(w1, -w0)));
}

// The seed of two points on the three axes; false: it leaves the grid.
TGMS_HD bool seed(const inflate::Grid& g, const double (&a)[3], const double (&b)[3], int32_t (&lo)[3],
                  int32_t (&hi)[3]) {
    bool inside = true;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        double mn, mx, flo, fhi;
        inflate::seed_axis(g.o[ax], g.h, a[ax], b[ax], mn, mx, flo, fhi);
        inside = inside && flo >= 0.0 && fhi <= (double)(g.n[ax] - 1);
        lo[ax] = inside ? (int32_t)flo : 0;
        hi[ax] = inside ? (int32_t)fhi : 0;
    }
    return inside;
}

// The piece P(i0) -> P(i1) of the finite leg w0 -> w1.
TGMS_HD bool clear(const inflate::Grid& g, const int32_t* __restrict__ table, const double (&w0)[3],
                   const double (&w1)[3], int i0, int i1) {
    double a[3], b[3];
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        a[ax] = point(w0[ax], w1[ax], i0);
        b[ax] = point(w0[ax], w1[ax], i1);
    }
    int32_t lo[3], hi[3];
    if (!seed(g, a, b, lo, hi)) return false;
    return inflate::box_count(g, table, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]) == 0;
}

// Whether the leg can be subdivided at all: every waypoint coordinate and every difference finite,
// and the leg's own seed inside the grid.
TGMS_HD int32_t leg_status(const inflate::Grid& g, const double (&w0)[3], const double (&w1)[3]) {
    double chk = 0.0;
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        const double d = inflate::add_rn(w1[ax], -w0[ax]);
        chk = __builtin_fma(w0[ax], 0.0, __builtin_fma(w1[ax], 0.0, __builtin_fma(d, 0.0, chk)));
    }
    if (!(chk == 0.0)) return LEG_NONFINITE;
    int32_t lo[3], hi[3];
    return seed(g, w0, w1, lo, hi) ? LEG_OK : LEG_OUTSIDE;
}

// The pieces of a level: bits 2^k - 1 .. 2^(k+1) - 2; of the levels above it: bits 0 .. 2^k - 2.
TGMS_HD uint32_t level_bits(int k) { return (uint32_t)(((uint64_t)1 << ((2 << k) - 1)) - ((uint64_t)1 << ((1 << k) - 1))); }
TGMS_HD uint32_t above_bits(int k) { return ((uint32_t)1 << ((1 << k) - 1)) - 1u; }

// The one traversal of a leg that can be subdivided (LEG_OK): the pieces that are reached down to
// max_depth and those of them that are clear.
TGMS_HD void traverse(const inflate::Grid& g, const int32_t* __restrict__ table, const double (&w0)[3],
                      const double (&w1)[3], int max_depth, uint32_t& reached, uint32_t& clr) {
    reached = 1u;
    clr = 0u;
    const int pieces = (2 << max_depth) - 1;
    for (int p = 0; p < pieces; ++p) {
        if (!((reached >> p) & 1u)) continue;
        const int k = 31 - __builtin_clz((unsigned)(p + 1)), j = p + 1 - (1 << k), step = GRID >> k;
        if (clear(g, table, w0, w1, j * step, (j + 1) * step))
            clr |= 1u << p;
        else if (k < max_depth)
            reached |= 3u << (2 * p + 1);
    }
}

// need(leg, D), D <= the max_depth of the traversal: the clear pieces above level D and every
// reached piece of level D.
TGMS_HD int need(uint32_t reached, uint32_t clr, int D) {
    return __builtin_popcount(clr & above_bits(D)) + __builtin_popcount(reached & level_bits(D));
}

// The leaf starts of the leg at depth D on the 1/16 grid (bit i: a leaf starts at P(i)): the start
// of every reached piece down to level D.  starts: the starts of the given pieces of level k.
TGMS_HD uint32_t starts(uint32_t pieces, int k) {
    uint32_t m = 0u;
    const int n = 1 << k, sh = MAX_DEPTH - k;
    for (int j = 0; j < n; ++j) m |= ((pieces >> (n - 1 + j)) & 1u) << (j << sh);
    return m;
}
TGMS_HD uint32_t leaves(uint32_t reached, int D) {
    uint32_t m = 0u;
    for (int k = 0; k <= D; ++k) m |= starts(reached, k);
    return m;
}
TGMS_HD uint32_t blocked(uint32_t reached, uint32_t clr, int D) { return starts(reached & ~clr, D); }

// What the plan leaves per leg: bits 0..15 the leaf starts, bits 16..31 the starts of the leaves
// that are not clear.  A leg that is never subdivided has the one leaf 0; bits 17 and 18, which
// cannot be blocked leaves then, say why.
TGMS_HD int32_t pack_leg(int32_t status, uint32_t leaf, uint32_t blk) {
    if (status == LEG_OUTSIDE) return (int32_t)(1u | (1u << 17));
    if (status == LEG_NONFINITE) return (int32_t)(1u | (1u << 18));
    return (int32_t)(leaf | (blk << 16));
}
TGMS_HD int32_t word_flags(int32_t word) {  // the flags of all leaves of the leg together
    const uint32_t w = (uint32_t)word;
    if ((w & 0xFFFFu) == 1u && (w & (3u << 17))) return (w & (1u << 17)) ? TGMS_SUB_OUTSIDE : TGMS_FEAS_NONFINITE;
    return (w >> 16) ? TGMS_SUB_BLOCKED : 0;
}
TGMS_HD int32_t leaf_flag(int32_t word, int i0) {
    const uint32_t w = (uint32_t)word;
    if ((w & 0xFFFFu) == 1u && (w & (3u << 17))) return (w & (1u << 17)) ? TGMS_SUB_OUTSIDE : TGMS_FEAS_NONFINITE;
    return ((w >> (16 + i0)) & 1u) ? TGMS_SUB_BLOCKED : 0;
}

// Leaf n (from the left) of a leg with leaf starts `leaf`: its first and last point.
TGMS_HD void leaf_span(uint32_t leaf, int n, int& i0, int& i1) {
    uint32_t m = leaf & 0xFFFFu;
    for (int q = 0; q < n; ++q) m &= m - 1u;  // drop the n lowest starts
    i0 = __builtin_ctz(m | (1u << GRID));
    m &= m - 1u;
    i1 = __builtin_ctz(m | (1u << GRID));
}

// The time of a leaf of `len` sixteenths: T 2^-k, exact; a whole leg keeps its bits.
TGMS_HD double leaf_time(double T, int len) { return len == GRID ? T : T * ((double)len * (1.0 / GRID)); }

// The depth of a trajectory from its legs' summed demands sum[D]: the largest D <= max_depth
// with sum[D] <= TGMS_MAX_SEGMENTS.  sum[0] = M always fits.
TGMS_HD int pick_depth(const int (&sum)[MAX_DEPTH + 1], int max_depth) {
    int D = 0;
    for (int d = 1; d <= MAX_DEPTH; ++d) D = (d <= max_depth && sum[d] <= TGMS_MAX_SEGMENTS) ? d : D;
    return D;
}

}  // namespace subdivide
}  // namespace tgms
