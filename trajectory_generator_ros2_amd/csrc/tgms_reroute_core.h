// tgms_reroute_core.h — corridor re-route: a leg whose own lattice box holds a non-free node is
// replaced by a detour through the free nodes of a bounded window of the map, reduced to a few
// pieces with certified free boxes.  Shared by the gfx950 kernels (tgms_reroute.hip) and the host
// backend (tgms_host.cpp).  Plain C++17, as its siblings.  include/tgms.h states the result to
// the bit; this file holds the pieces both backends must take from one place:
//   - which legs are searched (classify): finite, not degenerate, the seed inside the grid and
//     holding a non-free node -- the legs the inflation reports TGMS_INF_BLOCKED for;
//   - the window (window) and the end nodes (nearest);
//   - the six neighbours of a window node in the order +x -x +y -y +z -z (neighbour): the search
//     and the descent both walk them, the descent taking the first with dist - 1;
//   - the points of a path (node_point), whether two points have a clear box (clear_points, the
//     subdivision's predicate) and what a failed test means for the greedy (on_fail);
//   - lengths and piece times (length, piece_time);
//   - the record a leg leaves for the write stage (Record: 32 bytes a segment).
// The search itself is not here: a queue on the host, level-synchronous in LDS on the device.
// dist is an exact integer, so how it is found cannot change a result.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tgms_inflate_core.h"
#include "tgms_subdivide_core.h"

namespace tgms {
namespace reroute {

constexpr int MAX_PIECES = 8;
constexpr int64_t WINDOW_NODES = TGMS_RRT_WINDOW_NODES;
// The search's distances are 16 bits: a path inside a window has at most WINDOW_NODES - 1 steps.
constexpr uint16_t D_NOT_FREE = 0xFFFFu, D_UNREACHED = 0xFFFEu;
static_assert(WINDOW_NODES - 1 < D_UNREACHED, "a hop count must not collide with the sentinels");

TGMS_HD uint64_t bits(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}
TGMS_HD bool same_point(const double (&a)[3], const double (&b)[3]) {
    return bits(a[0]) == bits(b[0]) && bits(a[1]) == bits(b[1]) && bits(a[2]) == bits(b[2]);
}

// The flag of a leg that is not searched, or -1: a candidate, lo / hi its seed.
TGMS_HD int32_t classify(const inflate::Grid& g, const int32_t* __restrict__ table, const double (&w0)[3],
                         const double (&w1)[3], int32_t (&lo)[3], int32_t (&hi)[3]) {
    double chk = 0.0;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        chk = __builtin_fma(w0[a], 0.0, __builtin_fma(w1[a], 0.0, chk));
        lo[a] = hi[a] = 0;
    }
    if (!(chk == 0.0)) return TGMS_FEAS_NONFINITE;
    if (!subdivide::seed(g, w0, w1, lo, hi)) return TGMS_RRT_OUTSIDE;
    if (inflate::box_count(g, table, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]) == 0) return 0;
    return same_point(w0, w1) ? TGMS_RRT_BLOCKED : -1;
}

// The window: the seed widened by margin nodes on each side, clipped to the grid.
struct Window {
    int32_t lo[3], n[3];
    int64_t nodes;
};
TGMS_HD Window window(const inflate::Grid& g, const int32_t (&lo)[3], const int32_t (&hi)[3], int32_t margin) {
    Window w;
    w.nodes = 1;
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) {
        const int64_t l = (int64_t)lo[a] - margin, h = (int64_t)hi[a] + margin;
        const int32_t l32 = (int32_t)(l < 0 ? 0 : l), h32 = (int32_t)(h > g.n[a] - 1 ? g.n[a] - 1 : h);
        w.lo[a] = l32;
        w.n[a] = h32 - l32 + 1;
        w.nodes *= w.n[a];  // at most (2^31 - 1)^(1/3) per axis: the table's rule
    }
    return w;
}
TGMS_HD int32_t window_index(const Window& w, int32_t x, int32_t y, int32_t z) {  // window coordinates
    return (z * w.n[1] + y) * w.n[0] + x;
}

// The nearest node to a coordinate, clamped to the seed.
TGMS_HD int32_t nearest(double origin, double h, double v, int32_t lo, int32_t hi) {
    const double f = floor(inflate::add_rn(inflate::add_rn(v, -origin) / h, 0.5));
    return f < (double)lo ? lo : (f > (double)hi ? hi : (int32_t)f);
}

TGMS_HD bool node_free(const inflate::Grid& g, const int32_t* __restrict__ table, int32_t i, int32_t j, int32_t k) {
    return inflate::box_count(g, table, i, i, j, j, k, k) == 0;
}

// Neighbour d (+x -x +y -y +z -z) of the window node (x, y, z): false when it leaves the window.
TGMS_HD bool neighbour(const Window& w, int32_t x, int32_t y, int32_t z, int d, int32_t& nx, int32_t& ny, int32_t& nz) {
    const int s = (d & 1) ? -1 : 1, a = d >> 1;
    nx = x + (a == 0 ? s : 0);
    ny = y + (a == 1 ? s : 0);
    nz = z + (a == 2 ? s : 0);
    return nx >= 0 && nx < w.n[0] && ny >= 0 && ny < w.n[1] && nz >= 0 && nz < w.n[2];
}

// Grid nodes as one int32 (the table's rule keeps nx ny nz inside it).
TGMS_HD int32_t node_id(const inflate::Grid& g, int32_t i, int32_t j, int32_t k) { return (k * g.n[1] + j) * g.n[0] + i; }
TGMS_HD void node_point(const inflate::Grid& g, int32_t id, double (&p)[3]) {
    const int32_t i = id % g.n[0], r = id / g.n[0];
    const int32_t ix[3] = {i, r % g.n[1], r / g.n[1]};
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) p[a] = inflate::plane(g.o[a], g.h, (double)ix[a]);
}

// The subdivision's predicate on two points.
TGMS_HD bool clear_points(const inflate::Grid& g, const int32_t* __restrict__ table, const double (&a)[3],
                          const double (&b)[3]) {
    int32_t lo[3], hi[3];
    if (!subdivide::seed(g, a, b, lo, hi)) return false;
    return inflate::box_count(g, table, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]) == 0;
}

// The greedy.  The targets of a leg are its path nodes in order, then w1; target -1 is w0.  From
// anchor a the first target f > a whose box with the anchor is not clear ends the piece at f - 1.
// What that means with `anchors` interior anchors recorded so far: 0, target f - 1 is the next
// anchor; or the flag that ends the leg.
TGMS_HD int32_t on_fail(int a, int f, int anchors, int max_pieces) {
    if (f == a + 1) return TGMS_RRT_ENDS;
    return anchors + 2 > max_pieces ? TGMS_RRT_LONG : 0;
}

TGMS_HD double length(const double (&u)[3], const double (&v)[3]) {
    const double dx = inflate::add_rn(v[0], -u[0]), dy = inflate::add_rn(v[1], -u[1]), dz = inflate::add_rn(v[2], -u[2]);
    return sqrt(inflate::add_rn(inflate::add_rn(inflate::mul_rn(dx, dx), inflate::mul_rn(dy, dy)), inflate::mul_rn(dz, dz)));
}
TGMS_HD double piece_time(double T, double piece, double leg) { return inflate::mul_rn(T, piece / leg); }

// What a leg leaves for the count and the write: its pieces (1: kept whole), its flag when kept
// (without the budget's say) and the interior anchors as grid nodes.  32 bytes a segment.
struct Record {
    int32_t head;                      // pieces | flag << 8
    int32_t anchor[MAX_PIECES - 1];
};
TGMS_HD int32_t pack_head(int pieces, int32_t flag) { return pieces | (flag << 8); }
TGMS_HD int head_pieces(int32_t head) { return head & 0xFF; }
TGMS_HD int32_t head_flag(int32_t head) { return head >> 8; }
// The flag of a kept leg once the trajectory's budget is known: under TGMS_RRT_FULL a candidate
// carries TGMS_RRT_BLOCKED alone.
TGMS_HD int32_t kept_flag(int32_t head, bool full) {
    const int32_t f = head_flag(head);
    if (head_pieces(head) > 1) return full ? TGMS_RRT_BLOCKED : 0;
    return (full && (f & TGMS_RRT_BLOCKED)) ? TGMS_RRT_BLOCKED : f;
}

}  // namespace reroute
}  // namespace tgms
