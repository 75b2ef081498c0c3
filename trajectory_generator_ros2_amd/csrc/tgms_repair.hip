// tgms_repair.hip — waypoint repair (tgms_field_nearest_free_dev, tgms_waypoints_repair_batch_dev)
// on gfx950.  include/tgms.h has the result to the bit, tgms_repair_core.h the tie rule, what a
// pass leaves for the next and the decision for one waypoint.
//
// The nearest-free map is the separable pass of tgms_sep_pass.h with the argument carried, three
// launches:
//   - k_near_rows: a node is a target when it is free; a node stores the index of the nearer of
//     its two targets, the left one when both are equally far, or NONE beyond max_shift.
//   - k_near_lines<false> (y) and k_near_lines<true> (z): the staging lane turns the site its
//     entry holds into the square the pass starts from (repair::f_row, f_plane).  The pass keeps
//     the lowest entry of the least sum: the tie rule, whatever the tiling.  After the walk a lane
//     reads the winning entry's site once more and stores (j', i'), or in the z pass the linear
//     index and the square.
// The x pass writes into the output map, the y pass into the caller's workspace (N int32), the z
// pass back into the output map: no pass reads what it writes.
//
// k_repair: a lane per segment (wave_tile of tgms_seg_tile.h).  A lane decides both waypoints of
// its leg (repair::waypoint: at most nine 4-byte gathers each), writes the row of the first, as
// the last leg of its trajectory also the row of the second, and the leg's time.  A waypoint
// between two legs is decided twice from the same inputs; the lanes share nothing, so no result
// depends on the launch shape.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_repair_core.h"
#include "tgms_seg_tile.h"
#include "tgms_sep_pass.h"

namespace tgms {
namespace {

using namespace sep_pass;  // BLOCK and WAVES are the segment tile's too
using seg_tile::Lane;
static_assert(BLOCK == seg_tile::BLOCK, "k_repair is launched with this file's BLOCK");

__global__ __launch_bounds__(BLOCK) void k_near_rows(const float* __restrict__ values, float r_free, int32_t nx,
                                                     int64_t rows, int32_t R, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const float* const in = values + row * nx;
        int32_t* const o = out + row * nx;
        row_sweep(
            nx, lane, wave, [&](int32_t i) { return inflate::node_free(in[i], r_free); },
            [&](int32_t i, int32_t dl, int32_t dr) {
                const int32_t g = dl <= dr ? dl : dr;
                o[i] = g > R ? repair::NONE : (dl <= dr ? i - dl : i + dr);
            });
    }
}

// Along every line: the lowest entry j' with the least f(j') + (j - j')^2 below K, f the square
// the entry's site stands for.  !LAST (y): `in` holds the x pass' i', out gets (j', i').  LAST
// (z): `in` holds the y pass' pairs, out gets the site's linear index and dsq the square.
template <bool LAST>
__global__ __launch_bounds__(BLOCK) void k_near_lines(const int32_t* __restrict__ in, Lines ln, int32_t R, int32_t K,
                                                      int32_t tiles_j, int32_t nx, int32_t ny,
                                                      int32_t* __restrict__ out, int32_t* __restrict__ dsq) {
    const LineLane p = line_lane(ln, tiles_j);
    // the line's own coordinates: x in the y pass, (x, y) in the z pass
    const int32_t li = p.valid ? (int32_t)(p.q % nx) : 0, lj = p.valid && LAST ? (int32_t)(p.q / nx) : 0;
    int32_t acc[LINE_U], src[LINE_U];
    line_pass<true>(
        in, ln, p, R, K, repair::NONE,
        [&](int32_t v) { return LAST ? repair::f_plane(v, li, lj, K) : repair::f_row(v, li, K); }, acc, src);
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) {
        const int32_t j = p.jw + u;
        if (!p.valid || j >= ln.n) continue;
        const int64_t node = p.base + (int64_t)j * ln.step;
        int32_t site = repair::NONE;
        if (src[u] >= 0) {
            const int32_t w = in[p.base + (int64_t)src[u] * ln.step];  // the winning entry's own site
            site = LAST ? (src[u] * ny + repair::site_y(w)) * nx + repair::site_x(w) : repair::pack_yx(src[u], w);
        }
        out[node] = site;
        if (LAST && dsq) dsq[node] = src[u] >= 0 ? acc[u] : repair::NONE;
    }
}

__global__ __launch_bounds__(BLOCK) void k_repair(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                  const double* __restrict__ W, const double* __restrict__ T,
                                                  inflate::Grid g, const int32_t* __restrict__ nearest, int32_t mode,
                                                  double* __restrict__ W_out, double* __restrict__ T_out,
                                                  int32_t* __restrict__ wp_flags, int32_t* __restrict__ shift,
                                                  int32_t* __restrict__ flags) {
    Lane l;
    if (!seg_tile::wave_tile(B, seg_offsets, l)) return;
    int32_t fl = 0;
    if (l.mine) {
        const int64_t row = l.gs + l.b0 + l.tr;  // rows s + b and s + b + 1
        const double* w = W + row * 3;
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        const bool first = l.lane == l.sb, last = l.lane - l.sb == l.M - 1;
        double p0[3], p1[3];
        int32_t sh0, sh1;
        const int32_t f0 = repair::waypoint(g, nearest, w0, first && (mode & TGMS_RPR_KEEP_FIRST), p0, sh0);
        const int32_t f1 = repair::waypoint(g, nearest, w1, last && (mode & TGMS_RPR_KEEP_LAST), p1, sh1);
        double* o = W_out + row * 3;  // rows of 24 bytes: 8-byte stores
        seg_tile::copy3(o, p0);
        if (wp_flags) wp_flags[row] = f0;
        if (shift) shift[row] = sh0;
        fl = f0;
        if (last) {
            seg_tile::copy3(o + 3, p1);
            if (wp_flags) wp_flags[row + 1] = f1;
            if (shift) shift[row + 1] = sh1;
            fl |= f1;
        }
        if (T_out) {
            const double t = T[l.gs];
            T_out[l.gs] = ((f0 | f1) & TGMS_RPR_MOVED) ? repair::leg_time(t, w0, w1, p0, p1) : t;
        }
    }
    constexpr int32_t BITS[5] = {TGMS_RPR_MOVED, TGMS_RPR_STUCK, TGMS_RPR_KEPT, TGMS_RPR_OUTSIDE, TGMS_FEAS_NONFINITE};
    seg_tile::store_flags(l, seg_tile::trajectory_flags(fl, l.mine, l.sb, l.M, BITS), flags);
}

}  // namespace

size_t nearest_free_work_bytes(const tgms_field& fld) {
    return sizeof(int32_t) * (size_t)fld.n[0] * (size_t)fld.n[1] * (size_t)fld.n[2];
}

hipError_t launch_nearest_free(const tgms_field& fld, const float* values, double r_free, int32_t max_shift,
                               int32_t* nearest, int32_t* dsq, void* work, hipStream_t stream) {
    const int32_t nx = fld.n[0], ny = fld.n[1], R = max_shift, K = repair::limit(max_shift);
    int32_t* const b = static_cast<int32_t*>(work);
    const Geometry g = geometry(fld);
    TGMS_LAUNCH(k_near_rows, dim3(g.row_blocks), dim3(BLOCK), 0, stream, values, (float)r_free, nx, g.rows, R, nearest);
    TGMS_LAUNCH(k_near_lines<false>, dim3(g.by), dim3(BLOCK), 0, stream, nearest, g.ly, R, K, g.ty, nx, ny, b, nullptr);
    TGMS_LAUNCH(k_near_lines<true>, dim3(g.bz), dim3(BLOCK), 0, stream, b, g.lz, R, K, g.tz, nx, ny, nearest, dsq);
    return hipSuccess;
}

hipError_t launch_repair(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const tgms_field& fld,
                         const int32_t* nearest, int32_t mode, double* W_out, double* T_out, int32_t* wp_flags,
                         int32_t* shift, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    TGMS_LAUNCH(k_repair, dim3(seg_tile::wave_tile_blocks(B)), dim3(BLOCK), 0, stream, B, seg_offsets, W, T,
                inflate::make_grid(fld), nearest, mode, W_out, T_out, wp_flags, shift, flags);
    return hipSuccess;
}

}  // namespace tgms
