// tgms_repair.hip — waypoint repair (tgms_field_nearest_free_dev, tgms_waypoints_repair_batch_dev)
// on gfx950.  include/tgms.h has the result to the bit, tgms_repair_core.h the tie rule, what a
// pass leaves for the next and the decision for one waypoint.
//
// The nearest-free map is the distance-field build's separable transform (tgms_edt.hip) with the
// argument carried, three launches:
//   - k_near_rows: a wavefront per row (j, k), rows by grid-stride.  64 values make one ballot of
//     free nodes.  A sweep from the row's end keeps per 64-node chunk its ballot and the first
//     free node beyond it in LDS; the sweep from the row's start gives every lane its nearest
//     free node to the left and to the right and stores the index of the nearer one, the left
//     one when both are equally far, or NONE beyond max_shift.
//   - k_near_lines<false> (y) and k_near_lines<true> (z): the min-plus over an LDS tile of
//     k_edt_lines: a workgroup owns LINE_JT = 32 consecutive outputs of 64 neighbouring lines,
//     consecutive lanes on consecutive lines, so every load and store of a wavefront is
//     contiguous.  The staging lane turns the site its entry holds into the square the pass starts
//     from (repair::f_row, f_plane), so the tile is [entry][line] int32 as in the EDT: a read of
//     one entry is 64 consecutive words, no bank conflict.  Each lane folds every staged entry
//     into its LINE_U = 8 outputs, the sum and the entry it came from side by side.  The entries
//     are walked in ascending order and an entry replaces the kept one only when its sum is
//     strictly less, so of equal sums the lowest entry stays: the tie rule, whatever the tiling.
//     After the walk a lane reads the winning entry's site once more and stores (j', i'), or in
//     the z pass the linear index and the square.
// Integers throughout.  The x pass writes into the output map, the y pass into the caller's
// workspace (N int32), the z pass back into the output map: no pass reads what it writes.
//
// k_repair: the segment tile of tgms_seg_tile.h, a wavefront per four trajectories and a lane per
// segment, four wavefronts a workgroup with a tile each, no LDS and no barrier.  A lane decides
// both waypoints of its leg (repair::waypoint: at most nine 4-byte gathers each), writes the row
// of the first, as the last leg of its trajectory also the row of the second, and the leg's time.
// A waypoint between two legs is decided twice from the same inputs; the lanes share nothing, so
// no result depends on the launch shape.  The trajectory's flags are the OR of its lanes' by
// ballots.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_repair_core.h"
#include "tgms_seg_tile.h"

namespace tgms {
namespace {

using namespace seg_tile;  // TILE, Tile, load_tile, lane_segment

constexpr int BLOCK = 256;               // threads of every workgroup here
constexpr int WAVES = BLOCK / W64;       // its wavefronts
constexpr int32_t MAX_BLOCKS = 256 * 8;  // k_near_rows grid-strides beyond: eight workgroups a CU
constexpr int MAX_CHUNKS = edt::MAX_NODES_PER_AXIS / W64;  // 64-node chunks of the longest row
constexpr int LINE_U = 8;                // outputs of a line a lane owns
constexpr int LINE_JT = WAVES * LINE_U;  // outputs of a line a workgroup owns
constexpr int LINE_CH = 64;              // source entries of a line staged at a time
constexpr int32_t FAR = 1 << 20;         // farther than any max_shift and any row is long

__global__ __launch_bounds__(BLOCK) void k_near_rows(const float* __restrict__ values, float r_free, int32_t nx,
                                                     int64_t rows, int32_t R, int32_t* __restrict__ out) {
    // a wavefront's own slices; every lane stores the same word, so each reads what it wrote
    __shared__ unsigned long long s_mask[WAVES][MAX_CHUNKS];
    __shared__ int32_t s_next[WAVES][MAX_CHUNKS];
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    const int32_t chunks = (nx + W64 - 1) / W64;
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const float* const in = values + row * nx;
        int32_t* const o = out + row * nx;
        int32_t next = 2 * FAR;  // the first free node beyond the chunk
        for (int32_t c = chunks - 1; c >= 0; --c) {
            const int32_t i = c * W64 + lane;
            const bool target = i < nx && inflate::node_free(in[i], r_free);
            const unsigned long long m = __ballot(target);
            s_mask[wave][c] = m;
            s_next[wave][c] = next;
            if (m != 0ull) next = c * W64 + __builtin_ctzll(m);
        }
        int32_t last = -FAR;  // the last free node before the chunk
        for (int32_t c = 0; c < chunks; ++c) {
            const unsigned long long m = s_mask[wave][c];
            const int32_t i = c * W64 + lane;
            const unsigned long long le = m & ((2ull << lane) - 1ull), ge = m & (~0ull << lane);
            const int32_t dl = le != 0ull ? lane - (63 - __builtin_clzll(le)) : i - last;
            const int32_t dr = ge != 0ull ? __builtin_ctzll(ge) - lane : s_next[wave][c] - i;
            const int32_t g = dl <= dr ? dl : dr;
            if (i < nx) o[i] = g > R ? repair::NONE : (dl <= dr ? i - dl : i + dr);
            if (m != 0ull) last = c * W64 + 63 - __builtin_clzll(m);
        }
    }
}

// Line q of `lines` starts at (q / width) outer + q % width and has n entries `step` apart.
struct Lines {
    int64_t lines, width, outer, step;
    int32_t n;
};

// Along every line: the lowest entry j' with the least f(j') + (j - j')^2 below K, f the square
// the entry's site stands for.  !LAST (y): `in` holds the x pass' i', out gets (j', i').  LAST
// (z): `in` holds the y pass' pairs, out gets the site's linear index and dsq the square.
template <bool LAST>
__global__ __launch_bounds__(BLOCK) void k_near_lines(const int32_t* __restrict__ in, Lines ln, int32_t R, int32_t K,
                                                      int32_t tiles_j, int32_t nx, int32_t ny,
                                                      int32_t* __restrict__ out, int32_t* __restrict__ dsq) {
    __shared__ int32_t tile[LINE_CH][W64];
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    const int64_t q = (int64_t)(blockIdx.x / (unsigned)tiles_j) * W64 + lane;
    const int32_t j0 = (int32_t)(blockIdx.x % (unsigned)tiles_j) * LINE_JT;
    const bool valid = q < ln.lines;
    const int64_t base = valid ? (q / ln.width) * ln.outer + q % ln.width : 0;
    // the line's own coordinates: x in the y pass, (x, y) in the z pass
    const int32_t li = valid ? (int32_t)(q % nx) : 0, lj = valid && LAST ? (int32_t)(q / nx) : 0;
    const int32_t jw = j0 + wave * LINE_U;  // the wavefront's first output
    const int32_t s_lo = std::max(0, j0 - R), s_hi = std::min(ln.n, j0 + LINE_JT + R);
    int32_t acc[LINE_U], src[LINE_U];
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) {
        acc[u] = K;
        src[u] = repair::NONE;
    }
    for (int32_t s = s_lo; s < s_hi; s += LINE_CH) {
        const int32_t staged = std::min(LINE_CH, s_hi - s);
        int32_t v[LINE_CH / WAVES];
#pragma unroll
        for (int u = 0; u < LINE_CH / WAVES; ++u) {
            const int32_t r = wave + u * WAVES;
            v[u] = valid && r < staged ? in[base + (int64_t)(s + r) * ln.step] : repair::NONE;
        }
#pragma unroll
        for (int u = 0; u < LINE_CH / WAVES; ++u)
            tile[wave + u * WAVES][lane] = LAST ? repair::f_plane(v[u], li, lj, K) : repair::f_row(v[u], li, K);
        __syncthreads();
        int32_t d = s - jw;  // source index less output index, a scalar
#pragma unroll 4
        for (int32_t r = 0; r < staged; ++r, ++d) {
            const int32_t f = tile[r][lane];
#pragma unroll
            for (int u = 0; u < LINE_U; ++u) {
                const int32_t e = d - u, c = f + e * e;
                src[u] = c < acc[u] ? s + r : src[u];
                acc[u] = std::min(acc[u], c);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) {
        const int32_t j = jw + u;
        if (!valid || j >= ln.n) continue;
        const int64_t node = base + (int64_t)j * ln.step;
        int32_t site = repair::NONE;
        if (src[u] >= 0) {
            const int32_t w = in[base + (int64_t)src[u] * ln.step];  // the winning entry's own site
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
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    const int64_t b0 = ((int64_t)blockIdx.x * WAVES + wave) * TILE;
    if (b0 >= B) return;  // the whole wavefront
    const int nb = (int)std::min<int64_t>(TILE, B - b0);
    Tile x;
    load_tile(seg_offsets, b0, nb, x);
    int tr, sb, M;
    int64_t gs;
    lane_segment(x, lane, tr, sb, M, gs);
    const bool mine = lane < x.base[TILE];
    int32_t fl = 0;
    if (mine) {
        const int64_t row = gs + b0 + tr;  // rows s + b and s + b + 1
        const double* w = W + row * 3;
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        const bool first = lane == sb, last = lane - sb == M - 1;
        double p0[3], p1[3];
        int32_t sh0, sh1;
        const int32_t f0 = repair::waypoint(g, nearest, w0, first && (mode & TGMS_RPR_KEEP_FIRST), p0, sh0);
        const int32_t f1 = repair::waypoint(g, nearest, w1, last && (mode & TGMS_RPR_KEEP_LAST), p1, sh1);
        double* o = W_out + row * 3;  // rows of 24 bytes: 8-byte stores
        o[0] = p0[0];
        o[1] = p0[1];
        o[2] = p0[2];
        if (wp_flags) wp_flags[row] = f0;
        if (shift) shift[row] = sh0;
        fl = f0;
        if (last) {
            o[3] = p1[0];
            o[4] = p1[1];
            o[5] = p1[2];
            if (wp_flags) wp_flags[row + 1] = f1;
            if (shift) shift[row + 1] = sh1;
            fl |= f1;
        }
        if (T_out) {
            const double t = T[gs];
            T_out[gs] = ((f0 | f1) & TGMS_RPR_MOVED) ? repair::leg_time(t, w0, w1, p0, p1) : t;
        }
    }
    // the trajectory's flags: the OR over its lanes sb .. sb + M - 1, bit by bit
    const unsigned long long span = mine ? ((1ull << M) - 1ull) << sb : 0ull;  // M <= 16
    constexpr int32_t BITS[5] = {TGMS_RPR_MOVED, TGMS_RPR_STUCK, TGMS_RPR_KEPT, TGMS_RPR_OUTSIDE, TGMS_FEAS_NONFINITE};
    int32_t all = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) all |= (__ballot((fl & BITS[i]) != 0) & span) != 0ull ? BITS[i] : 0;
    if (flags) {
        if (mine && lane == sb) flags[b0 + tr] = all;
#pragma unroll
        for (int t = 0; t < TILE; ++t)
            if (x.oob[t] && lane == t) flags[b0 + t] = TGMS_FEAS_NONFINITE;  // a bad count: nothing read
    }
}

}  // namespace

size_t nearest_free_work_bytes(const tgms_field& fld) {
    return sizeof(int32_t) * (size_t)fld.n[0] * (size_t)fld.n[1] * (size_t)fld.n[2];
}

hipError_t launch_nearest_free(const tgms_field& fld, const float* values, double r_free, int32_t max_shift,
                               int32_t* nearest, int32_t* dsq, void* work, hipStream_t stream) {
    const int64_t nx = fld.n[0], ny = fld.n[1], nz = fld.n[2];
    const int32_t R = max_shift, K = repair::limit(max_shift);
    int32_t* const b = static_cast<int32_t*>(work);
    const int64_t rows = ny * nz;
    const int32_t row_blocks = (int32_t)std::min<int64_t>((rows + WAVES - 1) / WAVES, MAX_BLOCKS);
    const Lines ly = {nx * nz, nx, nx * ny, nx, (int32_t)ny}, lz = {nx * ny, nx * ny, 0, nx * ny, (int32_t)nz};
    const int32_t ty = (int32_t)((ny + LINE_JT - 1) / LINE_JT), tz = (int32_t)((nz + LINE_JT - 1) / LINE_JT);
    const unsigned by = (unsigned)(((ly.lines + W64 - 1) / W64) * ty), bz = (unsigned)(((lz.lines + W64 - 1) / W64) * tz);
    TGMS_LAUNCH(k_near_rows, dim3((unsigned)row_blocks), dim3(BLOCK), 0, stream, values, (float)r_free, (int32_t)nx, rows,
                R, nearest);
    TGMS_LAUNCH(k_near_lines<false>, dim3(by), dim3(BLOCK), 0, stream, nearest, ly, R, K, ty, (int32_t)nx, (int32_t)ny, b,
                nullptr);
    TGMS_LAUNCH(k_near_lines<true>, dim3(bz), dim3(BLOCK), 0, stream, b, lz, R, K, tz, (int32_t)nx, (int32_t)ny, nearest,
                dsq);
    return hipSuccess;
}

hipError_t launch_repair(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const tgms_field& fld,
                         const int32_t* nearest, int32_t mode, double* W_out, double* T_out, int32_t* wp_flags,
                         int32_t* shift, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    TGMS_LAUNCH(k_repair, dim3((unsigned)((tiles + WAVES - 1) / WAVES)), dim3(BLOCK), 0, stream, B, seg_offsets, W, T,
                inflate::make_grid(fld), nearest, mode, W_out, T_out, wp_flags, shift, flags);
    return hipSuccess;
}

}  // namespace tgms
