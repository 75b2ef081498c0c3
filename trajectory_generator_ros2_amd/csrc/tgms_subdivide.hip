// tgms_subdivide.hip — corridor subdivision (tgms_corridor_subdivide_batch_device) on gfx950.
//
// The step before the corridor inflation: a leg whose own lattice bounding box holds a non-free
// node is halved, down to sixteenths, until every piece has a free box, and the batch (offsets,
// waypoints, times) is rebuilt on the device.  tgms_subdivide_core.h has every decision; this
// file has the mapping, which is the corridor split's and the cut's.  Three stages, launched in
// order on one stream:
//   1. k_sub_plan: the segment tile of tgms_seg_tile.h in k_inflate's shape, a wavefront per
//      TILE = 4 trajectories and a lane per leg, four wavefronts per workgroup, each with a tile
//      of its own, no LDS and no barrier.  A lane runs its leg's traversal alone: at most 31
//      tests, each eight 4-byte gathers from the occupancy table issued together and one count.
//      What the kernel waits for is those gathers; only other wavefronts hide them, so the
//      registers are kept to full occupancy (DESIGN.md has the counts).  The four demands
//      need(1..4) of a leg travel packed in one word (6, 7, 8 and 9 bits: the sums over 16 legs
//      are at most 32, 64, 128 and 256) and are summed over the lanes of the trajectory with 16
//      shuffles; every lane of the trajectory then picks the same depth.  Per leg the leaf word
//      (pack_leg) goes to scratch, per trajectory the new segment count; the flags go to the caller.
//   2. the scan: the exclusive prefix sum of the new segment counts over B, the split's three
//      k_scan_* launches from where they are (launch_count_scan; its second, int64 lane of counts
//      is zero here).
//   3. k_sub_write: the tile again, a lane per OUTPUT row (a tile has at most 64: the depth rule
//      holds every trajectory to TGMS_MAX_SEGMENTS).  The lanes scan their legs' leaf counts,
//      a row finds its leg by a six-step search through that scan, its leaf by the leg's word,
//      recomputes its first point from the leg's two waypoints and writes waypoint, time, parent
//      and flag: consecutive lanes write consecutive rows.
// No workgroup ever waits for another: each stage ends before the next begins because they are
// separate launches on one stream.
// Every store is guarded by the capacity the header names (min(2^max_depth S, 16 B) segments, B
// more waypoints, S = seg_offsets[B]); only offsets that are not a CSR (a count below 1) can
// reach a guard.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_seg_tile.h"
#include "tgms_subdivide_core.h"

namespace tgms {
namespace {

using namespace seg_tile;  // TILE, Tile, load_tile, lane_segment

constexpr int BLOCK = 256;          // threads of every workgroup here
constexpr int WAVES = BLOCK / W64;  // its wavefronts
constexpr int LEGS = TGMS_MAX_SEGMENTS;  // leaf words per trajectory in the scratch

__device__ __forceinline__ int wave_inclusive(int v, int lane) {
#pragma unroll
    for (int o = 1; o < W64; o <<= 1) {
        const int up = __shfl_up(v, o, W64);
        v += lane >= o ? up : 0;
    }
    return v;
}

__global__ __launch_bounds__(BLOCK) void k_sub_plan(int32_t B, const int32_t* __restrict__ so,
                                                    const double* __restrict__ W, inflate::Grid g,
                                                    const int32_t* __restrict__ table, int max_depth,
                                                    int32_t* __restrict__ cntS, int64_t* __restrict__ cntF,
                                                    int32_t* __restrict__ words, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    const int64_t b0 = ((int64_t)blockIdx.x * WAVES + wave) * TILE;
    if (b0 >= B) return;  // the whole wavefront
    const int nb = (int)std::min<int64_t>(TILE, B - b0);
    Tile x;
    load_tile(so, b0, nb, x);
    int tr, sb, M;
    int64_t gs;
    lane_segment(x, lane, tr, sb, M, gs);
    const bool mine = lane < x.base[TILE];
    int32_t status = subdivide::LEG_NONFINITE;
    uint32_t reached = 1u, clr = 1u;  // a leg that is never subdivided: one leaf at every depth
    if (mine) {
        const double* w = W + (gs + b0 + tr) * 3;  // rows s + b and s + b + 1
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        status = subdivide::leg_status(g, w0, w1);
        if (status == subdivide::LEG_OK) subdivide::traverse(g, table, w0, w1, max_depth, reached, clr);
    }
    // the demands of the trajectory: the sum over its lanes sb .. sb + M - 1
    int packed = 0;
    if (mine) {
        constexpr int SH[subdivide::MAX_DEPTH] = {0, 6, 13, 21};
#pragma unroll
        for (int d = 1; d <= subdivide::MAX_DEPTH; ++d)
            packed |= (d <= max_depth ? subdivide::need(reached, clr, d) : 0) << SH[d - 1];
    }
    int tot = 0;
#pragma unroll
    for (int j = 0; j < TGMS_MAX_SEGMENTS; ++j) {
        const int v = __shfl(packed, std::min(sb + j, W64 - 1), W64);
        tot += j < M ? v : 0;
    }
    const int sum[subdivide::MAX_DEPTH + 1] = {M, tot & 63, (tot >> 6) & 127, (tot >> 13) & 255, (tot >> 21) & 511};
    const int D = subdivide::pick_depth(sum, max_depth);
    int S1 = sum[0];
#pragma unroll
    for (int d = 1; d <= subdivide::MAX_DEPTH; ++d) S1 = D == d ? sum[d] : S1;
    const int32_t word =
        subdivide::pack_leg(status, subdivide::leaves(reached, D), subdivide::blocked(reached, clr, D));
    const int32_t fl = mine ? subdivide::word_flags(word) : 0;
    if (mine) words[(b0 + tr) * LEGS + (lane - sb)] = word;
    // the trajectory's flags: the OR over its lanes, bit by bit
    const unsigned long long span = mine ? ((1ull << M) - 1ull) << sb : 0ull;  // M <= 16
    constexpr int32_t BITS[3] = {TGMS_SUB_BLOCKED, TGMS_SUB_OUTSIDE, TGMS_FEAS_NONFINITE};
    int32_t all = (S1 > M ? TGMS_SUB_DONE : 0) | (D < max_depth ? TGMS_SUB_FULL : 0);
#pragma unroll
    for (int i = 0; i < 3; ++i) all |= (__ballot((fl & BITS[i]) != 0) & span) != 0ull ? BITS[i] : 0;
    if (mine && lane == sb) {
        cntS[b0 + tr] = S1;
        cntF[b0 + tr] = 0;
        if (flags) flags[b0 + tr] = all;
    }
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
        if (!(x.oob[t] && lane == t)) continue;  // a bad count: one placeholder segment, nothing read
        cntS[b0 + t] = 1;
        cntF[b0 + t] = 0;
        if (flags) flags[b0 + t] = TGMS_FEAS_NONFINITE;
    }
}

__global__ void k_sub_empty(int32_t* __restrict__ so_out, int64_t* __restrict__ totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        so_out[0] = 0;
        totals[0] = 0;
    }
}

__global__ __launch_bounds__(BLOCK) void k_sub_write(int32_t B, const int32_t* __restrict__ so,
                                                     const double* __restrict__ W, const double* __restrict__ T,
                                                     int max_depth, const int32_t* __restrict__ words,
                                                     const int32_t* __restrict__ so_out,
                                                     const int64_t* __restrict__ scan_totals,
                                                     double* __restrict__ W_out, double* __restrict__ T_out,
                                                     int32_t* __restrict__ parent, int32_t* __restrict__ seg_flags,
                                                     int64_t* __restrict__ totals) {
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[0] = scan_totals[0];
    const int64_t b0 = ((int64_t)blockIdx.x * WAVES + wave) * TILE;
    if (b0 >= B) return;  // the whole wavefront
    const int nb = (int)std::min<int64_t>(TILE, B - b0);
    // the capacities of the caller's buffers (include/tgms.h)
    const int64_t capS = std::min<int64_t>((int64_t)so[B] * (1 << max_depth), (int64_t)TGMS_MAX_SEGMENTS * B),
                  capW = capS + B;
    const double nan = __builtin_nan("");
    Tile x;
    load_tile(so, b0, nb, x);
    // as a leg: this lane's leaf word and the leaves of the tile's legs up to it
    int tr, sb, M;
    int64_t gs;
    lane_segment(x, lane, tr, sb, M, gs);
    const int32_t word = lane < x.base[TILE] ? words[(b0 + tr) * LEGS + (lane - sb)] : 0;
    const int cnt = __popc((unsigned)word & 0xFFFFu);
    const int inc = wave_inclusive(cnt, lane);
    const int total = __shfl(inc, W64 - 1, W64);  // <= 64: TGMS_MAX_SEGMENTS a trajectory
    // as an output row: the leg whose leaves hold row `lane` of the tile is the number of legs
    // whose inclusive count is at most `lane`
    int leg = 0;
#pragma unroll
    for (int step = W64 / 2; step >= 1; step >>= 1) {
        const int v = __shfl(inc, leg + step - 1, W64);
        leg += v <= lane ? step : 0;
    }
    const bool live = lane < total;
    leg = std::min(leg, W64 - 1);
    const int32_t lw = __shfl(word, leg, W64);
    const int nleaf = lane - __shfl(inc - cnt, leg, W64);  // the row's leaf within its leg
    int ltr, lsb, lM;
    int64_t lgs;
    lane_segment(x, leg, ltr, lsb, lM, lgs);
    // the row's trajectory: its first row in the tile, its rows, its first row afterwards
    int tbase = 0, tcnt = 0;
    int64_t so2 = 0;
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
        if (t >= nb) continue;
        const int32_t so_t = __builtin_amdgcn_readfirstlane(so_out[b0 + t]);
        const int hi = x.base[t + 1] > 0 ? __shfl(inc, x.base[t + 1] - 1, W64) : 0;
        const int lo = x.base[t] > 0 ? __shfl(inc, x.base[t] - 1, W64) : 0;
        tbase = ltr == t ? lo : tbase;
        tcnt = ltr == t ? hi - lo : tcnt;
        so2 = ltr == t ? (int64_t)so_t : so2;
        if (x.oob[t] && lane == 0) {
            // a segment count outside 1..16: one placeholder segment, a NaN time, two NaN
            // waypoints; the solve that follows rejects this row alone
            const int64_t w0 = so_t + b0 + t;
            if (so_t < capS) {
                if (T_out) T_out[so_t] = nan;
                if (parent) parent[so_t] = TGMS_NEAR_NONE;
                if (seg_flags) seg_flags[so_t] = TGMS_FEAS_NONFINITE;
            }
            for (int e = 0; e < 6; ++e)
                if (w0 + e / 3 < capW) W_out[w0 * 3 + e] = nan;
        }
    }
    if (!live) return;
    const int64_t b = b0 + ltr;
    const int q = lane - tbase;  // the row within its trajectory
    const int64_t orow = so2 + q;
    int i0, i1;
    subdivide::leaf_span((uint32_t)lw, nleaf, i0, i1);
    const double* w = W + (lgs + b) * 3;  // the leg's rows s + b and s + b + 1
    const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
    if (orow + b < capW) {
        double* o = W_out + (orow + b) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = subdivide::point(w0[a], w1[a], i0);
    }
    if (q == tcnt - 1 && orow + 1 + b < capW) {  // the trajectory's last waypoint
        double* o = W_out + (orow + 1 + b) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = w1[a];
    }
    if (orow < capS) {
        if (T_out) T_out[orow] = subdivide::leaf_time(T[lgs], i1 - i0);
        if (parent) parent[orow] = (int32_t)lgs;
        if (seg_flags) seg_flags[orow] = subdivide::leaf_flag(lw, i0);
    }
}

struct Scratch {
    int64_t *cntF, *sumS, *sumF, *totals;
    int32_t *cntS, *words;
    size_t bytes;
};

Scratch layout(int32_t B, void* base) {
    const size_t n = (size_t)std::max(B, 0), nblk = count_scan_blocks(B);
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    char* p = static_cast<char*>(base);
    size_t off = 0;
    Scratch s;
    s.cntF = reinterpret_cast<int64_t*>(p + off);
    off = up(off + n * sizeof(int64_t));
    s.sumS = reinterpret_cast<int64_t*>(p + off);
    off = up(off + nblk * sizeof(int64_t));
    s.sumF = reinterpret_cast<int64_t*>(p + off);
    off = up(off + nblk * sizeof(int64_t));
    s.totals = reinterpret_cast<int64_t*>(p + off);
    off = up(off + 2 * sizeof(int64_t));
    s.cntS = reinterpret_cast<int32_t*>(p + off);
    off = up(off + n * sizeof(int32_t));
    s.words = reinterpret_cast<int32_t*>(p + off);
    off = up(off + n * LEGS * sizeof(int32_t));
    s.bytes = off;
    return s;
}

}  // namespace

size_t subdivide_scratch_bytes(int32_t B) { return layout(B, nullptr).bytes; }

hipError_t launch_subdivide(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                            const tgms_field& fld, const int32_t* table, int32_t max_depth, void* scratch,
                            int32_t* so_out, double* W_out, double* T_out, int32_t* parent, int32_t* seg_flags,
                            int64_t* totals, int32_t* flags, hipStream_t stream) {
    if (B <= 0) {
        TGMS_LAUNCH(k_sub_empty, dim3(1), dim3(W64), 0, stream, so_out, totals);
        return hipSuccess;
    }
    const Scratch s = layout(B, scratch);
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const unsigned blocks = (unsigned)((tiles + WAVES - 1) / WAVES);
    TGMS_LAUNCH(k_sub_plan, dim3(blocks), dim3(BLOCK), 0, stream, B, seg_offsets, W, inflate::make_grid(fld), table,
                (int)max_depth, s.cntS, s.cntF, s.words, flags);
    if (const hipError_t e = launch_count_scan(B, s.cntS, s.cntF, s.sumS, s.sumF, 0, so_out, s.totals, stream);
        e != hipSuccess)
        return e;
    TGMS_LAUNCH(k_sub_write, dim3(blocks), dim3(BLOCK), 0, stream, B, seg_offsets, W, T, (int)max_depth, s.words,
                so_out, s.totals, W_out, T_out, parent, seg_flags, totals);
    return hipSuccess;
}

}  // namespace tgms
