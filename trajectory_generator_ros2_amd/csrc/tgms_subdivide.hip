// tgms_subdivide.hip — corridor subdivision (tgms_corridor_subdivide_batch_device) on gfx950.
//
// The step before the corridor inflation: a leg whose own lattice bounding box holds a non-free
// node is halved, down to sixteenths, until every piece has a free box, and the batch (offsets,
// waypoints, times) is rebuilt on the device.  tgms_subdivide_core.h has every decision,
// tgms_seg_tile.h the mapping.  Three stages, launched in order on one stream:
//   1. k_sub_plan: a lane per leg (wave_tile).  A lane runs its leg's traversal alone: at most 31
//      tests, each eight 4-byte gathers from the occupancy table issued together and one count.
//      What the kernel waits for is those gathers; only other wavefronts hide them, so the
//      registers are kept to full occupancy (DESIGN.md has the counts).  The four demands
//      need(1..4) of a leg travel packed in one word (6, 7, 8 and 9 bits: the sums over 16 legs
//      are at most 32, 64, 128 and 256) through one trajectory_sum; every lane of the trajectory
//      then picks the same depth.  Per leg the leaf word (pack_leg) goes to scratch, per
//      trajectory the new segment count; the flags go to the caller.
//   2. the scan of the new segment counts (launch_count_scan).
//   3. k_sub_write: a lane per output row (row_map; the depth rule holds every trajectory to
//      TGMS_MAX_SEGMENTS rows).  A row finds its leaf by its leg's word, recomputes its first
//      point from the leg's two waypoints and writes waypoint, time, parent and flag:
//      consecutive lanes write consecutive rows.
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

using namespace seg_tile;

constexpr int LEGS = TGMS_MAX_SEGMENTS;  // leaf words per trajectory in the scratch

__global__ __launch_bounds__(BLOCK) void k_sub_plan(int32_t B, const int32_t* __restrict__ so,
                                                    const double* __restrict__ W, inflate::Grid g,
                                                    const int32_t* __restrict__ table, int max_depth,
                                                    int32_t* __restrict__ cntS, int64_t* __restrict__ cntF,
                                                    int32_t* __restrict__ words, int32_t* __restrict__ flags) {
    Lane l;
    if (!wave_tile(B, so, l)) return;
    const int M = l.M;
    int32_t status = subdivide::LEG_NONFINITE;
    uint32_t reached = 1u, clr = 1u;  // a leg that is never subdivided: one leaf at every depth
    if (l.mine) {
        const double* w = W + (l.gs + l.b0 + l.tr) * 3;  // rows s + b and s + b + 1
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        status = subdivide::leg_status(g, w0, w1);
        if (status == subdivide::LEG_OK) subdivide::traverse(g, table, w0, w1, max_depth, reached, clr);
    }
    // the demands of the trajectory
    int packed = 0;
    if (l.mine) {
        constexpr int SH[subdivide::MAX_DEPTH] = {0, 6, 13, 21};
#pragma unroll
        for (int d = 1; d <= subdivide::MAX_DEPTH; ++d)
            packed |= (d <= max_depth ? subdivide::need(reached, clr, d) : 0) << SH[d - 1];
    }
    const int tot = trajectory_sum(packed, l.sb, M);
    const int sum[subdivide::MAX_DEPTH + 1] = {M, tot & 63, (tot >> 6) & 127, (tot >> 13) & 255, (tot >> 21) & 511};
    const int D = subdivide::pick_depth(sum, max_depth);
    int S1 = sum[0];
#pragma unroll
    for (int d = 1; d <= subdivide::MAX_DEPTH; ++d) S1 = D == d ? sum[d] : S1;
    const int32_t word =
        subdivide::pack_leg(status, subdivide::leaves(reached, D), subdivide::blocked(reached, clr, D));
    const int32_t fl = l.mine ? subdivide::word_flags(word) : 0;
    if (l.mine) words[(l.b0 + l.tr) * LEGS + (l.lane - l.sb)] = word;
    constexpr int32_t BITS[3] = {TGMS_SUB_BLOCKED, TGMS_SUB_OUTSIDE, TGMS_FEAS_NONFINITE};
    const int32_t all = (S1 > M ? TGMS_SUB_DONE : 0) | (D < max_depth ? TGMS_SUB_FULL : 0) |
                        trajectory_flags(fl, l.mine, l.sb, M, BITS);
    store_plan(l, S1, all, cntS, cntF, flags);
}

__global__ void k_sub_empty(int32_t* __restrict__ so_out, int64_t* __restrict__ totals) { empty_batch(so_out, totals); }

__global__ __launch_bounds__(BLOCK) void k_sub_write(int32_t B, const int32_t* __restrict__ so,
                                                     const double* __restrict__ W, const double* __restrict__ T,
                                                     int max_depth, const int32_t* __restrict__ words,
                                                     const int32_t* __restrict__ so_out,
                                                     const int64_t* __restrict__ scan_totals,
                                                     double* __restrict__ W_out, double* __restrict__ T_out,
                                                     int32_t* __restrict__ parent, int32_t* __restrict__ seg_flags,
                                                     int64_t* __restrict__ totals) {
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[0] = scan_totals[0];
    Lane l;
    if (!wave_tile(B, so, l)) return;
    // the capacities of the caller's buffers (include/tgms.h)
    const int64_t capS = std::min<int64_t>((int64_t)so[B] * (1 << max_depth), (int64_t)TGMS_MAX_SEGMENTS * B),
                  capW = capS + B;
    // as a leg: this lane's leaf word; as an output row: a leaf of leg r.leg
    const int32_t word = l.mine ? words[(l.b0 + l.tr) * LEGS + (l.lane - l.sb)] : 0;
    const Row r = row_map(l, __popc((unsigned)word & 0xFFFFu), so_out);
    const int32_t lw = __shfl(word, r.leg, W64);
    placeholder_rows(l, r, capS, capW, W_out, T_out, parent, seg_flags);
    if (!r.live) return;
    const int64_t b = l.b0 + r.ltr;
    const int q = l.lane - r.tbase;  // the row within its trajectory
    const int64_t orow = r.so2 + q;
    int i0, i1;
    subdivide::leaf_span((uint32_t)lw, r.at, i0, i1);
    const double* w = W + (r.lgs + b) * 3;  // the leg's rows s + b and s + b + 1
    const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
    if (orow + b < capW) {
        double* o = W_out + (orow + b) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = subdivide::point(w0[a], w1[a], i0);
    }
    if (q == r.tcnt - 1 && orow + 1 + b < capW) copy3(W_out + (orow + 1 + b) * 3, w1);  // the trajectory's last waypoint
    if (orow < capS) {
        if (T_out) T_out[orow] = subdivide::leaf_time(T[r.lgs], i1 - i0);
        if (parent) parent[orow] = (int32_t)r.lgs;
        if (seg_flags) seg_flags[orow] = subdivide::leaf_flag(lw, i0);
    }
}

struct Scratch : ScanScratch {
    int32_t *cntS, *words;
    Scratch(int32_t B, void* base) : ScanScratch(B, base, true) {
        cntS = take<int32_t>(n);
        words = take<int32_t>(n * LEGS);
    }
};

}  // namespace

size_t subdivide_scratch_bytes(int32_t B) { return Scratch(B, nullptr).off; }

hipError_t launch_subdivide(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                            const tgms_field& fld, const int32_t* table, int32_t max_depth, void* scratch,
                            int32_t* so_out, double* W_out, double* T_out, int32_t* parent, int32_t* seg_flags,
                            int64_t* totals, int32_t* flags, hipStream_t stream) {
    if (B <= 0) {
        TGMS_LAUNCH(k_sub_empty, dim3(1), dim3(W64), 0, stream, so_out, totals);
        return hipSuccess;
    }
    const Scratch s(B, scratch);
    const unsigned blocks = wave_tile_blocks(B);
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
