// tgms_clearance.hip — obstacle clearance (tgms_clearance_batch_device) on gfx950.
//
// Per trajectory i the closest static box whose distance falls below r_min, how many do, and
// how many reached the exact computation.  include/tgms.h has the semantics;
// tgms_clearance_core.h the combinations, the exact item and the argument that the boxes and
// the cull threshold of tgms_neighbors_core.h stay sound here.
//
// Two launches on handle scratch laid out as k_neighbors' (per trajectory, sized by B: the
// segment total of a device batch is not known on the host), with one word per obstacle behind:
//   ub   [B][6]      the hull of the trajectory's boxes: what a sweep reads
//   kn   [B][18]     prefix sums of the times (knots 0..M with start 0), the last time in slot 17
//   bx   [B][18][6]  boxes: held start, segments, held end
//   meta [B][2]      int32: the segment count M (0: the trajectory is unusable), the first segment
//   ook  [K]         int32: 1 when the obstacle is usable
//
// k_clearance_boxes: a lane per trajectory runs neighbors::vehicle_boxes with start 0, and a
// lane per obstacle clearance::obstacle_ok.  The only place that looks at every coefficient.
//
// k_clearance: a wavefront per workgroup owns `rows` consecutive trajectories (1..ROWS, chosen
// by the launch; no result depends on it).  Its lanes sweep the obstacles in chunks of 64, a
// lane per obstacle:
//   - the chunk's boxes are staged in LDS once and tested against each row's hull, then
//     against the row's segment boxes (from L2) until one survives;
//   - survivors are compacted by ballot / mbcnt into an LDS queue of (row, obstacle); every
//     queued pair runs the exact computation, so the queue's traffic is `tested`;
//   - whenever the queue holds TILE = 16 pairs, and once more after the last chunk, 16 pairs
//     leave its tail.  Their 16 x 16 (pair, segment) slots are tested against the segment box
//     again, each survivor gets its mask of admissible states and its number of combinations,
//     and an exclusive prefix sum over the 256 slots numbers the (pair, segment, combination)
//     items.  The item list is never written: a round takes the next 64 item numbers, a lane
//     finds its slot by bisection of the prefix sums and its combination by counting through
//     the mask, runs clearance::combo_item and leaves (d^2, t) in LDS; lane p < 16 then folds
//     the part of the round that belongs to pair p (a contiguous range, in item order, strict
//     <) into registers it keeps across the rounds.  LDS holds 64 results, whatever the tile
//     expands to (up to 16 x 16 x 26 items);
//   - separation::finish makes the pair's record, and lane r < rows folds the tile's records
//     of its row into the row's running result (neighbors::row_update: smallest stored d_min,
//     ties to the lowest obstacle; order-free).
// One store per output per row at the end, no atomics, and no loop whose depth depends on a
// coefficient beyond the count of admissible combinations: a combination is bisected 40 times
// per sign change or not at all.
#include <algorithm>

#include "tgms_clearance_core.h"
#include "tgms_device.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

using clearance::OBS_STRIDE;
using neighbors::BOX_STRIDE;
using neighbors::BOXES;
using neighbors::KNOT_STRIDE;

constexpr int TILE = 16;                         // pairs of one narrow tile
constexpr int SLOTS = TILE * TGMS_MAX_SEGMENTS;  // (pair, segment) slots of a tile: 256
constexpr int ROWS = 16;                         // most rows of one workgroup
constexpr int QCAP = TILE - 1 + W64;             // what a sweep step can leave in the queue
constexpr int PREP_BLOCK = 64;
static_assert(TILE <= W64 && ROWS <= W64 && SLOTS % W64 == 0, "one pass of the wavefront");

struct ClrScale {
    double s[3];
};

// As k_neighbors': the lane index as a value the compiler cannot tie to an earlier copy, so
// that what the rarely run sections derive from it is not held across the item loop.
__device__ __forceinline__ int fresh_lane() {
    int l = threadIdx.x;
    asm volatile("" : "+v"(l));
    return l;
}

__global__ __launch_bounds__(PREP_BLOCK) void k_clearance_boxes(int32_t B, int32_t K,
                                                                const int32_t* __restrict__ seg_offsets,
                                                                const double* __restrict__ T,
                                                                const double* __restrict__ C,
                                                                const double* __restrict__ obs,
                                                                int32_t* __restrict__ meta, double* __restrict__ ub,
                                                                double* __restrict__ kn, double* __restrict__ bx,
                                                                int32_t* __restrict__ ook) {
    const int32_t b = blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (b < K) ook[b] = clearance::obstacle_ok(obs + (int64_t)b * OBS_STRIDE) ? 1 : 0;
    if (b >= B) return;
    const int32_t s0 = seg_offsets[b];
    const int32_t M = seg_offsets[b + 1] - s0;
    bool ok = M >= 1 && M <= TGMS_MAX_SEGMENTS;  // the offsets are the caller's: another span reads nothing
    ok = ok && neighbors::vehicle_boxes(M, C + (int64_t)s0 * 24, T + s0, 0.0, kn + (int64_t)b * KNOT_STRIDE,
                                        bx + (int64_t)b * (BOXES * BOX_STRIDE), ub + (int64_t)b * BOX_STRIDE);
    meta[2 * b] = ok ? M : 0;
    meta[2 * b + 1] = s0;
}

__global__ __launch_bounds__(W64) void k_clearance(int32_t B, int32_t K, int32_t rows, const double* __restrict__ T,
                                                   const double* __restrict__ C, const int32_t* __restrict__ meta,
                                                   const double* __restrict__ ub, const double* __restrict__ kn,
                                                   const double* __restrict__ bx, const double* __restrict__ obs,
                                                   const int32_t* __restrict__ ook, ClrScale sc, double r_min,
                                                   double r2, double* __restrict__ near, int32_t* __restrict__ obs_out,
                                                   int32_t* __restrict__ count, int32_t* __restrict__ tested,
                                                   int32_t* __restrict__ flags) {
    // the narrow tile
    __shared__ int32_t pre[SLOTS + 1];  // first item of a slot; [SLOTS]: the tile's items
    __shared__ int32_t smask[SLOTS];    // admissible states of a slot
    __shared__ double2 res[W64];        // a round's (d^2, t)
    __shared__ double2 prec[TILE];      // a pair's record
    __shared__ int32_t pfl[TILE];
    // the sweep
    __shared__ double cob[W64][OBS_STRIDE];   // the chunk's obstacles
    __shared__ double rub[ROWS][BOX_STRIDE];  // the rows' hulls
    __shared__ int32_t rM[ROWS];
    __shared__ int32_t cok[W64];
    __shared__ int32_t qr[QCAP], qk[QCAP];  // the queue: row of the tile, obstacle
    __shared__ neighbors::Row row[ROWS];

    const int lane = threadIdx.x;
    const double scale[3] = {sc.s[0], sc.s[1], sc.s[2]};
    const int32_t i0 = blockIdx.x * rows;
    const int nr = std::min<int32_t>(rows, B - i0);
    if (lane < nr) {
        row[lane] = neighbors::row_init();
        rM[lane] = meta[2 * (i0 + lane)];
        for (int q = 0; q < BOX_STRIDE; ++q) rub[lane][q] = ub[(int64_t)(i0 + lane) * BOX_STRIDE + q];
    }
    const int chunks = (K + W64 - 1) / W64;
    const int steps = chunks * nr;
    int qn = 0;             // wave-uniform
    bool bad_seen = false;  // this lane staged an unusable obstacle
    for (int step = 0; step <= steps; ++step) {
        __syncthreads();
        if (step < steps) {
            const int chunk = step / nr, r = step - chunk * nr;
            const int32_t k = chunk * W64 + lane, i = i0 + r;
            if (r == 0) {
                int32_t ok = 0;
                if (k < K) {
                    ok = ook[k];
                    bad_seen = bad_seen || ok == 0;
                    for (int q = 0; q < OBS_STRIDE; ++q) cob[lane][q] = obs[(int64_t)k * OBS_STRIDE + q];
                }
                cok[lane] = ok;
            }
            const int Mi = rM[r];
            bool live = Mi > 0 && cok[lane] != 0;  // own-lane data: no barrier needed after the staging
            if (live) live = neighbors::gap2(rub[r], cob[lane], scale) < r2;
            if (live) {
                const double* b = bx + (int64_t)i * (BOXES * BOX_STRIDE);
                bool any = false;
                for (int m = 1; m <= Mi; ++m) any = any || neighbors::gap2(b + m * BOX_STRIDE, cob[lane], scale) < r2;
                live = any;
            }
            const unsigned long long m = __ballot(live);
            if (live) {
                const int at = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                qr[at] = r;  // at < qn + 64 <= QCAP
                qk[at] = k;
            }
            qn += __popcll(m);
        }
        const int limit = step < steps ? TILE : 1;  // the last pass drains what is left
        while (qn >= limit) {
            const int np = std::min(qn, TILE);
            const int q0 = qn - np;
            qn = q0;
            __syncthreads();  // the queue is written; the previous tile's readers are done
            // the slots: lane l takes 4 * l .. 4 * l + 3, so that its own sum starts the scan
            int c4[4], sum = 0;
            TGMS_UNROLL
            for (int q = 0; q < SLOTS / W64; ++q) {
                const int e = (SLOTS / W64) * lane + q;
                const int p = e / TGMS_MAX_SEGMENTS, m = e - p * TGMS_MAX_SEGMENTS;
                int mask = 0, c = 0;
                if (p < np) {
                    const int r = qr[q0 + p];
                    if (m < rM[r]) {
                        const double* box = bx + (int64_t)(i0 + r) * (BOXES * BOX_STRIDE) + (m + 1) * BOX_STRIDE;
                        const double* ob = obs + (int64_t)qk[q0 + p] * OBS_STRIDE;
                        if (neighbors::gap2(box, ob, scale) < r2) {
                            mask = clearance::admissible(box, ob);
                            c = clearance::combo_count(mask);
                        }
                    }
                }
                smask[e] = mask;
                c4[q] = c;
                sum += c;
            }
            int incl = sum;  // inclusive scan over the wavefront
            for (int d = 1; d < W64; d <<= 1) {
                const int v = __shfl_up(incl, d);
                incl += lane >= d ? v : 0;
            }
            int first = incl - sum;
            TGMS_UNROLL
            for (int q = 0; q < SLOTS / W64; ++q) {
                pre[(SLOTS / W64) * lane + q] = first;
                first += c4[q];
            }
            if (lane == W64 - 1) pre[SLOTS] = incl;  // <= SLOTS * 26
            __syncthreads();
            const int total = __builtin_amdgcn_readfirstlane(pre[SLOTS]);
            // lane p < np folds pair p; every queued pair has a surviving segment, so an item
            double best = __builtin_inf(), at = 0.0;
            bool bad = false;
            for (int c0 = 0; c0 < total; c0 += W64) {
                const int it = c0 + lane;
                if (it < total) {
                    int lo = 0, hi = SLOTS;  // the last slot with pre[slot] <= it; empty slots repeat their successor's
                    for (int d = 0; d < 8; ++d) {  // 2^8 = SLOTS
                        const int mid = (lo + hi) >> 1;
                        const bool le = pre[mid] <= it;
                        lo = le ? mid : lo;
                        hi = le ? hi : mid;
                    }
                    const int p = lo / TGMS_MAX_SEGMENTS, m = lo - p * TGMS_MAX_SEGMENTS;
                    const int32_t i = i0 + qr[q0 + p];
                    const int32_t s0 = meta[2 * i + 1];
                    const double Tm = T[s0 + m];
                    const double* kni = kn + (int64_t)i * KNOT_STRIDE;
                    const int combo = clearance::nth_combo(smask[lo], it - pre[lo]);
                    double d2, u;
                    clearance::combo_item(C + ((int64_t)s0 + m) * 24, Tm, obs + (int64_t)qk[q0 + p] * OBS_STRIDE, scale,
                                          combo, d2, u);
                    res[lane] = make_double2(d2, clearance::time_of(kni[m], Tm, u, kni[rM[qr[q0 + p]]]));
                }
                __syncthreads();
                if (const int pl = fresh_lane(); pl < np) {
                    const int a = std::max(c0, pre[pl * TGMS_MAX_SEGMENTS]);
                    const int b = std::min(std::min(c0 + W64, total), pre[(pl + 1) * TGMS_MAX_SEGMENTS]);
                    for (int q = a; q < b; ++q) {
                        const double2 x = res[q - c0];
                        separation::fold(x.x, x.y, best, at, bad);
                    }
                }
                __syncthreads();
            }
            if (const int pl = fresh_lane(); pl < np) {
                double rec[TGMS_SEP_STRIDE];
                pfl[pl] = separation::finish(best, at, bad, r_min, rec);
                prec[pl] = make_double2(rec[0], rec[1]);
            }
            __syncthreads();
            if (const int rl = fresh_lane(); rl < nr) {
                neighbors::Row x = row[rl];
                for (int p = 0; p < np; ++p) {
                    if (qr[q0 + p] != rl) continue;
                    const double2 v = prec[p];
                    const double rec[TGMS_SEP_STRIDE] = {v.x, v.y};
                    neighbors::row_update(x, qk[q0 + p], rec, pfl[p]);
                }
                row[rl] = x;
            }
        }
    }
    const bool bad_obstacle = __ballot(bad_seen) != 0ull;
    __syncthreads();
    if (const int rl = fresh_lane(); rl < nr) {
        const int32_t i = i0 + rl;
        const neighbors::Row x = row[rl];
        const bool usable = rM[rl] > 0;
        double rec[TGMS_SEP_STRIDE];
        int32_t ob, ct;
        const int32_t fl = neighbors::row_finish(x, usable, rec, ob, ct);
        if (near) *reinterpret_cast<double2*>(near + (int64_t)i * TGMS_SEP_STRIDE) = make_double2(rec[0], rec[1]);
        if (obs_out) obs_out[i] = ob;
        if (count) count[i] = ct;
        if (tested) tested[i] = (fl & TGMS_SEP_NONFINITE) ? 0 : x.tested;
        if (flags) flags[i] = clearance::row_flags(fl, bad_obstacle);
    }
}

}  // namespace

size_t clearance_scratch_bytes(int32_t B, int32_t K) {
    return (size_t)B * (2 * sizeof(int32_t) + (BOX_STRIDE + KNOT_STRIDE + BOXES * BOX_STRIDE) * sizeof(double)) +
           (size_t)K * sizeof(int32_t);
}

hipError_t launch_clearance(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, int32_t K,
                            const double* obstacles, const double (&scale)[3], double r_min, void* scratch,
                            double* near, int32_t* obs, int32_t* count, int32_t* tested, int32_t* flags,
                            hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // the fp64 arrays first (the scratch is 256-byte aligned), the int32 words behind them
    double* ub = static_cast<double*>(scratch);
    double* kn = ub + (size_t)B * BOX_STRIDE;
    double* bx = kn + (size_t)B * KNOT_STRIDE;
    int32_t* meta = reinterpret_cast<int32_t*>(bx + (size_t)B * BOXES * BOX_STRIDE);
    int32_t* ook = meta + (size_t)B * 2;
    const int32_t n = std::max(B, K);
    TGMS_LAUNCH(k_clearance_boxes, dim3((unsigned)((n + PREP_BLOCK - 1) / PREP_BLOCK)), dim3(PREP_BLOCK), 0, stream, B, K,
                seg_offsets, T, C, obstacles, meta, ub, kn, bx, ook);
    // rows of a workgroup: one while that leaves the GPU short of wavefronts (256 CUs x 8), up
    // to ROWS for a large batch, where a row tile shares one staging of the obstacles
    const int32_t rows = std::max(1, std::min(ROWS, B / 2048));
    const ClrScale sc{{scale[0], scale[1], scale[2]}};
    TGMS_LAUNCH(k_clearance, dim3((unsigned)((B + rows - 1) / rows)), dim3(W64), 0, stream, B, K, rows, T, C, meta, ub,
                kn, bx, obstacles, ook, sc, r_min, neighbors::cull_r2(r_min), near, obs, count, tested, flags);
    return hipSuccess;
}

}  // namespace tgms
