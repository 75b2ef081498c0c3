// tgms_neighbors.hip — swarm neighbour search (tgms_neighbors_batch_device) on gfx950.
//
// Per vehicle i the closest other vehicle whose closest approach is below r_min, how many
// come that close, and how many pairs reached the exact computation.  include/tgms.h has the
// semantics; tgms_neighbors_core.h the boxes, their margins and the cull test;
// tgms_separation_core.h the exact closest approach, which is called here, not copied.
//
// Two launches on handle scratch that is laid out per vehicle (sized by B alone: the segment
// total of a device batch is not known on the host), so no index into it depends on the
// caller's offsets:
//   meta [B][2]   int32: the segment count M (0: the vehicle is unusable), the first segment
//   ub   [B][6]   the hull of the vehicle's boxes, apart from the rest: this is what a sweep reads
//   kn   [B][18]  global knots 0..M, the last time in slot 17
//   bx   [B][18][6] boxes: held start, segments, held end
//
// k_neighbor_boxes: a lane per vehicle runs neighbors::vehicle_boxes.  This is the only place
// that looks at every coefficient, so it is where non-finite input is found.
//
// k_neighbors: a wavefront per workgroup owns `rows` consecutive vehicles i (1..ROWS, chosen
// by the launch so that a small swarm still fills the GPU; the result of a row does not
// depend on it).  Its lanes sweep j in chunks of 64, a lane per j:
//   - the chunk's hulls are staged in LDS once and tested against each row's hull (a
//     wave-uniform LDS read), then the survivors walk the pair's merged knots over the
//     per-segment boxes (neighbors::walk, reading both vehicles' knots and boxes from L2);
//   - what is left is compacted by ballot / mbcnt into an LDS queue of (row, j);
//   - whenever the queue holds TILE = 16 pairs, and once more after the last chunk, 16 pairs
//     leave the queue's tail and run as k_separation's tile does: 32 lanes look the sides up
//     (from the scratch, where the knots already are), 16 lanes merge, all lanes take the
//     (pair, interval) items through separation::interval_item, 16 lanes fold and finish;
//   - lane r < rows then folds the tile's records of its row into the row's running result in
//     LDS (neighbors::row_update: smallest stored d_min, ties to the lowest j; order-free).
// One store per output per row at the end, no atomics, and no loop whose depth depends on a
// coefficient: the walk is M_i + M_j + 1 steps, an interval is bisected 40 times or not at all.
// The narrow tile appears once in the code (the sweep and the final drain share one loop), so
// the item keeps k_separation's register budget.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_neighbors_core.h"

namespace tgms {
namespace {

using neighbors::BOX_STRIDE;
using neighbors::BOXES;
using neighbors::KNOT_STRIDE;
using neighbors::TLAST;
using separation::MAX_INTERVALS;
using separation::MAX_KNOTS;
using separation::MAX_MERGED;

constexpr int TILE = 16;                     // pairs of one narrow tile
constexpr int SIDES = 2 * TILE;              // one lane each in the look-up
constexpr int ITEMS = TILE * MAX_INTERVALS;  // 528
constexpr int ROWS = 16;                     // most rows of one workgroup
constexpr int QCAP = TILE - 1 + W64;         // what a sweep step can leave in the queue
constexpr int BOX_BLOCK = 64;
static_assert(SIDES <= W64 && ROWS <= W64, "one pass of the wavefront");

struct NbrScale {
    double s[3];
};

// The lane index as a value the compiler cannot tie to an earlier copy: what a rarely run
// section derives from it (LDS and output addresses) is then formed there, not held in
// registers across the item loop, whose budget is k_separation's 256 VGPRs.
__device__ __forceinline__ int fresh_lane() {
    int l = threadIdx.x;
    asm volatile("" : "+v"(l));
    return l;
}

__global__ __launch_bounds__(BOX_BLOCK) void k_neighbor_boxes(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                              const double* __restrict__ T,
                                                              const double* __restrict__ C,
                                                              const double* __restrict__ t0, int32_t* __restrict__ meta,
                                                              double* __restrict__ ub, double* __restrict__ kn,
                                                              double* __restrict__ bx) {
    const int32_t b = blockIdx.x * BOX_BLOCK + threadIdx.x;
    if (b >= B) return;
    const int32_t s0 = seg_offsets[b];
    const int32_t M = seg_offsets[b + 1] - s0;
    bool ok = M >= 1 && M <= TGMS_MAX_SEGMENTS;  // the offsets are the caller's: another span reads nothing
    double start = 0.0;
    if (ok && t0) start = t0[b];
    ok = ok && neighbors::vehicle_boxes(M, C + (int64_t)s0 * 24, T + s0, start, kn + (int64_t)b * KNOT_STRIDE,
                                        bx + (int64_t)b * (BOXES * BOX_STRIDE), ub + (int64_t)b * BOX_STRIDE);
    meta[2 * b] = ok ? M : 0;
    meta[2 * b + 1] = s0;
}

__global__ __launch_bounds__(W64) void k_neighbors(int32_t B, int32_t rows, const double* __restrict__ C,
                                                   const int32_t* __restrict__ meta, const double* __restrict__ ub,
                                                   const double* __restrict__ kn, const double* __restrict__ bx,
                                                   NbrScale sc, double r_min, double r2, double* __restrict__ near,
                                                   int32_t* __restrict__ nbr, int32_t* __restrict__ count,
                                                   int32_t* __restrict__ tested, int32_t* __restrict__ flags) {
    // the narrow tile, as k_separation's
    __shared__ double tkn[SIDES][MAX_KNOTS];
    __shared__ double tl[SIDES];
    __shared__ double mk[TILE][MAX_MERGED];
    __shared__ double2 res[ITEMS];
    __shared__ int32_t sg[TILE][MAX_INTERVALS];
    __shared__ int32_t sM[SIDES];
    __shared__ int32_t sS0[SIDES];
    __shared__ int32_t sV[SIDES];  // the side's vehicle
    __shared__ int32_t cnt[TILE];
    __shared__ int32_t cfirst[TILE];  // first item of a pair
    __shared__ int32_t ctotal;
    __shared__ int32_t imap[ITEMS];
    __shared__ double2 prec[TILE];  // a pair's record
    __shared__ int32_t pfl[TILE];
    // the sweep
    __shared__ double cub[W64][BOX_STRIDE];   // the chunk's hulls
    __shared__ double rub[ROWS][BOX_STRIDE];  // the rows' hulls
    __shared__ int32_t rM[ROWS];
    __shared__ int32_t cM[W64];
    __shared__ int32_t qr[QCAP], qj[QCAP];  // the queue: row of the tile, j
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
    const int chunks = (B + W64 - 1) / W64;
    const int steps = chunks * nr;
    int qn = 0;  // wave-uniform
    for (int step = 0; step <= steps; ++step) {
        __syncthreads();
        if (step < steps) {
            const int chunk = step / nr, r = step - chunk * nr;
            const int32_t j = chunk * W64 + lane, i = i0 + r;
            if (r == 0) {
                int32_t M = 0;
                if (j < B) {
                    M = meta[2 * j];
                    for (int q = 0; q < BOX_STRIDE; ++q) cub[lane][q] = ub[(int64_t)j * BOX_STRIDE + q];
                }
                cM[lane] = M;
            }
            const int Mi = rM[r], Mj = cM[lane];  // own-lane data: no barrier needed after the staging
            bool live = Mi > 0 && Mj > 0 && j != i;
            if (live) live = neighbors::gap2(rub[r], cub[lane], scale) < r2;
            if (live)
                live = neighbors::walk(kn + (int64_t)i * KNOT_STRIDE, Mi, bx + (int64_t)i * (BOXES * BOX_STRIDE),
                                       kn + (int64_t)j * KNOT_STRIDE, Mj, bx + (int64_t)j * (BOXES * BOX_STRIDE), scale,
                                       r2);
            const unsigned long long m = __ballot(live);
            if (live) {
                const int at = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                qr[at] = r;  // at < qn + 64 <= QCAP
                qj[at] = j;
            }
            qn += __popcll(m);
        }
        const int limit = step < steps ? TILE : 1;  // the last pass drains what is left
        while (qn >= limit) {
            const int np = std::min(qn, TILE);
            const int q0 = qn - np;
            qn = q0;
            __syncthreads();  // the queue is written; the previous tile's readers are done
            if (lane < SIDES) {
                const int p = lane >> 1, side = lane & 1;
                int M = 0, s0 = 0, v = 0;
                if (p < np) {
                    v = side ? qj[q0 + p] : i0 + qr[q0 + p];
                    M = meta[2 * v];
                    s0 = meta[2 * v + 1];
                }
                sM[lane] = M;
                sS0[lane] = s0;
                sV[lane] = v;
                tl[lane] = M ? kn[(int64_t)v * KNOT_STRIDE + TLAST] : 0.0;
            }
            __syncthreads();
            for (int e = lane; e < SIDES * MAX_KNOTS; e += W64) {
                const int l = e / MAX_KNOTS, m = e - l * MAX_KNOTS;
                if (sM[l] && m <= sM[l]) tkn[l][m] = kn[(int64_t)sV[l] * KNOT_STRIDE + m];
            }
            __syncthreads();
            if (lane < TILE) {
                const int Mi = sM[2 * lane], Mj = sM[2 * lane + 1];
                const int n = (lane < np && Mi > 0 && Mj > 0) ? Mi + Mj + 1 : 0;
                if (n) separation::merge_knots(tkn[2 * lane], Mi, tkn[2 * lane + 1], Mj, mk[lane], sg[lane]);
                cnt[lane] = n;
            }
            __syncthreads();
            if (lane < TILE) {  // the item list: pair | interval << 8, pair after pair
                int first = 0;
                for (int t = 0; t < lane; ++t) first += cnt[t];
                const int n = cnt[lane];
                for (int q = 0; q < n; ++q) imap[first + q] = lane | (q << 8);
                cfirst[lane] = first;
                if (lane == TILE - 1) ctotal = first + n;  // <= ITEMS
            }
            __syncthreads();
            const int total = __builtin_amdgcn_readfirstlane(ctotal);
            for (int it = lane; it < total; it += W64) {
                const int pq = imap[it];
                const int p = pq & 255, q = pq >> 8;
                const double a = mk[p][q], b = mk[p][q + 1], h = b - a;
                const int32_t pk = sg[p][q];
                const int li = 2 * p, lj = 2 * p + 1;
                const separation::Side si = separation::side_of((pk & 255) - 1, sM[li], tkn[li], tl[li], a, h);
                const separation::Side sj = separation::side_of((pk >> 8) - 1, sM[lj], tkn[lj], tl[lj], a, h);
                const double* ci = C + ((int64_t)sS0[li] + si.seg) * 24;
                const double* cj = C + ((int64_t)sS0[lj] + sj.seg) * 24;
                double d2, u;
                separation::interval_item(ci, si, cj, sj, scale, h, d2, u);
                res[it] = make_double2(d2, fmin(__builtin_fma(h, u, a), b));
            }
            __syncthreads();
            if (lane < np) {
                const int first = cfirst[lane];
                const int n = cnt[lane];
                double best = __builtin_inf(), at = 0.0;
                bool bad = n == 0;
                for (int q = 0; q < n; ++q) {
                    const double2 x = res[first + q];
                    separation::fold(x.x, x.y, best, at, bad);
                }
                double rec[TGMS_SEP_STRIDE];
                pfl[lane] = separation::finish(best, at, bad, r_min, rec);
                prec[lane] = make_double2(rec[0], rec[1]);
            }
            __syncthreads();
            if (const int rl = fresh_lane(); rl < nr) {
                neighbors::Row x = row[rl];
                for (int p = 0; p < np; ++p) {
                    if (qr[q0 + p] != rl) continue;
                    const double2 v = prec[p];
                    const double rec[TGMS_SEP_STRIDE] = {v.x, v.y};
                    neighbors::row_update(x, qj[q0 + p], rec, pfl[p]);
                }
                row[rl] = x;
            }
        }
    }
    __syncthreads();
    if (const int rl = fresh_lane(); rl < nr) {
        const int32_t i = i0 + rl;
        const neighbors::Row x = row[rl];
        const bool usable = rM[rl] > 0;
        double rec[TGMS_SEP_STRIDE];
        int32_t nb, ct;
        const int32_t fl = neighbors::row_finish(x, usable, rec, nb, ct);
        if (near) *reinterpret_cast<double2*>(near + (int64_t)i * TGMS_SEP_STRIDE) = make_double2(rec[0], rec[1]);
        if (nbr) nbr[i] = nb;
        if (count) count[i] = ct;
        if (tested) tested[i] = (fl & TGMS_SEP_NONFINITE) ? 0 : x.tested;
        if (flags) flags[i] = fl;
    }
}

}  // namespace

size_t neighbors_scratch_bytes(int32_t B) {
    return (size_t)B * (2 * sizeof(int32_t) + (BOX_STRIDE + KNOT_STRIDE + BOXES * BOX_STRIDE) * sizeof(double));
}

hipError_t launch_neighbors(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                            const double* start_times, const double (&scale)[3], double r_min, void* scratch,
                            double* near, int32_t* nbr, int32_t* count, int32_t* tested, int32_t* flags,
                            hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // the fp64 arrays first (the scratch is 256-byte aligned), the int32 words behind them
    double* ub = static_cast<double*>(scratch);
    double* kn = ub + (size_t)B * BOX_STRIDE;
    double* bx = kn + (size_t)B * KNOT_STRIDE;
    int32_t* meta = reinterpret_cast<int32_t*>(bx + (size_t)B * BOXES * BOX_STRIDE);
    TGMS_LAUNCH(k_neighbor_boxes, dim3((unsigned)((B + BOX_BLOCK - 1) / BOX_BLOCK)), dim3(BOX_BLOCK), 0, stream, B,
                seg_offsets, T, C, start_times, meta, ub, kn, bx);
    // rows of a workgroup: one while that leaves the GPU short of wavefronts (256 CUs x 8), up
    // to ROWS for a large swarm, where a row tile shares one sweep of the hulls
    const int32_t rows = std::max(1, std::min(ROWS, B / 2048));
    const NbrScale sc{{scale[0], scale[1], scale[2]}};
    TGMS_LAUNCH(k_neighbors, dim3((unsigned)((B + rows - 1) / rows)), dim3(W64), 0, stream, B, rows, C, meta, ub, kn, bx,
                sc, r_min, neighbors::cull_r2(r_min), near, nbr, count, tested, flags);
    return hipSuccess;
}

}  // namespace tgms
