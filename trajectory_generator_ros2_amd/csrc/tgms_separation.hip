// tgms_separation.hip — continuous swarm separation (tgms_separation_batch_device) on gfx950.
//
// Per pair (i, j) of trajectories one record d_min t_min and a word of TGMS_SEP_* bits: the
// closest approach over the union of the two global intervals, each vehicle holding its end
// point outside its own.  The algorithm, its bisection budget and its error argument are in
// tgms_separation_core.h; include/tgms.h has the semantics.
//
// Mapping.  The unit of work is (pair, interval of the pair's merged knot list): every item
// runs the same fully unrolled degree-13 ladder (worst case 40 * sum_{d<=13} d^2 = 32,760
// Horner FMAs), so there are no phases as in k_bounds.  A wavefront takes a tile of TILE = 16
// consecutive pairs, at most 16 * 33 = 528 items, and its lanes take the tile's items in
// passes of 64 (M = 10 on both sides: 21 intervals a pair, 336 items, 6 passes at 87.5 %).
//   - one wavefront per workgroup, grid-stride over the tiles;
//   - lane l < 32 looks up side l & 1 of pair l >> 1: the index (read, or decoded from the
//     all-pairs order), its segment span and start time; an index outside 0..B-1 or a span
//     outside 1..TGMS_MAX_SEGMENTS reads nothing further;
//   - the sides' times are staged in LDS by all lanes and turned into global knots in place
//     (finite, T > 0 checked in the same pass); one lane per pair merges the two knot lists;
//   - an item fetches its two segments' coefficients from global memory (in an all-pairs call
//     a trajectory is reused B - 1 times and sits in L2) and checks them for finiteness;
//   - the root list and all coefficients are registers (compile-time indices only); the
//     control flow has no data-dependent depth: an interval is bisected BISECTIONS times or
//     not at all, so non-finite input cannot keep a lane busy;
//   - every item leaves (min d^2, its global time) in LDS; lane p < TILE folds pair p's
//     intervals left to right and stores the record (one 16-B store) and the flags from the
//     same registers.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_separation_core.h"

namespace tgms {
namespace {

using separation::MAX_INTERVALS;
using separation::MAX_KNOTS;
using separation::MAX_MERGED;

constexpr int TILE = 16;                     // pairs of one wavefront
constexpr int SIDES = 2 * TILE;              // one lane each in the look-up
constexpr int ITEMS = TILE * MAX_INTERVALS;  // 528
constexpr int GRID_CAP = 4096;               // workgroups of one launch
static_assert(SIDES <= W64, "the look-up is one pass of the wavefront");

struct SepScale {
    double s[3];
};

__global__ __launch_bounds__(W64) void k_separation(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                    const double* __restrict__ T, const double* __restrict__ C,
                                                    const double* __restrict__ t0, int64_t P,
                                                    const int32_t* __restrict__ pairs, SepScale sc, double r_min,
                                                    double* __restrict__ sep, int32_t* __restrict__ flags) {
    __shared__ double kn[SIDES][MAX_KNOTS];  // a side's times [1..M], then its global knots [0..M]
    __shared__ double tl[SIDES];             // a side's last time
    __shared__ double mk[TILE][MAX_MERGED];
    __shared__ double2 res[ITEMS];
    __shared__ int32_t sg[TILE][MAX_INTERVALS];
    __shared__ int32_t sM[SIDES];   // segment count, 0: the side rules its pair out
    __shared__ int32_t sS0[SIDES];  // first segment
    __shared__ int32_t cnt[TILE];   // intervals of a pair
    const int lane = threadIdx.x;
    const double scale[3] = {sc.s[0], sc.s[1], sc.s[2]};
    const int64_t tiles = (P + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * TILE;
        const int np = (int)std::min<int64_t>(TILE, P - n0);
        __syncthreads();  // the previous tile's readers are done with the LDS
        if (lane < SIDES) {
            const int p = lane >> 1, side = lane & 1;
            int M = 0, s0 = 0;
            double start = 0.0;
            if (p < np) {
                int32_t idx[2];
                if (pairs) {
                    idx[0] = pairs[(n0 + p) * 2];
                    idx[1] = pairs[(n0 + p) * 2 + 1];
                } else {
                    separation::decode_pair(n0 + p, B, P, idx[0], idx[1]);
                }
                const int32_t b = side ? idx[1] : idx[0];
                if (b >= 0 && b < B) {
                    s0 = seg_offsets[b];
                    M = seg_offsets[b + 1] - s0;
                    // the offsets are the caller's (no host plan here): a span outside 1..16 reads nothing
                    M = (M < 1 || M > TGMS_MAX_SEGMENTS) ? 0 : M;
                    if (M && t0) start = t0[b];
                    if (!finite(start)) M = 0;
                }
            }
            sM[lane] = M;
            sS0[lane] = s0;
            kn[lane][0] = start;
        }
        __syncthreads();
        for (int e = lane; e < SIDES * TGMS_MAX_SEGMENTS; e += W64) {
            const int l = e / TGMS_MAX_SEGMENTS, m = e - l * TGMS_MAX_SEGMENTS;
            if (m < sM[l]) kn[l][m + 1] = T[(int64_t)sS0[l] + m];
        }
        __syncthreads();
        if (lane < SIDES) {
            const int M = sM[lane];
            const double start = kn[lane][0];
            double acc = 0.0, chk = 0.0, last = 0.0;
            bool neg = false;
            for (int m = 0; m < M; ++m) {
                last = kn[lane][m + 1];
                neg = neg || !(last > 0.0);
                acc += last;  // the same order as the extrema record's duration
                kn[lane][m + 1] = start + acc;
                chk = __builtin_fma(start + acc, 0.0, chk);
            }
            tl[lane] = last;
            if (neg || chk != 0.0) sM[lane] = 0;
        }
        __syncthreads();
        if (lane < TILE) {
            const int Mi = sM[2 * lane], Mj = sM[2 * lane + 1];
            const int n = (lane < np && Mi > 0 && Mj > 0) ? Mi + Mj + 1 : 0;
            if (n) separation::merge_knots(kn[2 * lane], Mi, kn[2 * lane + 1], Mj, mk[lane], sg[lane]);
            cnt[lane] = n;
        }
        __syncthreads();
        int base[TILE + 1];  // wave-uniform: first item of every pair
        base[0] = 0;
#pragma unroll
        for (int t = 0; t < TILE; ++t) base[t + 1] = base[t] + __builtin_amdgcn_readfirstlane(cnt[t]);
        const int total = base[TILE];  // <= ITEMS
        for (int it = lane; it < total; it += W64) {
            int p = 0, first = 0;
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                p += it >= base[t] ? 1 : 0;
                first = it >= base[t] ? base[t] : first;
            }
            const int q = it - first;
            const double a = mk[p][q], b = mk[p][q + 1], h = b - a;
            const int32_t pk = sg[p][q];
            const int li = 2 * p, lj = 2 * p + 1;
            const separation::Side si = separation::side_of((pk & 255) - 1, sM[li], kn[li], tl[li], a, h);
            const separation::Side sj = separation::side_of((pk >> 8) - 1, sM[lj], kn[lj], tl[lj], a, h);
            const double* ci = C + ((int64_t)sS0[li] + si.seg) * 24;
            const double* cj = C + ((int64_t)sS0[lj] + sj.seg) * 24;
            double d2, u;
            separation::interval_item(ci, si, cj, sj, scale, h, d2, u);
            res[it] = make_double2(d2, fmin(__builtin_fma(h, u, a), b));
        }
        __syncthreads();
        if (lane < np) {
            int first = 0;
#pragma unroll
            for (int t = 1; t < TILE; ++t) first = lane == t ? base[t] : first;
            const int n = cnt[lane];
            double best = __builtin_inf(), at = 0.0;
            bool bad = n == 0;
            for (int q = 0; q < n; ++q) {
                const double2 r = res[first + q];
                separation::fold(r.x, r.y, best, at, bad);
            }
            double rec[TGMS_SEP_STRIDE];
            const int32_t fl = separation::finish(best, at, bad, r_min, rec);
            if (sep) *reinterpret_cast<double2*>(sep + (n0 + lane) * TGMS_SEP_STRIDE) = make_double2(rec[0], rec[1]);
            if (flags) flags[n0 + lane] = fl;
        }
    }
}

}  // namespace

hipError_t launch_separation(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                             const double* start_times, int64_t P, const int32_t* pairs, const double (&scale)[3],
                             double r_min, double* sep, int32_t* flags, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    // one workgroup per tile of TILE pairs up to GRID_CAP workgroups (16 per CU, as
    // launch_bounds), more pairs by grid-stride
    const int64_t tiles = (P + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, GRID_CAP);
    const SepScale sc{{scale[0], scale[1], scale[2]}};
    TGMS_LAUNCH(k_separation, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, start_times, P, pairs,
                sc, r_min, sep, flags);
    return hipSuccess;
}

}  // namespace tgms
