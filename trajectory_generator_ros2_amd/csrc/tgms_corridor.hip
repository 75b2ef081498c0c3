// tgms_corridor.hip — corridor containment (tgms_corridor_batch_device) on gfx950.
//
// Per segment the largest n . p(t) - d over its faces and [0, T], per trajectory the largest of
// those, each with a time and the face that attains it: tgms_corridor_core.h has the item (a
// degree-6 derivative ladder on the coefficients projected onto n, values from the axis
// polynomials), the ordered folds and the flags.
//
// Mapping: k_bounds' tile, but the unit of lane work is the (segment, face) item, not the
// segment.  A wavefront per workgroup takes a tile of TILE = 4 consecutive trajectories, at most
// 64 segments, by grid-stride:
//   - the tile's coefficients and times are staged in LDS with coalesced loads, the
//     finiteness / T > 0 check in the same pass; a trajectory whose segment count is outside
//     1..TGMS_MAX_SEGMENTS stages nothing;
//   - the lane of a segment reads its face span, checks it, and the wavefront numbers the
//     tile's items through the segments' face counts: an exclusive prefix in LDS.  An unusable
//     trajectory contributes no item;
//   - lanes take the items 64 at a time.  An item finds its segment by a six-step search in
//     the prefix, reads its face straight from global memory as two 16-byte loads (consecutive
//     items read consecutive rows within a segment) and leaves margin and u in LDS; a segment
//     with 40 faces beside one with 4 idles nobody.  After each pass the lane of a segment
//     folds its own items of that pass in face order; a segment's faces may straddle passes,
//     and a tile may have no item at all;
//   - lane t < TILE then folds trajectory t's segments left to right (the knots are the prefix
//     sums of T, the last one the duration), stores the record, the place and the flags, and
//     leaves the knots for the lanes of the segments, which store the per-segment rows;
//   - the root list is registers (compile-time indices only); no loop has a data-dependent
//     depth other than the pass count and the folds: an interval is bisected BISECTIONS times
//     or not at all.
#include <algorithm>

#include "tgms_corridor_core.h"
#include "tgms_device.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment in the folds
static_assert(SEGS == W64, "the segments of a tile are one pass of the wavefront");

__global__ __launch_bounds__(W64) void k_corridor(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                  const double* __restrict__ T, const double* __restrict__ C,
                                                  int64_t F, const double* __restrict__ faces,
                                                  const int64_t* __restrict__ face_offsets, double r,
                                                  double* __restrict__ rec, int32_t* __restrict__ where,
                                                  double* __restrict__ seg_rec, int32_t* __restrict__ seg_face,
                                                  int32_t* __restrict__ flags) {
    __shared__ double cf[SEGS * 24];
    __shared__ double tau[SEGS];
    __shared__ double2 res[W64];       // a pass' items: margin, u
    __shared__ double2 sres[SEGS];     // a segment's best: margin, u
    __shared__ double kn[SEGS];        // a segment's knot
    __shared__ int64_t fbase[SEGS];    // a segment's first face
    __shared__ int32_t sface[SEGS];    // a segment's best face
    __shared__ int pre[SEGS + 1];      // items before a segment; pre[SEGS]: the tile's items
    __shared__ double dur[TILE];
    __shared__ int bad[TILE], bad_face[TILE];
    const int lane = threadIdx.x;
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TILE;
        const int nb = (int)std::min<int64_t>(TILE, B - b0);
        // wave-uniform: the tile's trajectories, their segment counts and LDS bases
        int Mt[TILE], base[TILE + 1];
        int64_t s0[TILE];
        base[0] = 0;
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            int M = 0;
            s0[t] = 0;
            if (t < nb) {
                s0[t] = seg_offsets[b0 + t];
                M = __builtin_amdgcn_readfirstlane(seg_offsets[b0 + t + 1] - (int32_t)s0[t]);
            }
            // the offsets are the caller's (no host plan here): a span outside 1..16 reads nothing
            Mt[t] = (M < 1 || M > TGMS_MAX_SEGMENTS) ? 0 : M;
            base[t + 1] = base[t] + Mt[t];
        }
        const int S = base[TILE];  // <= SEGS
        // this lane's segment: its trajectory in the tile and its row in the batch
        int tr = 0;
#pragma unroll
        for (int t = 1; t < TILE; ++t) tr += lane >= base[t] ? 1 : 0;
        int64_t gs = s0[0] + lane;
#pragma unroll
        for (int t = 1; t < TILE; ++t) gs = tr == t ? s0[t] + (lane - base[t]) : gs;
        __syncthreads();  // the previous tile's readers are done with the LDS
        if (lane < TILE) bad[lane] = bad_face[lane] = 0;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            double chk = 0.0;  // stays 0 while every staged value is finite, NaN afterwards
            bool neg = false;
            for (int e = lane; e < Mt[t] * 24; e += W64) {
                const double c = C[s0[t] * 24 + e];
                chk = __builtin_fma(c, 0.0, chk);
                cf[base[t] * 24 + e] = c;
            }
            if (lane < Mt[t]) {
                const double x = T[s0[t] + lane];
                chk = __builtin_fma(x, 0.0, chk);
                neg = !(x > 0.0);
                tau[base[t] + lane] = x;
            }
            if (chk != 0.0 || neg) bad[t] = 1;  // every writer stores the same value
        }
        // the face span of this lane's segment
        int cnt = 0;
        int64_t fb = 0;
        if (lane < S) {
            int64_t fe = F;
            if (face_offsets) {
                fb = face_offsets[gs];
                fe = face_offsets[gs + 1];
            }
            if (corridor::span_ok(fb, fe, F))
                cnt = (int)(fe - fb);
            else
                bad[tr] = 1;
            fbase[lane] = fb;
        }
        __syncthreads();
        if (lane < S && bad[tr] != 0) cnt = 0;  // an unusable trajectory has no item
        // the exclusive prefix of the counts over the wavefront
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < W64; o <<= 1) {
            const int up = __shfl_up(inc, o, W64);
            inc += lane >= o ? up : 0;
        }
        pre[lane] = inc - cnt;
        if (lane == W64 - 1) pre[SEGS] = inc;
        __syncthreads();
        const int mine = inc - cnt;                                    // this segment's first item
        const int total = __builtin_amdgcn_readfirstlane(pre[SEGS]);  // <= SEGS * TGMS_COR_MAX_FACES
        corridor::SegBest best = corridor::seg_init();
        for (int c0 = 0; c0 < total; c0 += W64) {
            const int q = c0 + lane;
            if (q < total) {
                // the last segment whose first item is <= q: it has pre[seg + 1] > q, so it is not empty
                int seg = 0;
#pragma unroll
                for (int step = SEGS / 2; step >= 1; step >>= 1) seg += pre[seg + step] <= q ? step : 0;
                const int64_t fi = fbase[seg] + (q - pre[seg]);
                const double2* row = reinterpret_cast<const double2*>(faces + fi * 4);
                const double2 nxy = row[0], nzd = row[1];
                double2 out = make_double2(-__builtin_inf(), 0.0);  // a face left out: never taken
                if (corridor::face_ok(nxy.x, nxy.y, nzd.x, nzd.y)) {
                    corridor::item(cf + seg * 24, tau[seg], nxy.x, nxy.y, nzd.x, nzd.y, out.x, out.y);
                } else {
                    int t2 = 0;
#pragma unroll
                    for (int t = 1; t < TILE; ++t) t2 += seg >= base[t] ? 1 : 0;
                    bad_face[t2] = 1;
                }
                res[lane] = out;
            }
            __syncthreads();
            if (lane < S) {
                const int a = std::max(c0, mine), b = std::min(std::min(c0 + W64, total), mine + cnt);
                for (int i = a; i < b; ++i) {
                    const double2 x = res[i - c0];
                    if (x.x != -__builtin_inf()) corridor::seg_take(best, x.x, x.y, (int32_t)(fb + (i - mine)));
                }
            }
            __syncthreads();  // before the next pass overwrites res
        }
        if (lane < S) {
            sres[lane] = make_double2(best.m, best.u);
            sface[lane] = best.face;
            if (best.bad) bad[tr] = 1;
        }
        __syncthreads();
        if (lane < nb) {
            int M = Mt[0], sb = base[0];
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                M = lane == t ? Mt[t] : M;
                sb = lane == t ? base[t] : sb;
            }
            corridor::Fold f = corridor::fold_init();
            for (int i = 0; i < M; ++i) {
                const double2 x = sres[sb + i];
                kn[sb + i] = f.next;
                corridor::fold(f, corridor::SegBest{x.x, x.y, sface[sb + i], false}, i, tau[sb + i]);
            }
            double out[TGMS_COR_STRIDE];
            int32_t wh[2];
            const int32_t fl = corridor::finish(f, M == 0 || bad[lane] != 0, bad_face[lane] != 0, r, out, wh);
            dur[lane] = f.next;
            bad[lane] = (fl & TGMS_FEAS_NONFINITE) != 0;
            const int64_t b = b0 + lane;
            if (rec) *reinterpret_cast<double2*>(rec + b * TGMS_COR_STRIDE) = make_double2(out[0], out[1]);
            if (where) {
                where[b * 2] = wh[0];
                where[b * 2 + 1] = wh[1];
            }
            if (flags) flags[b] = fl;
        }
        __syncthreads();
        if (lane < S && (seg_rec || seg_face)) {
            double m, t;
            int32_t face;
            corridor::seg_row(best, kn[lane], tau[lane], dur[tr], bad[tr] != 0, m, t, face);
            if (seg_rec) *reinterpret_cast<double2*>(seg_rec + gs * TGMS_COR_STRIDE) = make_double2(m, t);
            if (seg_face) seg_face[gs] = face;
        }
    }
}

}  // namespace

hipError_t launch_corridor(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, int64_t F,
                           const double* faces, const int64_t* face_offsets, double r, double* rec, int32_t* where,
                           double* seg_rec, int32_t* seg_face, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // k_bounds' grid: one workgroup per tile of TILE trajectories up to 4,096, the rest by grid-stride
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_corridor, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, F, faces,
                face_offsets, r, rec, where, seg_rec, seg_face, flags);
    return hipSuccess;
}

}  // namespace tgms
