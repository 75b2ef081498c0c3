// tgms_bounds.hip — continuous feasibility bounds (tgms_bounds_batch_device) on gfx950.
//
// Per trajectory one record of TGMS_EXTREMA_STRIDE doubles, pmin[3] pmax[3] v_peak a_peak
// j_peak duration, and a word of TGMS_FEAS_* bits, from the piecewise polynomial itself: per
// segment the extrema of p_x, p_y, p_z and of |p'|^2, |p''|^2, |p'''|^2 over the closed
// interval, by the derivative ladder of tgms_bounds_core.h (the algorithm, its bisection
// budget and its error argument are written there).  No dt: the work is O(M) per trajectory.
//
// Mapping.  The unit of work is (segment, quantity), and the four kinds of quantity run
// different, fully unrolled code (derivative degrees 6, 11, 9, 7; worst case 40 * sum d^2 =
// 3,640 / 20,240 / 11,400 / 5,600 Horner FMAs).  A wavefront whose lanes held different
// kinds would run all four one after the other with a fraction of its lanes each, which is
// what one trajectory per wavefront amounts to (M = 10: 60 lanes, 10 of them in the degree-11
// code).  So a wavefront takes a tile of TILE = 4 consecutive trajectories, at most 64
// segments, and runs the kinds as phases over the tile's segments: |p'|^2, |p''|^2, |p'''|^2
// with one lane per segment, then the 3 S position items in up to three passes.  Every phase
// is one kind of code in every lane.  4 is the largest tile whose segments always fit one
// pass of a phase and one 12 KiB coefficient stage, whatever the M (ragged batches need no
// plan, so the call can be captured into a graph); at M = 10 the norm phases run 40 of 64
// lanes, against 10 of 64 for a wavefront per trajectory.
//   - one wavefront per workgroup, grid-stride over the tiles;
//   - the tile's coefficients and times are staged in LDS with coalesced loads, the
//     finiteness / T > 0 check in the same pass; a trajectory whose segment count is outside
//     1..TGMS_MAX_SEGMENTS stages nothing;
//   - the root lists are registers (compile-time indices only, tgms_bounds_core.h); the
//     control flow has no data-dependent depth: an interval is bisected BISECTIONS times or
//     not at all, so non-finite input cannot keep a lane busy;
//   - every item leaves its result in LDS (9 doubles per segment); lane t < TILE then folds
//     trajectory t's segments left to right (the duration is the sampled check's prefix sum)
//     and stores the record (five 16-B stores) and the flags from the same registers.
#include <algorithm>

#include "tgms_bounds_core.h"
#include "tgms_device.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment in a norm phase
constexpr int RES = 9;                          // per segment: lo[3] hi[3] n2[3]
static_assert(SEGS == W64, "a norm phase is one pass of the wavefront");

__global__ __launch_bounds__(W64) void k_bounds(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                const double* __restrict__ T, const double* __restrict__ C,
                                                tgms_limits lim, double* __restrict__ ext,
                                                int32_t* __restrict__ flags) {
    __shared__ double cf[SEGS * 24];
    __shared__ double tau[SEGS];
    __shared__ double res[SEGS * RES];
    __shared__ int bad[TILE];
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
        __syncthreads();           // the previous tile's readers are done with the LDS
        if (lane < TILE) bad[lane] = 0;
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
        __syncthreads();
        if (lane < S) {
            const double* c = cf + lane * 24;
            const double Ti = tau[lane];
            res[lane * RES + 6] = bounds::norm_item<1>(c, Ti);
        }
        if (lane < S) {
            const double* c = cf + lane * 24;
            const double Ti = tau[lane];
            res[lane * RES + 7] = bounds::norm_item<2>(c, Ti);
        }
        if (lane < S) {
            const double* c = cf + lane * 24;
            const double Ti = tau[lane];
            res[lane * RES + 8] = bounds::norm_item<3>(c, Ti);
        }
        for (int it = lane; it < 3 * S; it += W64) {  // it = segment * 3 + axis
            const int seg = it / 3, a = it - seg * 3;
            double lo, hi;
            bounds::position_item(cf + it * 8, tau[seg], lo, hi);
            res[seg * RES + a] = lo;
            res[seg * RES + 3 + a] = hi;
        }
        __syncthreads();
        if (lane < nb) {
            int M = Mt[0], sb = base[0];
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                M = lane == t ? Mt[t] : M;
                sb = lane == t ? base[t] : sb;
            }
            double lo[3], hi[3], n2[3], dur = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = __builtin_inf();
                hi[a] = -__builtin_inf();
                n2[a] = 0.0;
            }
            for (int i = 0; i < M; ++i) {
                const double* r = res + (sb + i) * RES;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    lo[a] = fmin(lo[a], r[a]);
                    hi[a] = fmax(hi[a], r[3 + a]);
                    n2[a] = fmax(n2[a], r[6 + a]);
                }
                dur += tau[sb + i];
            }
            double rec[TGMS_EXTREMA_STRIDE];
            const int32_t fl = bounds::finish(lo, hi, n2, dur, M == 0 || bad[lane] != 0, lim, rec);
            const int64_t b = b0 + lane;
            if (ext) {
                double2* o = reinterpret_cast<double2*>(ext + b * TGMS_EXTREMA_STRIDE);
#pragma unroll
                for (int q = 0; q < TGMS_EXTREMA_STRIDE / 2; ++q) o[q] = make_double2(rec[2 * q], rec[2 * q + 1]);
            }
            if (flags) flags[b] = fl;
        }
    }
}

}  // namespace

hipError_t launch_bounds(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                         const tgms_limits& lim, double* ext, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // one workgroup per tile of TILE trajectories up to 4,096 workgroups (16 per CU, twice
    // the 2,048 wavefronts the register budget keeps resident), larger batches by grid-stride
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_bounds, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, lim, ext, flags);
    return hipSuccess;
}

}  // namespace tgms
