// tgms_retime.hip — segment re-timing (tgms_retime_batch_dev) on gfx950: per segment the peaks of
// |p'|, |p''|, |p'''| over its closed interval, the factor r_i they ask of its time and the time
// s_i T_i; per trajectory the largest r_i, the durations before and after, and the flags.  The
// rule and the fold are written in tgms_retime_core.h, the peaks' algorithm in tgms_bounds_core.h.
//
// Mapping: k_bounds' tile without its position items (tgms_bounds.hip has the reasoning).  A
// wavefront per workgroup takes TILE = 4 consecutive trajectories, at most 64 segments, by
// grid-stride; coefficients and times are staged in LDS with the finiteness / T > 0 check in the
// same pass, and a trajectory whose segment count is outside 1..TGMS_MAX_SEGMENTS stages nothing.
//   - Three phases, a lane per segment: bounds::norm_item<1>, <2>, <3>, one kind of code per
//     phase.  A phase whose limit is +inf is skipped when seg_rec is not asked for (its peak
//     contributes 0 to r_i either way); the limits are kernel arguments, so that is wave-uniform.
//   - Lane < S forms its row, s_i and s_i T_i (retime::segment) and leaves r_i, s_i and the
//     product in LDS; lane t < TILE folds trajectory t left to right (retime::fold, finish),
//     stores its record and flags and leaves in LDS whether the trajectory is unusable.
//   - Lane < S then stores its row (two 16-B stores) and its time: NaNs and the time unchanged
//     for an unusable trajectory.  The times were read into LDS before anything is written, and
//     a tile writes only its own rows, so T_out may be T.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_retime_core.h"
#include "tgms_seg_tile.h"

namespace tgms {
namespace {

using seg_tile::SEGS;
using seg_tile::TILE;
constexpr int RES = 6;  // per segment: n2[3], then r s T_out

// T and T_out may be the same array: no __restrict__ on them.
__global__ __launch_bounds__(W64) void k_retime(int32_t B, const int32_t* __restrict__ seg_offsets, const double* T,
                                                const double* __restrict__ C, retime::Lim lim, double s_lo, double s_hi,
                                                double* T_out, double* __restrict__ seg_rec, double* __restrict__ rec,
                                                int32_t* __restrict__ flags) {
    __shared__ double cf[SEGS * 24];
    __shared__ double tau[SEGS];
    __shared__ double res[SEGS * RES];
    __shared__ int bad[TILE];
    const int lane = threadIdx.x;
    const bool run_v = seg_rec || lim.v_max < __builtin_inf(), run_a = seg_rec || lim.a_max < __builtin_inf();
    const bool run_j = seg_rec || lim.j_max < __builtin_inf();
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TILE;
        const int nb = (int)std::min<int64_t>(TILE, B - b0);
        // the offsets are the caller's (no host plan here): a span outside 1..16 reads and writes nothing
        seg_tile::Tile x;
        seg_tile::load_tile(seg_offsets, b0, nb, x);
        const int S = x.base[TILE];  // <= SEGS
        int tr, sb, Ml;
        int64_t gs;
        seg_tile::lane_segment(x, lane, tr, sb, Ml, gs);
        __syncthreads();  // the previous tile's readers are done with the LDS
        if (lane < TILE) bad[lane] = 0;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            double chk = 0.0;  // stays 0 while every staged value is finite, NaN afterwards
            bool neg = false;
            for (int e = lane; e < x.Mt[t] * 24; e += W64) {
                const double c = C[x.s0[t] * 24 + e];
                chk = __builtin_fma(c, 0.0, chk);
                cf[x.base[t] * 24 + e] = c;
            }
            if (lane < x.Mt[t]) {
                const double v = T[x.s0[t] + lane];
                chk = __builtin_fma(v, 0.0, chk);
                neg = !(v > 0.0);
                tau[x.base[t] + lane] = v;
            }
            if (chk != 0.0 || neg) bad[t] = 1;  // every writer stores the same value
        }
        __syncthreads();
        if (lane < S) res[lane * RES + 0] = run_v ? bounds::norm_item<1>(cf + lane * 24, tau[lane]) : 0.0;
        if (lane < S) res[lane * RES + 1] = run_a ? bounds::norm_item<2>(cf + lane * 24, tau[lane]) : 0.0;
        if (lane < S) res[lane * RES + 2] = run_j ? bounds::norm_item<3>(cf + lane * 24, tau[lane]) : 0.0;
        retime::Seg g;
        if (lane < S) {
            double* r = res + lane * RES;
            const double n2[3] = {r[0], r[1], r[2]};
            g = retime::segment(n2, tau[lane], lim, s_lo, s_hi);
            r[3] = g.row[3];
            r[4] = g.s;
            r[5] = g.T_out;
        }
        __syncthreads();
        if (lane < nb) {
            int M = x.Mt[0], fb = x.base[0];
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                M = lane == t ? x.Mt[t] : M;
                fb = lane == t ? x.base[t] : fb;
            }
            retime::Fold f = retime::fold_init();
            for (int i = 0; i < M; ++i) {
                const double* r = res + (fb + i) * RES;
                retime::fold(f, i, r[3], r[4], tau[fb + i], r[5]);
            }
            double row[TGMS_RETIME_REC];
            const int32_t fl = retime::finish(f, M == 0 || bad[lane] != 0, s_hi, row);
            const int64_t b = b0 + lane;
            if (rec) {  // rows of 24 B: 8-B stores
#pragma unroll
                for (int q = 0; q < TGMS_RETIME_REC; ++q) rec[b * TGMS_RETIME_REC + q] = row[q];
            }
            if (flags) flags[b] = fl;
            bad[lane] = (fl & TGMS_FEAS_NONFINITE) ? 1 : 0;
        }
        __syncthreads();
        if (lane < S) {
            const bool nanrow = bad[tr] != 0;
            const double nan = __builtin_nan("");
            if (seg_rec) {
                double2* o = reinterpret_cast<double2*>(seg_rec + gs * TGMS_RETIME_STRIDE);
                o[0] = nanrow ? make_double2(nan, nan) : make_double2(g.row[0], g.row[1]);
                o[1] = nanrow ? make_double2(nan, nan) : make_double2(g.row[2], g.row[3]);
            }
            if (T_out) T_out[gs] = nanrow ? tau[lane] : g.T_out;
        }
    }
}

}  // namespace

hipError_t launch_retime(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                         const retime::Lim& lim, double s_lo, double s_hi, double* T_out, double* seg_rec, double* rec,
                         int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // k_bounds' grid: one workgroup per tile of TILE trajectories up to 4,096, the rest by grid-stride
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_retime, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, lim, s_lo, s_hi, T_out,
                seg_rec, rec, flags);
    return hipSuccess;
}

}  // namespace tgms
