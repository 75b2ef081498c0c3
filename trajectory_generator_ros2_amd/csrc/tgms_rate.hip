// tgms_rate.hip — continuous roll/pitch body-rate bound (tgms_rate_batch_device) on gfx950.
//
// Per trajectory one record of TGMS_RATE_STRIDE doubles, omega_max t_omega, a word of flags, and
// per segment a row of the same layout with the segment's own maximum and local time, from
// omega = ||f x p'''|| / ||f||^2 of the piecewise polynomial itself: per segment the maximum over
// the closed interval by the degree-25 derivative ladder of tgms_rate_core.h (the polynomial,
// the candidates and the error argument are written there).  No dt.
//
// Mapping: k_thrust's (tgms_bounds.hip has the reasoning).  A wavefront per workgroup takes a
// tile of TILE = 4 consecutive trajectories, at most 64 segments, by grid-stride:
//   - the tile's coefficients and times are staged in LDS with coalesced loads, the
//     finiteness / T > 0 check in the same pass; a trajectory whose segment count is outside
//     1..TGMS_MAX_SEGMENTS stages nothing;
//   - one phase with one lane per segment: the 26 coefficients of G, the 25-level ladder, 27
//     candidates.  The coefficients and the root list are registers (compile-time indices
//     only), about 80 doubles live at the deepest level: the kernel is built for one wave per
//     SIMD (512 registers a lane), which a 64-thread workgroup allows.  No loop has a
//     data-dependent depth: an interval is bisected BISECTIONS times or not at all;
//   - lane t < TILE then folds trajectory t's segments left to right (the knots are the
//     prefix sums of T, the last one the duration) and stores the record as one 16-B store and
//     the flags from the same registers; the lanes of the segments store the per-segment rows.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_rate_core.h"

namespace tgms {
namespace {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment
static_assert(SEGS == W64, "the segments of a tile are one pass of the wavefront");

__global__ __launch_bounds__(W64) void k_rate(int32_t B, const int32_t* __restrict__ seg_offsets,
                                              const double* __restrict__ T, const double* __restrict__ C, double g,
                                              double omega_limit, double* __restrict__ out,
                                              double* __restrict__ seg_out, int32_t* __restrict__ flags) {
    __shared__ double cf[SEGS * 24];
    __shared__ double tau[SEGS];
    __shared__ double2 res[SEGS];  // a segment's omega^2 and u
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
        // this lane's segment: its trajectory in the tile and its row in the batch
        int tr = 0;
#pragma unroll
        for (int t = 1; t < TILE; ++t) tr += lane >= base[t] ? 1 : 0;
        int64_t gs = s0[0] + lane;
#pragma unroll
        for (int t = 1; t < TILE; ++t) gs = tr == t ? s0[t] + (lane - base[t]) : gs;
        __syncthreads();  // the previous tile's readers are done with the LDS
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
        rate::Item it{0.0, 0.0};
        if (lane < S) {
            rate::rate_item(cf + lane * 24, tau[lane], g, it);
            res[lane] = make_double2(it.w2, it.u);
        }
        __syncthreads();
        if (lane < nb) {
            int M = Mt[0], sb = base[0];
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                M = lane == t ? Mt[t] : M;
                sb = lane == t ? base[t] : sb;
            }
            rate::Fold f = rate::fold_init();
            for (int i = 0; i < M; ++i) {
                const double2 x = res[sb + i];
                rate::fold(f, rate::Item{x.x, x.y}, tau[sb + i]);
            }
            double rec[TGMS_RATE_STRIDE];
            const int32_t fl = rate::finish(f, M == 0 || bad[lane] != 0, omega_limit, rec);
            bad[lane] = (fl & TGMS_FEAS_NONFINITE) != 0;
            const int64_t b = b0 + lane;
            if (out) *reinterpret_cast<double2*>(out + b * TGMS_RATE_STRIDE) = make_double2(rec[0], rec[1]);
            if (flags) flags[b] = fl;
        }
        __syncthreads();
        if (lane < S && seg_out) {
            double w, t;
            rate::seg_row(it, tau[lane], bad[tr] != 0, w, t);
            *reinterpret_cast<double2*>(seg_out + gs * TGMS_RATE_STRIDE) = make_double2(w, t);
        }
    }
}

}  // namespace

hipError_t launch_rate(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, double g,
                       double omega_limit, double* rec, double* seg_rec, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // k_bounds' grid: one workgroup per tile of TILE trajectories up to 4,096, the rest by grid-stride
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_rate, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, g, omega_limit, rec, seg_rec,
                flags);
    return hipSuccess;
}

}  // namespace tgms
