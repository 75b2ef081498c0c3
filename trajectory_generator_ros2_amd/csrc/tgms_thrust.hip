// tgms_thrust.hip — continuous thrust and tilt bounds (tgms_thrust_batch_device) on gfx950.
//
// Per trajectory one record of TGMS_THRUST_STRIDE doubles, f_min t_fmin f_max t_fmax tilt_max
// t_tilt, and a word of TGMS_THRUST_* bits, from the mass-normalised thrust vector f = p'' + g
// e_z of the piecewise polynomial itself: per segment the extremes of ||f||^2 and of the angle
// between f and +z over the closed interval, by the derivative ladders of tgms_thrust_core.h
// (the polynomials, the candidates and the error argument are written there).  No dt.
//
// Mapping: k_bounds' (tgms_bounds.hip has the reasoning).  A wavefront per workgroup takes a
// tile of TILE = 4 consecutive trajectories, at most 64 segments, by grid-stride:
//   - the tile's coefficients and times are staged in LDS with coalesced loads, the
//     finiteness / T > 0 check in the same pass; a trajectory whose segment count is outside
//     1..TGMS_MAX_SEGMENTS stages nothing;
//   - two phases with one lane per segment, so that every lane runs one kind of code: the
//     thrust phase (a degree-9 ladder, 11 candidates), then the tilt phase (a degree-13
//     ladder, 13 more candidates).  A lane keeps its segment's six results in registers
//     between the phases and leaves them in LDS after the second;
//   - the root lists are registers (compile-time indices only); no loop has a data-dependent
//     depth: an interval is bisected BISECTIONS times or not at all;
//   - lane t < TILE then folds trajectory t's segments left to right (the knots are the
//     prefix sums of T, the last one the duration) and stores the record as three 16-B stores
//     and the flags from the same registers.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_thrust_core.h"

namespace tgms {
namespace {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment in a phase
constexpr int RES = 6;                          // per segment: thrust::Item
static_assert(SEGS == W64, "a phase is one pass of the wavefront");

__global__ __launch_bounds__(W64) void k_thrust(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                const double* __restrict__ T, const double* __restrict__ C,
                                                double g, tgms_thrust_limits lim, double* __restrict__ out,
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
        thrust::Item it;
        if (lane < S) thrust::thrust_item(cf + lane * 24, tau[lane], g, it);
        if (lane < S) {
            thrust::tilt_item(cf + lane * 24, tau[lane], g, it);
            double* r = res + lane * RES;
            r[0] = it.f2min;
            r[1] = it.umin;
            r[2] = it.f2max;
            r[3] = it.umax;
            r[4] = it.tilt;
            r[5] = it.utilt;
        }
        __syncthreads();
        if (lane < nb) {
            int M = Mt[0], sb = base[0];
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                M = lane == t ? Mt[t] : M;
                sb = lane == t ? base[t] : sb;
            }
            thrust::Fold f = thrust::fold_init();
            for (int i = 0; i < M; ++i) {
                const double* r = res + (sb + i) * RES;
                const thrust::Item x{r[0], r[1], r[2], r[3], r[4], r[5]};
                thrust::fold(f, x, tau[sb + i]);
            }
            double rec[TGMS_THRUST_STRIDE];
            const int32_t fl = thrust::finish(f, M == 0 || bad[lane] != 0, lim, rec);
            const int64_t b = b0 + lane;
            if (out) {
                double2* o = reinterpret_cast<double2*>(out + b * TGMS_THRUST_STRIDE);
#pragma unroll
                for (int q = 0; q < TGMS_THRUST_STRIDE / 2; ++q) o[q] = make_double2(rec[2 * q], rec[2 * q + 1]);
            }
            if (flags) flags[b] = fl;
        }
    }
}

}  // namespace

hipError_t launch_thrust(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, double g,
                         const tgms_thrust_limits& lim, double* rec, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // k_bounds' grid: one workgroup per tile of TILE trajectories up to 4,096, the rest by grid-stride
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_thrust, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, g, lim, rec, flags);
    return hipSuccess;
}

}  // namespace tgms
