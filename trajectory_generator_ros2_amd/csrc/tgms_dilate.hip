// tgms_dilate.hip — time dilation (tgms_dilate_batch_device) on gfx950: per trajectory the least
// uniform stretch s in [s_lo, s_hi] that meets the speed, acceleration, jerk, thrust and tilt
// limits, and the times and coefficients scaled by it.  The algorithm, its order of
// evaluations and its error argument are written in tgms_dilate_core.h.
//
// Mapping: k_thrust's tile (tgms_bounds.hip has the reasoning).  A wavefront per workgroup takes
// TILE = 4 consecutive trajectories, at most 64 segments, by grid-stride; coefficients and times
// are staged in LDS with the finiteness / T > 0 check in the same pass, and a trajectory whose
// segment count is outside 1..TGMS_MAX_SEGMENTS stages nothing.
//   - Phase 1, a lane per segment: the squared peaks of |p'|, |p''|, |p'''| (bounds::norm_item,
//     one kind of code per pass; the speed and jerk passes are skipped when their limit is
//     unchecked, which is wave-uniform).  Lane t < TILE folds trajectory t and opens its search
//     (dilate::init), which lives in LDS: st[t].
//   - Phase 2, the search.  Per round every lane evaluates thrust_item, then tilt_item (the
//     two ladders in separate passes, as in k_thrust; the tilt pass is skipped when tilt_max is
//     unchecked), of its segment at its own trajectory's g' = g / st[t].x; lane t < TILE folds
//     and takes the step (dilate::step).  Only the scalar x per trajectory changes between
//     rounds.  A trajectory that is done is neither evaluated nor stepped again, so its result
//     does not depend on its tile-mates; the wave leaves the loop when all four are done, and
//     the round count is bounded by dilate::MAX_EVALS + 3 whatever the data.
//   - Phase 3: the tile's coefficients leave as c_k r^k in coalesced 16-B stores (a lane per
//     pair of coefficients), the times as s T; lane t < TILE stores scale, active and flags.  The
//     inputs were read into LDS before anything is written, and a tile writes only its own
//     rows, so the outputs may be the inputs.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_dilate_core.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment in a pass
constexpr int RES = 6;                          // per segment: thrust::Item (phase 1 uses 3)
static_assert(SEGS == W64, "a pass is one pass of the wavefront");

// T, C and T_out, C_out may be the same arrays: no __restrict__ on them.
__global__ __launch_bounds__(W64) void k_dilate(int32_t B, const int32_t* __restrict__ seg_offsets, const double* T,
                                                const double* C, double g, dilate::Lim lim, double s_lo, double s_hi,
                                                double* __restrict__ scale, int32_t* __restrict__ active,
                                                int32_t* __restrict__ flags, double* T_out, double* C_out) {
    __shared__ double cf[SEGS * 24];
    __shared__ double tau[SEGS];
    __shared__ double res[SEGS * RES];
    __shared__ dilate::Search st[TILE];
    __shared__ int bad[TILE];
    const int lane = threadIdx.x;
    const bool chk_v = lim.v_max < __builtin_inf(), chk_j = lim.j_max < __builtin_inf();
    const bool chk_tilt = lim.tilt < __builtin_inf();
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
            // the offsets are the caller's (no host plan here): a span outside 1..16 reads and writes nothing
            Mt[t] = (M < 1 || M > TGMS_MAX_SEGMENTS) ? 0 : M;
            base[t + 1] = base[t] + Mt[t];
        }
        const int S = base[TILE];  // <= SEGS
        int tr = 0;                // the tile row of this lane's segment
#pragma unroll
        for (int t = 1; t < TILE; ++t) tr += lane >= base[t] ? 1 : 0;
        tr = tr < TILE ? tr : TILE - 1;
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
        // ---- phase 1: the peaks, one kind of code per pass ----
        if (lane < S) res[lane * RES + 0] = chk_v ? bounds::norm_item<1>(cf + lane * 24, tau[lane]) : 0.0;
        if (lane < S) res[lane * RES + 1] = bounds::norm_item<2>(cf + lane * 24, tau[lane]);
        if (lane < S) res[lane * RES + 2] = chk_j ? bounds::norm_item<3>(cf + lane * 24, tau[lane]) : 0.0;
        __syncthreads();
        if (lane < TILE) {
            int M = Mt[0], sb = base[0];
#pragma unroll
            for (int t = 1; t < TILE; ++t) {
                M = lane == t ? Mt[t] : M;
                sb = lane == t ? base[t] : sb;
            }
            double n2[3] = {0.0, 0.0, 0.0};
            for (int i = 0; i < M; ++i) {
                const double* r = res + (sb + i) * RES;
#pragma unroll
                for (int a = 0; a < 3; ++a) n2[a] = fmax(n2[a], r[a] == r[a] ? r[a] : __builtin_inf());
            }
            dilate::Search q;
            dilate::init(q, M == 0 || bad[lane] != 0, dilate::Kin{sqrt(n2[0]), sqrt(n2[1]), sqrt(n2[2])}, g, lim, s_lo,
                         s_hi);
            if (lane >= nb) q.stage = dilate::ST_DONE;
            st[lane] = q;
        }
        __syncthreads();
        // ---- phase 2: the search; the depth is bounded whatever the data ----
        for (int round = 0; round < dilate::MAX_EVALS + 3; ++round) {
            int live = 0;
#pragma unroll
            for (int t = 0; t < TILE; ++t) live |= st[t].stage != dilate::ST_DONE ? 1 : 0;
            if (__builtin_amdgcn_readfirstlane(live) == 0) break;
            const bool on = lane < S && st[tr].stage != dilate::ST_DONE;
            const double gp = on ? g / st[tr].x : g;
            thrust::Item it;
            if (on) thrust::thrust_item(cf + lane * 24, tau[lane], gp, it);
            if (on && chk_tilt) thrust::tilt_item(cf + lane * 24, tau[lane], gp, it);
            if (on) {
                double* r = res + lane * RES;
                r[0] = it.f2min;
                r[1] = it.umin;
                r[2] = it.f2max;
                r[3] = it.umax;
                r[4] = it.tilt;
                r[5] = it.utilt;
            }
            __syncthreads();
            if (lane < TILE && st[lane].stage != dilate::ST_DONE) {
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
                dilate::Search q = st[lane];
                dilate::step(q, f, lim, s_lo, s_hi);
                st[lane] = q;
            }
            __syncthreads();
        }
        // ---- phase 3: the scaled rows, then the three per-trajectory results ----
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            const double s = st[t].s;
            const bool keep = !(s == s);  // unusable: the rows are copied unchanged
            const double r = keep ? 1.0 : 1.0 / s;
            if (C_out) {
                double2* o = reinterpret_cast<double2*>(C_out + s0[t] * 24);
                for (int e = lane; e < Mt[t] * 12; e += W64) {
                    const int k = (2 * e) & 7;
                    const double c0 = cf[base[t] * 24 + 2 * e], c1 = cf[base[t] * 24 + 2 * e + 1];
                    o[e] = make_double2(keep ? c0 : dilate::scaled(c0, k, r), keep ? c1 : dilate::scaled(c1, k + 1, r));
                }
            }
            if (T_out && lane < Mt[t]) {
                const double x = tau[base[t] + lane];
                T_out[s0[t] + lane] = keep ? x : s * x;
            }
        }
        if (lane < nb) {
            const int64_t b = b0 + lane;
            if (scale) scale[b] = st[lane].s;
            if (active) active[b] = st[lane].active;
            if (flags) flags[b] = st[lane].flags;
        }
    }
}

}  // namespace

hipError_t launch_dilate(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, double g,
                         const dilate::Lim& lim, double s_lo, double s_hi, double* scale, int32_t* active,
                         int32_t* flags, double* T_out, double* C_out, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // k_bounds' grid: one workgroup per tile of TILE trajectories up to 4,096, the rest by grid-stride
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const int32_t blocks = (int32_t)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_dilate, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, T, C, g, lim, s_lo, s_hi, scale,
                active, flags, T_out, C_out);
    return hipSuccess;
}

}  // namespace tgms
