// tgms_extrema.hip — batched feasibility check (tgms_extrema_batch_device) on gfx950.
//
// Per trajectory the sampler's samples (tgms_sample.hip: t_k = k*dt, its segment scan, its
// four Horner chains, the pinned last sample) are reduced on the fly to one record of
// TGMS_EXTREMA_STRIDE doubles, pmin[3] pmax[3] v_peak a_peak j_peak duration, and a word of
// TGMS_FEAS_* bits against the caller's limits.  Nothing per sample reaches memory: the
// kernel reads 192 B per segment and writes 84 B per trajectory, so it is bound by the
// 66 FP64 FMAs of a sample (DESIGN.md §4 k_extrema).
//   - one wavefront per trajectory, one wavefront per workgroup (grid-stride, no workgroup
//     of several waves to keep in step): the trajectory's derivative forms c_j, j c_j,
//     j(j-1) c_j, j(j-1)(j-2) c_j sit packed in LDS (26 doubles per segment and axis,
//     9.75 KiB at M = 16);
//   - the wavefront walks the segments one after the other (the sampler's scan, turned into
//     the first sample index of every segment), so the coefficient address is the same in
//     every lane and does not change inside a segment: the compiler reads a segment's 78
//     forms from LDS once and keeps them in registers (212 VGPRs, two waves per SIMD), and
//     the loop over the segment's samples, U = 4, 2 or 1 per lane and step, is FMAs alone.
//     (Lanes that each followed their own segment, as the sampler's do, would re-read 78
//     doubles per sample: more LDS cycles than the sample's FMAs cost the SIMD.);
//   - a lane past the segment's last sample re-evaluates that last sample, which changes
//     no minimum or maximum, so the inner loop has no masks;
//   - every lane keeps 3 minima, 3 maxima and 3 squared-norm maxima; lane 0 folds in the
//     pinned final sample; one butterfly at the end; lane 0 stores the record (five 16-B
//     stores) and the flags, both from the same registers.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

constexpr int FORMS = 26;                 // 8 + 7 + 6 + 5 non-zero derivative-form entries
// entry (q, j) of a (segment, axis) block sits at foff(q) + j - q: 0, 8, 15, 21
constexpr int foff(int q) { return q * 8 - q * (q - 1) / 2; }

struct Acc {
    double lo[3], hi[3], n2[3];  // position extents; max of |v|^2, |a|^2, |j|^2
};

__device__ __forceinline__ int64_t uniform64(int64_t v) {  // a wave-uniform value into SGPRs
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffff));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((int64_t)hi << 32) | (unsigned int)lo;
}

// The sampler's sample time and local time: t = k*dt rounded, then t - t_cur (its kernel
// compares t against the knots, so the product is a value of its own there).  Contracting the
// two into one FMA here would move a sample by an ulp of time.
__device__ __forceinline__ double sample_time(double k, double dt) {
#pragma clang fp contract(off)
    return k * dt;
}
__device__ __forceinline__ double local_time(double k, double dt, double t_cur) {
#pragma clang fp contract(off)
    const double t = k * dt;
    return t - t_cur;
}

// U samples per lane of one segment: sample indices kd + 64 u (as doubles, exact below
// 2^53), clamped to the segment's last one.  f: the segment's forms, the same address in
// every lane.
template <int U>
__device__ __forceinline__ void eval(const double* f, double kd, double klast, double dt, double t_cur, Acc& A) {
    double lt[U], n2[3][U];
#pragma unroll
    for (int u = 0; u < U; ++u) lt[u] = local_time(fmin(kd + (double)(W64 * u), klast), dt, t_cur);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        __builtin_amdgcn_sched_barrier(0);  // one axis' forms in flight at a time (registers)
        const double* fa = f + a * FORMS;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double s[U];
            const double c7 = fa[foff(q) + 7 - q];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = c7;
#pragma unroll
            for (int j = 6; j >= q; --j) {
                const double c = fa[foff(q) + j - q];
#pragma unroll
                for (int u = 0; u < U; ++u) s[u] = __builtin_fma(s[u], lt[u], c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (q == 0) {
                    A.lo[a] = fmin(A.lo[a], s[u]);
                    A.hi[a] = fmax(A.hi[a], s[u]);
                } else {
                    n2[q - 1][u] = a == 0 ? s[u] * s[u] : __builtin_fma(s[u], s[u], n2[q - 1][u]);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int u = 0; u < U; ++u) A.n2[q] = fmax(A.n2[q], n2[q][u]);
}

// lane 0 stores one trajectory's record and flags (both nullable)
__device__ __forceinline__ void store_record(const double (&r)[TGMS_EXTREMA_STRIDE], int32_t fl, int64_t b,
                                             double* __restrict__ ext, int32_t* __restrict__ flags) {
    if (ext) {
        double2* o = reinterpret_cast<double2*>(ext + b * TGMS_EXTREMA_STRIDE);
#pragma unroll
        for (int q = 0; q < TGMS_EXTREMA_STRIDE / 2; ++q) o[q] = make_double2(r[2 * q], r[2 * q + 1]);
    }
    if (flags) flags[b] = fl;
}

__global__ __launch_bounds__(W64) void k_extrema(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                 const double* __restrict__ W, const double* __restrict__ T,
                                                 const double* __restrict__ ED, const double* __restrict__ C,
                                                 double dt, tgms_limits lim, double* __restrict__ ext,
                                                 int32_t* __restrict__ flags) {
    __shared__ double cf[TGMS_MAX_SEGMENTS * 3 * FORMS];
    __shared__ double tau[TGMS_MAX_SEGMENTS + 1];
    __shared__ int64_t kb[TGMS_MAX_SEGMENTS + 1];  // segment i holds the samples [kb[i], kb[i+1])
    const int lane = threadIdx.x;
    double nanrec[TGMS_EXTREMA_STRIDE];  // the record of a trajectory with TGMS_FEAS_NONFINITE
#pragma unroll
    for (int q = 0; q < TGMS_EXTREMA_STRIDE; ++q) nanrec[q] = __builtin_nan("");
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const int64_t s0 = seg_offsets[b];
        const int M = __builtin_amdgcn_readfirstlane(seg_offsets[b + 1] - (int32_t)s0);
        // the offsets are the caller's (no host plan here): a span outside 1..16 reads nothing
        if (M < 1 || M > TGMS_MAX_SEGMENTS) {  // wave-uniform
            if (lane == 0) store_record(nanrec, TGMS_FEAS_NONFINITE, b, ext, flags);
            continue;
        }
        __syncthreads();  // the previous trajectory's readers are done with cf / tau / kb
        double chk = 0.0;  // stays 0 while every staged value is finite, NaN afterwards
        for (int e = lane; e < M * 24; e += W64) {  // e = (segment*3 + axis)*8 + j
            const int j = e & 7;
            const double c = C[s0 * 24 + e];
            chk = __builtin_fma(c, 0.0, chk);
            double* f = cf + (e >> 3) * FORMS;
            f[j] = c;
            if (j >= 1) f[foff(1) + j - 1] = (double)j * c;
            if (j >= 2) f[foff(2) + j - 2] = (double)(j * (j - 1)) * c;
            if (j >= 3) f[foff(3) + j - 3] = (double)(j * (j - 1) * (j - 2)) * c;
        }
        if (lane < M) tau[lane + 1] = T[s0 + lane];
        __syncthreads();
        if (lane == 0) {  // prefix sums in the sampler's order
            double acc = 0.0;
            tau[0] = 0.0;
            for (int i = 1; i <= M; ++i) {
                acc += tau[i];
                tau[i] = acc;
            }
        }
        __syncthreads();
        // tgms_sample_count(total, dt); beyond 2^53 samples k*dt cannot index them
        const double total = tau[M];
        const double x = ceil(total / dt - 1e-9);
        const bool countable = total >= 0.0 && x < 9007199254740992.0;  // false for NaN and inf
        const int64_t ns = uniform64(countable ? std::max<int64_t>(1, (int64_t)x) + 1 : 2);
        // first sample of segment m: the smallest k with tau[m] <= k*dt, where the sampler's
        // scan (t_next <= t advances) enters it; k*dt is monotonic in k
        if (lane <= M) {
            int64_t k = lane == 0 ? 0 : ns - 1;
            if (lane > 0 && lane < M && countable) {
                const double tm = tau[lane], top = (double)(ns - 1);
                double g = fmin(fmax(ceil(tm / dt), 0.0), top);
                while (g > 0.0 && sample_time(g - 1.0, dt) >= tm) g -= 1.0;
                while (g < top && sample_time(g, dt) < tm) g += 1.0;
                k = (int64_t)g;
            }
            kb[lane] = k;
        }
        __syncthreads();
        if (lane == 0)  // times that are not positive cannot take the bounds out of order
            for (int i = 1; i < M; ++i) kb[i] = std::max(kb[i], kb[i - 1]);
        __syncthreads();
        chk = __builtin_fma(total, 0.0, chk);
        if (__any(chk != 0.0) || !countable) {  // wave-uniform
            if (lane == 0) store_record(nanrec, TGMS_FEAS_NONFINITE, b, ext, flags);
            continue;
        }

        Acc A;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            A.lo[a] = __builtin_inf();
            A.hi[a] = -__builtin_inf();
            A.n2[a] = 0.0;
        }
        for (int i = 0; i < M; ++i) {
            const int64_t k0 = uniform64(kb[i]);
            int64_t rem = uniform64(kb[i + 1]) - k0;
            if (rem <= 0) continue;
            const double t_cur = tau[i];
            const double* f = cf + i * 3 * FORMS;
            const double klast = (double)(k0 + rem - 1);
            double kd = (double)k0 + (double)lane;
            for (; rem > 2 * W64; rem -= 4 * W64, kd += 4.0 * W64) eval<4>(f, kd, klast, dt, t_cur, A);
            if (rem > W64)
                eval<2>(f, kd, klast, dt, t_cur, A);
            else if (rem > 0)
                eval<1>(f, kd, klast, dt, t_cur, A);
        }
        double pchk = 0.0;
        if (lane == 0) {  // the pinned final sample, by exactly one lane
            const double* wl = W + (s0 + b + M) * 3;
            const double* edf = ED ? ED + b * 18 + 9 : nullptr;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double p = wl[a];
                pchk = __builtin_fma(p, 0.0, pchk);
                A.lo[a] = fmin(A.lo[a], p);
                A.hi[a] = fmax(A.hi[a], p);
            }
            if (edf) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double dx = edf[q * 3], dy = edf[q * 3 + 1], dz = edf[q * 3 + 2];
                    const double n = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
                    pchk = __builtin_fma(n, 0.0, pchk);
                    A.n2[q] = fmax(A.n2[q], n);
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                A.lo[a] = fmin(A.lo[a], __shfl_xor(A.lo[a], off));
                A.hi[a] = fmax(A.hi[a], __shfl_xor(A.hi[a], off));
                A.n2[a] = fmax(A.n2[a], __shfl_xor(A.n2[a], off));
            }
        }
        if (lane == 0) {
            double r[TGMS_EXTREMA_STRIDE];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                r[a] = A.lo[a];
                r[3 + a] = A.hi[a];
                r[6 + a] = sqrt(A.n2[a]);
            }
            r[9] = total;
            double fin = pchk;
#pragma unroll
            for (int q = 0; q < TGMS_EXTREMA_STRIDE; ++q) fin = __builtin_fma(r[q], 0.0, fin);
            if (fin != 0.0) {  // a result (or the pinned sample) is not finite
                store_record(nanrec, TGMS_FEAS_NONFINITE, b, ext, flags);
            } else {  // the flags from the very values that are stored; strict comparisons
                int32_t fl = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    fl |= (r[a] < lim.pmin[a] || r[3 + a] > lim.pmax[a]) ? TGMS_FEAS_BOX : 0;
                fl |= r[6] > lim.v_max ? TGMS_FEAS_SPEED : 0;
                fl |= r[7] > lim.a_max ? TGMS_FEAS_ACCEL : 0;
                fl |= r[8] > lim.j_max ? TGMS_FEAS_JERK : 0;
                store_record(r, fl, b, ext, flags);
            }
        }
    }
}

}  // namespace

hipError_t launch_extrema(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                          const double* ED, const double* C, double dt, const tgms_limits& lim, double* ext,
                          int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    // one workgroup per trajectory up to 15,360, larger batches by grid-stride: 7.5 rounds
    // of the 2,048 wavefronts resident at once (256 CUs x 4 SIMDs x 2, the register limit),
    // enough for the hardware to level trajectories of different length
    const int32_t blocks = std::min<int32_t>(B, 15360);
    TGMS_LAUNCH(k_extrema, dim3((unsigned)blocks), dim3(W64), 0, stream, B, seg_offsets, W, T, ED, C, dt, lim,
                ext, flags);
    return hipSuccess;
}

}  // namespace tgms
