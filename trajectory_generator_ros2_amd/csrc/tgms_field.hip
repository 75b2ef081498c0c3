// tgms_field.hip — distance-field clearance (tgms_field_clearance_batch_device) on gfx950.
//
// Per trajectory the least value of a voxel distance field along it, certified to a stated
// tolerance by the branch-and-bound of tgms_field_core.h.  include/tgms.h has the semantics.
//
// k_field: a lane per segment, a DPP row of 16 lanes per trajectory, four trajectories per
// wavefront, one wavefront per workgroup.  A lane keeps its segment's 24 coefficients, the
// two bounds V and A and its place in the interval tree (a level and an index) in registers;
// there is no stack, no LDS and no scratch.  The wavefront runs rounds: every lane that still
// has a node evaluates its centre (three Horner chains for the position, three for the speed,
// eight 4-byte gathers, a blend), then the row's least value so far is shared by four DPP
// rotations, and every lane tests its node against it: one segment's find prunes the others.
// The loop is wave-uniform (it ends when no lane of the wavefront has a node left), so the
// DPP moves always run with all 64 lanes enabled; a lane without work only skips the
// evaluation.  What the kernel waits for is the gathers, not the arithmetic: the map sits in
// L2 / Infinity Cache at best, and only other wavefronts hide that latency.
//   - The budget is kept per row: the lanes of a row count the row's active lanes from the
//     ballot before a round; a round that would pass max_evals is not run, the row stops and
//     carries TGMS_FLD_UNRESOLVED.  Rounds are the same whatever the launch, so is the result.
//   - The winner (least value, then lowest segment) stores the row's outputs itself.
//
// k_field_lip / k_field_lip_fold (lip == 0): a grid-stride pass over the nodes, each taking the
// edge to its +x, +y and +z neighbour, per-block maxima of the three directions into scratch,
// and a one-block fold of them into L.  A maximum does not depend on the order it is taken in.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_field_core.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

constexpr int ROW = 16;  // lanes of a trajectory: a DPP row
static_assert(ROW == TGMS_MAX_SEGMENTS, "a lane per segment");

// row_ror:n -- lane i of a row reads lane (i - n) mod 16 of the same row.
template <int N>
__device__ __forceinline__ double row_ror(double v) {
    return dpp_f64<0x120 + N>(v);
}
__device__ __forceinline__ double row_min(double v) {
    v = fmin(v, row_ror<8>(v));
    v = fmin(v, row_ror<4>(v));
    v = fmin(v, row_ror<2>(v));
    return fmin(v, row_ror<1>(v));
}
__device__ __forceinline__ double row_next(double v) { return row_ror<15>(v); }  // from lane i + 1

__global__ __launch_bounds__(W64) void k_field(int32_t B, const int32_t* __restrict__ seg_offsets,
                                               const double* __restrict__ T, const double* __restrict__ C,
                                               field::Grid world, const float* __restrict__ values, double lip,
                                               const double* __restrict__ d_lip, double r_min, double tol,
                                               int32_t max_evals, double* __restrict__ near, int32_t* __restrict__ evals_out,
                                               int32_t* __restrict__ flags) {
    const int lane = threadIdx.x, s = lane & (ROW - 1), shift = lane & ~(ROW - 1);
    const int32_t b = blockIdx.x * (W64 / ROW) + lane / ROW;
    const double L = d_lip ? *d_lip : lip;
    int32_t s0 = 0, M = 0;
    if (b < B) {
        s0 = seg_offsets[b];
        M = seg_offsets[b + 1] - s0;
    }
    const bool row_ok = M >= 1 && M <= TGMS_MAX_SEGMENTS;  // another span reads nothing
    const bool mine = row_ok && s < M;
    // the knots as every sibling forms them: a left-to-right prefix sum, the same in every lane
    double knot = 0.0, D = 0.0, Ts = 1.0, chk = 0.0;
    bool bad = false;
    if (row_ok) {
        for (int m = 0; m < M; ++m) {
            const double t = T[s0 + m];
            bad = bad || !(t > 0.0);
            chk = __builtin_fma(t, 0.0, chk);
            knot = m == s ? D : knot;
            Ts = m == s ? t : Ts;
            D += t;
        }
        chk = __builtin_fma(D, 0.0, chk);
    }
    double c[3][8];
    TGMS_UNROLL
    for (int ax = 0; ax < 3; ++ax) {
        TGMS_UNROLL
        for (int k = 0; k < 8; k += 2) {
            const double2 x = mine ? *reinterpret_cast<const double2*>(C + ((int64_t)s0 + s) * 24 + ax * 8 + k)
                                   : make_double2(0.0, 0.0);
            c[ax][k] = x.x;
            c[ax][k + 1] = x.y;
        }
    }
    if (mine) field::to_grid_frame(world, c);  // from here on positions are relative to node (0,0,0)
    const field::Grid g = field::grid_frame(world);
    double V, A;
    field::speed_bounds(c, Ts, V, A, chk);
    bad = bad || chk != 0.0;
    bad = ((__ballot(bad) >> shift) & 0xffffull) != 0ull;  // the row's: one bad segment spoils it
    const bool live = mine && !bad;

    // the knots: every lane its left end, the last one its right end too
    double best = HUGE_VAL, at = 0.0, fl = HUGE_VAL, fr = HUGE_VAL, pe[3] = {0.0, 0.0, 0.0};
    bool nonfinite = false;
    if (live) {
        const double p0[3] = {c[0][0], c[1][0], c[2][0]};
        fl = field::phi(g, values, p0);
        nonfinite = !(fl * 0.0 == 0.0);
        best = fl;
        field::position(c, Ts, pe);
        if (s == M - 1) {
            fr = field::phi(g, values, pe);
            nonfinite = nonfinite || !(fr * 0.0 == 0.0);
            at = fr < best ? Ts : at;
            best = fmin(best, fr);
        }
    }
    int32_t evals = row_ok && !bad ? M + 1 : 0;  // the same in every lane of the row
    {
        // the right end's value is the next lane's left end, less L times the jump at the knot
        const double nfl = row_next(fl), nx = row_next(c[0][0]), ny = row_next(c[1][0]), nz = row_next(c[2][0]);
        if (live && s < M - 1) {
            const double dx = nx - pe[0], dy = ny - pe[1], dz = nz - pe[2];
            fr = nfl - L * sqrt(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)));
        }
    }
    double rbest = row_min(best);
    int level = 0;
    uint64_t index = 0;
    bool active = live && !field::ends_rule_out(fl, fr, L, V, Ts, field::threshold(rbest, tol, r_min));
    bool unresolved = evals > max_evals;  // the knots alone are past the budget
    for (;;) {
        // a row with a value that is not finite stops: its result is NaN whatever follows
        const unsigned long long nf = __ballot(nonfinite);
        active = active && ((nf >> shift) & 0xffffull) == 0ull;
        const unsigned long long act = __ballot(active);
        if (act == 0ull) break;
        const int n_act = __popcll((act >> shift) & 0xffffull);
        if (n_act > max_evals - evals) {  // uniform in the row: all its active lanes run or none
            unresolved = unresolved || n_act > 0;
            active = false;
        } else {
            evals += n_act;
        }
        double f = HUGE_VAL, reach = 0.0;
        if (active) {
            double hwu, speed;
            const double u = field::centre(level, index, hwu);
            f = field::eval(g, values, c, u * Ts, speed);
            nonfinite = !(f * 0.0 == 0.0);
            reach = field::reach(V, A, speed, hwu * Ts);
            at = f < best ? u * Ts : at;
            best = fmin(best, f);
        }
        rbest = row_min(best);
        if (active) {
            if (f - L * reach >= field::threshold(rbest, tol, r_min)) {
                active = field::advance(level, index);
            } else if (level < field::MAX_LEVEL) {
                field::descend(level, index);
            } else {
                unresolved = true;
                active = false;
            }
        }
    }
    unresolved = ((__ballot(unresolved) >> shift) & 0xffffull) != 0ull;
    nonfinite = ((__ballot(nonfinite) >> shift) & 0xffffull) != 0ull;
    // the winner: the least value, then the lowest segment; an unusable row is written by its lane 0
    const unsigned long long win = (__ballot(live && best == rbest) >> shift) & 0xffffull;
    const bool usable = row_ok && !bad && !nonfinite && win != 0ull;
    const int writer = usable ? __ffsll((long long)win) - 1 : 0;
    if (b < B && s == writer) {
        double rec[TGMS_SEP_STRIDE];
        const int fw = field::finish(best, knot + at, D, !usable, unresolved, r_min, rec);
        if (near) *reinterpret_cast<double2*>(near + (int64_t)b * TGMS_SEP_STRIDE) = make_double2(rec[0], rec[1]);
        if (evals_out) evals_out[b] = (fw & TGMS_SEP_NONFINITE) ? 0 : evals;
        if (flags) flags[b] = fw;
    }
}

__global__ __launch_bounds__(field::LIP_BLOCK) void k_field_lip(field::Grid g, int64_t total,
                                                                const float* __restrict__ values,
                                                                double* __restrict__ partial) {
    __shared__ double sm[3][field::LIP_BLOCK];
    double m[3] = {0.0, 0.0, 0.0};
    const int32_t n[3] = {g.n[0], g.n[1], g.n[2]};
    for (int64_t e = (int64_t)blockIdx.x * field::LIP_BLOCK + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * field::LIP_BLOCK)
        field::edge_max(values, n, e, m);
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) sm[a][threadIdx.x] = m[a];
    __syncthreads();
    for (int d = field::LIP_BLOCK / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            TGMS_UNROLL
            for (int a = 0; a < 3; ++a) sm[a][threadIdx.x] = fmax(sm[a][threadIdx.x], sm[a][threadIdx.x + d]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = sm[threadIdx.x][0];
}

__global__ __launch_bounds__(field::LIP_BLOCKS) void k_field_lip_fold(int32_t blocks, double ih,
                                                                      const double* __restrict__ partial,
                                                                      double* __restrict__ lip) {
    __shared__ double sm[3][field::LIP_BLOCKS];
    TGMS_UNROLL
    for (int a = 0; a < 3; ++a) sm[a][threadIdx.x] = (int)threadIdx.x < blocks ? partial[threadIdx.x * 3 + a] : 0.0;
    __syncthreads();
    for (int d = field::LIP_BLOCKS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            TGMS_UNROLL
            for (int a = 0; a < 3; ++a) sm[a][threadIdx.x] = fmax(sm[a][threadIdx.x], sm[a][threadIdx.x + d]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double m[3] = {sm[0][0], sm[1][0], sm[2][0]};
        *lip = field::lipschitz(m, ih);
    }
}

}  // namespace

size_t field_scratch_bytes() { return (1 + 3 * (size_t)field::LIP_BLOCKS) * sizeof(double); }

hipError_t launch_field(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, const tgms_field& fld,
                        const float* values, double lip, double r_min, double tol, int32_t max_evals, void* scratch,
                        double* near, int32_t* evals, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    const field::Grid g = field::make_grid(fld);
    double* d_lip = nullptr;
    if (scratch) {  // lip == 0: L from the values, left on the device
        d_lip = static_cast<double*>(scratch);
        double* partial = d_lip + 1;
        const int64_t total = (int64_t)fld.n[0] * fld.n[1] * fld.n[2];
        const int32_t blocks =
            (int32_t)std::min<int64_t>(field::LIP_BLOCKS, (total + field::LIP_BLOCK - 1) / field::LIP_BLOCK);
        TGMS_LAUNCH(k_field_lip, dim3((unsigned)blocks), dim3(field::LIP_BLOCK), 0, stream, g, total, values, partial);
        TGMS_LAUNCH(k_field_lip_fold, dim3(1), dim3(field::LIP_BLOCKS), 0, stream, blocks, g.ih, partial, d_lip);
    }
    constexpr int ROWS = W64 / ROW;
    TGMS_LAUNCH(k_field, dim3((unsigned)((B + ROWS - 1) / ROWS)), dim3(W64), 0, stream, B, seg_offsets, T, C, g, values,
                lip, d_lip, r_min, tol, max_evals, near, evals, flags);
    return hipSuccess;
}

}  // namespace tgms
