// tgms_cut.hip — replan cut (tgms_cut_batch_device) on gfx950.
//
// Every trajectory of a solved batch is restarted from its state at t_cut: the segments behind
// the cut go, the one it falls in is shortened, and the batch (offsets, waypoints, times, end
// derivatives, coefficients) is rebuilt on the device.  tgms_cut_core.h has every decision.  Three
// stages, launched in order on one stream:
//   1. k_cut_plan: the segment tile of tgms_seg_tile.h, tiles by grid-stride, one wavefront a
//      workgroup.  The lanes of a trajectory form its knots with shuffles, count the interior
//      knots at or before the cut with a ballot, fetch the knot and time of that segment with
//      two more shuffles and resolve the plan: the first kept segment s, the local time, the
//      flags, the new segment count and t0.
//   2. the scan of the new segment counts (launch_count_scan).
//   3. k_cut_write: the tile again.  The lane of a kept segment writes its time, its start
//      waypoint and its parent row; the lane of the first one also the end derivatives and,
//      where the cut is inside the segment, the Taylor-shifted row, computed in registers with
//      compile-time indices.  Every other coefficient row (192 B) is copied as twelve 16-byte
//      items, numbered through the tile's output rows, consecutive lanes on consecutive items.
// No workgroup ever waits for another: each stage ends before the next begins because they are
// separate launches on one stream.
// Every store is guarded by the capacity the header names (S segments, S + B waypoints, S =
// seg_offsets[B]); only offsets that are not a CSR (a count below 1) can reach a guard.
#include <algorithm>

#include "tgms_cut_core.h"
#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_seg_tile.h"

namespace tgms {
namespace {

using namespace seg_tile;

constexpr int ROW_ITEMS = 12;  // a coefficient row [3][8] as 16-byte items
constexpr int64_t SRC_SELF = -1, SRC_NAN = -2;  // an output row its own lane writes; a placeholder's

__device__ __forceinline__ int32_t pack(int kind, int s) { return kind | (s << 8); }

__global__ __launch_bounds__(W64) void k_cut_plan(int32_t B, const int32_t* __restrict__ so,
                                                  const double* __restrict__ W, const double* __restrict__ T,
                                                  const double* __restrict__ ED, const double* __restrict__ C,
                                                  const double* __restrict__ t_cut, double min_frac,
                                                  int32_t* __restrict__ cntS, int64_t* __restrict__ cntF,
                                                  int32_t* __restrict__ code, double* __restrict__ tloc,
                                                  double* __restrict__ t0_out, int32_t* __restrict__ flags) {
    __shared__ int bad[TILE];
    const int lane = threadIdx.x;
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TILE;
        const int nb = (int)std::min<int64_t>(TILE, B - b0);
        Tile x;
        load_tile(so, b0, nb, x);
        const int S = x.base[TILE];
        int tr, sb, M;
        int64_t gs;
        lane_segment(x, lane, tr, sb, M, gs);
        const int li = lane - sb;
        __syncthreads();  // the previous tile's readers are done with the LDS
        if (lane < TILE) bad[lane] = 0;
        __syncthreads();
        // every input of the trajectory finite, every time positive, t_cut not NaN
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            if (x.Mt[t] == 0) continue;  // wave-uniform: not there, or nothing can be read
            double chk = 0.0;
            bool neg = false;
            for (int e = lane; e < x.Mt[t] * 24; e += W64) chk = split::finite_chk(C[x.s0[t] * 24 + e], chk);
            if (lane < (x.Mt[t] + 1) * 3) chk = split::finite_chk(W[(x.s0[t] + b0 + t) * 3 + lane], chk);
            if (ED && lane < 18) chk = split::finite_chk(ED[(b0 + t) * 18 + lane], chk);
            if (lane < x.Mt[t]) {
                const double tt = T[x.s0[t] + lane];
                chk = split::finite_chk(tt, chk);
                neg = !(tt > 0.0);
            }
            if (lane == 0) {
                const double tc = t_cut[b0 + t];
                neg = neg || !(tc == tc);
            }
            if (chk != 0.0 || neg) bad[t] = 1;  // every writer stores the same value
        }
        __syncthreads();
        const bool live = lane < S;
        const double Tm = live ? T[gs] : 0.0;
        const double tc = live ? t_cut[b0 + tr] : 0.0;
        const double knot = lane_knot(Tm, sb, li);
        const double next = knot + Tm;  // the knot after this segment, the prefix sum's own addition
        const double D = __shfl(next, std::max(sb + M - 1, 0), W64);
        const uint64_t at = __ballot(live && li >= 1 && cut::in_or_after(knot, cut::clamp_cut(tc, D)));
        const uint64_t span = M ? (~0ull >> (64 - M)) << sb : 0ull;
        const int s = __popcll(at & span);  // <= M - 1
        const int from = std::min(sb + s, W64 - 1);
        const double k_s = __shfl(knot, from, W64), T_s = __shfl(Tm, from, W64), k_next = __shfl(next, from, W64);
        if (live && li == 0) {
            const cut::Plan p = bad[tr] ? cut::through(M) : cut::resolve(M, tc, D, s, k_s, T_s, k_next, min_frac);
            const int64_t b = b0 + tr;
            cntS[b] = p.M_out;
            cntF[b] = 0;
            code[b] = pack(p.kind, p.s);
            tloc[b] = p.t_loc;
            if (t0_out) t0_out[b] = p.t0;
            if (flags) flags[b] = p.flags;
        }
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            if (!(x.oob[t] && lane == t)) continue;  // a bad count: the placeholder and the cut's own words of it
            plan_placeholder(b0 + t, cntS, cntF, flags);
            code[b0 + t] = pack(cut::PLACEHOLDER, 0);
            tloc[b0 + t] = 0.0;
            if (t0_out) t0_out[b0 + t] = __builtin_nan("");
        }
    }
}

__global__ void k_cut_empty(int32_t* __restrict__ so_out, int64_t* __restrict__ totals) { empty_batch(so_out, totals); }

__global__ __launch_bounds__(W64) void k_cut_write(
    int32_t B, const int32_t* __restrict__ so, const double* __restrict__ W, const double* __restrict__ T,
    const double* __restrict__ ED, const double* __restrict__ C, const int32_t* __restrict__ code,
    const double* __restrict__ tloc, const int32_t* __restrict__ so_out, const int64_t* __restrict__ scan_totals,
    double* __restrict__ W_out, double* __restrict__ T_out, double* __restrict__ ED_out, double* __restrict__ C_out,
    int32_t* __restrict__ parent, int64_t* __restrict__ totals) {
    __shared__ int64_t src[SEGS];  // the input row of each of the tile's output rows, or SRC_*
    const int lane = threadIdx.x;
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    // the capacities of the caller's buffers (include/tgms.h)
    const int64_t capS = so[B], capW = capS + B;
    const double nan = __builtin_nan("");
    if (blockIdx.x == 0 && lane == 0) totals[0] = scan_totals[0];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * TILE;
        const int nb = (int)std::min<int64_t>(TILE, B - b0);
        Tile x;
        load_tile(so, b0, nb, x);
        const int S = x.base[TILE];
        int tr, sb, M;
        int64_t gs;
        lane_segment(x, lane, tr, sb, M, gs);
        const int li = lane - sb;
        const int64_t b = b0 + tr;
        const int64_t out0 = __builtin_amdgcn_readfirstlane(so_out[b0]);
        const int rows = (int)std::min<int64_t>(
            std::max<int64_t>((int64_t)__builtin_amdgcn_readfirstlane(so_out[b0 + nb]) - out0, 0), SEGS);
        __syncthreads();  // the previous tile's readers are done with the LDS
        src[lane] = SRC_SELF;
        __syncthreads();
        // the plan of this lane's trajectory
        int32_t cd = 0;
        int64_t so2 = 0;
        double t_loc = 0.0;
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            if (t >= nb) continue;
            const int32_t cd_t = __builtin_amdgcn_readfirstlane(code[b0 + t]);
            const int32_t so_t = __builtin_amdgcn_readfirstlane(so_out[b0 + t]);
            const double tl_t = tloc[b0 + t];
            cd = tr == t ? cd_t : cd;
            so2 = tr == t ? (int64_t)so_t : so2;
            t_loc = tr == t ? tl_t : t_loc;
            if (x.oob[t] && lane == 0) {
                // a segment count outside 1..16: one placeholder segment, a NaN time, two NaN
                // waypoints, NaN end derivatives; the solve that follows rejects this row alone
                const int64_t w0 = so_t + b0 + t;
                if (so_t < capS) {
                    T_out[so_t] = nan;
                    if (parent) parent[so_t] = TGMS_NEAR_NONE;
                }
                for (int e = 0; e < 6; ++e)
                    if (w0 + e / 3 < capW) W_out[w0 * 3 + e] = nan;
                for (int e = 0; e < 18; ++e) ED_out[(b0 + t) * 18 + e] = nan;
                if ((uint64_t)(so_t - out0) < (uint64_t)SEGS) src[so_t - out0] = SRC_NAN;
            }
        }
        const int kind = cd & 0xFF, s = cd >> 8;
        const bool live = lane < S, hold = kind == cut::FINISHED;
        const bool kept = live && (hold ? li == M - 1 : li >= s);
        const bool first = kept && (hold || li == s);
        const int64_t orow = hold ? so2 : so2 + (li - s);
        if (kept) {
            const double Tm = T[gs];
            const double* w0 = W + (gs + b) * 3;
            const bool inside = first && !hold && t_loc > 0.0;  // the cut is inside this segment
            if (orow < capS) {
                T_out[orow] = inside ? cut::first_time(Tm, t_loc) : Tm;
                if (parent) parent[orow] = (int32_t)gs;
            }
            int64_t from = gs;
            if (first) {
                // the start state, and the row that is not a copy
                double c[24], p[3], d[9], ed[18];
                bool own = false;
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    ed[e] = 0.0;
                    ed[9 + e] = (ED && !hold) ? ED[b * 18 + 9 + e] : 0.0;
                }
                if (hold) {
#pragma unroll
                    for (int e = 0; e < 24; ++e) c[e] = 0.0;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) c[ax * 8] = p[ax] = w0[3 + ax];
                    own = true;
                } else if (s == 0 && !inside) {
                    // nothing is removed at this end: the input's start derivatives, or rest
#pragma unroll
                    for (int e = 0; e < 9; ++e) ed[e] = ED ? ED[b * 18 + e] : 0.0;
                } else {
                    double in[24];
                    const double2* row = reinterpret_cast<const double2*>(C + gs * 24);
#pragma unroll
                    for (int e = 0; e < ROW_ITEMS; ++e) {
                        const double2 v = row[e];
                        in[2 * e] = v.x;
                        in[2 * e + 1] = v.y;
                    }
                    cut::shift_row(in, t_loc, c, p, d);
#pragma unroll
                    for (int e = 0; e < 9; ++e) ed[e] = d[e];
                    own = inside;
                }
                double2* eo = reinterpret_cast<double2*>(ED_out + b * 18);
#pragma unroll
                for (int e = 0; e < 9; ++e) eo[e] = make_double2(ed[2 * e], ed[2 * e + 1]);
                if (own) {
                    from = SRC_SELF;
                    if (orow + b < capW) copy3(W_out + (orow + b) * 3, p);
                    if (C_out && orow < capS) {
                        double2* co = reinterpret_cast<double2*>(C_out + orow * 24);
#pragma unroll
                        for (int e = 0; e < ROW_ITEMS; ++e) co[e] = make_double2(c[2 * e], c[2 * e + 1]);
                    }
                }
            }
            if (from != SRC_SELF && orow + b < capW) copy3(W_out + (orow + b) * 3, w0);
            if (li == M - 1 && orow + 1 + b < capW) copy3(W_out + (orow + 1 + b) * 3, w0 + 3);
            if ((uint64_t)(orow - out0) < (uint64_t)SEGS) src[orow - out0] = from;
        }
        __syncthreads();
        if (!C_out) continue;  // wave-uniform
        // the copied coefficient rows: four items per lane and pass, the loads before the stores
        const double2* Cin = reinterpret_cast<const double2*>(C);
        double2* Cout = reinterpret_cast<double2*>(C_out);
        const int total = rows * ROW_ITEMS;
        for (int c0 = 0; c0 < total; c0 += 4 * W64) {
            double2 v[4];
            int64_t dst[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = c0 + k * W64 + lane;
                dst[k] = -1;
                v[k] = make_double2(nan, nan);
                if (q < total) {
                    const int row = q / ROW_ITEMS, it = q - row * ROW_ITEMS;
                    const int64_t sr = src[row];
                    if (sr != SRC_SELF && out0 + row < capS) {
                        dst[k] = (out0 + row) * ROW_ITEMS + it;
                        if (sr >= 0) v[k] = Cin[sr * ROW_ITEMS + it];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (dst[k] >= 0) Cout[dst[k]] = v[k];
        }
    }
}

struct Scratch : ScanScratch {
    double* tloc;
    int32_t *cntS, *code;
    Scratch(int32_t B, void* base) : ScanScratch(B, base, true) {
        tloc = take<double>(n);
        cntS = take<int32_t>(n);
        code = take<int32_t>(n);
    }
};

}  // namespace

size_t cut_scratch_bytes(int32_t B) { return Scratch(B, nullptr).off; }

hipError_t launch_cut(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const double* ED,
                      const double* C, const double* t_cut, double min_frac, void* scratch, int32_t* so_out,
                      double* W_out, double* T_out, double* ED_out, double* C_out, int32_t* parent, double* t0_out,
                      int64_t* totals, int32_t* flags, hipStream_t stream) {
    if (B <= 0) {
        TGMS_LAUNCH(k_cut_empty, dim3(1), dim3(W64), 0, stream, so_out, totals);
        return hipSuccess;
    }
    const Scratch s(B, scratch);
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const unsigned blocks = (unsigned)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_cut_plan, dim3(blocks), dim3(W64), 0, stream, B, seg_offsets, W, T, ED, C, t_cut, min_frac, s.cntS,
                s.cntF, s.code, s.tloc, t0_out, flags);
    if (const hipError_t e = launch_count_scan(B, s.cntS, s.cntF, s.sumS, s.sumF, 0, so_out, s.totals, stream);
        e != hipSuccess)
        return e;
    TGMS_LAUNCH(k_cut_write, dim3(blocks), dim3(W64), 0, stream, B, seg_offsets, W, T, ED, C, s.code, s.tloc, so_out,
                s.totals, W_out, T_out, ED_out, C_out, parent, totals);
    return hipSuccess;
}

}  // namespace tgms
