// tgms_corridor_split.hip — corridor split (tgms_corridor_split_batch_device) on gfx950.
//
// The third step of the planner's loop: the segments that a corridor call found outside get a
// waypoint at their worst excursion, and the batch (offsets, waypoints, times, the CSR of faces)
// is rebuilt on the device.  tgms_corridor_split_core.h has every decision; this file has the
// mapping.  Three stages, launched in order on one stream:
//   1. k_split_plan: k_corridor's tile (a wavefront per TILE = 4 trajectories, a lane per
//      segment, grid-stride).  The lanes of a trajectory decide wanted / at a waypoint, rank
//      the wanted segments among themselves with shuffles (at most 16, so 16 steps), apply the
//      segment cap, and the tile leaves per trajectory the new segment count, the new face
//      count, a 16-bit split mask and the flags.
//   2. the scan: exclusive prefix sums of the two counts over B, as three launches of SCAN-wide
//      workgroups: k_scan_sums (a sum per workgroup), k_scan_top (ONE workgroup walks the sums
//      in chunks of SCAN with a carry, so there is no third level however large B is, and
//      writes the totals), k_scan_add (each workgroup scans its own entries again and adds its
//      base).  Segments are int32, faces int64 (2 F can pass 2^31).
//   3. k_split_write: the tile again.  The lane of a segment writes its one or two times, its
//      start waypoint, the inserted one, its parent rows and face offsets; the face rows are
//      copied as the items of k_corridor: numbered through the tile's face counts, taken 128 at a
//      time, two 16-byte loads and two or four 16-byte stores per row, consecutive lanes on
//      consecutive rows.
// No workgroup ever waits for another: no look-back, no grid barrier, no flag.  Each stage ends
// before the next begins because they are separate launches on one stream.
// Every store is guarded by the capacity the header names (2 S segments, 2 S + B waypoints, 2 F
// faces, S = seg_offsets[B]); only offsets that are not a CSR (a count below 1) can reach a
// guard.
#include <algorithm>

#include "tgms_corridor_split_core.h"
#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_seg_tile.h"

namespace tgms {
namespace {

using namespace seg_tile;  // the tile by grid-stride, one wavefront a workgroup: not wave_tile
constexpr int SCAN = 256;  // entries of one workgroup of the scan (tests/test_gpu_split.py pins its seams)

// The face span of segment gs: its first face and count; -1: not usable.
__device__ __forceinline__ void face_span(int64_t F, const int64_t* __restrict__ fo, int64_t gs, int64_t& fb,
                                          int& cnt) {
    int64_t fe = F;
    fb = 0;
    if (fo) {
        fb = fo[gs];
        fe = fo[gs + 1];
    }
    cnt = corridor::span_ok(fb, fe, F) ? (int)(fe - fb) : -1;
}

__global__ __launch_bounds__(W64) void k_split_plan(int32_t B, const int32_t* __restrict__ so,
                                                    const double* __restrict__ W, const double* __restrict__ T,
                                                    const double* __restrict__ C, int64_t F,
                                                    const int64_t* __restrict__ fo,
                                                    const double* __restrict__ seg_rec,
                                                    const int32_t* __restrict__ seg_face, double r,
                                                    int32_t* __restrict__ cntS, int64_t* __restrict__ cntF,
                                                    int32_t* __restrict__ mask, int32_t* __restrict__ flags) {
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
        // every input of the trajectory finite, every time positive
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            double chk = 0.0;
            bool neg = false;
            for (int e = lane; e < x.Mt[t] * 24; e += W64) chk = split::finite_chk(C[x.s0[t] * 24 + e], chk);
            if (x.Mt[t] > 0 && lane < (x.Mt[t] + 1) * 3) chk = split::finite_chk(W[(x.s0[t] + b0 + t) * 3 + lane], chk);
            if (lane < x.Mt[t]) {
                const double tt = T[x.s0[t] + lane];
                chk = split::finite_chk(tt, chk);
                neg = !(tt > 0.0);
            }
            if (chk != 0.0 || neg) bad[t] = 1;  // every writer stores the same value
        }
        double Tm = 0.0, m = -__builtin_inf(), ts = 0.0;
        int cnt = 0;
        bool want = false;
        if (lane < S) {
            Tm = T[gs];
            const double2 rec = *reinterpret_cast<const double2*>(seg_rec + gs * TGMS_COR_STRIDE);
            m = rec.x;
            ts = rec.y;
            const int32_t face = seg_face[gs];
            int64_t fb;
            face_span(F, fo, gs, fb, cnt);
            want = split::wanted(m, r);
            const bool in_span = cnt >= 0 && (int64_t)face >= fb && (int64_t)face < fb + cnt;
            if (cnt < 0 || !(m == m) || !(ts == ts) || (want && !in_span)) bad[tr] = 1;
        }
        __syncthreads();
        const bool usable = lane < S && bad[tr] == 0;
        const double knot = lane_knot(Tm, sb, li);
        const bool end = split::at_end(split::local_time(ts, knot, Tm), Tm);
        const bool cand = usable && want && !end;
        // the wanted segments of the trajectory that are taken before this one
        int rank = 0;
#pragma unroll
        for (int j = 0; j < TGMS_MAX_SEGMENTS; ++j) {
            const int src = std::min(sb + j, W64 - 1);
            const double mj = __shfl(m, src, W64);
            const int cj = __shfl((int)cand, src, W64);
            rank += (j < M && cj != 0 && split::before(mj, j, m, li)) ? 1 : 0;
        }
        const bool take = cand && split::taken(rank, M);
        const uint64_t b_take = __ballot(take), b_full = __ballot(cand && !take),
                       b_end = __ballot(usable && want && end);
        // the faces this segment owns afterwards: both children own a copy
        const int keep = (lane < S && cnt > 0 && fo) ? cnt : 0;
        const int inc = wave_inclusive(keep * (take ? 2 : 1), lane);
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            if (t >= nb) continue;
            const int hi = x.base[t + 1] > 0 ? __shfl(inc, x.base[t + 1] - 1, W64) : 0;
            const int lo = x.base[t] > 0 ? __shfl(inc, x.base[t] - 1, W64) : 0;
            if (lane != t) continue;
            const uint64_t span = x.Mt[t] ? (~0ull >> (64 - x.Mt[t])) << x.base[t] : 0ull;
            const int32_t mk = (int32_t)((b_take & span) >> x.base[t]);
            int32_t fl = mk ? TGMS_SPLIT_DONE : 0;
            fl |= (b_full & span) ? TGMS_SPLIT_FULL : 0;
            fl |= (b_end & span) ? TGMS_SPLIT_AT_END : 0;
            const bool unusable = x.oob[t] || bad[t] != 0;
            const int64_t b = b0 + t;
            cntS[b] = x.oob[t] ? 1 : x.Mt[t] + __popc((unsigned)mk);  // a bad count: one placeholder segment
            cntF[b] = hi - lo;
            mask[b] = unusable ? 0 : mk;
            if (flags) flags[b] = unusable ? TGMS_FEAS_NONFINITE : fl;
        }
    }
}

// ---- the scan: exclusive prefix sums of cntS and cntF over B ----

// Exclusive prefix of (a, b) over the SCAN threads of the workgroup; ta, tb: the workgroup's sums.
__device__ __forceinline__ void block_exclusive(int64_t& a, int64_t& b, int64_t& ta, int64_t& tb) {
    constexpr int WAVES = SCAN / W64;
    __shared__ int64_t part[2][WAVES];
    const int lane = threadIdx.x % W64, wave = threadIdx.x / W64;
    int64_t ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < W64; o <<= 1) {
        const int64_t ua = __shfl_up(ia, o, W64), ub = __shfl_up(ib, o, W64);
        ia += lane >= o ? ua : 0;
        ib += lane >= o ? ub : 0;
    }
    __syncthreads();  // the previous use of part is over
    if (lane == W64 - 1) {
        part[0][wave] = ia;
        part[1][wave] = ib;
    }
    __syncthreads();
    int64_t oa = 0, ob = 0;
    ta = tb = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        oa += w < wave ? part[0][w] : 0;
        ob += w < wave ? part[1][w] : 0;
        ta += part[0][w];
        tb += part[1][w];
    }
    a = oa + ia - a;
    b = ob + ib - b;
}

__global__ __launch_bounds__(SCAN) void k_scan_sums(int32_t B, const int32_t* __restrict__ cntS,
                                                    const int64_t* __restrict__ cntF, int64_t* __restrict__ sumS,
                                                    int64_t* __restrict__ sumF) {
    const int64_t i = (int64_t)blockIdx.x * SCAN + threadIdx.x;
    int64_t a = i < B ? cntS[i] : 0, b = i < B ? cntF[i] : 0, ta, tb;
    block_exclusive(a, b, ta, tb);
    if (threadIdx.x == 0) {
        sumS[blockIdx.x] = ta;
        sumF[blockIdx.x] = tb;
    }
}

// One workgroup: the sums of the n workgroups become their exclusive prefixes, in chunks of SCAN
// with a carry; then the totals.  shared_F >= 0: shared mode, F' = F.
__global__ __launch_bounds__(SCAN) void k_scan_top(int32_t n, int64_t* __restrict__ sumS, int64_t* __restrict__ sumF,
                                                   int64_t shared_F, int32_t B, int32_t* __restrict__ so_out,
                                                   int64_t* __restrict__ totals) {
    int64_t cs = 0, cf = 0;
    for (int32_t c0 = 0; c0 < n; c0 += SCAN) {
        const int32_t i = c0 + (int32_t)threadIdx.x;
        int64_t a = i < n ? sumS[i] : 0, b = i < n ? sumF[i] : 0, ta, tb;
        block_exclusive(a, b, ta, tb);
        if (i < n) {
            sumS[i] = cs + a;
            sumF[i] = cf + b;
        }
        cs += ta;
        cf += tb;
    }
    if (threadIdx.x == 0) {
        so_out[B] = (int32_t)cs;
        totals[0] = cs;
        totals[1] = shared_F >= 0 ? shared_F : cf;
    }
}

__global__ __launch_bounds__(SCAN) void k_scan_add(int32_t B, const int32_t* __restrict__ cntS,
                                                   int64_t* __restrict__ cntF, const int64_t* __restrict__ sumS,
                                                   const int64_t* __restrict__ sumF, int32_t* __restrict__ so_out) {
    const int64_t i = (int64_t)blockIdx.x * SCAN + threadIdx.x;
    int64_t a = i < B ? cntS[i] : 0, b = i < B ? cntF[i] : 0, ta, tb;
    block_exclusive(a, b, ta, tb);
    if (i < B) {
        so_out[i] = (int32_t)(sumS[blockIdx.x] + a);
        cntF[i] = sumF[blockIdx.x] + b;  // in place: the trajectory's first face afterwards
    }
}

__global__ void k_split_empty(int64_t F1, int32_t* __restrict__ so_out, int64_t* __restrict__ totals) {
    empty_batch(so_out, totals);
    if (threadIdx.x == 0 && blockIdx.x == 0) totals[1] = F1;
}

// ---- the write ----

__global__ __launch_bounds__(W64) void k_split_write(
    int32_t B, const int32_t* __restrict__ so, const double* __restrict__ W, const double* __restrict__ T,
    const double* __restrict__ C, int64_t F, const double* __restrict__ faces, const int64_t* __restrict__ fo,
    const double* __restrict__ seg_rec, const int32_t* __restrict__ seg_face, double r, int mode, double min_frac,
    const int32_t* __restrict__ mask, const int64_t* __restrict__ face_base, const int32_t* __restrict__ so_out,
    double* __restrict__ W_out, double* __restrict__ T_out, double* __restrict__ faces_out,
    int64_t* __restrict__ fo_out, int32_t* __restrict__ parent) {
    __shared__ int pre[SEGS + 1];    // face rows before a segment; pre[SEGS]: the tile's rows
    __shared__ int64_t fin[SEGS];    // a segment's first face
    __shared__ int64_t fout[SEGS];   // its first face afterwards
    __shared__ int dup[SEGS];        // its face count where it is split: the second copy's distance
    const int lane = threadIdx.x;
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    // the capacities of the caller's buffers (include/tgms.h)
    const int64_t S_in = so[B], capS = 2 * S_in, capW = capS + B, capF = 2 * F;
    const double nan = __builtin_nan("");
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
        // the plan of this lane's trajectory
        int32_t mk = 0;
        int64_t so2 = 0, fb2 = 0;
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            if (t >= nb) continue;
            const int32_t mk_t = __builtin_amdgcn_readfirstlane(mask[b0 + t]);
            const int32_t so_t = __builtin_amdgcn_readfirstlane(so_out[b0 + t]);
            const int64_t fb_t = fo ? face_base[b0 + t] : 0;
            mk = tr == t ? mk_t : mk;
            so2 = tr == t ? (int64_t)so_t : so2;
            fb2 = tr == t ? fb_t : fb2;
            if (x.oob[t] && lane == 0) {
                // a segment count outside 1..16: one placeholder segment, a NaN time, two NaN
                // waypoints and no face; the solve that follows rejects this row alone
                const int64_t w0 = so_t + b0 + t;
                if (so_t < capS) {
                    T_out[so_t] = nan;
                    if (parent) parent[so_t] = TGMS_NEAR_NONE;
                    if (fo) fo_out[so_t] = fb_t;
                }
                for (int e = 0; e < 6; ++e)
                    if (w0 + e / 3 < capW) W_out[w0 * 3 + e] = nan;
                if (fo && b0 + t == (int64_t)B - 1 && so_t + 1 <= capS) fo_out[so_t + 1] = fb_t;
            }
        }
        const bool live = lane < S;
        const bool cut = live && ((mk >> (li & 31)) & 1) != 0;
        const int64_t orow = so2 + li + __popc((unsigned)mk & ((1u << (li & 31)) - 1u));
        const int nsub = cut ? 2 : 1;
        const double Tm = live ? T[gs] : 0.0;
        const double knot = lane_knot(Tm, sb, li);
        if (live) {
            const double* w0 = W + (gs + b) * 3;
            if (orow + b < capW) copy3(W_out + (orow + b) * 3, w0);
            if (li == M - 1 && orow + nsub + b < capW) copy3(W_out + (orow + nsub + b) * 3, w0 + 3);
            if (parent && orow < capS) parent[orow] = (int32_t)gs;
            if (!cut) {
                if (orow < capS) T_out[orow] = Tm;
            } else {
                double tl, trr, w[3];
                split::split_times(split::local_time(seg_rec[gs * TGMS_COR_STRIDE + 1], knot, Tm), Tm, min_frac, tl,
                                   trr);
                if (mode == TGMS_SPLIT_PULL) {
                    const double2* row = reinterpret_cast<const double2*>(faces + (int64_t)seg_face[gs] * 4);
                    const double2 nxy = row[0], nzd = row[1];
                    split::insert_pull(C + gs * 24, tl, nxy.x, nxy.y, nzd.x, nzd.y, r, w);
                } else {
                    split::insert_chord(w0, w0 + 3, tl, Tm, w);
                }
                if (orow + 1 < capS) {
                    T_out[orow] = tl;
                    T_out[orow + 1] = trr;
                    if (parent) parent[orow + 1] = (int32_t)gs;
                }
                if (orow + 1 + b < capW) copy3(W_out + (orow + 1 + b) * 3, w);
            }
        }
        if (!fo) continue;  // shared mode: the faces stay as they are (wave-uniform)
        // the face offsets of the new segments and the copy of the face rows
        int64_t fb = 0;
        int cnt = 0;
        if (live) face_span(F, fo, gs, fb, cnt);
        cnt = cnt > 0 ? cnt : 0;  // a span that is not usable owns nothing afterwards
        const int inc_out = wave_inclusive(cnt * nsub, lane);
        const int before_tr = __shfl(inc_out, std::max(sb - 1, 0), W64);
        const int64_t first = fb2 + (inc_out - cnt * nsub) - (sb > 0 ? before_tr : 0);
        const int inc_in = wave_inclusive(cnt, lane);
        __syncthreads();  // the previous tile's readers are done with the LDS
        pre[lane] = inc_in - cnt;
        if (lane == W64 - 1) pre[SEGS] = inc_in;
        fin[lane] = fb;
        fout[lane] = first;
        dup[lane] = cut ? cnt : 0;
        if (live) {
            if (orow < capS) fo_out[orow] = first;
            if (cut && orow + 1 < capS) fo_out[orow + 1] = first + cnt;
            if (b == (int64_t)B - 1 && li == M - 1 && orow + nsub <= capS) fo_out[orow + nsub] = first + cnt * nsub;
        }
        __syncthreads();
        const int total = __builtin_amdgcn_readfirstlane(pre[SEGS]);  // <= SEGS * TGMS_COR_MAX_FACES
        for (int c0 = 0; c0 < total; c0 += 2 * W64) {
            // two rows per lane and pass, the loads of both before the stores
            double2 va[2], vb[2];
            int64_t dst[2];
            int second[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int q = c0 + k * W64 + lane;
                dst[k] = -1;
                second[k] = 0;
                va[k] = vb[k] = make_double2(0.0, 0.0);
                if (q < total) {
                    // the last segment whose first row is <= q: it has pre[seg + 1] > q, so it is not empty
                    int seg = 0;
#pragma unroll
                    for (int step = SEGS / 2; step >= 1; step >>= 1) seg += pre[seg + step] <= q ? step : 0;
                    const int kk = q - pre[seg];
                    const double2* row = reinterpret_cast<const double2*>(faces + (fin[seg] + kk) * 4);
                    va[k] = row[0];
                    vb[k] = row[1];
                    dst[k] = fout[seg] + kk;
                    second[k] = dup[seg];
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (dst[k] >= 0 && dst[k] < capF) {
                    double2* o = reinterpret_cast<double2*>(faces_out + dst[k] * 4);
                    o[0] = va[k];
                    o[1] = vb[k];
                }
                if (second[k] > 0 && dst[k] + second[k] < capF) {
                    double2* o = reinterpret_cast<double2*>(faces_out + (dst[k] + second[k]) * 4);
                    o[0] = va[k];
                    o[1] = vb[k];
                }
            }
        }
    }
}

struct Scratch : ScanScratch {
    int32_t *cntS, *mask;
    Scratch(int32_t B, void* base) : ScanScratch(B, base, false) {  // the scan's totals are the caller's
        cntS = take<int32_t>(n);
        mask = take<int32_t>(n);
    }
};

}  // namespace

size_t corridor_split_scratch_bytes(int32_t B) { return Scratch(B, nullptr).off; }

size_t count_scan_blocks(int32_t B) { return ((size_t)std::max(B, 0) + SCAN - 1) / SCAN; }

hipError_t launch_count_scan(int32_t B, const int32_t* cntS, int64_t* cntF, int64_t* sumS, int64_t* sumF,
                             int64_t shared_F, int32_t* so_out, int64_t* totals, hipStream_t stream) {
    const unsigned nblk = (unsigned)count_scan_blocks(B);
    TGMS_LAUNCH(k_scan_sums, dim3(nblk), dim3(SCAN), 0, stream, B, cntS, cntF, sumS, sumF);
    TGMS_LAUNCH(k_scan_top, dim3(1), dim3(SCAN), 0, stream, (int32_t)nblk, sumS, sumF, shared_F, B, so_out, totals);
    TGMS_LAUNCH(k_scan_add, dim3(nblk), dim3(SCAN), 0, stream, B, cntS, cntF, sumS, sumF, so_out);
    return hipSuccess;
}

hipError_t launch_corridor_split(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                                 const double* C, int64_t F, const double* faces, const int64_t* face_offsets,
                                 const double* seg_rec, const int32_t* seg_face, double r, int mode, double min_frac,
                                 void* scratch, int32_t* so_out, double* W_out, double* T_out, double* faces_out,
                                 int64_t* fo_out, int32_t* parent, int64_t* totals, int32_t* flags,
                                 hipStream_t stream) {
    const int64_t shared_F = face_offsets ? -1 : F;
    if (B <= 0) {
        TGMS_LAUNCH(k_split_empty, dim3(1), dim3(W64), 0, stream, face_offsets ? (int64_t)0 : F, so_out, totals);
        return hipSuccess;
    }
    const Scratch s(B, scratch);
    const int64_t tiles = ((int64_t)B + TILE - 1) / TILE;
    const unsigned blocks = (unsigned)std::min<int64_t>(tiles, 4096);
    TGMS_LAUNCH(k_split_plan, dim3(blocks), dim3(W64), 0, stream, B, seg_offsets, W, T, C, F, face_offsets, seg_rec,
                seg_face, r, s.cntS, s.cntF, s.mask, flags);
    if (const hipError_t e = launch_count_scan(B, s.cntS, s.cntF, s.sumS, s.sumF, shared_F, so_out, totals, stream);
        e != hipSuccess)
        return e;
    TGMS_LAUNCH(k_split_write, dim3(blocks), dim3(W64), 0, stream, B, seg_offsets, W, T, C, F, faces, face_offsets,
                seg_rec, seg_face, r, mode, min_frac, s.mask, s.cntF, so_out, W_out, T_out, faces_out, fo_out,
                parent);
    return hipSuccess;
}

}  // namespace tgms
