// tgms_reroute.hip — corridor re-route (tgms_corridor_reroute_batch_dev) on gfx950.
//
// The step between the subdivision and the inflation: a leg whose own lattice box holds a non-free
// node gets a detour through the free nodes of a bounded window of the map, reduced to a few
// pieces with free boxes, and the batch (offsets, waypoints, times, parents) is rebuilt on the
// device.  tgms_reroute_core.h has every decision, tgms_seg_tile.h the mapping of every stage but
// the search.  Stages, launched in order on one stream:
//   1. k_rrt_classify: a lane per leg (wave_tile).  A leg that is not searched leaves its record;
//      a candidate appends its slot to the candidate list (one atomic per wavefront; the order of
//      the list is not part of any result).  The list and its count stay on the device: no host
//      sync.
//   2. k_rrt_search, the hot path: a persistent grid of SEARCH_BLOCKS workgroups strides over the
//      candidate list; no workgroup waits for another.  A workgroup holds the window's distances
//      as uint16 dist[Nw] in dynamic LDS (64 KiB at the cap of 32,768 nodes, and three control
//      words beside it, which is why the size is above the static limit and set with
//      hipFuncAttributeMaxDynamicSharedMemorySize): two workgroups share a CU's 160 KiB.  Per-node
//      occupancy is the eight-corner difference of the table; non-free and unreached nodes are
//      two sentinels.  Levels are separated by one barrier each: a node takes level + 1 only from
//      a neighbour that holds exactly `level`, so the in-place updates of a level cannot feed it.
//      A level that reaches A or changes nothing ends the search (both facts travel through the
//      control word, so every thread leaves at the same barrier).  Every node the descent visits
//      then holds its final distance.  Descent and greedy run in the first wavefront: the descent
//      one step at a time (six lanes look at the six neighbours, a ballot picks the first), the
//      clear tests of up to 64 path nodes one per lane with a ballot for the first failure.  The
//      leg leaves its piece count and its interior anchors as grid nodes, not doubles.
//   3. k_rrt_count: a lane per leg; a trajectory's pieces are summed, the budget decided, the new
//      segment count and the trajectory's flags written.
//   4. the scan of the new segment counts (launch_count_scan).
//   5. k_rrt_write: a lane per output row (row_map): points from the anchors, lengths and times,
//      and the copies of everything else.
// Every store is guarded by the capacity the header names (min(max_pieces S, 16 B) segments, B
// more waypoints); only offsets that are not a CSR can reach a guard.  Every window index is
// below Nw <= 32,768 by construction of the window; the search is not entered above the cap.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_internal.h"
#include "tgms_reroute_core.h"
#include "tgms_seg_tile.h"

namespace tgms {
namespace {

using namespace seg_tile;

constexpr int LEGS = TGMS_MAX_SEGMENTS;  // record slots per trajectory in the scratch
constexpr int SEARCH_THREADS = 512;  // eight wavefronts; two such workgroups a CU
constexpr int SEARCH_BLOCKS = 512;   // the persistent grid: two workgroups for each of 256 CUs
constexpr int CTL_WORDS = 4;
constexpr size_t SEARCH_LDS = (size_t)reroute::WINDOW_NODES * sizeof(uint16_t) + CTL_WORDS * sizeof(int);

__global__ __launch_bounds__(BLOCK) void k_rrt_classify(int32_t B, const int32_t* __restrict__ so,
                                                        const double* __restrict__ W, inflate::Grid g,
                                                        const int32_t* __restrict__ table,
                                                        reroute::Record* __restrict__ recs, int32_t* __restrict__ list,
                                                        int32_t* __restrict__ count, int32_t* __restrict__ hops) {
    Lane l;
    if (!wave_tile(B, so, l)) return;
    int32_t fl = 0;
    if (l.mine) {
        const double* w = W + (l.gs + l.b0 + l.tr) * 3;  // rows s + b and s + b + 1
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        int32_t lo[3], hi[3];
        fl = reroute::classify(g, table, w0, w1, lo, hi);
    }
    const int64_t slot = (l.b0 + l.tr) * LEGS + (l.lane - l.sb);
    const bool cand = l.mine && fl < 0;
    if (l.mine) {
        recs[slot].head = reroute::pack_head(1, cand ? TGMS_RRT_BLOCKED : fl);
        if (hops && l.gs < so[B]) hops[l.gs] = TGMS_NEAR_NONE;  // offsets that are not a CSR must not reach past S
    }
    const unsigned long long m = __ballot(cand);
    if (m != 0ull) {
        const int leader = __ffsll(m) - 1;
        int base = 0;
        if (l.lane == leader) base = atomicAdd(count, __popcll(m));
        base = __shfl(base, leader, W64);
        if (cand) list[base + __popcll(m & ((1ull << l.lane) - 1ull))] = (int32_t)slot;
    }
}

__global__ __launch_bounds__(SEARCH_THREADS) void k_rrt_search(int32_t B, const int32_t* __restrict__ so,
                                                               const double* __restrict__ W, inflate::Grid g,
                                                               const int32_t* __restrict__ table, int32_t margin,
                                                               int max_pieces, reroute::Record* __restrict__ recs,
                                                               const int32_t* __restrict__ list,
                                                               const int32_t* __restrict__ count,
                                                               int32_t* __restrict__ hops) {
    extern __shared__ uint16_t dist[];  // [WINDOW_NODES], then the control words
    int* ctl = reinterpret_cast<int*>(dist + reroute::WINDOW_NODES);
    const int tid = threadIdx.x, lane = tid & (W64 - 1);
    const int ncand = __builtin_amdgcn_readfirstlane(count[0]);
    for (int c = blockIdx.x; c < ncand; c += gridDim.x) {
        __syncthreads();  // the candidate before this one is done with dist and ctl
        const int32_t slot = __builtin_amdgcn_readfirstlane(list[c]);
        const int32_t b = slot / LEGS, leg = slot % LEGS;
        const int64_t gs = (int64_t)__builtin_amdgcn_readfirstlane(so[b]) + leg;
        const double* w = W + (gs + b) * 3;
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        reroute::Record* rec = recs + slot;
        int32_t lo[3], hi[3];
        subdivide::seed(g, w0, w1, lo, hi);  // inside the grid: the leg is a candidate
        const reroute::Window win = reroute::window(g, lo, hi, margin);
        if (win.nodes > reroute::WINDOW_NODES) {
            if (tid == 0) rec->head = reroute::pack_head(1, TGMS_RRT_BLOCKED | TGMS_RRT_WINDOW);
            continue;
        }
        int32_t A[3], Z[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            A[a] = reroute::nearest(g.o[a], g.h, w0[a], lo[a], hi[a]);
            Z[a] = reroute::nearest(g.o[a], g.h, w1[a], lo[a], hi[a]);
        }
        if (!reroute::node_free(g, table, A[0], A[1], A[2]) || !reroute::node_free(g, table, Z[0], Z[1], Z[2])) {
            if (tid == 0) rec->head = reroute::pack_head(1, TGMS_RRT_BLOCKED | TGMS_RRT_ENDS);
            continue;
        }
        const int nodes = (int)win.nodes, plane_n = win.n[0] * win.n[1];
        const int qa = reroute::window_index(win, A[0] - win.lo[0], A[1] - win.lo[1], A[2] - win.lo[2]);
        const int qz = reroute::window_index(win, Z[0] - win.lo[0], Z[1] - win.lo[1], Z[2] - win.lo[2]);
        for (int q = tid; q < nodes; q += SEARCH_THREADS) {
            const int z = q / plane_n, r = q - z * plane_n, y = r / win.n[0], xx = r - y * win.n[0];
            const bool fr = reroute::node_free(g, table, win.lo[0] + xx, win.lo[1] + y, win.lo[2] + z);
            dist[q] = q == qz ? (uint16_t)0 : (fr ? reroute::D_UNREACHED : reroute::D_NOT_FREE);
        }
        if (tid < CTL_WORDS) ctl[tid] = 0;
        __syncthreads();
        // the levels: bit 0 of a level's control word says that it changed a node, bit 1 that it reached A
        bool found = qa == qz;
        for (int level = 0; !found; ++level) {
            int mine = 0;
            for (int q = tid; q < nodes; q += SEARCH_THREADS) {
                if (dist[q] != reroute::D_UNREACHED) continue;
                const int z = q / plane_n, r = q - z * plane_n, y = r / win.n[0], xx = r - y * win.n[0];
                bool take = false;
#pragma unroll
                for (int d = 0; d < 6; ++d) {
                    int32_t nx, ny, nz;
                    if (reroute::neighbour(win, xx, y, z, d, nx, ny, nz))
                        take = take || dist[reroute::window_index(win, nx, ny, nz)] == (uint16_t)level;
                }
                if (take) {
                    dist[q] = (uint16_t)(level + 1);
                    mine |= q == qa ? 3 : 1;
                }
            }
            const int slot_l = level % 3;
            if (mine) atomicOr(&ctl[slot_l], mine);
            __syncthreads();
            const int word = ctl[slot_l];
            if (tid == 0) ctl[(level + 2) % 3] = 0;  // last read a level ago, next written a level on
            found = (word & 2) != 0;
            if (word == 0) break;
        }
        if (!found) {  // the same for every thread: it came through the control word
            if (tid == 0) rec->head = reroute::pack_head(1, TGMS_RRT_BLOCKED | TGMS_RRT_NOPATH);
            continue;
        }
        if (tid >= W64) continue;  // the first wavefront: descent and greedy
        const int nhops = dist[qa];
        double pt[3];
        reroute::node_point(g, reroute::node_id(g, A[0], A[1], A[2]), pt);
        const int first = reroute::same_point(pt, w0) ? 1 : 0;
        reroute::node_point(g, reroute::node_id(g, Z[0], Z[1], Z[2]), pt);
        const int last = nhops - (reroute::same_point(pt, w1) ? 1 : 0);
        const int n = std::max(0, last - first + 1) + 1;  // the targets: path nodes first .. last, then w1
        int32_t cx = A[0] - win.lo[0], cy = A[1] - win.lo[1], cz = A[2] - win.lo[2];
        int pos = 0, anchor = -1, anchors = 0;
        int32_t why = 0, prev_id = TGMS_NEAR_NONE;
        double qanc[3] = {w0[0], w0[1], w0[2]};
        for (int t0 = 0; t0 < n && why == 0; t0 += W64) {
            int32_t my_id = TGMS_NEAR_NONE;
            for (int l = 0; l < W64 && t0 + l < n - 1; ++l) {
                while (pos < first + t0 + l) {  // one step of the descent
                    const int want = (int)dist[reroute::window_index(win, cx, cy, cz)] - 1;
                    int32_t nx, ny, nz;
                    const bool in = reroute::neighbour(win, cx, cy, cz, lane < 6 ? lane : 0, nx, ny, nz);
                    const bool hit = lane < 6 && in && (int)dist[in ? reroute::window_index(win, nx, ny, nz) : 0] == want;
                    const unsigned long long m = __ballot(hit);
                    const int d = m != 0ull ? __ffsll(m) - 1 : 0;
                    if (m != 0ull) reroute::neighbour(win, cx, cy, cz, d, nx, ny, nz), cx = nx, cy = ny, cz = nz;
                    ++pos;
                }
                const int32_t id = reroute::node_id(g, win.lo[0] + cx, win.lo[1] + cy, win.lo[2] + cz);
                my_id = lane == l ? id : my_id;
            }
            const int t = t0 + lane;
            if (t < n - 1) {
                reroute::node_point(g, my_id, pt);
            } else {
                pt[0] = w1[0], pt[1] = w1[1], pt[2] = w1[2];
            }
            for (;;) {
                const bool fail = t < n && t > anchor && !reroute::clear_points(g, table, qanc, pt);
                const unsigned long long m = __ballot(fail);
                if (m == 0ull) break;
                const int fl = __ffsll(m) - 1, f = t0 + fl;
                why = reroute::on_fail(anchor, f, anchors, max_pieces);
                if (why != 0) break;
                const int32_t up = __shfl(my_id, std::max(fl - 1, 0), W64);
                const int32_t aid = fl > 0 ? up : prev_id;
                if (lane == 0) rec->anchor[anchors] = aid;
                ++anchors;
                anchor = f - 1;
                reroute::node_point(g, aid, qanc);
            }
            prev_id = __shfl(my_id, W64 - 1, W64);
        }
        if (lane == 0) {
            rec->head = why != 0 ? reroute::pack_head(1, TGMS_RRT_BLOCKED | why) : reroute::pack_head(anchors + 1, 0);
            if (hops && gs < so[B]) hops[gs] = nhops;
        }
    }
}

// The tile's legs: this lane's record head, its rows once the budget is known, and the budget.
struct LegRows {
    int32_t head;
    int rows, sum;  // rows of this leg; of its trajectory
    bool full;
};
__device__ __forceinline__ LegRows leg_rows(const reroute::Record* __restrict__ recs, const Lane& l) {
    LegRows r;
    r.head = l.mine ? recs[(l.b0 + l.tr) * LEGS + (l.lane - l.sb)].head : 0;
    const int sum = trajectory_sum(reroute::head_pieces(r.head), l.sb, l.M);
    r.full = sum > TGMS_MAX_SEGMENTS;
    r.rows = l.mine ? (r.full ? 1 : reroute::head_pieces(r.head)) : 0;
    r.sum = r.full ? l.M : sum;
    return r;
}

__global__ __launch_bounds__(BLOCK) void k_rrt_count(int32_t B, const int32_t* __restrict__ so,
                                                     const reroute::Record* __restrict__ recs,
                                                     int32_t* __restrict__ cntS, int64_t* __restrict__ cntF,
                                                     int32_t* __restrict__ flags) {
    Lane l;
    if (!wave_tile(B, so, l)) return;
    const LegRows r = leg_rows(recs, l);
    const int32_t fl = l.mine ? reroute::kept_flag(r.head, r.full) : 0;
    constexpr int32_t BITS[7] = {TGMS_RRT_BLOCKED, TGMS_RRT_OUTSIDE, TGMS_FEAS_NONFINITE, TGMS_RRT_WINDOW,
                                 TGMS_RRT_ENDS,    TGMS_RRT_NOPATH,  TGMS_RRT_LONG};
    const int32_t all = (r.full ? TGMS_RRT_FULL : (r.sum > l.M ? TGMS_RRT_DONE : 0)) |
                        trajectory_flags(fl, l.mine, l.sb, l.M, BITS);
    store_plan(l, r.sum, all, cntS, cntF, flags);
}

__global__ void k_rrt_empty(int32_t* __restrict__ so_out, int64_t* __restrict__ totals) { empty_batch(so_out, totals); }

__global__ __launch_bounds__(BLOCK) void k_rrt_write(int32_t B, const int32_t* __restrict__ so,
                                                     const double* __restrict__ W, const double* __restrict__ T,
                                                     inflate::Grid g, int max_pieces,
                                                     const reroute::Record* __restrict__ recs,
                                                     const int32_t* __restrict__ so_out,
                                                     const int64_t* __restrict__ scan_totals,
                                                     double* __restrict__ W_out, double* __restrict__ T_out,
                                                     int32_t* __restrict__ parent, int32_t* __restrict__ seg_flags,
                                                     int64_t* __restrict__ totals) {
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[0] = scan_totals[0];
    Lane l;
    if (!wave_tile(B, so, l)) return;
    // the capacities of the caller's buffers (include/tgms.h)
    const int64_t capS = std::min<int64_t>((int64_t)so[B] * max_pieces, (int64_t)TGMS_MAX_SEGMENTS * B), capW = capS + B;
    // as a leg: this lane's rows; as an output row: piece r.at of leg r.leg
    const LegRows mr = leg_rows(recs, l);
    const Row r = row_map(l, mr.rows, so_out);
    const int32_t lhead = __shfl(mr.head, r.leg, W64);
    const int lfull = __shfl((int)mr.full, r.leg, W64);
    const int lrows = __shfl(mr.rows, r.leg, W64);
    placeholder_rows(l, r, capS, capW, W_out, T_out, parent, seg_flags);
    if (!r.live) return;
    const int64_t b = l.b0 + r.ltr;
    const int q = l.lane - r.tbase, piece = r.at;  // the row within its trajectory, within its leg
    const int64_t orow = r.so2 + q;
    const reroute::Record* rec = recs + (b * LEGS + (r.leg - r.lsb));
    const double* w = W + (r.lgs + b) * 3;  // the leg's rows s + b and s + b + 1
    const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
    double a[3] = {w0[0], w0[1], w0[2]}, e[3] = {w1[0], w1[1], w1[2]};
    if (piece > 0) reroute::node_point(g, rec->anchor[piece - 1], a);
    if (piece < lrows - 1) reroute::node_point(g, rec->anchor[piece], e);
    if (orow + b < capW) copy3(W_out + (orow + b) * 3, a);
    if (q == r.tcnt - 1 && orow + 1 + b < capW) copy3(W_out + (orow + 1 + b) * 3, w1);  // the trajectory's last waypoint
    if (orow < capS) {
        if (T_out) {
            const double Ts = T[r.lgs];
            T_out[orow] = lrows > 1 ? reroute::piece_time(Ts, reroute::length(a, e), reroute::length(w0, w1)) : Ts;
        }
        if (parent) parent[orow] = (int32_t)r.lgs;
        if (seg_flags) seg_flags[orow] = lrows > 1 ? 0 : reroute::kept_flag(lhead, lfull != 0);
    }
}

struct Scratch : ScanScratch {
    int32_t *cntS, *count, *list;
    reroute::Record* recs;
    Scratch(int32_t B, void* base) : ScanScratch(B, base, true) {
        cntS = take<int32_t>(n);
        count = take<int32_t>(1);
        list = take<int32_t>(n * LEGS);
        recs = take<reroute::Record>(n * LEGS);
    }
};

}  // namespace

size_t reroute_scratch_bytes(int32_t B) { return Scratch(B, nullptr).off; }

hipError_t reroute_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_rrt_search), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)SEARCH_LDS);
}

hipError_t launch_reroute(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const tgms_field& fld,
                          const int32_t* table, int32_t margin, int32_t max_pieces, void* scratch, int32_t* so_out,
                          double* W_out, double* T_out, int32_t* parent, int32_t* seg_flags, int32_t* hops,
                          int64_t* totals, int32_t* flags, hipStream_t stream) {
    if (B <= 0) {
        TGMS_LAUNCH(k_rrt_empty, dim3(1), dim3(W64), 0, stream, so_out, totals);
        return hipSuccess;
    }
    const Scratch s(B, scratch);
    const inflate::Grid g = inflate::make_grid(fld);
    const unsigned blocks = wave_tile_blocks(B);
    if (const hipError_t e = hipMemsetAsync(s.count, 0, sizeof(int32_t), stream); e != hipSuccess) return e;
    TGMS_LAUNCH(k_rrt_classify, dim3(blocks), dim3(BLOCK), 0, stream, B, seg_offsets, W, g, table, s.recs, s.list, s.count,
                hops);
    TGMS_LAUNCH(k_rrt_search, dim3(SEARCH_BLOCKS), dim3(SEARCH_THREADS), SEARCH_LDS, stream, B, seg_offsets, W, g, table,
                margin, (int)max_pieces, s.recs, s.list, s.count, hops);
    TGMS_LAUNCH(k_rrt_count, dim3(blocks), dim3(BLOCK), 0, stream, B, seg_offsets, s.recs, s.cntS, s.cntF, flags);
    if (const hipError_t e = launch_count_scan(B, s.cntS, s.cntF, s.sumS, s.sumF, 0, so_out, s.totals, stream);
        e != hipSuccess)
        return e;
    TGMS_LAUNCH(k_rrt_write, dim3(blocks), dim3(BLOCK), 0, stream, B, seg_offsets, W, T, g, (int)max_pieces, s.recs, so_out,
                s.totals, W_out, T_out, parent, seg_flags, totals);
    return hipSuccess;
}

}  // namespace tgms
