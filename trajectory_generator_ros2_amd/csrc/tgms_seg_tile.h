// tgms_seg_tile.h — the segment tile: a wavefront per TILE = 4 trajectories, one lane per segment,
// and everything the kernels over it share that is mapping and not decision.  Device code but
// for wave_tile_blocks.
//   - the tile and a lane's segment in it (Tile, load_tile, lane_segment, lane_knot): every user;
//   - sums and flag folds over a trajectory's lanes (wave_inclusive, trajectory_sum,
//     trajectory_flags, store_flags);
//   - the 256-thread shape with a tile per wavefront, no LDS and no barrier (Lane, wave_tile,
//     wave_tile_blocks): k_inflate, k_repair and the plan, count and write kernels of
//     tgms_subdivide.hip and tgms_reroute.hip.  The split and the cut (tgms_corridor_split.hip,
//     tgms_cut.hip) walk tiles by grid-stride with one wavefront a workgroup and keep their own
//     loops and placeholder rows;
//   - the rebuild of a batch whose legs each become 1..16 rows, a lane per OUTPUT row (Row,
//     row_map, placeholder_rows), and what a plan stores for it (store_plan, plan_placeholder);
//   - empty_batch and copy3.
// Every shuffle and ballot in here is executed by all 64 lanes: call these functions from
// wave-uniform control flow only, before any `if (!live) return`.
#pragma once

#include <algorithm>

#include "tgms_device.h"

namespace tgms {
namespace seg_tile {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment
static_assert(SEGS == W64, "the segments of a tile are one pass of the wavefront");
constexpr int BLOCK = 256;          // threads of a workgroup of the tile-per-wavefront kernels
constexpr int WAVES = BLOCK / W64;  // its wavefronts

// Wave-uniform: the tile's trajectories, their segment counts (0: outside 1..16, nothing is
// read) and lane bases.
struct Tile {
    int Mt[TILE], base[TILE + 1];
    int64_t s0[TILE];
    bool oob[TILE];  // a segment count outside 1..TGMS_MAX_SEGMENTS
};

__device__ __forceinline__ void load_tile(const int32_t* __restrict__ so, int64_t b0, int nb, Tile& x) {
    x.base[0] = 0;
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
        int M = 0;
        x.s0[t] = 0;
        x.oob[t] = false;
        if (t < nb) {
            const int32_t a = __builtin_amdgcn_readfirstlane(so[b0 + t]);
            M = __builtin_amdgcn_readfirstlane(so[b0 + t + 1]) - a;
            x.s0[t] = a;
            x.oob[t] = M < 1 || M > TGMS_MAX_SEGMENTS;
        }
        x.Mt[t] = (M < 1 || M > TGMS_MAX_SEGMENTS) ? 0 : M;
        x.base[t + 1] = x.base[t] + x.Mt[t];
    }
}

// This lane's segment: its trajectory in the tile, its first lane, its segment count, its row.
__device__ __forceinline__ void lane_segment(const Tile& x, int lane, int& tr, int& sb, int& M, int64_t& gs) {
    tr = 0;
#pragma unroll
    for (int t = 1; t < TILE; ++t) tr += lane >= x.base[t] ? 1 : 0;
    sb = x.base[0];
    M = x.Mt[0];
    gs = x.s0[0] + lane;
#pragma unroll
    for (int t = 1; t < TILE; ++t) {
        sb = tr == t ? x.base[t] : sb;
        M = tr == t ? x.Mt[t] : M;
        gs = tr == t ? x.s0[t] + (lane - x.base[t]) : gs;
    }
}

// The knot of this lane's segment: the times of the trajectory's earlier segments added left
// to right, the corridor call's prefix sum.
__device__ __forceinline__ double lane_knot(double T, int sb, int li) {
    double knot = 0.0;
#pragma unroll
    for (int j = 0; j < TGMS_MAX_SEGMENTS - 1; ++j) {
        const double Tj = __shfl(T, std::min(sb + j, W64 - 1), W64);
        knot = j < li ? knot + Tj : knot;
    }
    return knot;
}

// The sum of v over the lanes up to and including this one.
__device__ __forceinline__ int wave_inclusive(int v, int lane) {
#pragma unroll
    for (int o = 1; o < W64; o <<= 1) {
        const int up = __shfl_up(v, o, W64);
        v += lane >= o ? up : 0;
    }
    return v;
}

// The sum of v over the lanes sb .. sb + M - 1 of this lane's trajectory.
__device__ __forceinline__ int trajectory_sum(int v, int sb, int M) {
    int tot = 0;
#pragma unroll
    for (int j = 0; j < TGMS_MAX_SEGMENTS; ++j) {
        const int x = __shfl(v, std::min(sb + j, W64 - 1), W64);
        tot += j < M ? x : 0;
    }
    return tot;
}

// The OR of fl over the lanes of this lane's trajectory, one ballot per bit of `bits`.
template <int N>
__device__ __forceinline__ int32_t trajectory_flags(int32_t fl, bool mine, int sb, int M, const int32_t (&bits)[N]) {
    const unsigned long long span = mine ? ((1ull << M) - 1ull) << sb : 0ull;  // M <= 16
    int32_t all = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) all |= (__ballot((fl & bits[i]) != 0) & span) != 0ull ? bits[i] : 0;
    return all;
}

// A lane of a BLOCK-thread workgroup whose wavefronts have a tile each: the tile x of the
// trajectories b0 .. b0 + nb - 1 and lane_segment's answers; mine: the lane has a segment.
struct Lane {
    int lane, wave, nb, tr, sb, M;
    int64_t b0, gs;
    bool mine;
    Tile x;
};

// false: the whole wavefront is beyond the batch.
__device__ __forceinline__ bool wave_tile(int32_t B, const int32_t* __restrict__ so, Lane& l) {
    l.lane = threadIdx.x & (W64 - 1);
    l.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    l.b0 = ((int64_t)blockIdx.x * WAVES + l.wave) * TILE;
    if (l.b0 >= B) return false;
    l.nb = (int)std::min<int64_t>(TILE, B - l.b0);
    load_tile(so, l.b0, l.nb, l.x);
    lane_segment(l.x, l.lane, l.tr, l.sb, l.M, l.gs);
    l.mine = l.lane < l.x.base[TILE];
    return true;
}
inline unsigned wave_tile_blocks(int32_t B) {  // the grid that gives every tile a wavefront
    return (unsigned)((((int64_t)B + TILE - 1) / TILE + WAVES - 1) / WAVES);
}

// The flags of a call that rebuilds nothing (nullable): a trajectory's by its first lane,
// TGMS_FEAS_NONFINITE for a bad count, of which nothing was read.
__device__ __forceinline__ void store_flags(const Lane& l, int32_t all, int32_t* __restrict__ flags) {
    if (!flags) return;
    if (l.mine && l.lane == l.sb) flags[l.b0 + l.tr] = all;
#pragma unroll
    for (int t = 0; t < TILE; ++t)
        if (l.x.oob[t] && l.lane == t) flags[l.b0 + t] = TGMS_FEAS_NONFINITE;
}

// Trajectory b has a bad count: the plan is one placeholder segment; nothing of it is read.
__device__ __forceinline__ void plan_placeholder(int64_t b, int32_t* __restrict__ cntS, int64_t* __restrict__ cntF,
                                                 int32_t* __restrict__ flags) {
    cntS[b] = 1;
    cntF[b] = 0;
    if (flags) flags[b] = TGMS_FEAS_NONFINITE;
}

// What a plan leaves per trajectory for launch_count_scan: its new segment count (the scan's
// second lane of counts is zero) and its flags, stored by its first lane.
__device__ __forceinline__ void store_plan(const Lane& l, int count, int32_t all, int32_t* __restrict__ cntS,
                                           int64_t* __restrict__ cntF, int32_t* __restrict__ flags) {
    if (l.mine && l.lane == l.sb) {
        cntS[l.b0 + l.tr] = count;
        cntF[l.b0 + l.tr] = 0;
        if (flags) flags[l.b0 + l.tr] = all;
    }
#pragma unroll
    for (int t = 0; t < TILE; ++t)
        if (l.x.oob[t] && l.lane == t) plan_placeholder(l.b0 + t, cntS, cntF, flags);
}

// A lane as OUTPUT row `lane` of its tile, where leg j of the tile becomes cnt_j consecutive rows
// (64 at the most: TGMS_MAX_SEGMENTS a trajectory).  leg: the lane of the row's leg, for the
// caller to shuffle that leg's own words from; at: the row within the leg; ltr, lsb, lgs:
// lane_segment of the leg; tbase, tcnt: the first row of the row's trajectory in the tile and
// its rows; so2: that trajectory's first row afterwards; so: so_out of the tile (wave-uniform).
struct Row {
    bool live;
    int leg, at, ltr, lsb, tbase, tcnt;
    int64_t lgs, so2;
    int32_t so[TILE];
};

__device__ __forceinline__ Row row_map(const Lane& l, int cnt, const int32_t* __restrict__ so_out) {
    Row r;
    const int inc = wave_inclusive(cnt, l.lane);
    const int total = __shfl(inc, W64 - 1, W64);
    // the leg whose rows hold row `lane` is the number of legs whose inclusive count is at most `lane`
    int leg = 0;
#pragma unroll
    for (int step = W64 / 2; step >= 1; step >>= 1) {
        const int v = __shfl(inc, leg + step - 1, W64);
        leg += v <= l.lane ? step : 0;
    }
    r.live = l.lane < total;
    r.leg = std::min(leg, W64 - 1);
    r.at = l.lane - __shfl(inc - cnt, r.leg, W64);
    int lM;
    lane_segment(l.x, r.leg, r.ltr, r.lsb, lM, r.lgs);
    r.tbase = r.tcnt = 0;
    r.so2 = 0;
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
        r.so[t] = 0;
        if (t >= l.nb) continue;
        r.so[t] = __builtin_amdgcn_readfirstlane(so_out[l.b0 + t]);
        const int hi = l.x.base[t + 1] > 0 ? __shfl(inc, l.x.base[t + 1] - 1, W64) : 0;
        const int lo = l.x.base[t] > 0 ? __shfl(inc, l.x.base[t] - 1, W64) : 0;
        r.tbase = r.ltr == t ? lo : r.tbase;
        r.tcnt = r.ltr == t ? hi - lo : r.tcnt;
        r.so2 = r.ltr == t ? (int64_t)r.so[t] : r.so2;
    }
    return r;
}

// The row of a segment count outside 1..16: one placeholder segment, a NaN time, two NaN
// waypoints; the solve that follows rejects this row alone.  capS, capW: the capacities of the
// caller's segment and waypoint buffers; T_out, parent and seg_flags nullable.
__device__ __forceinline__ void placeholder_rows(const Lane& l, const Row& r, int64_t capS, int64_t capW,
                                                 double* __restrict__ W_out, double* __restrict__ T_out,
                                                 int32_t* __restrict__ parent, int32_t* __restrict__ seg_flags) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
        if (!(l.x.oob[t] && l.lane == 0)) continue;
        const int64_t w0 = r.so[t] + l.b0 + t;
        if (r.so[t] < capS) {
            if (T_out) T_out[r.so[t]] = nan;
            if (parent) parent[r.so[t]] = TGMS_NEAR_NONE;
            if (seg_flags) seg_flags[r.so[t]] = TGMS_FEAS_NONFINITE;
        }
        for (int e = 0; e < 6; ++e)
            if (w0 + e / 3 < capW) W_out[w0 * 3 + e] = nan;
    }
}

// The whole output of a call on an empty batch, by one thread.
__device__ __forceinline__ void empty_batch(int32_t* __restrict__ so_out, int64_t* __restrict__ totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        so_out[0] = 0;
        totals[0] = 0;
    }
}

__device__ __forceinline__ void copy3(double* __restrict__ dst, const double* __restrict__ src) {
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

}  // namespace seg_tile
}  // namespace tgms
