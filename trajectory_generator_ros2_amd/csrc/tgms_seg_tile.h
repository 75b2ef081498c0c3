// tgms_seg_tile.h — the segment tile of the compactions (tgms_corridor_split.hip, tgms_cut.hip):
// a wavefront per TILE = 4 trajectories, one lane per segment.  Device code only.
#pragma once

#include <algorithm>

#include "tgms_device.h"

namespace tgms {
namespace seg_tile {

constexpr int TILE = 4;                         // trajectories of one wavefront
constexpr int SEGS = TILE * TGMS_MAX_SEGMENTS;  // 64: one lane per segment
static_assert(SEGS == W64, "the segments of a tile are one pass of the wavefront");

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

}  // namespace seg_tile
}  // namespace tgms
