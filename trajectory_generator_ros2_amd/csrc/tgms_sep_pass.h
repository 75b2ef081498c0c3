// tgms_sep_pass.h — the separable pass over a voxel map that the distance-field build
// (tgms_edt.hip) and the nearest-free map (tgms_repair.hip) share: the nearest target along x by
// two ballot sweeps, then a min-plus along y and along z over an LDS tile.  Integers throughout:
// no order of evaluation can change a bit.  What a target is, what is stored from a row and what
// a line's result becomes stay with the kernels.
#pragma once

#include <algorithm>

#include "tgms_device.h"
#include "tgms_edt_core.h"

namespace tgms {
namespace sep_pass {

constexpr int BLOCK = 256;               // threads of every workgroup of the pass
constexpr int WAVES = BLOCK / W64;       // its wavefronts
constexpr int32_t MAX_BLOCKS = 256 * 8;  // the row kernels grid-stride beyond: eight workgroups a CU
constexpr int MAX_CHUNKS = edt::MAX_NODES_PER_AXIS / W64;  // 64-node chunks of the longest row
constexpr int LINE_U = 8;                // outputs of a line a lane owns
constexpr int LINE_JT = WAVES * LINE_U;  // outputs of a line a workgroup owns
constexpr int LINE_CH = 64;              // source entries of a line staged at a time
constexpr int32_t FAR = 1 << 20;         // farther than any cap and any row is long

// Line q of `lines` starts at (q / width) outer + q % width and has n entries `step` apart.
struct Lines {
    int64_t lines, width, outer, step;
    int32_t n;
};

// The launches of one transform: the rows (j, k), the lines along y and along z, their tiles of
// LINE_JT outputs and the three grids.
struct Geometry {
    int64_t rows;
    Lines ly, lz;
    int32_t ty, tz;
    unsigned row_blocks, by, bz;
};
inline Geometry geometry(const tgms_field& fld) {
    const int64_t nx = fld.n[0], ny = fld.n[1], nz = fld.n[2];
    Geometry g;
    g.rows = ny * nz;
    g.row_blocks = (unsigned)std::min<int64_t>((g.rows + WAVES - 1) / WAVES, MAX_BLOCKS);
    g.ly = {nx * nz, nx, nx * ny, nx, (int32_t)ny};
    g.lz = {nx * ny, nx * ny, 0, nx * ny, (int32_t)nz};
    g.ty = (int32_t)((ny + LINE_JT - 1) / LINE_JT);
    g.tz = (int32_t)((nz + LINE_JT - 1) / LINE_JT);
    g.by = (unsigned)(((g.ly.lines + W64 - 1) / W64) * g.ty);
    g.bz = (unsigned)(((g.lz.lines + W64 - 1) / W64) * g.tz);
    return g;
}

// One row of nx nodes by one wavefront of a BLOCK-thread workgroup, 64 nodes a ballot.  A sweep
// from the row's end keeps per 64-node chunk its ballot of target(i) and the first target beyond
// it in LDS; the sweep from the row's start then hands every node i < nx to store(i, dl, dr): its
// distance to the nearest target at or to the left of it (the leading zeros of the ballot masked
// to the lanes up to it, else the scalar carry of the last target before the chunk) and at or to
// the right of it (the trailing zeros, else the kept index); beyond FAR: there is none.
template <class Target, class Store>
__device__ __forceinline__ void row_sweep(int32_t nx, int lane, int wave, Target target, Store store) {
    // a wavefront's own slices; every lane stores the same word, so each reads what it wrote
    __shared__ unsigned long long s_mask[WAVES][MAX_CHUNKS];
    __shared__ int32_t s_next[WAVES][MAX_CHUNKS];
    const int32_t chunks = (nx + W64 - 1) / W64;
    int32_t next = 2 * FAR;  // the first target beyond the chunk
    for (int32_t c = chunks - 1; c >= 0; --c) {
        const int32_t i = c * W64 + lane;
        const unsigned long long m = __ballot(i < nx && target(i));
        s_mask[wave][c] = m;
        s_next[wave][c] = next;
        if (m != 0ull) next = c * W64 + __builtin_ctzll(m);
    }
    int32_t last = -FAR;  // the last target before the chunk
    for (int32_t c = 0; c < chunks; ++c) {
        const unsigned long long m = s_mask[wave][c];
        const int32_t i = c * W64 + lane;
        const unsigned long long le = m & ((2ull << lane) - 1ull), ge = m & (~0ull << lane);
        const int32_t dl = le != 0ull ? lane - (63 - __builtin_clzll(le)) : i - last;
        const int32_t dr = ge != 0ull ? __builtin_ctzll(ge) - lane : s_next[wave][c] - i;
        if (i < nx) store(i, dl, dr);
        if (m != 0ull) last = c * W64 + 63 - __builtin_clzll(m);
    }
}

// A lane of a line kernel: line q (base: its first entry; valid: it exists), the workgroup's
// first output j0 of the line and the wavefront's, jw.  Consecutive lanes sit on consecutive
// lines, so every load and store of a wavefront is contiguous.
struct LineLane {
    int lane, wave;
    int64_t q, base;
    int32_t j0, jw;
    bool valid;
};
__device__ __forceinline__ LineLane line_lane(const Lines& ln, int32_t tiles_j) {
    LineLane p;
    p.lane = threadIdx.x & (W64 - 1);
    p.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    p.q = (int64_t)(blockIdx.x / (unsigned)tiles_j) * W64 + p.lane;
    p.j0 = (int32_t)(blockIdx.x % (unsigned)tiles_j) * LINE_JT;
    p.valid = p.q < ln.lines;
    p.base = p.valid ? (p.q / ln.width) * ln.outer + p.q % ln.width : 0;
    p.jw = p.j0 + p.wave * LINE_U;
    return p;
}

// The min-plus of a workgroup: LINE_JT consecutive outputs of 64 neighbouring lines.  It walks the
// source entries max(0, j0 - R) .. min(n, j0 + LINE_JT + R) of its lines LINE_CH at a time: the
// four wavefronts stage stage(entry) of 64 entries x 64 lines in LDS (`none` for an entry that is
// not there; [entry][line], so a wavefront's read of one entry is 64 consecutive words: no bank
// conflict at any stride), then each lane folds every staged entry j' into its LINE_U outputs
// j_u = jw + u: acc[u] = min(acc[u], f + (j' - j_u)^2) from K, the square a scalar.  CARRY: src[u]
// (LINE_U entries, else unused) is the entry acc[u] came from, -1 for none.
// The contract: the entries are walked in ascending order and an entry replaces the kept one only
// when its sum is strictly less, so of equal sums the lowest entry stays, whatever the tiling;
// and every staged chunk has two barriers, one before its first read and one after its last.
template <bool CARRY, class Stage>
__device__ __forceinline__ void line_pass(const int32_t* __restrict__ in, const Lines& ln, const LineLane& p, int32_t R,
                                          int32_t K, int32_t none, Stage stage, int32_t (&acc)[LINE_U], int32_t* src) {
    __shared__ int32_t tile[LINE_CH][W64];
    const int32_t s_lo = std::max(0, p.j0 - R), s_hi = std::min(ln.n, p.j0 + LINE_JT + R);
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) {
        acc[u] = K;
        if (CARRY) src[u] = -1;
    }
    for (int32_t s = s_lo; s < s_hi; s += LINE_CH) {
        const int32_t staged = std::min(LINE_CH, s_hi - s);
        int32_t v[LINE_CH / WAVES];
#pragma unroll
        for (int u = 0; u < LINE_CH / WAVES; ++u) {
            const int32_t r = p.wave + u * WAVES;
            v[u] = p.valid && r < staged ? in[p.base + (int64_t)(s + r) * ln.step] : none;
        }
#pragma unroll
        for (int u = 0; u < LINE_CH / WAVES; ++u) tile[p.wave + u * WAVES][p.lane] = stage(v[u]);
        __syncthreads();
        int32_t d = s - p.jw;  // source index less output index, a scalar
#pragma unroll 4
        for (int32_t r = 0; r < staged; ++r, ++d) {
            const int32_t f = tile[r][p.lane];
#pragma unroll
            for (int u = 0; u < LINE_U; ++u) {
                const int32_t e = d - u, c = f + e * e;
                if (CARRY) src[u] = c < acc[u] ? s + r : src[u];
                acc[u] = std::min(acc[u], c);
            }
        }
        __syncthreads();
    }
}

}  // namespace sep_pass
}  // namespace tgms
