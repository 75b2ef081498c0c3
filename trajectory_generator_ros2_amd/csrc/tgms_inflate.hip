// tgms_inflate.hip — corridor inflation (tgms_field_occupancy_device,
// tgms_corridor_inflate_batch_device) on gfx950.  include/tgms.h has the result to the bit,
// tgms_inflate_core.h the seed, the eight-corner count and the growth loop.
//
// The table, three launches:
//   - k_occ_rows: a wavefront per table row (j, k), rows by grid-stride.  A row of the border
//     planes j = 0 or k = 0 is zeroed; any other row is the inclusive scan along x of the
//     threshold mask of value row (j - 1, k - 1), 64 nodes a pass: coalesced 4-byte loads, a
//     six-step shuffle scan, the carry in a scalar, coalesced stores one entry to the right
//     (entry 0 of the row is the zero of the plane i = 0).
//   - k_occ_lines, twice: a lane per line, consecutive lanes on consecutive x.  The y pass gives
//     a lane the ny entries (i, 1..ny, k) and adds each to the running sum of those before it,
//     the z pass the nz entries (i, j, 1..nz); a lane loads LINE_UNROLL entries of its line
//     before it adds and stores them, so the loads of a step are in flight together and every
//     wave-instruction moves 256 contiguous bytes.  Integer sums: no order can change a bit.
//
// k_inflate: a lane per segment (wave_tile of tgms_seg_tile.h), so a lane knows its trajectory
// and with it its waypoint rows s + b and s + b + 1.  A lane runs its segment's growth alone:
// every slab test is eight 4-byte gathers from the table issued together and one count, at most
// 6 max_grow of them one after the other.  What the kernel waits for is those gathers; only
// other wavefronts hide them, so the registers are kept to full occupancy (DESIGN.md has the
// counts).
#include <algorithm>

#include "tgms_device.h"
#include "tgms_inflate_core.h"
#include "tgms_internal.h"
#include "tgms_seg_tile.h"

namespace tgms {
namespace {

using namespace seg_tile;  // BLOCK and WAVES are k_occ_rows' too

constexpr int LINE_UNROLL = 8;            // entries of a line a lane has in flight
constexpr int32_t MAX_BLOCKS = 256 * 8;   // grid-stride beyond: eight workgroups a CU

__global__ __launch_bounds__(BLOCK) void k_occ_rows(inflate::Grid g, const float* __restrict__ values, float r_free,
                                                    int32_t* __restrict__ table) {
    const int lane = threadIdx.x & (W64 - 1);
    const int32_t nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int64_t rows = (int64_t)(ny + 1) * (nz + 1);
    for (int64_t row = (int64_t)blockIdx.x * WAVES + threadIdx.x / W64; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const int32_t k = (int32_t)(row / (ny + 1)), j = (int32_t)(row - (int64_t)k * (ny + 1));
        int32_t* const out = table + row * (nx + 1);
        if (j == 0 || k == 0) {
            for (int32_t i = lane; i <= nx; i += W64) out[i] = 0;
            continue;
        }
        const float* const in = values + ((int64_t)(k - 1) * ny + (j - 1)) * nx;
        if (lane == 0) out[0] = 0;
        int32_t carry = 0;
        for (int32_t c0 = 0; c0 < nx; c0 += W64) {
            const int32_t i = c0 + lane;
            int32_t inc = (i < nx && !inflate::node_free(in[i], r_free)) ? 1 : 0;
#pragma unroll
            for (int o = 1; o < W64; o <<= 1) {
                const int32_t up = __shfl_up(inc, o, W64);
                inc += lane >= o ? up : 0;
            }
            if (i < nx) out[i + 1] = carry + inc;
            carry += __shfl(inc, W64 - 1, W64);
        }
    }
}

// Line q = (q / width, q % width) starts at first + (q / width) outer + q % width and has
// `count` entries `step` apart; entry e becomes the sum of the entries up to it.
__global__ __launch_bounds__(W64) void k_occ_lines(int32_t* __restrict__ table, int64_t lines, int32_t width,
                                                   int64_t first, int64_t outer, int64_t step, int32_t count) {
    const int64_t q = (int64_t)blockIdx.x * W64 + threadIdx.x;
    if (q >= lines) return;
    int32_t* p = table + first + (q / width) * outer + q % width;
    int32_t run = 0;
    for (int32_t e0 = 0; e0 < count; e0 += LINE_UNROLL) {
        int32_t v[LINE_UNROLL];
#pragma unroll
        for (int u = 0; u < LINE_UNROLL; ++u) v[u] = e0 + u < count ? p[u * step] : 0;
#pragma unroll
        for (int u = 0; u < LINE_UNROLL; ++u) {
            run += v[u];
            if (e0 + u < count) p[u * step] = run;
        }
        p += LINE_UNROLL * step;
    }
}

__global__ __launch_bounds__(BLOCK) void k_inflate(int32_t B, const int32_t* __restrict__ seg_offsets,
                                                   const double* __restrict__ W, inflate::Grid g,
                                                   const int32_t* __restrict__ table, int32_t max_grow,
                                                   int32_t* __restrict__ box, double* __restrict__ faces,
                                                   int64_t* __restrict__ face_offsets, int32_t* __restrict__ seg_flags,
                                                   int32_t* __restrict__ flags) {
    Lane l;
    if (!wave_tile(B, seg_offsets, l)) return;
    const int64_t gs = l.gs;
    int32_t fl = 0;
    if (l.mine) {
        const double* w = W + (gs + l.b0 + l.tr) * 3;  // rows s + b and s + b + 1
        const double w0[3] = {w[0], w[1], w[2]}, w1[3] = {w[3], w[4], w[5]};
        int32_t bx[6];
        double fc[6];
        fl = inflate::segment(g, table, w0, w1, max_grow, bx, fc);
        if (box) {
#pragma unroll
            for (int d = 0; d < 6; ++d) box[gs * 6 + d] = bx[d];  // an int32 array: 4-byte aligned is all it is
        }
        if (faces) {
            double2* const out = reinterpret_cast<double2*>(faces + gs * 24);
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                double row[4];
                inflate::face_row(d, fc[d], row);
                out[2 * d] = make_double2(row[0], row[1]);
                out[2 * d + 1] = make_double2(row[2], row[3]);
            }
        }
        if (face_offsets) {
            face_offsets[gs] = 6 * gs;
            if (l.b0 + l.tr == B - 1 && l.lane - l.sb == l.M - 1) face_offsets[gs + 1] = 6 * (gs + 1);
        }
        if (seg_flags) seg_flags[gs] = fl;
    }
    constexpr int32_t BITS[4] = {TGMS_INF_BLOCKED, TGMS_INF_OUTSIDE, TGMS_INF_CAPPED, TGMS_FEAS_NONFINITE};
    store_flags(l, trajectory_flags(fl, l.mine, l.sb, l.M, BITS), flags);
}

}  // namespace

hipError_t launch_field_occupancy(const tgms_field& fld, const float* values, double r_free, int32_t* table,
                                  hipStream_t stream) {
    const inflate::Grid g = inflate::make_grid(fld);
    const int64_t w = fld.n[0] + 1, wy = fld.n[1] + 1, rows = wy * (fld.n[2] + 1);
    const int32_t blocks = (int32_t)std::min<int64_t>((rows + WAVES - 1) / WAVES, MAX_BLOCKS);
    TGMS_LAUNCH(k_occ_rows, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, g, values, (float)r_free, table);
    const int64_t first = (wy + 1) * w;  // entry (0, 1, 1)
    const int64_t ylines = w * fld.n[2], zlines = w * fld.n[1];
    TGMS_LAUNCH(k_occ_lines, dim3((unsigned)((ylines + W64 - 1) / W64)), dim3(W64), 0, stream, table, ylines,
                (int32_t)w, first, wy * w, w, fld.n[1]);
    TGMS_LAUNCH(k_occ_lines, dim3((unsigned)((zlines + W64 - 1) / W64)), dim3(W64), 0, stream, table, zlines,
                (int32_t)w, first, w, wy * w, fld.n[2]);
    return hipSuccess;
}

hipError_t launch_inflate(int32_t B, const int32_t* seg_offsets, const double* W, const tgms_field& fld,
                          const int32_t* table, int32_t max_grow, int32_t* box, double* faces, int64_t* face_offsets,
                          int32_t* seg_flags, int32_t* flags, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    TGMS_LAUNCH(k_inflate, dim3(wave_tile_blocks(B)), dim3(BLOCK), 0, stream, B, seg_offsets, W,
                inflate::make_grid(fld), table, max_grow, box, faces, face_offsets, seg_flags, flags);
    return hipSuccess;
}

}  // namespace tgms
