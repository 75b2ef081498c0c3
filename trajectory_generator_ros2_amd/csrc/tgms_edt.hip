// tgms_edt.hip — distance-field build (tgms_field_edt_device) on gfx950: the exact Euclidean
// distance transform of an occupancy grid.  include/tgms.h has the result to the bit,
// tgms_edt_core.h the cap, the saturation argument and the conversion of a square into a value,
// tgms_sep_pass.h the passes themselves.
//
// The separable transform on int32 squares, three launches per transform (one transform for the
// unsigned mode; the signed mode runs a second one on the complement, which writes the occupied
// nodes):
//   - k_edt_rows: a wavefront per row (j, k), rows by grid-stride.  A node is a target by its
//     occupancy byte; a node stores min(g^2, K) of the nearer of its two targets.
//   - k_edt_lines<false> (y) and k_edt_lines<true> (z, which also converts): the min-plus over
//     the squares as they are.  A 128^3 map gives 1,024 workgroups = 4,096 wavefronts a pass, four
//     per SIMD.
// The passes ping-pong between the two halves of the caller's workspace (2 N int32), so no tile
// needs to own whole lines.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_edt_core.h"
#include "tgms_internal.h"
#include "tgms_sep_pass.h"

namespace tgms {
namespace {

using namespace sep_pass;

__global__ __launch_bounds__(BLOCK) void k_edt_rows(const uint8_t* __restrict__ occ, int32_t nx, int64_t rows,
                                                    int32_t complement, int32_t R, int32_t K,
                                                    int32_t* __restrict__ out) {
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const uint8_t* const in = occ + row * nx;
        int32_t* const o = out + row * nx;
        row_sweep(
            nx, lane, wave, [&](int32_t i) { return (in[i] != 0) != (complement != 0); },
            [&](int32_t i, int32_t dl, int32_t dr) {
                const int32_t g = dl < dr ? dl : dr;
                o[i] = g > R ? K : g * g;
            });
    }
}

// out = min(min over j' of in[j'] + (j - j')^2, K) along every line; LAST: the square goes
// through edt::value / edt::squared into the outputs instead, in the signed mode only at the
// nodes this transform is for (the free ones, or with `complement` the occupied ones, negated).
template <bool LAST>
__global__ __launch_bounds__(BLOCK) void k_edt_lines(const int32_t* __restrict__ in, Lines ln, int32_t R, int32_t K,
                                                     int32_t tiles_j, int32_t* __restrict__ out, edt::Conv cv,
                                                     const uint8_t* __restrict__ occ, int32_t complement,
                                                     float* __restrict__ values, int32_t* __restrict__ d2) {
    const LineLane p = line_lane(ln, tiles_j);
    int32_t acc[LINE_U];
    line_pass<false>(in, ln, p, R, K, K, [](int32_t v) { return v; }, acc, nullptr);
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) {
        const int32_t j = p.jw + u;
        if (!p.valid || j >= ln.n) continue;
        const int64_t node = p.base + (int64_t)j * ln.step;
        if (!LAST) {
            out[node] = acc[u];
        } else {
            if (cv.is_signed && (occ[node] != 0) != (complement != 0)) continue;
            const float val = edt::value(cv, acc[u]);
            const int32_t sq = edt::squared(cv, acc[u]);
            if (values) values[node] = complement ? -val : val;
            if (d2) d2[node] = complement ? -sq : sq;
        }
    }
}

}  // namespace

size_t edt_work_bytes(const tgms_field& fld) {
    return 2 * sizeof(int32_t) * (size_t)fld.n[0] * (size_t)fld.n[1] * (size_t)fld.n[2];
}

hipError_t launch_edt(const tgms_field& fld, const uint8_t* occ, double max_dist, bool is_signed, float* values,
                      int32_t* d2, void* work, hipStream_t stream) {
    const edt::Cap cap = edt::make_cap(fld.h, max_dist);
    const edt::Conv cv = edt::make_conv(fld.h, max_dist, cap, is_signed);
    const Geometry g = geometry(fld);
    int32_t* const a = static_cast<int32_t*>(work);
    int32_t* const b = a + g.rows * fld.n[0];  // the second half
    for (int32_t complement = 0; complement < (is_signed ? 2 : 1); ++complement) {
        TGMS_LAUNCH(k_edt_rows, dim3(g.row_blocks), dim3(BLOCK), 0, stream, occ, (int32_t)fld.n[0], g.rows, complement,
                    cap.R, cap.K, a);
        TGMS_LAUNCH(k_edt_lines<false>, dim3(g.by), dim3(BLOCK), 0, stream, a, g.ly, cap.R, cap.K, g.ty, b, cv, nullptr,
                    complement, nullptr, nullptr);
        TGMS_LAUNCH(k_edt_lines<true>, dim3(g.bz), dim3(BLOCK), 0, stream, b, g.lz, cap.R, cap.K, g.tz, nullptr, cv, occ,
                    complement, values, d2);
    }
    return hipSuccess;
}

}  // namespace tgms
