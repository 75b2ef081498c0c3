// tgms_edt.hip — distance-field build (tgms_field_edt_device) on gfx950: the exact Euclidean
// distance transform of an occupancy grid.  include/tgms.h has the result to the bit,
// tgms_edt_core.h the cap, the saturation argument and the conversion of a square into a value.
//
// The separable transform on int32 squares, three launches per transform (one transform for the
// unsigned mode; the signed mode runs a second one on the complement, which writes the occupied
// nodes):
//   - k_edt_rows: a wavefront per row (j, k), rows by grid-stride.  64 occupancy bytes make one
//     ballot.  A sweep from the row's end keeps per 64-node chunk its ballot and the first target
//     beyond it in LDS; the sweep from the row's start then gives every lane its nearest target
//     to the left (the leading zeros of the ballot masked to the lanes up to it, else the scalar
//     carry of the last target before the chunk) and to the right (the trailing zeros, else the
//     kept index), and stores min(g^2, K).
//   - k_edt_lines<false> (y) and k_edt_lines<true> (z, which also converts): a whole-line or
//     windowed min-plus over an LDS tile.  A workgroup owns LINE_JT = 32 consecutive outputs of
//     64 neighbouring lines; consecutive lanes sit on consecutive lines, which are consecutive x
//     (in the z pass consecutive nodes of a plane), so every load and store of a wavefront is
//     contiguous.  It walks the source entries max(0, j0 - R) .. min(n, j0 + 32 + R) of its lines
//     LINE_CH = 64 at a time: the four wavefronts stage 64 entries x 64 lines in LDS ([entry]
//     [line], so a wavefront's read of one entry is 64 consecutive words: no bank conflict at any
//     stride), then each wavefront folds every staged entry into the LINE_U = 8 outputs per lane
//     it owns: out_u = min(out_u, f + (j' - j_u)^2), the square a scalar.  One LDS read serves
//     eight outputs.  A 128^3 map gives 1,024 workgroups = 4,096 wavefronts a pass, four per SIMD.
// Integers throughout: no order of evaluation can change a bit.  The passes ping-pong between
// the two halves of the caller's workspace (2 N int32), so no tile needs to own whole lines.
#include <algorithm>

#include "tgms_device.h"
#include "tgms_edt_core.h"
#include "tgms_internal.h"

namespace tgms {
namespace {

constexpr int BLOCK = 256;               // threads of every workgroup here
constexpr int WAVES = BLOCK / W64;       // its wavefronts
constexpr int32_t MAX_BLOCKS = 256 * 8;  // k_edt_rows grid-strides beyond: eight workgroups a CU
constexpr int MAX_CHUNKS = edt::MAX_NODES_PER_AXIS / W64;  // 64-node chunks of the longest row
constexpr int LINE_U = 8;                // outputs of a line a lane owns
constexpr int LINE_JT = WAVES * LINE_U;  // outputs of a line a workgroup owns
constexpr int LINE_CH = 64;              // source entries of a line staged at a time
constexpr int32_t FAR = 1 << 20;         // farther than any R and any row is long

__global__ __launch_bounds__(BLOCK) void k_edt_rows(const uint8_t* __restrict__ occ, int32_t nx, int64_t rows,
                                                    int32_t complement, int32_t R, int32_t K,
                                                    int32_t* __restrict__ out) {
    // a wavefront's own slices; every lane stores the same word, so each reads what it wrote
    __shared__ unsigned long long s_mask[WAVES][MAX_CHUNKS];
    __shared__ int32_t s_next[WAVES][MAX_CHUNKS];
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    const int32_t chunks = (nx + W64 - 1) / W64;
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const uint8_t* const in = occ + row * nx;
        int32_t* const o = out + row * nx;
        int32_t next = 2 * FAR;  // the first target beyond the chunk
        for (int32_t c = chunks - 1; c >= 0; --c) {
            const int32_t i = c * W64 + lane;
            const bool target = i < nx && ((in[i] != 0) != (complement != 0));
            const unsigned long long m = __ballot(target);
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
            const int32_t g = dl < dr ? dl : dr;
            if (i < nx) o[i] = g > R ? K : g * g;
            if (m != 0ull) last = c * W64 + 63 - __builtin_clzll(m);
        }
    }
}

// Line q of `lines` starts at (q / width) outer + q % width and has n entries `step` apart.
struct Lines {
    int64_t lines, width, outer, step;
    int32_t n;
};

// out = min(min over j' of in[j'] + (j - j')^2, K) along every line; LAST: the square goes
// through edt::value / edt::squared into the outputs instead, in the signed mode only at the
// nodes this transform is for (the free ones, or with `complement` the occupied ones, negated).
template <bool LAST>
__global__ __launch_bounds__(BLOCK) void k_edt_lines(const int32_t* __restrict__ in, Lines ln, int32_t R, int32_t K,
                                                     int32_t tiles_j, int32_t* __restrict__ out, edt::Conv cv,
                                                     const uint8_t* __restrict__ occ, int32_t complement,
                                                     float* __restrict__ values, int32_t* __restrict__ d2) {
    __shared__ int32_t tile[LINE_CH][W64];
    const int lane = threadIdx.x & (W64 - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / W64));
    const int64_t q = (int64_t)(blockIdx.x / (unsigned)tiles_j) * W64 + lane;
    const int32_t j0 = (int32_t)(blockIdx.x % (unsigned)tiles_j) * LINE_JT;
    const bool valid = q < ln.lines;
    const int64_t base = valid ? (q / ln.width) * ln.outer + q % ln.width : 0;
    const int32_t jw = j0 + wave * LINE_U;  // the wavefront's first output
    const int32_t s_lo = std::max(0, j0 - R), s_hi = std::min(ln.n, j0 + LINE_JT + R);
    int32_t acc[LINE_U];
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) acc[u] = K;
    for (int32_t s = s_lo; s < s_hi; s += LINE_CH) {
        const int32_t staged = std::min(LINE_CH, s_hi - s);
        int32_t v[LINE_CH / WAVES];
#pragma unroll
        for (int u = 0; u < LINE_CH / WAVES; ++u) {
            const int32_t r = wave + u * WAVES;
            v[u] = valid && r < staged ? in[base + (int64_t)(s + r) * ln.step] : K;
        }
#pragma unroll
        for (int u = 0; u < LINE_CH / WAVES; ++u) tile[wave + u * WAVES][lane] = v[u];
        __syncthreads();
        int32_t d = s - jw;  // source index less output index, a scalar
#pragma unroll 4
        for (int32_t r = 0; r < staged; ++r, ++d) {
            const int32_t f = tile[r][lane];
#pragma unroll
            for (int u = 0; u < LINE_U; ++u) {
                const int32_t e = d - u;
                acc[u] = std::min(acc[u], f + e * e);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < LINE_U; ++u) {
        const int32_t j = jw + u;
        if (!valid || j >= ln.n) continue;
        const int64_t node = base + (int64_t)j * ln.step;
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
    const int64_t nx = fld.n[0], ny = fld.n[1], nz = fld.n[2], N = nx * ny * nz;
    const edt::Cap cap = edt::make_cap(fld.h, max_dist);
    const edt::Conv cv = edt::make_conv(fld.h, max_dist, cap, is_signed);
    int32_t* const a = static_cast<int32_t*>(work);
    int32_t* const b = a + N;
    const int64_t rows = ny * nz;
    const int32_t row_blocks = (int32_t)std::min<int64_t>((rows + WAVES - 1) / WAVES, MAX_BLOCKS);
    const Lines ly = {nx * nz, nx, nx * ny, nx, (int32_t)ny}, lz = {nx * ny, nx * ny, 0, nx * ny, (int32_t)nz};
    const int32_t ty = (int32_t)((ny + LINE_JT - 1) / LINE_JT), tz = (int32_t)((nz + LINE_JT - 1) / LINE_JT);
    const unsigned by = (unsigned)(((ly.lines + W64 - 1) / W64) * ty), bz = (unsigned)(((lz.lines + W64 - 1) / W64) * tz);
    for (int32_t complement = 0; complement < (is_signed ? 2 : 1); ++complement) {
        TGMS_LAUNCH(k_edt_rows, dim3((unsigned)row_blocks), dim3(BLOCK), 0, stream, occ, (int32_t)nx, rows, complement,
                    cap.R, cap.K, a);
        TGMS_LAUNCH(k_edt_lines<false>, dim3(by), dim3(BLOCK), 0, stream, a, ly, cap.R, cap.K, ty, b, cv, nullptr,
                    complement, nullptr, nullptr);
        TGMS_LAUNCH(k_edt_lines<true>, dim3(bz), dim3(BLOCK), 0, stream, b, lz, cap.R, cap.K, tz, nullptr, cv, occ,
                    complement, values, d2);
    }
    return hipSuccess;
}

}  // namespace tgms
