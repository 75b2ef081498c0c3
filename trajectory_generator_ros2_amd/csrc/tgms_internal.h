// tgms_internal.h — declarations shared by the kernels TU and the C-ABI TU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tgms.h"

namespace tgms {

// Largest M solved at two wavefronts per SIMD (the axis-sequential state of larger M
// needs more than 256 registers); ragged batches launch one kernel per class.  13: the
// fused refinement loop keeps 4 VGPRs in scratch at M = 12..13 and still beats running
// them at one wave (config 5: 0.489-0.494 against 0.494-0.506 ms with 11, round 4).
#ifndef TGMS_TWO_WAVE_MAX_M
#define TGMS_TWO_WAVE_MAX_M 13
#endif
// ... and with end derivatives (their extra state spills the fused refinement loop by
// 79 VGPRs at M = 12..13 within 256 registers; M <= 11 fits with none)
#ifndef TGMS_TWO_WAVE_MAX_M_ED
#define TGMS_TWO_WAVE_MAX_M_ED 11
#endif
constexpr int two_wave_max_m(bool has_ed) { return has_ed ? TGMS_TWO_WAVE_MAX_M_ED : TGMS_TWO_WAVE_MAX_M; }

// Reduced-Hessian solve, uniform M (configs 2-4).  Grid: ceil(B/64) waves.
hipError_t launch_reduced_uniform(int M, int32_t B, const double* W, const double* T,
                                  const double* ED, double* C, int32_t* status,
                                  hipStream_t stream);

// Reduced-Hessian solve for one group of a ragged CSR batch: the n trajectories
// perm[0..n) all have M segments (the host groups a ragged batch by M so every
// wavefront runs a single M).
hipError_t launch_reduced_ragged_group(int M, int32_t n, const int32_t* perm,
                                       const int32_t* seg_offsets, const double* W,
                                       const double* T, const double* ED, double* C,
                                       int32_t* status, hipStream_t stream);

// Dense-KKT solve (survey a1-a3 literally): one wavefront per trajectory, KKT in LDS.
// Uniform M only (1..TGMS_DENSE_MAX_SEGMENTS); ragged batches loop over M groups.
hipError_t launch_dense_kkt(int M, int32_t n_traj, const int32_t* traj_ids /*nullable*/,
                            const int32_t* seg_offsets /*nullable if uniform*/, const double* W,
                            const double* T, const double* ED, double* C, int32_t* status,
                            hipStream_t stream);

// Band-KKT solve (the same KKT and partial-pivoting LU, segment-interleaved order, the
// structurally-zero entries skipped): sixteen trajectories per wavefront, persistent grid
// of `grid` wavefronts, each with private U slabs in `scratch` (band_scratch_bytes).
// grid = CUs x BAND_WAVES_PER_CU (the scratch is sized for it: two wavefronts per SIMD,
// the kernel's register budget); the launch uses the resident part of it.
#ifndef TGMS_BAND_WAVES_PER_CU
#define TGMS_BAND_WAVES_PER_CU 8
#endif
constexpr int BAND_WAVES_PER_CU = TGMS_BAND_WAVES_PER_CU;
size_t band_scratch_bytes(int M, int32_t grid);
hipError_t launch_band_kkt(int M, int32_t n_traj, const int32_t* traj_ids /*nullable*/,
                           const int32_t* seg_offsets /*nullable if uniform*/, const double* W,
                           const double* T, const double* ED, double* C, int32_t* status, double* scratch,
                           int32_t grid, hipStream_t stream);

// Time-allocation refinement step (solve + snap-cost gradient + log-space step on T):
// uniform batches, and one M group of a ragged batch.  Tout may not alias T.
hipError_t launch_refine_uniform(int M, int32_t B, const double* W, const double* T, const double* ED, double kT,
                                 double eta, double* Tout, double* cost, int32_t* status, hipStream_t stream);
hipError_t launch_refine_ragged_group(int M, int32_t n, const int32_t* perm, const int32_t* seg_offsets,
                                      const double* W, const double* T, const double* ED, double kT, double eta,
                                      double* Tout, double* cost, int32_t* status, hipStream_t stream);

// Several M groups of a ragged batch in one launch.  Group g owns wavefronts
// [blk_end[g-1], blk_end[g]) and its n[g] trajectories perm[g][0..n) have m[g] segments.
// cls 0 takes M in 1..two_wave_max_m(ED) (two waves per SIMD), cls 1 the larger M (one wave
// per SIMD).
constexpr int RAGGED_TPW = 32;  // trajectories per wavefront of the reduced kernels
struct GroupTable {
    int32_t ngroups;
    int32_t m[16];
    int32_t n[16];
    int32_t blk_end[16];
    const int32_t* perm[16];
};
hipError_t launch_ragged_multi(int cls, const GroupTable& tab, bool refine, const int32_t* seg_offsets,
                               const double* W, const double* T, const double* ED, double kT, double eta,
                               double* Tout, double* cost, double* C, int32_t* status, hipStream_t stream);

// The M-grouping permutation of a ragged batch computed on the device (stable counting
// sort of the ids by so[b+1] - so[b]; M validated on the host): starts[m] (m = 1..16) is
// where group m begins, hist a workspace of perm_hist_bytes(B).
size_t perm_hist_bytes(int32_t B);
hipError_t launch_group_perm(int32_t B, const int32_t* seg_offsets, const int32_t* starts, int32_t* hist,
                             int32_t* perm, hipStream_t stream);

// The launch plan of a ragged refinement loop computed entirely on the device (round 5):
// the per-M totals summed from k_perm_hist's block counts, the starts of the M groups in
// the permutation and both occupancy classes' group tables.  The host plans nothing per
// trajectory, and a captured graph stays valid for any offsets of the same B and S: each
// replay regroups (held by tests/test_gpu_refine_plan.py).  `so` may be a slice of a larger batch's offsets (so[0] != 0: the
// kernels subtract so_base = so[0]); offsets whose M leave 1..16 or whose span is not S
// mark the plan bad and nothing runs: statuses TGMS_ERR_INVALID_ARG, the S segments'
// coefficients (C, nullable) and the n costs (cost, nullable) exact zeros, times kept.
// This is the only per-trajectory check of tgms_refine_loop_multi_device's offsets.
struct DevPlan {
    GroupTable tab[2];
    int32_t starts[17];  // starts[m]: first index of group m in the permutation (m = 1..16)
    int32_t so_base;     // so[0]
    int32_t bad;
    // waves[1] > 0: the refinement loop's one-wave class runs as that many PERSISTENT
    // wavefronts (round 6, k_refine_loop_dev), each taking the class's tiles from the counter
    // next[1] (longest groups first) until none is left; 0: one block per tile (always for
    // the two-wave class, and for a one-wave class with no more tiles than SIMDs)
    int32_t waves[2];
    int32_t next[2];
};
// Grid of one class's loop launch: every wavefront a group table can hold, whatever the
// offsets (the blocks beyond the class's last group return at once).
inline unsigned dev_loop_grid(int32_t n) { return (unsigned)((n + RAGGED_TPW - 1) / RAGGED_TPW + 16); }
hipError_t launch_group_plan_dev(int32_t n, int64_t S, const int32_t* so, int has_ed, int32_t* hist, int32_t* perm,
                                 DevPlan* plan, int32_t* status, double* C, double* cost, hipStream_t stream);
hipError_t launch_refine_loop_dev(int cls, int32_t n, DevPlan* plan, const int32_t* so, const double* W,
                                  double* T, const double* ED, double kT, double eta, int32_t iters, double* cost,
                                  double* C, int32_t* status, hipStream_t stream);
// The ragged solve of one occupancy class from a device plan (k_reduced_multi's blocks).
hipError_t launch_reduced_multi_dev(int cls, int32_t n, const DevPlan* plan, const int32_t* so, const double* W,
                                    const double* T, const double* ED, double* C, int32_t* status,
                                    hipStream_t stream);

// Sampler: one workgroup per trajectory (grid-stride), 14 doubles per sample.
hipError_t launch_sample(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                         const double* ED, const double* C, double dt, int yaw_mode,
                         double yaw_const, const int64_t* sample_offsets, double* out,
                         hipStream_t stream);

// Feasibility check: the sampler's samples reduced per trajectory to ext [B][TGMS_EXTREMA_STRIDE]
// and flags [B] (either nullable), one wavefront per trajectory, nothing per sample stored.
hipError_t launch_extrema(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                          const double* ED, const double* C, double dt, const tgms_limits& lim, double* ext,
                          int32_t* flags, hipStream_t stream);

// Continuous feasibility bounds (tgms_bounds.hip): the same record and flags from the
// polynomials' stationary points, no dt; a wavefront per tile of 4 trajectories, one launch.
hipError_t launch_bounds(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                         const tgms_limits& lim, double* ext, int32_t* flags, hipStream_t stream);

// Continuous thrust and tilt bounds (tgms_thrust.hip): per trajectory f_min t_fmin f_max t_fmax
// tilt_max t_tilt of f = p'' + g e_z into rec [B][TGMS_THRUST_STRIDE] and flags [B] (either
// nullable); the mapping of launch_bounds, one launch.
hipError_t launch_thrust(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, double g,
                         const tgms_thrust_limits& lim, double* rec, int32_t* flags, hipStream_t stream);

// Continuous body-rate bound (tgms_rate.hip): per trajectory omega_max t_omega of ||f x p'''|| /
// ||f||^2 into rec [B][TGMS_RATE_STRIDE], per segment its own maximum and local time into seg_rec
// [S][TGMS_RATE_STRIDE] and flags [B] (each nullable); the mapping of launch_thrust, one launch.
hipError_t launch_rate(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, double g,
                       double omega_limit, double* rec, double* seg_rec, int32_t* flags, hipStream_t stream);

// Time dilation (tgms_dilate.hip): per trajectory the least stretch s in [s_lo, s_hi] that meets
// lim (tgms_dilate_core.h: the six limits, resolved) into scale [B], the active limit into active
// [B], flags [B], the scaled times into T_out [S] and coefficients into C_out [S][3][8] (each
// nullable; T_out / C_out may be T / C); the mapping of launch_thrust, one launch.
namespace dilate {
struct Lim;
}
hipError_t launch_dilate(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, double g,
                         const dilate::Lim& lim, double s_lo, double s_hi, double* scale, int32_t* active,
                         int32_t* flags, double* T_out, double* C_out, hipStream_t stream);

// Segment re-timing (tgms_retime.hip): per segment v a j r into seg_rec [S][TGMS_RETIME_STRIDE] and
// the time s T into T_out [S] (may be T), per trajectory r_max D_in D_out into rec
// [B][TGMS_RETIME_REC] and flags [B] (each nullable) against lim (tgms_retime_core.h: each limit
// > 0, +inf unchecked); the tile of launch_bounds, one launch.
namespace retime {
struct Lim;
}
hipError_t launch_retime(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                         const retime::Lim& lim, double s_lo, double s_hi, double* T_out, double* seg_rec, double* rec,
                         int32_t* flags, hipStream_t stream);

// Corridor containment (tgms_corridor.hip): per trajectory m_max t_max into rec
// [B][TGMS_COR_STRIDE], its segment and face into where [B][2], per segment m_s t_s into
// seg_rec [S][TGMS_COR_STRIDE] and its face into seg_face [S], flags [B] (each nullable);
// face_offsets NULL: all F <= TGMS_COR_MAX_FACES faces apply to every segment.  The tile of
// launch_bounds with the (segment, face) item as the unit of lane work, one launch.
hipError_t launch_corridor(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, int64_t F,
                           const double* faces, const int64_t* face_offsets, double r, double* rec, int32_t* where,
                           double* seg_rec, int32_t* seg_face, int32_t* flags, hipStream_t stream);

// Corridor split (tgms_corridor_split.hip): the segments whose margin of a corridor call exceeds
// -r get a waypoint at their worst excursion; the new offsets, waypoints, times, faces, face
// offsets, parent rows (nullable), totals [2] = S' F' and flags [B] (nullable).  Five launches on
// `stream`: the plan per tile of launch_corridor, three for the prefix sums over B, the write;
// `scratch` holds corridor_split_scratch_bytes(B) bytes, 256-byte aligned.  face_offsets NULL:
// shared mode, faces_out and fo_out are not touched.  B == 0 writes so_out[0] and the totals.
size_t corridor_split_scratch_bytes(int32_t B);
hipError_t launch_corridor_split(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                                 const double* C, int64_t F, const double* faces, const int64_t* face_offsets,
                                 const double* seg_rec, const int32_t* seg_face, double r, int mode, double min_frac,
                                 void* scratch, int32_t* so_out, double* W_out, double* T_out, double* faces_out,
                                 int64_t* fo_out, int32_t* parent, int64_t* totals, int32_t* flags,
                                 hipStream_t stream);

// The prefix sums of every call that rebuilds a batch (split, cut, subdivision, re-route), the
// k_scan_* kernels of tgms_corridor_split.hip: so_out [B+1] = the exclusive int32 scan of cntS
// [B] with the total at [B], cntF [B] (int64) scanned in place, totals [2] = both sums (totals[1]
// = shared_F when that is >= 0).  sumS and sumF hold count_scan_blocks(B) entries each.  Three
// launches; B > 0.
size_t count_scan_blocks(int32_t B);
hipError_t launch_count_scan(int32_t B, const int32_t* cntS, int64_t* cntF, int64_t* sumS, int64_t* sumF,
                             int64_t shared_F, int32_t* so_out, int64_t* totals, hipStream_t stream);

// The scratch of such a call, carved in 256-byte steps: the scan's cntF, sumS, sumF and (not in
// the split, which scans into the caller's) totals [2] first; take<T>(count) hands out each
// call's own fields after them, cntS among them, and `off` is then the size.  n = max(B, 0).
struct ScanScratch {
    char* p;
    size_t n, off = 0;
    int64_t *cntF, *sumS, *sumF, *totals = nullptr;
    template <class T>
    T* take(size_t count) {
        T* const at = reinterpret_cast<T*>(p + off);
        off = (off + count * sizeof(T) + 255) & ~size_t(255);
        return at;
    }
    ScanScratch(int32_t B, void* base, bool with_totals) : p(static_cast<char*>(base)), n(B > 0 ? (size_t)B : 0) {
        cntF = take<int64_t>(n);
        sumS = take<int64_t>(count_scan_blocks(B));
        sumF = take<int64_t>(count_scan_blocks(B));
        if (with_totals) totals = take<int64_t>(2);
    }
};

// Replan cut (tgms_cut.hip): every trajectory restarted from its state at t_cut [B]; the new
// offsets, waypoints, times, end derivatives, coefficients (nullable), parent rows (nullable), t0
// [B] (nullable), totals [1] = S' and flags [B] (nullable).  ED NULL: rest to rest.  Five launches
// on `stream`: the plan per tile of launch_corridor, launch_count_scan, the write; `scratch` holds
// cut_scratch_bytes(B) bytes, 256-byte aligned.  B == 0 writes so_out[0] and the total.
size_t cut_scratch_bytes(int32_t B);
hipError_t launch_cut(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const double* ED,
                      const double* C, const double* t_cut, double min_frac, void* scratch, int32_t* so_out,
                      double* W_out, double* T_out, double* ED_out, double* C_out, int32_t* parent, double* t0_out,
                      int64_t* totals, int32_t* flags, hipStream_t stream);

// Continuous swarm separation (tgms_separation.hip): per pair the closest approach d_min t_min
// into sep [P][TGMS_SEP_STRIDE] and flags [P] (either nullable); pairs NULL: every unordered
// pair, decoded on the device.  A wavefront per tile of 16 pairs, one launch.
hipError_t launch_separation(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                             const double* start_times, int64_t P, const int32_t* pairs, const double (&scale)[3],
                             double r_min, double* sep, int32_t* flags, hipStream_t stream);

// Swarm neighbour search (tgms_neighbors.hip): per vehicle the nearest other vehicle that comes
// within r_min (near [B][TGMS_SEP_STRIDE], nbr [B]), how many do (count [B]), how many pairs
// the exact computation ran for (tested [B]) and flags [B]; all nullable.  Two launches: the
// boxes of every vehicle into `scratch` (neighbors_scratch_bytes(B), 256-byte aligned), then a
// wavefront per tile of rows.
size_t neighbors_scratch_bytes(int32_t B);
hipError_t launch_neighbors(int32_t B, const int32_t* seg_offsets, const double* T, const double* C,
                            const double* start_times, const double (&scale)[3], double r_min, void* scratch,
                            double* near, int32_t* nbr, int32_t* count, int32_t* tested, int32_t* flags,
                            hipStream_t stream);

// Obstacle clearance (tgms_clearance.hip): per trajectory the nearest of K static boxes
// (obstacles [K][6] = lo[3] hi[3]) that comes within r_min (near [B][TGMS_SEP_STRIDE], obs [B]),
// how many do (count [B]), how many the exact computation ran for (tested [B]) and flags [B];
// all nullable.  Two launches: the boxes of every trajectory and a usable word per obstacle into
// `scratch` (clearance_scratch_bytes(B, K), 256-byte aligned), then a wavefront per tile of rows.
size_t clearance_scratch_bytes(int32_t B, int32_t K);
hipError_t launch_clearance(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, int32_t K,
                            const double* obstacles, const double (&scale)[3], double r_min, void* scratch,
                            double* near, int32_t* obs, int32_t* count, int32_t* tested, int32_t* flags,
                            hipStream_t stream);

// Distance-field clearance (tgms_field.hip): per trajectory the least value of the field
// `values` on the grid `fld` along it (near [B][TGMS_SEP_STRIDE]), the evaluations it took
// (evals [B]) and flags [B]; all nullable.  scratch NULL: one launch with the Lipschitz bound
// `lip`.  scratch (field_scratch_bytes(), 8-byte aligned): two launches before it reduce the
// bound from the values into the scratch's first double, which the search reads.
size_t field_scratch_bytes();
hipError_t launch_field(int32_t B, const int32_t* seg_offsets, const double* T, const double* C, const tgms_field& fld,
                        const float* values, double lip, double r_min, double tol, int32_t max_evals, void* scratch,
                        double* near, int32_t* evals, int32_t* flags, hipStream_t stream);

// Corridor inflation (tgms_inflate.hip).  launch_field_occupancy: the summed-volume table
// [(nz+1)][(ny+1)][(nx+1)] of the nodes of `values` below (float)r_free, three launches.
// launch_inflate: per segment the largest free lattice box around it (box [S][6], faces [6S][4],
// face_offsets [S+1], seg_flags [S]) and per trajectory the OR of its segments' flags (flags
// [B]); all nullable, one launch.  Neither uses scratch.
hipError_t launch_field_occupancy(const tgms_field& fld, const float* values, double r_free, int32_t* table,
                                  hipStream_t stream);
hipError_t launch_inflate(int32_t B, const int32_t* seg_offsets, const double* W, const tgms_field& fld,
                          const int32_t* table, int32_t max_grow, int32_t* box, double* faces, int64_t* face_offsets,
                          int32_t* seg_flags, int32_t* flags, hipStream_t stream);

// Distance-field build (tgms_edt.hip): the exact Euclidean transform of the occupancy bytes `occ`
// on the grid `fld` into values [nz][ny][nx] fp32 and the squared lattice distances d2 (either
// nullable), capped at max_dist; is_signed: negative inside, with the half-spacing offset.  Three
// launches, six when signed, ping-ponging in `work` (edt_work_bytes, 4-byte aligned).  No scratch.
size_t edt_work_bytes(const tgms_field& fld);
hipError_t launch_edt(const tgms_field& fld, const uint8_t* occ, double max_dist, bool is_signed, float* values,
                      int32_t* d2, void* work, hipStream_t stream);

// Corridor subdivision (tgms_subdivide.hip): the legs whose own lattice box holds a non-free node
// of `table` halved down to sixteenths; the new offsets, waypoints, times (T and T_out nullable
// together), parent rows, segment flags (both nullable), totals [1] = S' and flags [B]
// (nullable).  Five launches on `stream`: the plan per tile of launch_inflate, launch_count_scan,
// the write; `scratch` holds subdivide_scratch_bytes(B) bytes, 256-byte aligned.  B == 0 writes
// so_out[0] and the total.
size_t subdivide_scratch_bytes(int32_t B);
hipError_t launch_subdivide(int32_t B, const int32_t* seg_offsets, const double* W, const double* T,
                            const tgms_field& fld, const int32_t* table, int32_t max_depth, void* scratch,
                            int32_t* so_out, double* W_out, double* T_out, int32_t* parent, int32_t* seg_flags,
                            int64_t* totals, int32_t* flags, hipStream_t stream);

// Corridor re-route (tgms_reroute.hip): the legs whose own lattice box holds a non-free node of
// `table` detoured through the free nodes of a window of the map; the new offsets, waypoints,
// times (T and T_out nullable together), parent rows, segment flags, hops per input segment (all
// three nullable), totals [1] = S' and flags [B] (nullable).  A counter reset and seven launches on
// `stream`: classify, the persistent search, count, launch_count_scan, the write; `scratch` holds
// reroute_scratch_bytes(B) bytes, 256-byte aligned.  reroute_prepare raises the search kernel's
// dynamic LDS limit on the current device, once before the first launch there.  B == 0 writes
// so_out[0] and the total.
size_t reroute_scratch_bytes(int32_t B);
hipError_t reroute_prepare();
hipError_t launch_reroute(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const tgms_field& fld,
                          const int32_t* table, int32_t margin, int32_t max_pieces, void* scratch, int32_t* so_out,
                          double* W_out, double* T_out, int32_t* parent, int32_t* seg_flags, int32_t* hops,
                          int64_t* totals, int32_t* flags, hipStream_t stream);

// Waypoint repair (tgms_repair.hip).  launch_nearest_free: per node of `values` on the grid `fld`
// the linear index of the nearest free node within max_shift spacings (nearest [nz][ny][nx]) and
// its squared lattice distance (dsq, nullable), TGMS_NEAR_NONE where there is none; three launches,
// the middle pass in `work` (nearest_free_work_bytes, 4-byte aligned).  launch_repair: every
// waypoint whose own seed holds a node that is not its own site moves onto the site of its nearest
// node; the waypoints, the times (T and T_out nullable together), per waypoint its flag and shift,
// per trajectory the OR of its flags (all three nullable); one launch.  Neither uses scratch.
size_t nearest_free_work_bytes(const tgms_field& fld);
hipError_t launch_nearest_free(const tgms_field& fld, const float* values, double r_free, int32_t max_shift,
                               int32_t* nearest, int32_t* dsq, void* work, hipStream_t stream);
hipError_t launch_repair(int32_t B, const int32_t* seg_offsets, const double* W, const double* T, const tgms_field& fld,
                         const int32_t* nearest, int32_t mode, double* W_out, double* T_out, int32_t* wp_flags,
                         int32_t* shift, int32_t* flags, hipStream_t stream);
}  // namespace tgms
