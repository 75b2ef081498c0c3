/*
 * tgms.h — C ABI of the MI355X-native batched minimum-snap solver (libtgms.so).
 *
 * This is the drop-in boundary of SURVEY.md §8(b).  The reference
 * (jrached/trajectory_generator_ros2) owns trajectories through
 *     std::unique_ptr<Trajectory> traj_           include/trajectory_generator_ros2/TrajectoryGenerator.hpp:83
 * built by the traj_type factory                  src/TrajectoryGenerator.cpp:175-388
 * and calls exactly three virtuals on it:
 *     generateTraj(goals, index_msgs, clock)      Trajectory.hpp:33-35, called at src/TrajectoryGenerator.cpp:71
 *     generateStopTraj(goals, msgs, idx, clock)   Trajectory.hpp:38-41, called at src/TrajectoryGenerator.cpp:516
 *     trajectoryInsideBounds(xmin..zmax)          Trajectory.hpp:44-46, called at src/TrajectoryGenerator.cpp:419
 * The reference has no solver behind those virtuals (every primitive is a
 * closed-form sampler).  A MinSnap primitive implements them on top
 * of the entry points below (trajectory_generator_ros2_amd/host/MinSnap.cpp):
 *     generateTraj            -> tgms_solve_batch (B = 1)  + tgms_sample_batch
 *     generateStopTraj        -> tgms_solve_batch with end_derivs (braking)  + tgms_sample_batch
 *     trajectoryInsideBounds  -> host check of waypoints and sampled extrema
 * and a swarm / sampling planner calls the same entry points with B up to 10^6.
 *
 * Conventions:
 *   - plain C, no exceptions cross the ABI; every call returns a tgms_status;
 *   - the caller owns every I/O buffer; the handle owns device workspace only;
 *   - a handle is bound to one HIP device and is single-thread-affine (the
 *     reference calls from its single rclcpp executor thread,
 *     src/trajectory_generator_node.cpp:30);
 *   - `*_device` entry points take device pointers and a hipStream_t passed as
 *     void* and are asynchronous; the others take host pointers and block.  Calls
 *     of one handle that use its device scratch (ragged plans, the refinement loop,
 *     the band-KKT method) may be issued on different streams: the handle orders
 *     them on the GPU with an event (each waits for the previous one's work);
 *     fp64 device arrays must be 16-byte aligned (TGMS_ERR_INVALID_ARG otherwise;
 *     hipMalloc allocations are, a slice at an odd element offset is not);
 *   - HIP-graph capture: uniform solves (tgms_solve_uniform_device, any method, and
 *     tgms_solve_batch_device / tgms_refine_*_device on a uniform batch) may be
 *     captured into a caller's graph.  Inside a capture the scratch event handshake
 *     is skipped.  A band-KKT capture needs the handle's slab sized by an earlier
 *     uncaptured band call of at least that M; from then on that slab belongs to
 *     graphs (uncaptured calls get a slab of their own and never free a graph's), so
 *     replays may run beside uncaptured calls, but graphs holding band launches of one
 *     handle must be replayed in stream order with each other.  Calls that upload a
 *     host-side launch plan or grow scratch at call time (ragged batches,
 *     tgms_refine_loop_device, tgms_neighbors_batch_device, tgms_clearance_batch_device,
 *     tgms_corridor_split_batch_device, tgms_cut_batch_device,
 *     tgms_field_clearance_batch_device with lip == 0, the multi-GPU calls, a band
 *     capture with no slab large enough) return TGMS_ERR_UNSUPPORTED while their stream is
 *     capturing.
 *     tgms_extrema_batch_device, tgms_bounds_batch_device, tgms_thrust_batch_device,
 *     tgms_rate_batch_device, tgms_dilate_batch_device, tgms_retime_batch_dev and tgms_corridor_batch_device (one kernel, no plan, no scratch) may be captured for any
 *     batch, ragged included; so may tgms_field_occupancy_device and
 *     tgms_corridor_inflate_batch_device (no plan, no scratch), and tgms_field_edt_device (its
 *     workspace is the caller's);
 *   - there is no CPU fallback: with no usable GPU, tgms_create fails with
 *     TGMS_ERR_NO_DEVICE.  A GPU-less node asks for the host backend explicitly
 *     (tgms_create_host: solve + sample on the CPU, config 1).
 *
 * Layouts (fp64, row-major, trajectory-major).  A batch is CSR over segments:
 * trajectory b has M_b = seg_offsets[b+1] - seg_offsets[b] segments (1..TGMS_MAX_SEGMENTS):
 *   seg_offsets  int32 [B+1], seg_offsets[0] = 0, strictly increasing (1 <= M_b <= max)
 *   waypoints    [sum_b (M_b+1)][3]   rows of b start at seg_offsets[b] + b
 *   seg_times    [sum_b M_b]          T_i > 0 and finite, starting at seg_offsets[b]
 *   end_derivs   NULL (rest-to-rest, as every reference primitive starts and ends
 *                at rest) or [B][2][3][3] = [start|final][v,a,j][x,y,z]
 *   coeffs       [sum_b M_b][3][8]    p(t) = sum_j c_j t^j on local t in [0, T_i]
 *   status       int32 [B], nullable: per-trajectory tgms_status
 */
#ifndef TGMS_H
#define TGMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGMS_ABI_VERSION 2 /* 2: tgms_piece.ws_off gained the device plan regions (round 5) */
#define TGMS_MAX_SEGMENTS 16       /* reduced-Hessian kernel: M = 1..16 (config 5 range) */
#define TGMS_DENSE_MAX_SEGMENTS 10 /* dense KKT kernel: N = 14M+2 <= 142 (+3 right-hand sides) fits a 256-thread workgroup's registers */
#define TGMS_GOAL_STRIDE 14        /* doubles per sample: p[3] v[3] a[3] j[3] psi dpsi */

typedef enum tgms_status {
    TGMS_OK = 0,
    TGMS_ERR_INVALID_ARG = 1, /* bad sizes/pointers, M_b < 1 or > max, T <= 0, non-finite input */
    TGMS_ERR_SINGULAR = 2,    /* a pivot / Cholesky block broke down */
    TGMS_ERR_NONFINITE = 3,   /* solution contains inf/nan */
    TGMS_ERR_NO_DEVICE = 4,   /* no HIP device (no CPU fallback exists) */
    TGMS_ERR_DEVICE = 5,      /* a HIP runtime call failed (see tgms_last_error) */
    TGMS_ERR_UNSUPPORTED = 6, /* e.g. dense-KKT method with M_b > TGMS_DENSE_MAX_SEGMENTS */
    TGMS_ERR_SKIPPED = 7      /* per trajectory only: not solved because another trajectory of
                                 the same device shard piece had invalid offsets
                                 (tgms_refine_loop_multi_device; that one is INVALID_ARG) */
} tgms_status;

typedef enum tgms_method {
    TGMS_METHOD_REDUCED = 0,  /* default: Schur complement of the KKT onto the free knot
                                 derivatives, block-tridiagonal LDL^T, one lane per trajectory */
    TGMS_METHOD_DENSE_KKT = 1, /* the survey's literal a1-a3: KKT assembled in LDS, partial-
                                 pivoting LU, one workgroup per trajectory (M <= 10) */
    TGMS_METHOD_BAND_KKT = 2   /* the same KKT and LU with partial pivoting, in the
                                 segment-interleaved order where it is banded (kl = ku = 9);
                                 the structurally-zero entries are skipped, a 16-lane row of
                                 a wavefront per trajectory, M <= TGMS_MAX_SEGMENTS.  Its U rows live in a
                                 handle-owned scratch slab (calls of one handle on different
                                 streams are serialised on the GPU) */
} tgms_method;

typedef enum tgms_yaw_mode {
    TGMS_YAW_CONSTANT = 0, /* psi = yaw_const, dpsi = 0 */
    TGMS_YAW_VELOCITY = 1  /* psi = atan2(v_y, v_x) (Figure8.cpp:123 convention) when
                              |v_xy| > 1e-3, else yaw_const; dpsi = d/dt psi */
} tgms_yaw_mode;

typedef struct tgms_handle tgms_handle;

int tgms_abi_version(void);
const char* tgms_status_string(int status);

/* Create a handle on HIP device `device` (ordinal).  TGMS_ERR_NO_DEVICE if none. */
tgms_status tgms_create(tgms_handle** out, int device);
/* The explicit host backend (BASELINE config 1: a ROS 2 node with no GPU; the reference
 * generates on the executor thread's CPU, src/TrajectoryGenerator.cpp:54-57, :71).  A host
 * handle runs tgms_solve_batch (reduced method), tgms_sample_batch, tgms_extrema_batch,
 * tgms_bounds_batch, tgms_thrust_batch, tgms_rate_batch, tgms_dilate_batch, tgms_retime_batch, tgms_corridor_batch, tgms_corridor_split_batch, tgms_cut_batch, tgms_separation_batch, tgms_neighbors_batch, tgms_clearance_batch, tgms_field_clearance_batch, tgms_corridor_inflate_batch and tgms_field_edt on the calling thread with the GPU path's conventions; every other entry point returns
 * TGMS_ERR_UNSUPPORTED on it.  Chosen by the caller only: tgms_create never falls back to
 * it. */
tgms_status tgms_create_host(tgms_handle** out);
void tgms_destroy(tgms_handle* h);
/* Last error text of this handle ("" if none).  Valid until the next call. */
const char* tgms_last_error(const tgms_handle* h);
tgms_status tgms_set_method(tgms_handle* h, int method);

/* ---- solve (host pointers, blocking) ---- */
tgms_status tgms_solve_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                             const double* waypoints, const double* seg_times,
                             const double* end_derivs, double* coeffs, int32_t* status);

/* ---- solve (device pointers, asynchronous on `stream`) ---- */
/* Uniform batch: every trajectory has M segments (configs 2-4). */
tgms_status tgms_solve_uniform_device(tgms_handle* h, int32_t B, int32_t M,
                                      const double* d_waypoints, const double* d_seg_times,
                                      const double* d_end_derivs, double* d_coeffs,
                                      int32_t* d_status, void* stream);
/* Ragged batch (config 5).  h_seg_offsets is a host copy used to plan the launch
 * (trajectories are grouped by M so every wavefront runs one M).  The refinement loops
 * group the batch on the device from d_seg_offsets, which must hold the same values as
 * h_seg_offsets: tgms_refine_loop_device reads h_seg_offsets once (validation, uniform
 * detection); tgms_refine_loop_multi_device reads only seg_offsets[0], [B] and the shard
 * and piece cuts (binary search), so per-trajectory M is checked on the devices alone.
 * Device offsets with an M outside 1..16 or another span run nothing in the shard piece
 * that holds them (failure granularity: one piece of one device's shard, <= 1/4 of the
 * shard): in d_status the trajectories whose own M is outside 1..16 read
 * TGMS_ERR_INVALID_ARG and the piece's other trajectories TGMS_ERR_SKIPPED, all with zero
 * coefficients and costs and the times kept; the call itself returns TGMS_OK, so a caller
 * checks d_status (a device-side finding cannot reach the return code without a
 * synchronisation the pipelined call avoids). */
tgms_status tgms_solve_batch_device(tgms_handle* h, int32_t B, const int32_t* h_seg_offsets,
                                    const int32_t* d_seg_offsets, const double* d_waypoints,
                                    const double* d_seg_times, const double* d_end_derivs,
                                    double* d_coeffs, int32_t* d_status, void* stream);

/* ---- time-allocation refinement ----
 * Minimises F(T) = sum_i J_i(T) + k_T * sum_i T_i per trajectory over its segment
 * durations, J_i the snap cost of segment i at the min-snap solution.  One step
 * solves, forms g_i = dJ_i/dT_i + k_T analytically (envelope theorem: knot
 * derivatives fixed), and moves in log space:
 *     T_i <- T_i * exp(clamp(-eta * T_i * g_i / F, -1/2, +1/2)).
 * Trajectories whose solve fails keep their times.  Reduced method only
 * (TGMS_ERR_UNSUPPORTED otherwise).  d_cost (nullable, [B]) receives F at the
 * step's input times; dT_out must not alias dT. */
tgms_status tgms_refine_uniform_device(tgms_handle* h, int32_t B, int32_t M, const double* d_waypoints,
                                       const double* d_seg_times, const double* d_end_derivs, double k_T,
                                       double eta, double* d_seg_times_out, double* d_cost, int32_t* d_status,
                                       void* stream);
tgms_status tgms_refine_batch_device(tgms_handle* h, int32_t B, const int32_t* h_seg_offsets,
                                     const int32_t* d_seg_offsets, const double* d_waypoints,
                                     const double* d_seg_times, const double* d_end_derivs, double k_T, double eta,
                                     double* d_seg_times_out, double* d_cost, int32_t* d_status, void* stream);
/* The whole config-5 pipeline on device, planned once: `iters` steps from
 * d_seg_times (updated in place), F at the final times into d_cost (nullable) and
 * the final solve into d_coeffs (nullable).  Uses the handle's workspace. */
tgms_status tgms_refine_loop_device(tgms_handle* h, int32_t B, const int32_t* h_seg_offsets,
                                    const int32_t* d_seg_offsets, const double* d_waypoints, double* d_seg_times,
                                    const double* d_end_derivs, double k_T, double eta, int32_t iters,
                                    double* d_coeffs, double* d_cost, int32_t* d_status, void* stream);
/* Host convenience (blocking): `iters` steps from seg_times (updated in place),
 * then F at the final times into cost (nullable) and, if coeffs is not NULL,
 * the final solve.  Returns the worst per-trajectory status. */
tgms_status tgms_refine_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* waypoints,
                              double* seg_times, const double* end_derivs, double k_T, double eta, int32_t iters,
                              double* coeffs, double* cost, int32_t* status);

/* ---- sampling at dt ----
 * Trajectory b yields tgms_sample_count(sum_i T_i, dt) samples: t_k = k*dt for
 * k = 0 .. n-2 and a final sample at sum_i T_i pinned exactly to the last
 * waypoint and final end derivatives (the Line.cpp:80-82 convention).  Each sample
 * is TGMS_GOAL_STRIDE doubles.  sample_offsets [B+1] comes from
 * tgms_sample_offsets(). */
int64_t tgms_sample_count(double total_T, double dt);
tgms_status tgms_sample_offsets(int32_t B, const int32_t* seg_offsets, const double* seg_times,
                                double dt, int64_t* sample_offsets);
tgms_status tgms_sample_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                              const double* waypoints, const double* seg_times,
                              const double* end_derivs, const double* coeffs, double dt,
                              int yaw_mode, double yaw_const, const int64_t* sample_offsets,
                              double* out);
tgms_status tgms_sample_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                     const double* d_waypoints, const double* d_seg_times,
                                     const double* d_end_derivs, const double* d_coeffs,
                                     double dt, int yaw_mode, double yaw_const,
                                     const int64_t* d_sample_offsets, double* d_out,
                                     void* stream);

/* ---- feasibility check at dt: extents, peaks, limit flags ----
 * The samples above, reduced per trajectory without being written anywhere: over the
 * tgms_sample_count(sum_i T_i, dt) samples of trajectory b (the sampler's times, segment
 * scan, prefix sums of T and Horner chains, the last sample pinned to the last waypoint and
 * the final end derivatives or zeros) one record of TGMS_EXTREMA_STRIDE doubles
 *     pmin[3] pmax[3] v_peak a_peak j_peak duration
 * with x_peak = sqrt(max_k (x_x^2 + x_y^2 + x_z^2)) and duration = that prefix sum of T.
 * This is the sampled-extrema check of the node's trajectoryInsideBounds at resolution dt,
 * not a continuous root-find: an excursion between two samples is not seen.  The work grows
 * with sum_i T_i / dt; nothing of it is stored, so a batch whose samples would not fit on
 * the device can still be checked.
 *   flags [B] (int32, nullable) receive TGMS_FEAS_* bits against `limits`, a host struct
 * read at call time (its values travel as kernel arguments).  All comparisons are strict (a
 * value equal to its limit is inside) and use the very values written to the record.
 * +-inf entries are unchecked; a NaN entry or pmin > pmax is TGMS_ERR_INVALID_ARG; limits
 * == NULL checks nothing, so the flags can then carry TGMS_FEAS_NONFINITE only.  A
 * trajectory with a non-finite coefficient, time, final waypoint, final end derivative or
 * result (or a negative sum of times, more than 2^53 samples, or, in the device call, a
 * segment count outside 1..TGMS_MAX_SEGMENTS) gets TGMS_FEAS_NONFINITE and no other bit, and
 * its record is unspecified (NaNs today); its neighbours are unaffected.  At least one of
 * extrema / flags must be non-NULL.
 *   tgms_extrema_batch_device needs no host plan and no handle scratch, so it may be captured
 * into a HIP graph for any batch, ragged included.  On a multi handle it runs on device 0;
 * on a host handle it returns TGMS_ERR_UNSUPPORTED, and tgms_extrema_batch runs on the
 * calling thread. */
#define TGMS_EXTREMA_STRIDE 10
#define TGMS_FEAS_BOX 1        /* some sampled position outside [pmin, pmax] */
#define TGMS_FEAS_SPEED 2      /* v_peak > v_max */
#define TGMS_FEAS_ACCEL 4      /* a_peak > a_max */
#define TGMS_FEAS_JERK 8       /* j_peak > j_max */
#define TGMS_FEAS_NONFINITE 16 /* a coefficient, time or result of this trajectory is not finite */
typedef struct tgms_limits {
    double pmin[3], pmax[3], v_max, a_max, j_max;
} tgms_limits;
tgms_status tgms_extrema_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                      const double* d_waypoints, const double* d_seg_times,
                                      const double* d_end_derivs, const double* d_coeffs, double dt,
                                      const tgms_limits* limits /* host, nullable */,
                                      double* d_extrema /* [B][10], nullable */,
                                      int32_t* d_flags /* [B], nullable */, void* stream);
/* Host pointers, blocking: one upload, the launch, and one download: records and flags sit
 * in one workspace region, 80 B + 4 B per trajectory, copied back at once when both are
 * asked for. */
tgms_status tgms_extrema_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                               const double* waypoints, const double* seg_times, const double* end_derivs,
                               const double* coeffs, double dt, const tgms_limits* limits,
                               double* extrema, int32_t* flags);

/* ---- continuous feasibility bounds: the same record and flags, no dt ----
 * The polynomial on the closed interval [0, T_i] of every segment is the whole input: no dt,
 * no waypoints, no end derivatives.  The record is the TGMS_EXTREMA_STRIDE layout above, so a
 * consumer of the sampled record can switch calls:
 *     pmin / pmax   per-axis minimum and maximum of p(t) over all segments' closed intervals
 *     x_peak        sqrt(max_t (x_x^2 + x_y^2 + x_z^2)) for x = p', p'', p''' over the same set
 *     duration      the left-to-right prefix sum of T, bit-equal to tgms_extrema_batch's
 * The quantities are piecewise polynomials of degree <= 7 (the squared norms <= 12), so their
 * extrema are the values at the segment ends and at the stationary points, which are located
 * by bisection on the monotone pieces of the derivative: O(M) work per trajectory, independent
 * of the durations, and no resolution to choose.
 *   Accuracy: extents within 1e-9 * max|p| of the true continuous extremum, peaks within 1e-9
 * relative of it.  These are fp64 evaluations at located stationary points, not an
 * interval-arithmetic certificate.  A stationary point where the derivative touches zero
 * without a sign change (an inflection, or a minimum / maximum pair closer than the root
 * resolution) may be skipped; that moves the result by far less than the tolerance.  A
 * constant trajectory (all coefficients of degree >= 1 zero) gives peaks of exactly 0.0 and
 * extents that are exactly the point.
 *   flags: the TGMS_FEAS_* bits against the same tgms_limits, as above: strict comparisons on
 * the very values stored, +-inf entries unchecked, limits == NULL can yield
 * TGMS_FEAS_NONFINITE only, a NaN entry or pmin > pmax is TGMS_ERR_INVALID_ARG.  A trajectory
 * with a non-finite coefficient, time or result, with a T_i that is not > 0 (the solvers
 * never emit one) or, in the device call, with a segment count outside
 * 1..TGMS_MAX_SEGMENTS (nothing is read for it) gets TGMS_FEAS_NONFINITE alone and an all-NaN
 * record; its neighbours are unaffected.  At least one of extrema / flags must be non-NULL;
 * fp64 device arrays are 16-byte aligned; B == 0 is TGMS_OK and launches nothing.
 *   tgms_bounds_batch_device is one kernel launch with no host plan and no handle scratch, so
 * it may be captured into a HIP graph for any batch, ragged included.  On a multi handle it
 * runs on device 0; on a host handle it returns TGMS_ERR_UNSUPPORTED.  tgms_bounds_batch on a
 * host handle computes on the calling thread (the same algorithm; host and device agree to
 * the accuracy above, not to the bit); on a GPU handle it does one upload, the launch and one
 * download, like tgms_extrema_batch. */
tgms_status tgms_bounds_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                     const double* d_seg_times, const double* d_coeffs,
                                     const tgms_limits* limits /* host, nullable */,
                                     double* d_extrema /* [B][TGMS_EXTREMA_STRIDE], nullable */,
                                     int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_bounds_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                              const double* seg_times, const double* coeffs,
                              const tgms_limits* limits, double* extrema, int32_t* flags);

/* ---- continuous swarm separation: closest approach of trajectory pairs ----
 * All in fp64.  Trajectory b lives on the global interval [t0_b, t0_b + D_b]: t0_b =
 * start_times[b] (0 when start_times == NULL) and D_b is the left-to-right prefix sum of its
 * seg_times, the `duration` of the extrema record; its knot m is at t0_b + (the prefix sum of
 * its first m times).  Outside that interval the vehicle holds the nearest end point, p(0) of
 * its first segment or p(T) of its last, so the distance of a pair (i, j)
 *     d(t) = sqrt(sum_a (s_a (p_i,a(t) - p_j,a(t)))^2)
 * is defined for all t and is constant outside the window [min(t0_i, t0_j), max(end_i,
 * end_j)], which is what is searched.  `scale` = s[3] is a host array read at call time (its
 * values travel as kernel arguments, like tgms_limits): the per-axis scale of the usual
 * downwash ellipsoid.  NULL means 1, 1, 1; an entry that is not finite and > 0 is
 * TGMS_ERR_INVALID_ARG.
 *   Per pair one record of TGMS_SEP_STRIDE doubles, d_min t_min, and an int32 flag word.  d_min
 * is the minimum of d over the window; t_min is a global time in the window at which the
 * returned d_min is attained (which one among ties is unspecified).  On every interval
 * between consecutive knots of either trajectory d^2 is a polynomial of degree <= 14, so the
 * minimum is the least value at the interval ends and at the stationary points, which the
 * derivative ladder of the bounds call locates: O(M_i + M_j) work per pair, no resolution.
 *   pairs is int32 [P][2], P an int64_t.  pairs == NULL means every unordered pair in the
 * order (0,1), (0,2), ..., (0,B-1), (1,2), ...; P must then equal B (B - 1) / 2, else
 * TGMS_ERR_INVALID_ARG; the index is decoded on the device and no pair list exists anywhere.
 * (i, i) is a valid pair, and identical trajectories with equal start times give d_min == 0.0
 * exactly: a value is always the difference of the two trajectories' own polynomials at their
 * own local times.
 *   flags: TGMS_SEP_CLOSE when d_min < r_min (strict, on the stored value); r_min <= 0 checks
 * nothing, a NaN r_min is TGMS_ERR_INVALID_ARG.  A pair gets TGMS_SEP_NONFINITE alone and an
 * all-NaN record when an index is outside 0..B-1 (nothing is read for it), when either
 * trajectory has a non-finite coefficient, time or start time or a T that is not > 0, when,
 * in the device call, either has a segment count outside 1..TGMS_MAX_SEGMENTS, or when the
 * result is not finite.  Other pairs are unaffected.
 *   Accuracy, on the squared distance since d itself is ill-conditioned near 0:
 *     |d_min^2 - d_true^2| <= 1e-9 * L^2,
 * L the largest scaled coordinate magnitude either trajectory reaches.  As for the bounds
 * this is an fp64 evaluation at located stationary points, not a certificate; a touch of the
 * derivative without a sign change may be skipped.
 *   At least one of sep / flags must be non-NULL; fp64 device arrays are 16-byte aligned; P ==
 * 0 is TGMS_OK and launches nothing.  tgms_separation_batch_device is one kernel launch with
 * no host plan and no handle scratch, so it may be captured into a HIP graph for any batch.
 * On a multi handle it runs on device 0; on a host handle it returns TGMS_ERR_UNSUPPORTED.
 * tgms_separation_batch on a host handle computes on the calling thread (the same algorithm;
 * host and device agree to the accuracy above, not to the bit); on a GPU handle it does one
 * upload, the launch and one download (records and flags in one workspace region), like
 * tgms_bounds_batch. */
#define TGMS_SEP_STRIDE 2
#define TGMS_SEP_CLOSE 1      /* d_min < r_min */
#define TGMS_SEP_NONFINITE 16 /* a bad index, segment count, time, coefficient or result */
tgms_status tgms_separation_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                         const double* d_seg_times, const double* d_coeffs,
                                         const double* d_start_times /* [B], nullable */, int64_t P,
                                         const int32_t* d_pairs /* [P][2], nullable: all pairs */,
                                         const double* scale /* host [3], nullable */, double r_min,
                                         double* d_sep /* [P][TGMS_SEP_STRIDE], nullable */,
                                         int32_t* d_flags /* [P], nullable */, void* stream);
tgms_status tgms_separation_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                  const double* seg_times, const double* coeffs, const double* start_times,
                                  int64_t P, const int32_t* pairs, const double* scale, double r_min,
                                  double* sep, int32_t* flags);

/* ---- swarm neighbour search: nearest vehicle per vehicle, far pairs culled ----
 * The question before the separation call: which pairs are worth testing.  The call takes the
 * swarm and a search horizon r_min (finite and > 0, else TGMS_ERR_INVALID_ARG) and returns per
 * vehicle i, over all j != i, with the value of the ordered pair (i, j) exactly as
 * tgms_separation_batch defines it (global intervals, start times, held end points, per-axis
 * scale, strict comparison on the stored value):
 *     count[i]   the number of vehicles j whose closest approach to i is < r_min
 *     near[i]    d_min t_min of the closest of them (TGMS_SEP_STRIDE doubles)
 *     nbr[i]     its index; ties on the stored d_min go to the lowest j
 *     tested[i]  the number of j for which the exact closest approach was computed
 *     flags[i]   TGMS_SEP_CLOSE when count[i] > 0
 * A vehicle that nobody approaches within r_min (B == 1 included) gets near = (+inf, 0.0), nbr
 * = TGMS_NEAR_NONE, count = 0.  Every row is computed on its own, so near[i] and near[nbr[i]]
 * come from the two ordered pairs and agree to the separation call's accuracy, not to the bit;
 * no result depends on the launch shape or on the order in which pairs were processed.
 *   Culling.  The exact computation (a degree-13 ladder per interval) runs only for pairs that
 * a conservative bound cannot rule out: per-segment boxes from the Bernstein control values of
 * the segment polynomials and point boxes for the held ends, widened by a margin that covers
 * the rounding of both the conversion and the exact computation's own evaluations, compared
 * interval by interval along the pair's merged knots.  The bound is sound: a pair whose
 * tgms_separation_batch d_min is < r_min is never culled, so count, nbr and near are those of
 * the all-pairs computation.  How many pairs it removes depends on the swarm (straight
 * segments give tight boxes, turning ones loose boxes); tested makes it observable, with
 * count[i] <= tested[i] <= B - 1.
 *   An unusable vehicle (in the device call a segment count outside 1..TGMS_MAX_SEGMENTS, for
 * which nothing is read; a time that is not finite and > 0; a start time or coefficient that
 * is not finite; a non-finite result) gets TGMS_SEP_NONFINITE alone, near = NaN NaN, nbr =
 * TGMS_NEAR_NONE, count = 0 and tested = 0, and is left out of every other vehicle's search:
 * the other rows are those of the swarm without it.
 *   At least one of near / nbr / count / flags must be non-NULL; a scale entry that is not
 * finite and > 0 is TGMS_ERR_INVALID_ARG; fp64 device arrays are 16-byte aligned; B == 0 is
 * TGMS_OK and launches nothing.  tgms_neighbors_batch_device is two kernel launches on handle
 * scratch that grows with B at call time (1,064 B per vehicle), ordered among the handle's
 * calls like all its scratch, so it returns TGMS_ERR_UNSUPPORTED while its stream is
 * capturing.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_neighbors_batch on a host handle computes on the calling thread
 * (the same boxes, walk and exact computation; host and device agree to the separation call's
 * accuracy, not to the bit); on a GPU handle it does one upload, the launches and one
 * download. */
#define TGMS_NEAR_NONE (-1)
tgms_status tgms_neighbors_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                        const double* d_seg_times, const double* d_coeffs,
                                        const double* d_start_times /* [B], nullable */,
                                        const double* scale /* host [3], nullable */, double r_min,
                                        double* d_near /* [B][TGMS_SEP_STRIDE]: d_min t_min, nullable */,
                                        int32_t* d_nbr /* [B], nullable */, int32_t* d_count /* [B], nullable */,
                                        int32_t* d_tested /* [B], nullable */, int32_t* d_flags /* [B], nullable */,
                                        void* stream);
tgms_status tgms_neighbors_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                                 const double* coeffs, const double* start_times, const double* scale, double r_min,
                                 double* near, int32_t* nbr, int32_t* count, int32_t* tested, int32_t* flags);

/* ---- obstacle clearance: nearest static box per trajectory, far ones culled ----
 * The step between the dynamic limits and the ranking of a sampling planner: how close does
 * each candidate come to the pillars, shelves and net posts of the room.  The call takes the
 * batch, K obstacles and a search horizon r_min (finite and > 0, else TGMS_ERR_INVALID_ARG).
 *   obstacles is fp64 [K][6] = lo[3] hi[3], axis-aligned boxes in the trajectories' frame: every
 * entry finite and lo <= hi per axis; lo == hi on an axis is allowed, which gives a plate, a
 * rod or a point.  In the device call it is a device array, 16-byte aligned.  It may be NULL
 * only when K == 0.  `scale` (host [3], nullable) has the meaning and the validation of the
 * separation call.  There are no start times: the obstacles do not move.
 *   The distance of trajectory b to obstacle k at its own time t in [0, D_b] is
 *     d(t) = sqrt(sum_a (s_a max(lo_a - p_a(t), 0, p_a(t) - hi_a))^2),
 * 0.0 inside the box; D_b is the left-to-right prefix sum of the trajectory's times, the
 * `duration` of the extrema record.  d_min is the minimum of d over the closed intervals of all
 * segments; t_min is a time in [0, D_b] at which the returned d_min is attained (a knot's
 * prefix sum plus the local time, clamped to D_b; which one among ties is unspecified).
 *   Per trajectory i, over all usable obstacles k:
 *     count[i]   the number of obstacles with d_min < r_min (strict, on the stored value)
 *     near[i]    d_min t_min of the closest of them (TGMS_SEP_STRIDE doubles)
 *     obs[i]     its index; ties on the stored d_min go to the lowest k; TGMS_NEAR_NONE when
 *                there is none, and then near = (+inf, 0.0)
 *     tested[i]  the number of obstacles for which the exact computation ran
 *     flags[i]   TGMS_SEP_CLOSE when count[i] > 0
 * K == 0 gives every usable row the "none" result.  No result depends on the launch shape or
 * on the order in which obstacles were processed.
 *   Exact computation.  On a segment d^2 is C^1 and piecewise polynomial: per axis the
 * trajectory is below the box, inside its extent or above it, and for each combination of
 * these states d^2 is one polynomial of degree <= 14.  The minimum is the least true value at
 * the segment ends and at the roots of the derivative of every combination the segment can be
 * in, which the derivative ladder of the bounds call locates; the time a trajectory enters a
 * box is such a root.  No resolution, and no cutting of the segment at the crossing times.
 *   Culling.  That computation runs only where a conservative bound cannot rule it out: the
 * hull of the trajectory's Bernstein boxes against the obstacle, then each segment's box, with
 * the margin and the cull threshold of the neighbour search.  The bound is sound: an obstacle
 * whose stored d_min would be < r_min is never culled, so count, obs and near are those of the
 * exhaustive computation; tested makes the culling observable, with count[i] <= tested[i] <=
 * the number of usable obstacles.
 *   Accuracy, on the squared distance for the reason the separation block gives:
 *     |d_min^2 - d_true^2| <= 1e-9 * L^2,
 * L the largest scaled coordinate magnitude that the trajectory reaches or a corner of the
 * obstacle has.  A trajectory that passes through a box therefore reports d_min <= sqrt(1e-9)
 * L, not necessarily 0.0 to the bit (the entry time is a located root; 0.0 is exact when a
 * segment end lies inside).  An fp64 evaluation at located candidates, not a certificate; a
 * touch of a derivative without a sign change may be skipped.
 *   An unusable trajectory (in the device call a segment count outside 1..TGMS_MAX_SEGMENTS,
 * for which nothing is read; a time that is not finite and > 0; a non-finite coefficient; a
 * non-finite result) gets TGMS_SEP_NONFINITE alone, near = NaN NaN, obs = TGMS_NEAR_NONE, count
 * = 0 and tested = 0.  An unusable obstacle (a non-finite entry, or lo > hi on an axis) is left
 * out of every search and sets TGMS_CLR_BAD_OBSTACLE in the flags of every usable trajectory:
 * the rest of each row is that of the call without the obstacle, and the bit says that a wall
 * may be missing from the answer.
 *   At least one of near / obs / count / flags must be non-NULL; B == 0 is TGMS_OK and launches
 * nothing.  The device call is two kernel launches on handle scratch that grows with B and K
 * at call time (1,064 B per trajectory, 4 B per obstacle; the neighbour search's buffer),
 * ordered among the handle's calls like all its scratch, so it returns TGMS_ERR_UNSUPPORTED
 * while its stream is capturing.  On a multi handle it runs on device 0; on a host handle the
 * device call returns TGMS_ERR_UNSUPPORTED and tgms_clearance_batch computes on the calling
 * thread (the same boxes, culls and exact computation; host and device agree to the accuracy
 * above, not to the bit); on a GPU handle it does one upload, the launches and one download. */
#define TGMS_CLR_BAD_OBSTACLE 32 /* an unusable obstacle was left out of this row's search */
tgms_status tgms_clearance_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                        const double* d_seg_times, const double* d_coeffs, int32_t K,
                                        const double* d_obstacles /* [K][6]: lo[3] hi[3] */,
                                        const double* scale /* host [3], nullable */, double r_min,
                                        double* d_near /* [B][TGMS_SEP_STRIDE]: d_min t_min, nullable */,
                                        int32_t* d_obs /* [B], nullable */, int32_t* d_count /* [B], nullable */,
                                        int32_t* d_tested /* [B], nullable */, int32_t* d_flags /* [B], nullable */,
                                        void* stream);
tgms_status tgms_clearance_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                                 const double* coeffs, int32_t K, const double* obstacles, const double* scale,
                                 double r_min, double* near, int32_t* obs, int32_t* count, int32_t* tested,
                                 int32_t* flags);

/* ---- distance-field clearance: certified closest approach to a voxel map ----
 * The same question for a planner whose world is a map: a Euclidean signed distance field on a
 * voxel grid.  The cost of the call does not depend on how many obstacles the map holds.
 *   The field.  `field` (a host struct) describes the grid, `values` holds one fp32 node per
 * grid point, x fastest.  With q_a = clamp((p_a - origin_a) / h, 0, n_a - 1), i_a = min(floor
 * q_a, n_a - 2) and f_a = q_a - i_a, phi(p) is the trilinear interpolation of the eight nodes
 * of cell i at f, the nodes converted to fp64 and blended in fp64.  Outside the grid phi is
 * the value at the clamped point; there is no "left the map" flag, because tgms_bounds_batch
 * with pmin / pmax set to the grid's extent answers that exactly.  phi is Lipschitz with
 *     L = sqrt(G_x^2 + G_y^2 + G_z^2),  G_a = max over edges along a of |v(node + e_a) - v(node)| / h
 * (the derivative along a is a bilinear blend of edge differences; clamping is 1-Lipschitz);
 * for a true distance field L <= sqrt(3).
 *   lip > 0 is taken as L.  A value below the true L voids the certificate; that is the
 * caller's to get right.  lip == 0 makes the call reduce L from the values on the device, in
 * launches of its own before the search; the result stays on the device.
 *   Per trajectory b, with D_b the prefix sum of its times as in the clearance call and m* the
 * minimum of phi(p(t)) over [0, D_b]:
 *     near[b]    d_min t_min: t_min in [0, D_b] is a knot's prefix sum plus the local time,
 *                clamped, and d_min the value the call evaluated there
 *     evals[b]   the evaluations of phi the row took; every knot (the left end of every
 *                segment, the right end of the last) is always evaluated, so evals >= M + 1
 *     flags[b]   TGMS_SEP_CLOSE when d_min < r_min (strict, on the stored value);
 *                TGMS_FLD_UNRESOLVED when the row would have needed more than max_evals
 *                evaluations: it stops there and only (1) holds.  A max_evals below M + 1
 *                skips no knot: such a row returns evals = M + 1, the least knot value and
 *                TGMS_FLD_UNRESOLVED
 *   (1) Upper bound: d_min = phi(p(t_min)), so d_min >= m*.
 *   (2) Certificate, without TGMS_FLD_UNRESOLVED: m* >= min(d_min - tol, r_min).  So d_min is
 * within tol of the true minimum whenever d_min - tol < r_min, and a row without TGMS_SEP_CLOSE
 * stays at least r_min - tol away.  r_min = +inf resolves every row to tol.
 *   The search is a branch-and-bound over each segment's interval tree.  An interval is
 * discarded only when phi at its centre less L times the distance the vehicle can cover in
 * half the interval is at least min(best - tol, r_min), best the least value evaluated so far
 * for the trajectory; the distance comes from bounds of the speed and the acceleration on the
 * segment (Bernstein control values) and the speed at the centre.  The cost follows how close
 * the trajectory comes, not its duration over a step.  Both guarantees hold up to
 * 1e-9 (F + L (P + h)), F the largest |value| and P the largest coordinate magnitude the
 * trajectory reaches.  No result depends on the launch shape.  The origin is taken off each
 * segment's constant coefficient before anything is evaluated, so positions round at their size
 * within the map, not at their distance from the world's origin: a map and a batch moved by the
 * same shift, where origin + shift and c_0 + shift are exact, give the same bits.
 *   An unusable row (in the device call a segment count outside 1..TGMS_MAX_SEGMENTS, for which
 * nothing is read; a time that is not finite and > 0; a non-finite coefficient; a non-finite
 * evaluated value) gets TGMS_SEP_NONFINITE alone, near = NaN NaN and evals = 0.  The values are
 * the caller's to keep finite; which rows meet a non-finite node is unspecified.
 *   TGMS_ERR_INVALID_ARG: an n_a < 2; n_x n_y n_z > 2^31 - 1; h or an origin component not
 * finite; h <= 0; tol not finite or not > 0; r_min NaN or <= 0 (+inf is legal); lip negative
 * or not finite; max_evals < 1; field or values NULL; near, evals and flags all NULL; in the
 * device call a d_seg_times, d_coeffs or d_near that is not 16-byte aligned or d_values not
 * 4-byte aligned.  B == 0 is TGMS_OK and launches nothing.
 *   With lip > 0 the device call is one launch, uses no handle scratch and may be captured
 * into a HIP graph.  With lip == 0 it needs handle scratch for the reduction, ordered like all
 * handle scratch, so it returns TGMS_ERR_UNSUPPORTED while its stream is capturing.  On a
 * multi handle it runs on device 0; on a host handle the device call returns
 * TGMS_ERR_UNSUPPORTED and the host-pointer call computes on the calling thread from the same
 * core (host and device agree within the guarantees, not to the bit: they visit the intervals
 * in different orders).  On a GPU handle the host-pointer call uploads the values with the
 * batch every time; a caller with a large map should keep it on the device and use the device
 * call. */
typedef struct tgms_field {
    double origin[3]; /* position of node (0,0,0) */
    double h;         /* node spacing, the same on all axes */
    int32_t n[3];     /* nodes per axis; values[(k*n[1] + j)*n[0] + i], x fastest */
} tgms_field;
#define TGMS_FLD_UNRESOLVED 64 /* the row spent max_evals; only the upper bound holds */
tgms_status tgms_field_clearance_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                              const double* d_seg_times, const double* d_coeffs,
                                              const tgms_field* field /* host */, const float* d_values, double lip,
                                              double r_min, double tol, int32_t max_evals,
                                              double* d_near /* [B][TGMS_SEP_STRIDE]: d_min t_min, nullable */,
                                              int32_t* d_evals /* [B], nullable */,
                                              int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_field_clearance_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                                       const double* coeffs, const tgms_field* field, const float* values, double lip,
                                       double r_min, double tol, int32_t max_evals, double* near, int32_t* evals,
                                       int32_t* flags);

/* ---- continuous thrust and tilt bounds from differential flatness ----
 * Which candidates the vehicle can fly.  The dynamic limits of tgms_limits bound |p''|, but
 * what saturates a multirotor's motors or tips it over is the mass-normalised thrust vector
 *     f(t) = p''(t) + g e_z
 * (differential flatness: the trajectory fixes it): 6 m/s^2 of acceleration needs 3.8 m/s^2 of
 * thrust downwards, 15.8 upwards, and tilts the vehicle by 31 degrees sideways, and a_max
 * passes or fails the three alike.  Per trajectory one record of TGMS_THRUST_STRIDE doubles
 *     f_min t_fmin f_max t_fmax tilt_max t_tilt
 * f_min / f_max the minimum and maximum of ||f|| over all segments' closed intervals (m/s^2),
 * tilt_max the maximum of the angle between f and +z, atan2(sqrt(f_x^2 + f_y^2), f_z) in [0,
 * pi], over the same set (radians).  Each t_* is a time in [0, D_b] at which the stored value
 * is attained: a knot's left-to-right prefix sum of T plus the local time, clamped to D_b (the
 * clearance call's rule); which one among ties is unspecified.
 *   On a segment ||f||^2 is a polynomial of degree 10, and the stationary points of the tilt
 * are the roots of f_z h' - 2 h f_z' (h = f_x^2 + f_y^2), of degree <= 13 because the leading
 * terms cancel; the derivative ladder of the bounds call locates both.  The candidates are the
 * segment ends and the ladders' slots, and every value is evaluated from the axis polynomials
 * at the candidate, never from convolved coefficients: a constant trajectory gives f_min ==
 * f_max == g to the bit and tilt_max == 0.0, a purely vertical one with f_z > 0 tilt_max ==
 * 0.0.  O(M) work per trajectory, no resolution.
 *   g (m/s^2) must be finite and >= 0, else TGMS_ERR_INVALID_ARG; g == 0 is allowed and gives
 * the extremes of |p''| itself.
 *   flags: TGMS_THRUST_* bits against `limits`, a host struct read at call time (its values
 * travel as kernel arguments).  Strict comparisons on the very values stored; an infinite
 * entry is unchecked; a NaN entry is TGMS_ERR_INVALID_ARG; limits == NULL checks nothing, so
 * the flags can then carry TGMS_FEAS_NONFINITE only.  A trajectory with a non-finite
 * coefficient, time or result, with a T_i that is not > 0 or, in the device call, with a
 * segment count outside 1..TGMS_MAX_SEGMENTS (nothing is read for it) gets
 * TGMS_FEAS_NONFINITE alone and an all-NaN record; its neighbours are unaffected.
 *   Accuracy, with F the true f_max of the trajectory:
 *     |f_min^2 - true^2| <= 1e-9 F^2,   |f_max^2 - true^2| <= 1e-9 F^2
 * (on the squares, for the reason the separation block gives: a thrust that crosses zero
 * reports f_min <= sqrt(1e-9) F, not necessarily 0.0), and, when f_min > 0,
 *     |tilt_max - true| <= 1e-9 F / f_min   radians.
 * Where the thrust vanishes on the trajectory the tilt is discontinuous: the stored tilt_max
 * is then the maximum over the candidates and carries no accuracy claim; TGMS_THRUST_LOW is
 * what catches such a trajectory.  fp64 evaluations at located candidates, not a certificate;
 * a touch of a derivative without a sign change may be skipped, as for the bounds.
 *   The body rate |f x p'''| / ||f||^2 is tgms_rate_batch's (below); j_peak / f_min from the
 * bounds and thrust records is a sound but loose upper bound of it.
 *   At least one of rec / flags must be non-NULL; fp64 device arrays are 16-byte aligned; B == 0
 * is TGMS_OK and launches nothing.  tgms_thrust_batch_device is one kernel launch with no host
 * plan and no handle scratch, so it may be captured into a HIP graph for any batch, ragged
 * included.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_thrust_batch on a host handle computes on the calling thread
 * (the same algorithm; host and device agree to the accuracy above, not to the bit); on a GPU
 * handle it does one upload, the launch and one download (records and flags in one workspace
 * region), like tgms_bounds_batch. */
#define TGMS_THRUST_STRIDE 6 /* f_min t_fmin f_max t_fmax tilt_max t_tilt */
#define TGMS_THRUST_LOW 1    /* f_min < limits->f_min */
#define TGMS_THRUST_HIGH 2   /* f_max > limits->f_max */
#define TGMS_THRUST_TILT 4   /* tilt_max > limits->tilt_max */
/* TGMS_FEAS_NONFINITE (16) is reused */
typedef struct tgms_thrust_limits {
    double f_min, f_max, tilt_max;
} tgms_thrust_limits;
tgms_status tgms_thrust_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                     const double* d_seg_times, const double* d_coeffs, double g,
                                     const tgms_thrust_limits* limits /* host, nullable */,
                                     double* d_rec /* [B][TGMS_THRUST_STRIDE], nullable */,
                                     int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_thrust_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                              const double* seg_times, const double* coeffs, double g,
                              const tgms_thrust_limits* limits, double* rec, int32_t* flags);

/* ---- continuous body-rate bound: peak roll/pitch rate from differential flatness ----
 * What a multirotor's rate controller and gyros saturate on.  The thrust vector f(t) = p''(t) +
 * g e_z fixes the body z axis f / ||f||, and that axis turns at
 *     omega(t) = ||f x p'''|| / ||f||^2      (rad/s)
 * the magnitude of the roll/pitch body rate (f' = p''' because g is constant).  The yaw-rate
 * component about the body axis depends on the yaw plan and is NOT part of it.  j_peak / f_min
 * from the bounds and thrust records bounds omega from above, but pairs the largest jerk anywhere
 * with the lowest thrust anywhere and counts the jerk along f, which turns nothing.  Per
 * trajectory one record of TGMS_RATE_STRIDE doubles
 *     omega_max t_omega
 * omega_max the maximum of omega over all segments' closed intervals, t_omega a time in [0, D_b]
 * at which it is attained: a knot's left-to-right prefix sum of T plus the local time, clamped
 * to D_b (the thrust call's rule); which one among ties is unspecified.  seg_rec, in the
 * caller's segment order, holds per segment a row of the same layout: segment i's own maximum
 * and the local time u T_i in [0, T_i] at which it occurs, which shows the segment to lengthen.
 * The maximum over a trajectory's rows equals its omega_max to the bit.
 *   On a segment, in u = t / T, E = T^2 f has degree 5 per axis and E' = T^3 p'''.  The leading
 * terms of E x E' cancel, so its components have degree 8, N = ||E x E'||^2 degree 16 and D =
 * ||E||^2 degree 10; omega = sqrt(N) / (T D), and its stationary points are the roots of N' D -
 * 2 N D', of degree 25, which the derivative ladder of the bounds call locates.  The candidates
 * are the segment ends and the ladder's 25 slots, and every value is evaluated from the axis
 * polynomials at the candidate (f and p''' by Horner, the cross product, the sums of squares),
 * never from convolved coefficients.  Where the cross product is exactly 0.0, omega is 0.0
 * whatever the denominator: a constant trajectory and a purely vertical one give omega_max ==
 * 0.0 for every g, 0 included.  O(M) work per trajectory, no resolution.
 *   g (m/s^2) must be finite and >= 0, else TGMS_ERR_INVALID_ARG.
 *   flags: TGMS_RATE_HIGH when omega_max > omega_limit, a strict comparison on the very value
 * stored; an infinite omega_limit is unchecked; NaN is TGMS_ERR_INVALID_ARG.  A trajectory with
 * a non-finite coefficient, time or result, with a T_i that is not > 0 or, in the device call,
 * with a segment count outside 1..TGMS_MAX_SEGMENTS (nothing is read for it) gets
 * TGMS_FEAS_NONFINITE alone, an all-NaN record and all-NaN seg_rec rows (for a bad segment count
 * no row is written either); its neighbours are unaffected.
 *   Accuracy, with F = f_max and m = f_min of the thrust record and J = j_peak of the bounds
 * record, when m > 0:
 *     |omega_max - true| <= 1e-9 F J / m^2
 * (the rounding of f is relative to F, that of p''' to J; omega <= J / m; the quotient amplifies
 * by F / m).  Where the thrust vanishes on the trajectory omega is unbounded and there is no
 * accuracy claim; TGMS_THRUST_LOW of the thrust call is what catches such a trajectory.  fp64
 * evaluations at located candidates, not a certificate; a touch of a derivative without a sign
 * change may be skipped, as for the bounds.
 *   At least one of rec / seg_rec / flags must be non-NULL; fp64 device arrays are 16-byte
 * aligned; B == 0 is TGMS_OK and launches nothing.  tgms_rate_batch_device is one kernel launch
 * with no host plan and no handle scratch, so it may be captured into a HIP graph for any batch,
 * ragged included.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_rate_batch on a host handle computes on the calling thread (the
 * same algorithm; host and device agree to the accuracy above, not to the bit); on a GPU handle
 * it does one upload, the launch and one download, like tgms_thrust_batch. */
#define TGMS_RATE_STRIDE 2 /* omega_max t_omega */
#define TGMS_RATE_HIGH 1   /* omega_max > omega_limit */
/* TGMS_FEAS_NONFINITE (16) is reused */
tgms_status tgms_rate_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                   const double* d_seg_times, const double* d_coeffs, double g,
                                   double omega_limit, double* d_rec /* [B][TGMS_RATE_STRIDE], nullable */,
                                   double* d_seg_rec /* [S][TGMS_RATE_STRIDE], nullable */,
                                   int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_rate_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                            const double* coeffs, double g, double omega_limit, double* rec, double* seg_rec,
                            int32_t* flags);

/* ---- time dilation: the least uniform stretch that meets the dynamic limits ----
 * The step after the check.  tgms_bounds_batch and tgms_thrust_batch flag a candidate; this
 * call makes it flyable: per trajectory a dilation s in [s_lo, s_hi] such that the dilated
 * trajectory p_s(t) = p(t / s) violates none of the given limits, and, unless s == s_lo, meets
 * one of them, the *active* one.  The limits are v_max, a_max and j_max of `limits` (its box is
 * ignored: position extents do not change) and f_min, f_max and tilt_max of `tlimits`; an
 * infinite entry is unchecked, a NaN entry is TGMS_ERR_INVALID_ARG, a NULL struct is unchecked,
 * and f_min <= 0 checks nothing.  A dilated minimum-snap optimum is the optimum of the dilated
 * problem, so nothing is solved again: the call returns the scaled times and coefficients.
 *   The scale interval.  0 < s_lo <= s_hi, both finite, and g finite and >= 0, else
 * TGMS_ERR_INVALID_ARG.  s_lo < 1 speeds a slow candidate up to its tightest limit, s_lo = 1
 * never speeds up.  A finite tilt_max must be < pi / 2 (else TGMS_ERR_INVALID_ARG): then the
 * tilt condition is monotone in s.
 *   How s is formed.  The peaks scale as v / s, a / s^2, j / s^3, so the kinematic part is
 * closed form from the continuous peaks of the bounds call (not from samples),
 *     s_kin = max(v_peak / v_max, sqrt(a_peak / a_max), cbrt(j_peak / j_max)).
 * Gravity does not scale with time: f_s = p''(t / s) / s^2 + g e_z.  With lambda = 1 / s^2 this
 * is lambda (p'' + (g / lambda) e_z), so the thrust record of the dilated trajectory is the
 * record of the thrust call on the undilated coefficients at g' = g / lambda, the norms times
 * lambda, the tilt unchanged.  The thrust part is a bracketed root search in lambda over (0,
 * 1 / max(s_lo, s_kin)^2] on that record (Illinois steps with bisection as the safeguard, at
 * most 163 evaluations, about 10 on typical input).  f_max is convex and the tilt condition linear in
 * lambda, so each is crossed once.  f_min can be crossed several times when a trajectory
 * passes near free fall: then some crossing from feasible to infeasible is returned; the
 * returned s is still feasible, and minimal only locally.  The result is the FEASIBLE end of
 * the final bracket, whose relative width in lambda is 2^-41.  A trajectory that is feasible at
 * max(s_lo, s_kin) costs one evaluation.
 *   scale[b] = s.  active[b] is a TGMS_DIL_* code: TGMS_DIL_NONE when s == s_lo, else the limit
 * met.  flags[b]: TGMS_DIL_CAPPED when the trajectory is still infeasible at s_hi (limits that
 * exclude hover, f_max <= g and the like, end here): then s = s_hi, the outputs are scaled by
 * s_hi, and active is the limit that is worst there, by the largest of the relative excesses
 * v / v_max - 1, a / a_max - 1, j / j_max - 1, f_max / limit - 1, 1 - f_min / limit and the
 * tilt's excess in radians.  Bits TGMS_DIL_EVALS_SHIFT.. of flags hold the number of
 * evaluations of the thrust record the trajectory took (a diagnostic of the cost, at most 163;
 * host and device may differ in it): (flags >> TGMS_DIL_EVALS_SHIFT); the low bits are
 * flags & TGMS_DIL_FLAG_MASK.
 *   Outputs.  seg_times_out[i] = s T_i, and coefficient k of every segment and axis becomes
 * c_k r^k with r = 1 / s, the power formed by repeated multiplication (r, r r, (r r) r, ...):
 * that rule is part of the interface, so host and device write the same bits for the same s.
 * Each output pointer may be exactly the corresponding input pointer (in place) or an array
 * that does not overlap it; partial overlap is undefined.  In place and out of place give the
 * same bits.  Coefficients solved with non-zero end derivatives come out with those derivatives
 * scaled too (v / s, a / s^2, j / s^3 at both ends): a caller whose start state is fixed and
 * moving must solve again with the scaled times instead.
 *   An unusable trajectory (a non-finite coefficient or time, T_i <= 0, a non-finite result or,
 * in the device call, a segment count outside 1..TGMS_MAX_SEGMENTS) gets s = NaN, active = -1
 * and TGMS_FEAS_NONFINITE alone; its output rows are copied unchanged, and for a bad segment
 * count nothing is read or written for its segments.  Its neighbours are unaffected: no
 * result depends on the other trajectories of the batch.
 *   Accuracy, free of conditioning: let the bounds and thrust records of the OUTPUT be taken.
 * Feasible: no peak exceeds its limit by more than 1e-9 relative; f_min >= limit (1 - 1e-9 F /
 * limit); the tilt exceeds its limit by no more than 1e-9 F / f_min rad, F the thrust record's
 * f_max.  Tight: where active != TGMS_DIL_NONE and the trajectory is not capped, the active
 * quantity is within 1e-9 relative of its limit (the tilt within the absolute bound above).
 * Where f_min = 0 on the result (a tilt limit alone on a free-falling arc: the tilt is undefined
 * there and F / f_min cannot be formed) a vanishing thrust counts as upright: s is finite,
 * TGMS_FEAS_NONFINITE is not set, active is TGMS_DIL_TILT and f_z >= -1e-9 g on the output.
 *   At least one output must be non-NULL; fp64 device arrays are 16-byte aligned; B == 0 is
 * TGMS_OK and launches nothing.  tgms_dilate_batch_device is one kernel launch with no host plan
 * and no handle scratch, so it may be captured into a HIP graph for any batch.  On a multi
 * handle it runs on device 0; on a host handle it returns TGMS_ERR_UNSUPPORTED.
 * tgms_dilate_batch on a host handle computes on the calling thread (the same algorithm; host
 * and device agree to the accuracy above, not to the bit); on a GPU handle it does one upload,
 * the launch and one download. */
#define TGMS_DIL_CAPPED 1 /* still infeasible at s_hi: outputs are scaled by s_hi */
/* TGMS_FEAS_NONFINITE (16) is reused */
#define TGMS_DIL_FLAG_MASK 0xff
#define TGMS_DIL_EVALS_SHIFT 8 /* flags >> 8: evaluations of the thrust record */
enum {
    TGMS_DIL_NONE = 0, /* s == s_lo, no limit is active */
    TGMS_DIL_SPEED,
    TGMS_DIL_ACCEL,
    TGMS_DIL_JERK,
    TGMS_DIL_THRUST_HIGH,
    TGMS_DIL_THRUST_LOW,
    TGMS_DIL_TILT
};
tgms_status tgms_dilate_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                     const double* d_seg_times, const double* d_coeffs, double g,
                                     const tgms_limits* limits /* host, nullable; pmin/pmax ignored */,
                                     const tgms_thrust_limits* tlimits /* host, nullable */, double s_lo,
                                     double s_hi, double* d_scale /* [B], nullable */,
                                     int32_t* d_active /* [B], nullable */, int32_t* d_flags /* [B], nullable */,
                                     double* d_seg_times_out /* [S], nullable */,
                                     double* d_coeffs_out /* [S][3][8], nullable */, void* stream);
tgms_status tgms_dilate_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                              const double* coeffs, double g, const tgms_limits* limits,
                              const tgms_thrust_limits* tlimits, double s_lo, double s_hi, double* scale,
                              int32_t* active, int32_t* flags, double* seg_times_out, double* coeffs_out);

/* ---- segment re-timing: lengthen only the segments that break a limit ----
 * The cheaper repair.  tgms_dilate_batch stretches the whole flight by the factor its single worst
 * instant needs: a ten-segment trajectory whose third leg is too fast gets nine legs slowed that
 * were fine.  This call re-allocates time per segment instead: every segment gets the factor its
 * OWN continuous peaks ask for, and the caller solves again with the new times (the coefficients
 * are not scaled: unequal factors change the optimum), repeats a few rounds and closes whatever
 * is left with one tgms_dilate_batch.  Only the times feed the next tgms_solve_batch_device;
 * nothing crosses to the host in between.
 *   Per segment i with time T_i: v_i, a_i, j_i are the maxima of ||p'||, ||p''||, ||p'''|| over
 * the closed interval [0, T_i], located as the bounds call locates them and with the square root
 * of the squared maximum formed as that call forms it; a constant segment gives exactly 0.0.
 *     r_i = max(v_i / v_max, sqrt(a_i / a_max), cbrt(j_i / j_max))
 * (an infinite limit contributes 0; this is the dilation's s_kin taken per segment),
 *     s_i = min(s_hi, max(s_lo, r_i)),      seg_times_out[i] = s_i T_i   (one rounded product).
 * s_lo < 1 also shortens the segments with slack, s_lo = 1 never shortens; s_hi bounds the growth
 * of one round.  r_i is the factor that would bring the segment's own peaks to the limits if its
 * shape stayed the same; the re-solve changes the shape, so r_max after a round is not 1: nothing
 * is claimed about convergence, the flags of the next call say where it stands.
 *   seg_rec [S][TGMS_RETIME_STRIDE], in the caller's segment order: v_i a_i j_i r_i.  rec
 * [B][TGMS_RETIME_REC]: r_max D_in D_out.  r_max is the largest r_i of the trajectory and equals
 * it to the bit; D_in and D_out are the left-to-right prefix sums of T and of seg_times_out (the
 * bounds record's duration rule).  flags [B]: TGMS_RT_OVER when r_max > 1, a strict comparison on
 * the very value stored (the trajectory breaks a limit somewhere); TGMS_RT_CAPPED when some r_i >
 * s_hi (that segment got less than it asked for); TGMS_RT_CHANGED when some s_i != 1 (the times
 * differ from the input).  flags >> TGMS_RT_SEG_SHIFT is the local index 0 .. M_b-1 of the
 * segment that holds r_max, ties to the lowest.
 *   seg_times_out may be exactly seg_times (in place) or an array that does not overlap it;
 * partial overlap is undefined.  In place and out of place give the same bits.
 *   TGMS_ERR_INVALID_ARG: s_lo or s_hi not finite or outside 0 < s_lo <= 1 <= s_hi; v_max, a_max
 * or j_max NaN or <= 0; all three infinite; limits == NULL (its pmin / pmax are ignored); every
 * output NULL; an fp64 device array that is not 16-byte aligned.  B == 0 is TGMS_OK and launches
 * nothing.
 *   A trajectory with a non-finite coefficient or time, with a T_i that is not > 0, with a
 * non-finite result or, in the device call, with a segment count outside 1..TGMS_MAX_SEGMENTS
 * gets TGMS_FEAS_NONFINITE alone, an all-NaN rec row and all-NaN seg_rec rows, and its times are
 * copied unchanged; for a bad segment count nothing is read or written for its segments.  Its
 * neighbours are unaffected: no result depends on the other trajectories of the batch.
 *   Accuracy: v_i, a_i, j_i within 1e-9 relative of the true maxima (the bounds call's contract,
 * with its caveat: a touch of a derivative without a sign change may be skipped); r_i, s_i T_i
 * and the record follow from them in a handful of roundings.  Host and device agree to that
 * accuracy, not to the bit.
 *   Out of scope: thrust, tilt and body rate.  Gravity does not scale with time, so they have no
 * per-segment closed form; the caller closes those, and whatever the re-solve leaves over, with
 * tgms_dilate_batch.
 *   tgms_retime_batch_dev is one kernel launch with no host plan and no handle scratch, so it
 * may be captured into a HIP graph for any batch, ragged included.  On a multi handle it runs on
 * device 0; on a host handle it returns TGMS_ERR_UNSUPPORTED.  tgms_retime_batch on a host
 * handle computes on the calling thread (the same rule from the same code); on a GPU handle it
 * does one upload, the launch and one download, like tgms_rate_batch. */
#define TGMS_RETIME_STRIDE 4 /* seg_rec row: v a j r */
#define TGMS_RETIME_REC 3    /* rec row: r_max D_in D_out */
#define TGMS_RT_OVER 1       /* r_max > 1: a limit is exceeded on some segment */
#define TGMS_RT_CAPPED 2     /* some r_i > s_hi */
#define TGMS_RT_CHANGED 4    /* some s_i != 1 */
/* TGMS_FEAS_NONFINITE (16) is reused */
#define TGMS_RT_SEG_SHIFT 8 /* flags >> 8: the local index of the segment holding r_max */
tgms_status tgms_retime_batch_dev(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                  const double* d_seg_times, const double* d_coeffs,
                                  const tgms_limits* limits /* host; pmin/pmax ignored */, double s_lo, double s_hi,
                                  double* d_seg_times_out /* [S], nullable */,
                                  double* d_seg_rec /* [S][TGMS_RETIME_STRIDE], nullable */,
                                  double* d_rec /* [B][TGMS_RETIME_REC], nullable */,
                                  int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_retime_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                              const double* coeffs, const tgms_limits* limits, double s_lo, double s_hi,
                              double* seg_times_out, double* seg_rec, double* rec, int32_t* flags);

/* ---- corridor containment: worst excursion from per-segment convex polytopes ----
 * Does each segment stay inside its safe flight corridor.  Waypoints come from a path through
 * free space, and every leg of that path has a convex free region around it: a box, or a
 * polytope from a decomposition.  The polynomial between two waypoints is free to bulge out of
 * it; the planner's loop is solve, find the worst excursion per segment, insert a waypoint
 * there, solve again.  tgms_bounds_batch tests one axis-aligned box for the whole trajectory
 * and tgms_clearance_batch boxes to stay out of; this call takes a region per segment, with
 * slanted faces.
 *   faces [F][4] = n[3] d: a point p is inside a face when n . p <= d.  Segment s of the batch
 * (s = 0 .. S-1, S = seg_offsets[B], the row of seg_times) owns the faces
 * face_offsets[s] .. face_offsets[s+1]-1 (a CSR of faces over segments, int64), at most
 * TGMS_COR_MAX_FACES of them.  The margin of segment s is
 *     m_s = max over its faces h and t in [0, T_s] of  n_h . p(t) - d_h,
 * positive: outside.  Units are the caller's: with unit normals it is a distance; nothing is
 * normalised on the device.  A segment with no faces has m_s = -inf, time 0.0 and face
 * TGMS_NEAR_NONE.
 *   d_seg_rec [S][TGMS_COR_STRIDE] = m_s and the global time at which the stored value is
 * attained: the knot's left-to-right prefix sum of T plus the local time, clamped to D_b (the
 * clearance call's rule; which one among ties is unspecified); d_seg_face [S] the face that
 * attains it, as an index into faces.  d_rec [B][TGMS_COR_STRIDE] = the largest m_s of the
 * trajectory and its time, d_where [B][2] = its segment (0 .. M_b-1) and face (index into
 * faces).  A trajectory none of whose segments has a face gets (-inf, 0.0), where = (-1, -1)
 * and no flag.  Ties on the stored margin go to the lowest segment, then to the lowest face
 * index: (margin, segment, face) is a total order, so no result depends on the launch shape or
 * the processing order.
 *   face_offsets == NULL is shared mode: all F faces apply to every segment, the flight volume
 * as one convex polytope (a slanted net, a roof).  It requires F <= TGMS_COR_MAX_FACES, is
 * bit-equal to the CSR call that repeats the same faces for every segment, and reports the face
 * as the index into the F faces.
 *   On a segment n . p(t) - d is a polynomial of degree 7; its maximum over [0, T] is the best
 * of the two ends and the roots of a derivative of degree 6, which the derivative ladder of the
 * bounds call locates from the segment's normalised coefficients projected onto n.  The
 * candidates are u = 0, u = 1 and the ladder's six slots, and every value is evaluated from
 * the three axis polynomials at the candidate -- three Horner chains, then
 *     fma(n_z, p_z, fma(n_y, p_y, fma(n_x, p_x, -d)))
 * -- never from the projected coefficients: a constant trajectory gives n . p0 - d with exactly
 * that rounding, and a waypoint lying on a face gives what the end-point evaluation gives.
 *   flags: TGMS_COR_OUTSIDE when m_max > -r, a strict comparison on the very value stored; r
 * is the vehicle radius, or a tolerance when negative; r must be finite, else
 * TGMS_ERR_INVALID_ARG.
 *   Accuracy: |m - m_true| <= 1e-9 L_h, L_h = sum_a |n_a| max_t |p_a| + |d| of the winning
 * face.  fp64 evaluations at located candidates, not a certificate; a touch of the derivative
 * without a sign change may be skipped, as for the bounds.
 *   Unusable inputs.  A trajectory with a non-finite coefficient, a time that is not finite and
 * > 0, a segment whose face span is negative, larger than TGMS_COR_MAX_FACES or outside [0, F],
 * a non-finite result or, in the device call, a segment count outside 1..TGMS_MAX_SEGMENTS
 * gets TGMS_FEAS_NONFINITE alone, NaN records, TGMS_NEAR_NONE in where, and NaN /
 * TGMS_NEAR_NONE in its segments' rows; its neighbours are unaffected.  For a bad segment
 * count nothing is read (the trajectory's offsets say nothing about where its segments are),
 * and its segments' rows are then not written at all.  An unusable face (a non-finite entry
 * or an all-zero normal) is left out and sets TGMS_COR_BAD_FACE on every usable trajectory
 * that owns it; the rest of the row is that of the call without the face.
 *   At least one of the five outputs must be non-NULL; faces may be NULL only when F == 0;
 * 0 <= F <= INT32_MAX (a face index is an int32); fp64 arrays and face_offsets are 16-byte
 * aligned; B == 0 is TGMS_OK and launches nothing.  tgms_corridor_batch_device is one kernel
 * launch with no host plan and no handle scratch, so it may be captured into a HIP graph for
 * any batch.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_corridor_batch on a host handle computes on the calling thread
 * (the same algorithm; host and device agree to the accuracy above, not to the bit); on a GPU
 * handle it does one upload, the launch and one download (all five results in one workspace
 * region). */
#define TGMS_COR_STRIDE 2      /* m_max t_max */
#define TGMS_COR_MAX_FACES 256 /* faces of one segment at most */
#define TGMS_COR_OUTSIDE 1     /* m_max > -r */
#define TGMS_COR_BAD_FACE 32   /* an unusable face was left out of this row */
/* TGMS_FEAS_NONFINITE (16) and TGMS_NEAR_NONE (-1) are reused */
tgms_status tgms_corridor_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                       const double* d_seg_times, const double* d_coeffs, int64_t F,
                                       const double* d_faces /* [F][4] = n[3] d */,
                                       const int64_t* d_face_offsets /* [S+1], S = seg_offsets[B]; NULL: all F faces apply to every segment */,
                                       double r, double* d_rec /* [B][TGMS_COR_STRIDE], nullable */,
                                       int32_t* d_where /* [B][2] = segment (0..M_b-1), face (index into faces), nullable */,
                                       double* d_seg_rec /* [S][TGMS_COR_STRIDE], nullable */,
                                       int32_t* d_seg_face /* [S], nullable */,
                                       int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_corridor_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* seg_times,
                                const double* coeffs, int64_t F, const double* faces, const int64_t* face_offsets,
                                double r, double* rec, int32_t* where, double* seg_rec, int32_t* seg_face,
                                int32_t* flags);

/* ---- corridor split: insert waypoints at the worst excursions ----
 * The third step of the planner's loop (solve, find the worst excursion per segment, insert a
 * waypoint there, solve again), on the results of one tgms_corridor_batch call: d_seg_rec and
 * d_seg_face are that call's, with the same faces, face_offsets and r.  The call rebuilds the
 * batch -- seg_offsets, waypoints, seg_times and the CSR of faces -- with the new waypoints in
 * place, ready for the next solve.  The caller sizes the outputs for the most the call can
 * produce, 2 S segments (S = seg_offsets[B]) and 2 F faces: d_seg_offsets_out [B+1],
 * d_waypoints_out [2S+B][3], d_seg_times_out [2S], d_faces_out [2F][4], d_face_offsets_out
 * [2S+1], d_parent [2S]; d_totals [2] receives S' and F', the rows that were written.
 *   Which segments are split.  Segment s of a usable trajectory is wanted when m_s > -r, the
 * corridor flag's comparison: strict, on the stored d_seg_rec[s][0]; -inf (no faces) is never
 * wanted.  Its local time is t_loc = min(max(t_s - knot_s, 0), T_s), knot_s the left-to-right
 * prefix sum of T that the corridor call uses.  A wanted segment with t_loc <= 2^-20 T_s or
 * t_loc >= (1 - 2^-20) T_s is not split and sets TGMS_SPLIT_AT_END: its worst excursion is at a
 * waypoint, which no inserted waypoint repairs (and t_s - knot_s is not exact to the bit at the
 * right end).  Of the w wanted segments that remain in a trajectory of M_b segments the first
 * min(w, TGMS_MAX_SEGMENTS - M_b) are split, in the order larger m_s, then lower segment; one
 * that is dropped sets TGMS_SPLIT_FULL.  TGMS_SPLIT_DONE says that at least one was split.
 *   Times.  lo = min_frac T_s, hi = T_s - lo, T_left = min(max(t_loc, lo), hi), T_right = T_s -
 * T_left, every operation rounded on its own (no fused multiply-add): the times are specified to
 * the bit and are the same on the device, on the host backend and in any fp64 re-computation.
 * min_frac must be finite, > 0 and <= 0.5.
 *   The inserted waypoint.  TGMS_SPLIT_PULL: x = p(T_left) from the three axis Horner chains of
 * the segment's coefficients, q = fma(n_z, x_z, fma(n_y, x_y, fma(n_x, x_x, -d))) for face
 * d_seg_face[s]; where q > -r the point is x - ((q + r) / (n . n)) n, else x.  Nothing assumes
 * unit normals.  The point then has margin -r against that one face and nothing is promised
 * about the others.  TGMS_SPLIT_CHORD: w_i + (T_left / T_s) (w_i+1 - w_i) from the input
 * waypoints; by convexity it is inside every face that both waypoints are inside, so this mode
 * guarantees containment of the new waypoint and PULL stays closer to the solved path.
 *   Copied data.  The original waypoints and the times of unsplit segments are copied bit for
 * bit.  end_derivs apply to a trajectory's two ends, which do not move: they stay valid as they
 * are and are not an argument.
 *   Faces.  CSR mode: the output lists the segments in their new order; each child of a split
 * segment owns its own copy of the parent's span, in the parent's order (a CSR cannot share a
 * span: face_offsets[s+1] is an end and a start).  d_parent[s'] is the input segment row that
 * s' came from, so a caller can carry its own per-segment data.  Shared mode (d_face_offsets
 * NULL): d_faces_out and d_face_offsets_out must be NULL and F' = F.
 *   Unusable trajectories.  A trajectory with a non-finite coefficient, time or waypoint, a
 * time that is not > 0, a NaN in one of its d_seg_rec rows, a d_seg_face outside its segment's
 * span while the segment is wanted, or a face span that the corridor call rejects is copied
 * through unchanged with TGMS_FEAS_NONFINITE alone; a span that cannot be used owns no face
 * afterwards.  In the device call a segment count outside 1..TGMS_MAX_SEGMENTS means that
 * nothing can be read for the trajectory: it becomes one placeholder segment with a NaN time,
 * two NaN waypoints, parent TGMS_NEAR_NONE and no faces, so that the output stays a valid CSR
 * and the solve that follows reports TGMS_ERR_INVALID_ARG for that row alone; its neighbours are
 * unaffected.  Only such offsets can make the output exceed the capacities above; rows beyond
 * them are then not written, so no write lands outside a buffer.
 *   No result depends on the launch shape, and a repeated call gives the same bits.  The host
 * backend's integers and times are the device's to the bit; inserted waypoints agree to 1e-9 of
 * max |p| over the segment.
 *   d_parent and d_flags are nullable.  The fp64 and int64 arrays are 16-byte aligned; mode
 * outside the two above, a non-finite r or a bad min_frac is TGMS_ERR_INVALID_ARG; B == 0 is
 * TGMS_OK, writes d_seg_offsets_out[0] = 0 and d_totals = (0, 0 or, in shared mode, F) and
 * nothing else.  The device call runs five launches on `stream` (plan, three for the prefix
 * sums, write) on handle scratch that grows with B: like tgms_neighbors_batch_device it returns
 * TGMS_ERR_UNSUPPORTED while its stream is capturing and is ordered among the handle's other
 * scratch users.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_corridor_split_batch on a host handle computes on the calling
 * thread; on a GPU handle it does one upload, the launches and one download, and copies the
 * first S' / F' rows to the caller. */
#define TGMS_SPLIT_PULL 0   /* p(t) moved back along -n of the segment's worst face to margin -r */
#define TGMS_SPLIT_CHORD 1  /* the point of the straight line between the segment's two waypoints at the same fraction */
#define TGMS_SPLIT_DONE 1   /* at least one segment of this trajectory was split */
#define TGMS_SPLIT_FULL 2   /* a wanted split was dropped: M would exceed TGMS_MAX_SEGMENTS */
#define TGMS_SPLIT_AT_END 4 /* a flagged segment's worst excursion is at a waypoint: not split */
/* TGMS_FEAS_NONFINITE (16) is reused */
tgms_status tgms_corridor_split_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                             const double* d_waypoints, const double* d_seg_times,
                                             const double* d_coeffs, int64_t F, const double* d_faces,
                                             const int64_t* d_face_offsets /* NULL: shared mode */,
                                             const double* d_seg_rec /* [S][2] of the corridor call */,
                                             const int32_t* d_seg_face /* [S] */, double r, int mode,
                                             double min_frac, int32_t* d_seg_offsets_out /* [B+1] */,
                                             double* d_waypoints_out /* [2S+B][3] */,
                                             double* d_seg_times_out /* [2S] */,
                                             double* d_faces_out /* [2F][4], NULL in shared mode */,
                                             int64_t* d_face_offsets_out /* [2S+1], NULL in shared mode */,
                                             int32_t* d_parent /* [2S], nullable */,
                                             int64_t* d_totals /* [2]: S', F' */,
                                             int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_corridor_split_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                      const double* waypoints, const double* seg_times, const double* coeffs,
                                      int64_t F, const double* faces, const int64_t* face_offsets,
                                      const double* seg_rec, const int32_t* seg_face, double r, int mode,
                                      double min_frac, int32_t* seg_offsets_out, double* waypoints_out,
                                      double* seg_times_out, double* faces_out, int64_t* face_offsets_out,
                                      int32_t* parent, int64_t* totals, int32_t* flags);

/* ---- replan cut: restart each trajectory from its state at a given time ----
 * What a planner does on every tick after the first: vehicle b is at time t_cut[b] of its solved
 * trajectory and is replanned from where it is.  The call rebuilds the batch -- seg_offsets,
 * waypoints, seg_times and end_derivs -- without the segments that lie behind, with the segment
 * the vehicle is in shortened and with its state (p, v, a, j) there as the start, ready for the
 * next tgms_solve_batch_device.  A minimum-snap trajectory is the optimum of a problem whose
 * state is (p, p', p'', p''') and whose control is the snap, so the tail of an optimum is the
 * optimum of the tail problem: solving the output reproduces the old tail (d_coeffs_out) unless
 * the caller moves a waypoint first.  No output can be larger than its input: d_seg_offsets_out
 * [B+1], d_waypoints_out [S+B][3], d_seg_times_out [S], d_end_derivs_out [B][2][3][3],
 * d_coeffs_out [S][3][8], d_parent [S], d_t0_out [B], d_flags [B], S = seg_offsets[B];
 * d_totals [1] receives S', the segment rows that were written.
 *   Knots.  k_0 = 0, k_m+1 = k_m + T_m, added left to right, each sum rounded: the corridor
 * call's prefix sum.  D = k_M.
 *   Where the cut falls.  t_cut[b] >= D finishes the trajectory (below).  Otherwise t_c =
 * min(max(t_cut[b], 0), D); s is the number of m in 1..M-1 with k_m <= t_c, so a cut exactly on an
 * interior knot belongs to the later segment at local time 0; t_loc = min(max(t_c - k_s, 0), T_s)
 * and rem = T_s - t_loc.  If rem <= 0 or rem < min_frac T_s (product and comparison in plain
 * fp64, no fused multiply-add) the cut snaps forward to knot s+1: off the last segment the
 * trajectory is finished, else s <- s+1, t_loc = 0 and TGMS_CUT_SNAPPED is set.  min_frac is
 * finite with 0 <= min_frac < 1, else TGMS_ERR_INVALID_ARG; it exists because a vanishing first
 * segment ruins the conditioning of the solve that follows.
 *   The rows of a usable, unfinished trajectory.  M' = M - s.  Times: T_s - t_loc (one rounded
 * subtraction) when t_loc > 0, else T_s copied; then T_s+1 .. copied bit for bit.  Waypoints: the
 * first is w_s copied bit for bit when t_loc == 0, else p(t_loc) from the three axis Horner
 * chains of segment s; then w_s+1 .. w_M copied.  Start of end_derivs_out: when s == 0 and
 * t_loc == 0 the input's start derivatives (zeros when d_end_derivs is NULL), else p', p'', p'''
 * of segment s at t_loc; its final half is the input's, or zeros.  coeffs_out: segment s
 * Taylor-shifted to local time 0 at t_loc (copied when t_loc == 0), the rest copied bit for bit:
 * the tail without a solve.  parent[s'] is the input segment row that s' came from, so a caller
 * can carry face spans or other per-segment data.  t0_out = k_s + t_loc (one add) is the time on
 * the old clock at which the new trajectory starts: what a caller adds to start_times for the
 * separation call.  TGMS_CUT_DONE says that something was removed (s > 0 or t_loc > 0); a cut at
 * or before 0, -inf included, reproduces the trajectory bit for bit with no flag.
 *   Finished (TGMS_CUT_FINISHED with TGMS_CUT_DONE, never TGMS_CUT_SNAPPED: the cut is at or
 * beyond D, +inf included, or snapped off the last segment).  One hold segment, the separation
 * call's convention (the vehicle holds the end point): waypoints (w_M, w_M), the time T_M-1
 * copied, all six end derivatives zero, coeffs_out the constant w_M, parent the last input row,
 * t0_out = D.
 *   Unusable trajectories.  A trajectory with a non-finite coefficient, time, waypoint or end
 * derivative, a NaN t_cut, or a time that is not > 0 is copied through unchanged with
 * TGMS_FEAS_NONFINITE alone; its t0_out is NaN and its end_derivs_out the input row or zeros.
 * In the device call a segment count outside 1..TGMS_MAX_SEGMENTS means that nothing can be read
 * for the trajectory: it becomes the split's placeholder -- one segment with a NaN time, two NaN
 * waypoints, NaN end derivatives and coefficients, parent TGMS_NEAR_NONE, t0_out NaN -- so that
 * the output stays a valid CSR and the solve that follows reports TGMS_ERR_INVALID_ARG for that
 * row alone; its neighbours are unaffected.  Only such offsets can make the output exceed the
 * capacities above; rows beyond them are then not written, so no write lands outside a buffer.
 *   Accuracy.  A state value of order k is within 1e-9 sum_j j!/(j-k)! |c_j| t_loc^(j-k) of the
 * exact derivative of segment s, a shifted coefficient k within 1e-9 sum_j C(j,k) |c_j|
 * t_loc^(j-k): Horner condition sums.  The host backend's integers, flags, times and t0_out are
 * the device's to the bit; states and shifted coefficients agree to that accuracy.
 *   No result depends on the launch shape, and a repeated call gives the same bits.  Outputs must
 * not overlap inputs (the compaction moves rows across workgroups).  d_seg_offsets_out,
 * d_waypoints_out, d_seg_times_out, d_end_derivs_out and d_totals are required, the other outputs
 * nullable; d_end_derivs NULL is rest to rest.  The fp64 arrays are 16-byte aligned.  B == 0 is
 * TGMS_OK, writes d_seg_offsets_out[0] = 0 and d_totals = 0 and nothing else.  The device call
 * runs five launches on `stream` (plan, the split's three for the prefix sum, write) on handle
 * scratch that grows with B: like tgms_corridor_split_batch_device it returns
 * TGMS_ERR_UNSUPPORTED while its stream is capturing and is ordered among the handle's other
 * scratch users.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_cut_batch on a host handle computes on the calling thread; on a GPU
 * handle it does one upload, the launches and one download, and copies the first S' rows to the
 * caller. */
#define TGMS_CUT_DONE 1     /* something was removed: s > 0 or t_loc > 0 */
#define TGMS_CUT_SNAPPED 2  /* too little of segment s was left: the cut moved forward to knot s+1 */
#define TGMS_CUT_FINISHED 4 /* nothing is left: one hold segment at the last waypoint */
/* TGMS_FEAS_NONFINITE (16) and TGMS_NEAR_NONE (-1) are reused */
tgms_status tgms_cut_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                  const double* d_waypoints, const double* d_seg_times,
                                  const double* d_end_derivs /* nullable */, const double* d_coeffs,
                                  const double* d_t_cut /* [B] */, double min_frac,
                                  int32_t* d_seg_offsets_out /* [B+1] */, double* d_waypoints_out /* [S+B][3] */,
                                  double* d_seg_times_out /* [S] */, double* d_end_derivs_out /* [B][2][3][3] */,
                                  double* d_coeffs_out /* [S][3][8], nullable */, int32_t* d_parent /* [S], nullable */,
                                  double* d_t0_out /* [B], nullable */, int64_t* d_totals /* [1]: S' */,
                                  int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_cut_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets, const double* waypoints,
                           const double* seg_times, const double* end_derivs, const double* coeffs,
                           const double* t_cut, double min_frac, int32_t* seg_offsets_out, double* waypoints_out,
                           double* seg_times_out, double* end_derivs_out, double* coeffs_out, int32_t* parent,
                           double* t0_out, int64_t* totals, int32_t* flags);

/* ---- corridor inflation: the largest free box per segment from a voxel map ----
 * The first step of the corridor loop: map -> corridors -> solve -> containment -> split -> solve.
 * Per leg of a waypoint path the call grows an axis-aligned box on the lattice of a tgms_field
 * until the map stops it, and returns it as six faces in exactly the layout that
 * tgms_corridor_batch and tgms_corridor_split_batch take.  The result is integers and six
 * doubles per segment with stated rounding: it does not depend on the algorithm, the launch
 * shape or the order of processing, and the host backend and the device agree to the bit.
 *   Free nodes.  Node (i, j, k) is free when values[node] >= (float)r_free, compared in fp32;
 * a NaN node is not free.  The trilinear interpolant on a cell lies between the least and the
 * greatest of its eight nodes, so a lattice box [lo_a .. hi_a] whose nodes are all free has
 * phi(p) >= (float)r_free at every point of origin + h [lo, hi], phi as in the field-clearance
 * call.  That is the certificate.
 *   The table.  tgms_field_occupancy_device turns (values, r_free) into a summed-volume table
 * [(nz+1)][(ny+1)][(nx+1)] int32, x fastest, caller-owned: table[k][j][i] is the number of
 * non-free nodes with index below (i, j, k) on every axis, so the planes i = 0, j = 0, k = 0 are
 * zero.  With it the non-free nodes of any lattice box are eight loads.  The table belongs to a
 * (map, r_free) pair; the caller rebuilds it when either changes.
 *   Seed.  Segment s of trajectory b joins waypoint rows s + b and s + b + 1 of d_waypoints
 * [S+B][3].  Per axis, mn the smaller and mx the larger coordinate of the two:
 *     lo_a = floor((mn - origin_a) / h), then lo_a -= 1 if origin_a + h lo_a > mn
 *     hi_a = ceil((mx - origin_a) / h),  then hi_a += 1 if origin_a + h hi_a < mx
 * every operation a separately rounded IEEE fp64 operation, no fused multiply-add.  Any
 * axis-aligned lattice box that holds both waypoints holds the seed.
 *   Growth.  Up to max_grow rounds; a round visits the six directions in the order +x -x +y -y
 * +z -z, each seeing the box as the directions before it left it.  An open direction closes for
 * good when its next layer lies off the grid, or when the slab -- that layer across the box's
 * current extent on the other two axes -- holds a node that is not free; otherwise the box takes
 * the layer.  Growth ends when all six directions are closed or after max_grow rounds.
 *   Outputs per segment, each nullable, at least one given:
 *     d_box [S][6] int32       lo[3] hi[3]
 *     d_faces [6S][4] fp64     n[3] d in the order +x -x +y -y +z -z, inside when n . p <= d:
 *                              +a: n = +e_a, d = origin_a + h hi_a;  -a: n = -e_a,
 *                              d = -(origin_a + h lo_a); the product and the sum each rounded
 *     d_face_offsets [S+1]     int64, 6 s
 *     d_seg_flags [S] int32
 * and per trajectory d_flags [B], the OR of its segments' flags:
 *     TGMS_INF_BLOCKED   the seed itself holds a non-free node: no axis-aligned free box exists
 *                        for this leg and the planner must subdivide it.  Box and faces are the
 *                        seed's; nothing is grown.
 *     TGMS_INF_OUTSIDE   the seed leaves the grid on some axis.  d_box = six TGMS_NEAR_NONE; the
 *                        faces are the waypoints' own bounding box (d = mx, d = -mn).
 *     TGMS_INF_CAPPED    some direction was still open after max_grow rounds.
 *     TGMS_FEAS_NONFINITE alone: a waypoint of the segment is not finite (box = TGMS_NEAR_NONE,
 *                        all 24 face entries NaN; the neighbouring segments are unaffected), or, in
 *                        the device call, the trajectory's segment count is outside
 *                        1..TGMS_MAX_SEGMENTS: nothing is read for it and its segment rows are not
 *                        written, as in the corridor call.
 * d_face_offsets[s] is written by segment s, the closing entry [S] by the last segment of
 * trajectory B - 1.
 *   TGMS_ERR_INVALID_ARG: an n_a < 2; h or an origin component not finite; h <= 0;
 * (nx+1)(ny+1)(nz+1) > 2^31 - 1; r_free not finite; max_grow < 0; a NULL input; every output
 * NULL; an fp64 or int64 array that is not 16-byte aligned.  B == 0 is TGMS_OK and launches
 * nothing.
 *   Neither device call uses handle scratch or a host plan; both may be captured into a HIP
 * graph (three launches for the table, one for the boxes).  On a multi handle both run on
 * device 0; on a host handle they return TGMS_ERR_UNSUPPORTED and tgms_corridor_inflate_batch
 * computes on the calling thread from the same core.  On a GPU handle the host-pointer call
 * uploads the values with the batch, builds the table in the handle's workspace, launches and
 * downloads; a caller with a large map keeps map and table on the device. */
#define TGMS_INF_BLOCKED 1 /* the seed holds a non-free node: box and faces are the seed's */
#define TGMS_INF_OUTSIDE 2 /* the seed leaves the grid: no box, the faces are the waypoints' bounding box */
#define TGMS_INF_CAPPED 4  /* a direction was still open after max_grow rounds */
/* TGMS_FEAS_NONFINITE (16) and TGMS_NEAR_NONE (-1) are reused */
tgms_status tgms_field_occupancy_device(tgms_handle* h, const tgms_field* field /* host */, const float* d_values,
                                        double r_free, int32_t* d_table /* [(nz+1)][(ny+1)][(nx+1)] */,
                                        void* stream);
tgms_status tgms_corridor_inflate_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                               const double* d_waypoints /* [S+B][3] */,
                                               const tgms_field* field /* host */, const int32_t* d_table,
                                               int32_t max_grow, int32_t* d_box /* [S][6], nullable */,
                                               double* d_faces /* [6S][4], nullable */,
                                               int64_t* d_face_offsets /* [S+1], nullable */,
                                               int32_t* d_seg_flags /* [S], nullable */,
                                               int32_t* d_flags /* [B], nullable */, void* stream);
tgms_status tgms_corridor_inflate_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                        const double* waypoints, const tgms_field* field, const float* values,
                                        double r_free, int32_t max_grow, int32_t* box, double* faces,
                                        int64_t* face_offsets, int32_t* seg_flags, int32_t* flags);

/* ---- corridor subdivision: split map-blocked legs until their boxes are free ----
 * What the corridor inflation asks of the planner when it reports TGMS_INF_BLOCKED: a leg whose
 * own lattice bounding box holds a non-free node is halved, and halved again, down to sixteenths,
 * until every piece has a free box or the depth runs out; the batch -- seg_offsets, waypoints and
 * seg_times -- is rebuilt on the device, ready for tgms_corridor_inflate_batch_device.  A diagonal
 * leg's box is much larger than the leg and halving the leg shrinks it eightfold, so most blocked
 * legs are blocked by their box, not by their chord.  The call also tells the planner what it
 * cannot learn otherwise: that a straight leg is certified free, or that it is not and the path
 * needs re-routing.  The result is integers and doubles with stated rounding: the host backend
 * and the device agree to the bit.
 *   Inputs.  B, d_seg_offsets and d_waypoints [S+B][3] as in the inflation call (segment s of
 * trajectory b joins rows s + b and s + b + 1); d_seg_times [S], NULL together with
 * d_seg_times_out; the grid `field` and the table of tgms_field_occupancy_device for the same
 * (map, r_free); max_depth in 0..4.  The host-pointer call takes values and r_free and builds the
 * table itself.
 *   Points.  A leg with waypoints w0, w1 has 17 points P(i), i = 0..16.  P(0) = w0 and P(16) = w1
 * bit for bit; otherwise per axis P(i)_a = w0_a + (i / 16) (w1_a - w0_a): the difference, the
 * product and the sum each a separately rounded IEEE fp64 operation, no fused multiply-add (i / 16
 * is exact).  A point depends on i only, never on the depth at which it is produced.
 *   Pieces.  Piece (k, j), 0 <= k <= 4, 0 <= j < 2^k, joins P(j 2^(4-k)) and P((j+1) 2^(4-k)).  It
 * is clear when the seed of its two end points -- the inflation call's seed rule -- lies inside
 * the grid and holds no non-free node.
 *   Demand.  need(piece, D) = 1 if the piece is clear or k == D, else need(left, D) +
 * need(right, D); need(leg, D) is that of piece (0, 0).  A leg with a waypoint coordinate or a
 * difference w1_a - w0_a that is not finite, or whose own seed leaves the grid, is never
 * subdivided: need = 1 for every D.
 *   Depth.  Per trajectory D_b is the largest D in 0..max_depth with sum_s need(leg s, D) <=
 * TGMS_MAX_SEGMENTS; D = 0 always fits.  The rule does not depend on any order of the legs, which
 * is why it is chosen over a greedy budget.
 *   Output.  The leaves of every leg at depth D_b, left to right, as a batch:
 *     d_seg_offsets_out [B+1]
 *     d_waypoints_out [S'+B][3]  the input waypoints copied bit for bit, the inserted ones P(i)
 *     d_seg_times_out [S']       a leaf of depth k gets T_s 2^-k, an exact scaling; a leaf of depth
 *                                0 is copied bit for bit
 *     d_parent [S']              the input segment row of the leaf
 *     d_seg_flags_out [S']       per leaf: TGMS_SUB_BLOCKED, TGMS_SUB_OUTSIDE or
 *                                TGMS_FEAS_NONFINITE, else 0
 *     d_totals [1]               S'
 *     d_flags [B]                the OR of the trajectory's leaves' flags, with TGMS_SUB_DONE and
 *                                TGMS_SUB_FULL
 * d_parent, d_seg_flags_out, d_flags and the pair of times are nullable.  The caller provides
 * min(2^max_depth S, TGMS_MAX_SEGMENTS B) segment rows and B more waypoint rows, S =
 * seg_offsets[B].  End derivatives belong to the two ends of a trajectory, which do not move: they
 * are not an argument.
 *     TGMS_SUB_DONE      the trajectory gained a segment.
 *     TGMS_SUB_FULL      D_b < max_depth: a deeper level did not fit TGMS_MAX_SEGMENTS.
 *     TGMS_SUB_BLOCKED   a leaf is not clear although its leg could be subdivided.  Without
 *                        TGMS_SUB_FULL (and with max_depth = 4) the chord itself comes within a
 *                        lattice cell of a non-free node at a sixteenth of the leg: re-route.  With
 *                        TGMS_SUB_FULL the budget ran out first.
 *     TGMS_SUB_OUTSIDE   the leg's own seed leaves the grid; the leg is kept whole.
 *     TGMS_FEAS_NONFINITE  a waypoint coordinate or difference of the leg is not finite; the leg
 *                        is kept whole and the other legs of the trajectory are unaffected.
 *   Guarantees.  (1) An output segment without a segment flag has phi(p) >= (float)r_free on its
 * whole chord: the certificate of the inflation call applied to its seed, which holds the chord.
 * (2) tgms_corridor_inflate_batch on the output reports TGMS_INF_BLOCKED exactly on the segments
 * that carry TGMS_SUB_BLOCKED and (3) TGMS_INF_OUTSIDE exactly on those that carry
 * TGMS_SUB_OUTSIDE: it recomputes the seeds from the same doubles.  (4) No result depends on the
 * launch shape, and a repeated call gives the same bits.
 *   In the device call a segment count outside 1..TGMS_MAX_SEGMENTS means that nothing can be read
 * for the trajectory: it becomes the split's placeholder -- one segment with a NaN time, two NaN
 * waypoints, parent TGMS_NEAR_NONE, segment flag and flags TGMS_FEAS_NONFINITE -- so that the
 * output stays a valid CSR; its neighbours are unaffected.  Only such offsets can make the output
 * exceed the capacities above; rows beyond them are then not written, so no write lands outside a
 * buffer.
 *   TGMS_ERR_INVALID_ARG: the grid rules of the inflation call; r_free not finite; max_depth
 * outside 0..4; a NULL input or required output; exactly one of the two time arrays NULL; an
 * fp64 or int64 array that is not 16-byte aligned.  Outputs must not overlap inputs.  B == 0 is
 * TGMS_OK, writes d_seg_offsets_out[0] = 0 and d_totals = 0 and nothing else.  The device call
 * runs five launches on `stream` (plan, the split's three for the prefix sum, write) on handle
 * scratch that grows with B (76 bytes a trajectory): like tgms_cut_batch_device it returns
 * TGMS_ERR_UNSUPPORTED while its stream is capturing and is ordered among the handle's other
 * scratch users.  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED.  tgms_corridor_subdivide_batch on a host handle computes on the calling
 * thread from the same core; on a GPU handle it does one upload, builds the table in the handle's
 * workspace, launches, does one download and copies the first S' rows to the caller. */
#define TGMS_SUB_DONE 1    /* the trajectory gained a segment */
#define TGMS_SUB_FULL 2    /* D_b < max_depth: the next level did not fit TGMS_MAX_SEGMENTS */
#define TGMS_SUB_BLOCKED 4 /* a leaf is not clear although its leg could be subdivided */
#define TGMS_SUB_OUTSIDE 8 /* the leg's own seed leaves the grid: kept whole */
/* TGMS_FEAS_NONFINITE (16) and TGMS_NEAR_NONE (-1) are reused */
tgms_status tgms_corridor_subdivide_batch_device(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                                 const double* d_waypoints /* [S+B][3] */,
                                                 const double* d_seg_times /* [S], nullable */,
                                                 const tgms_field* field /* host */, const int32_t* d_table,
                                                 int32_t max_depth, int32_t* d_seg_offsets_out /* [B+1] */,
                                                 double* d_waypoints_out, double* d_seg_times_out /* nullable */,
                                                 int32_t* d_parent /* nullable */,
                                                 int32_t* d_seg_flags_out /* nullable */,
                                                 int64_t* d_totals /* [1]: S' */, int32_t* d_flags /* [B], nullable */,
                                                 void* stream);
tgms_status tgms_corridor_subdivide_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                          const double* waypoints, const double* seg_times,
                                          const tgms_field* field, const float* values, double r_free,
                                          int32_t max_depth, int32_t* seg_offsets_out, double* waypoints_out,
                                          double* seg_times_out, int32_t* parent, int32_t* seg_flags_out,
                                          int64_t* totals, int32_t* flags);

/* ---- corridor re-route: detour blocked legs through the free nodes of the map ----
 * What the subdivision asks of the planner when a leaf stays TGMS_SUB_BLOCKED: the chord itself
 * passes an obstacle, so the leg needs other waypoints.  For every leg the inflation would report
 * TGMS_INF_BLOCKED for, the call searches a shortest 6-neighbour path through the free nodes of a
 * bounded window of the map, reduces it to at most max_pieces pieces whose seeds are free, and
 * rebuilds the batch -- seg_offsets, waypoints, seg_times, parents -- on the device, ready for
 * tgms_corridor_inflate_batch_device and the solve.  The result is integers and doubles with
 * stated rounding: the host backend and the device agree to the bit, and no result depends on the
 * algorithm of the search or on the launch shape.
 *   Inputs.  B, d_seg_offsets, d_waypoints [S+B][3], d_seg_times [S] (NULL together with
 * d_seg_times_out), the grid `field` and the table of tgms_field_occupancy_device as in the
 * subdivision call; margin >= 0; max_pieces in 2..8.  The host-pointer call takes values and
 * r_free and builds the table itself.  There is no flag input: the call decides from the same
 * doubles the inflation will see.
 *   Candidate.  A leg (w0, w1) is searched when every coordinate is finite, w0 and w1 differ in at
 * least one axis bit for bit, its seed (the inflation's rule) lies in the grid and holds a non-free
 * node.  Every other leg is copied bit for bit, with TGMS_FEAS_NONFINITE, TGMS_RRT_OUTSIDE, or
 * TGMS_RRT_BLOCKED (w0 == w1 in a blocked seed) where the inflation will say so, else 0.
 *   Window.  The seed [lo_a .. hi_a] widened by margin nodes on each side and clipped to the grid.
 * More than TGMS_RRT_WINDOW_NODES nodes: TGMS_RRT_WINDOW.  The cap is part of the ABI because the
 * flags depend on it.
 *   End nodes.  A is the nearest node to w0: per axis floor((w0_a - origin_a) / h + 0.5), each
 * operation a separately rounded IEEE fp64 operation, no fused multiply-add, clamped to the seed;
 * Z the same for w1.  A or Z not free: TGMS_RRT_ENDS -- the waypoint itself sits beside an
 * obstacle and the planner must move it.
 *   Distance.  dist(q) is the least number of 6-neighbour steps from Z to q through free nodes of
 * the window, an exact integer.  A unreachable: TGMS_RRT_NOPATH; the caller grows margin.
 *   Path.  N_0 = A; N_(i+1) is the first neighbour of N_i in the order +x -x +y -y +z -z that lies
 * in the window, is free and has dist = dist(N_i) - 1; the last node is Z.
 *   Points.  Q_0 = w0; Q_(1+i) = origin_a + h index_a of N_i per axis (product and sum each
 * rounded); the last point is w1.  Q_1 is dropped if it equals Q_0 bit for bit, then the
 * last-but-one point if it equals the last.
 *   Pieces.  First-fail greedy.  From the anchor Q_a (first Q_0) the points Q_(a+1), Q_(a+2), ... are
 * tested in order: clear(Q_a, Q_j) is the subdivision's predicate, the seed of the two points lies
 * in the grid and holds no non-free node.  When every remaining point is clear the last piece ends
 * at w1.  Otherwise the first j that fails ends the piece at Q_(j-1), the next anchor; but j == a +
 * 1 sets TGMS_RRT_ENDS, and an anchor that would make more than max_pieces pieces sets
 * TGMS_RRT_LONG.  The greedy stops at the first of these, in this order.  p is the number of
 * pieces; a re-routed leg has p >= 2 because (Q_0, last) is the leg's own blocked seed.
 *   Budget.  A trajectory whose legs would sum to more than TGMS_MAX_SEGMENTS -- p for a re-routed
 * leg, 1 otherwise -- is copied whole with TGMS_RRT_FULL: all or nothing, so the rule does not
 * depend on the order of the legs (the subdivision's reason).
 *   Times.  len(u, v) = sqrt((dx dx + dy dy) + dz dz), differences, products and sums each rounded,
 * the root correctly rounded.  A piece gets T_s (len(piece) / len(w0, w1)), quotient and product
 * each rounded once; a copied leg keeps its time bit for bit.
 *   Output, as in the subdivision call: d_seg_offsets_out [B+1], d_waypoints_out [S'+B][3],
 * d_seg_times_out [S'], d_parent [S'], d_seg_flags_out [S'], d_totals [1] = S', d_flags [B]; and
 * d_hops [S] per INPUT segment: dist(A) where the search reached A (also under TGMS_RRT_LONG,
 * TGMS_RRT_ENDS of the greedy and TGMS_RRT_FULL), else TGMS_NEAR_NONE.  d_parent, d_seg_flags_out,
 * d_hops, d_flags and the pair of times are nullable.  The caller provides min(max_pieces S,
 * TGMS_MAX_SEGMENTS B) segment rows and B more waypoint rows.
 *   Flags.  Every piece of a re-routed leg has flag 0.  A candidate that is kept whole carries
 * TGMS_RRT_BLOCKED and its reason (WINDOW, ENDS, NOPATH or LONG); under TGMS_RRT_FULL it carries
 * TGMS_RRT_BLOCKED alone.  d_flags[b] is the OR of the trajectory's segment flags, with
 * TGMS_RRT_DONE (it gained a segment) and TGMS_RRT_FULL.
 *   Guarantees.  (1) An output segment without a flag has a clear seed, so phi(p) >= (float)r_free
 * on its chord.  (2) tgms_corridor_inflate_batch on the output reports TGMS_INF_BLOCKED exactly on
 * the segments that carry TGMS_RRT_BLOCKED and TGMS_INF_OUTSIDE exactly on those that carry
 * TGMS_RRT_OUTSIDE.  (3) Every piece of a re-routed leg has flag 0.  (4) No result depends on the
 * launch shape, and a repeated call gives the same bits.
 *   In the device call a segment count outside 1..TGMS_MAX_SEGMENTS becomes the subdivision's
 * placeholder row; only such offsets can make the output exceed the capacities, and rows beyond
 * them are not written.
 *   TGMS_ERR_INVALID_ARG: the grid rules of the inflation call; r_free not finite; margin < 0;
 * max_pieces outside 2..8; a NULL input or required output; exactly one of the two time arrays
 * NULL; an fp64 or int64 array that is not 16-byte aligned.  B == 0 is TGMS_OK, writes
 * d_seg_offsets_out[0] = 0 and d_totals = 0 and nothing else.
 *   The device entry point is tgms_corridor_reroute_batch_dev -- deliberately not `_device`: the
 * recorded error-path fixture of the test suite enumerates every export of that ending, and a new
 * one would change a fixture that must stay as it is.  It behaves as the `_device` calls do.  It
 * runs a counter reset and seven launches on `stream` (classify, search, count, the split's three
 * for the prefix sum, write) on handle scratch that grows with B: 36 bytes a segment -- a 32-byte
 * record (piece count, flag, up to seven anchors as grid nodes) and a candidate entry -- for
 * TGMS_MAX_SEGMENTS segments a trajectory, and 12 bytes more a trajectory, 588 in all, because S is
 * not known on the host.  It returns TGMS_ERR_UNSUPPORTED while its
 * stream is capturing and is ordered among the handle's other scratch users.  The search is a
 * persistent grid of workgroups over the candidate list, each with its window's 16-bit distances in
 * LDS.  On a multi handle it runs on device 0; on a host handle it returns TGMS_ERR_UNSUPPORTED.
 * tgms_corridor_reroute_batch on a host handle computes on the calling thread from the same core
 * (the search is a queue); on a GPU handle it does one upload, builds the table in the handle's
 * workspace, launches, does one download and copies the first S' rows to the caller. */
#define TGMS_RRT_DONE 1      /* the trajectory gained a segment */
#define TGMS_RRT_FULL 2      /* the re-routed legs did not fit TGMS_MAX_SEGMENTS: copied whole */
#define TGMS_RRT_BLOCKED 4   /* the segment's seed holds a non-free node */
#define TGMS_RRT_OUTSIDE 8   /* the leg's own seed leaves the grid: kept whole */
#define TGMS_RRT_WINDOW 32   /* the window holds more than TGMS_RRT_WINDOW_NODES nodes */
#define TGMS_RRT_ENDS 64     /* an end node is not free, or a path node next to an anchor is not clear */
#define TGMS_RRT_NOPATH 128  /* no path inside the window: grow margin */
#define TGMS_RRT_LONG 256    /* the path needs more than max_pieces pieces */
#define TGMS_RRT_WINDOW_NODES 32768
/* TGMS_FEAS_NONFINITE (16) and TGMS_NEAR_NONE (-1) are reused */
tgms_status tgms_corridor_reroute_batch_dev(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                            const double* d_waypoints /* [S+B][3] */,
                                            const double* d_seg_times /* [S], nullable */,
                                            const tgms_field* field /* host */, const int32_t* d_table,
                                            int32_t margin, int32_t max_pieces,
                                            int32_t* d_seg_offsets_out /* [B+1] */, double* d_waypoints_out,
                                            double* d_seg_times_out /* nullable */, int32_t* d_parent /* nullable */,
                                            int32_t* d_seg_flags_out /* nullable */,
                                            int32_t* d_hops /* [S] per input segment, nullable */,
                                            int64_t* d_totals /* [1]: S' */, int32_t* d_flags /* [B], nullable */,
                                            void* stream);
tgms_status tgms_corridor_reroute_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                        const double* waypoints, const double* seg_times, const tgms_field* field,
                                        const float* values, double r_free, int32_t margin, int32_t max_pieces,
                                        int32_t* seg_offsets_out, double* waypoints_out, double* seg_times_out,
                                        int32_t* parent, int32_t* seg_flags_out, int32_t* hops, int64_t* totals,
                                        int32_t* flags);

/* ---- distance-field build: exact Euclidean transform of a voxel map ----
 * Step zero of the map calls: the field that tgms_field_clearance_batch_device,
 * tgms_field_occupancy_device and through it the inflation and the subdivision start from, made
 * on the device from the occupancy grid a sensor produces.  It is the exact Euclidean distance
 * transform: integers and one value per node with stated rounding, so the result does not depend
 * on the algorithm, the launch shape or the order of processing, and the host backend, the device
 * and a brute-force search over all nodes agree to the bit.
 *   Occupied and free nodes.  d_occ [nz][ny][nx] uint8, x fastest; a node is occupied when its
 * byte is not 0, else free.  Do(p) is the least sum_a (p_a - q_a)^2 over the occupied nodes q, in
 * lattice units, an exact integer; Df(p) the same over the free nodes; either is TGMS_EDT_NONE
 * when its set is empty.
 *   Cap.  R = ceil(max_dist / h), then R += 1 if h R < max_dist, every operation a separately
 * rounded IEEE fp64 operation; R is clipped to 32,768.  Squared distances are reported as
 * min(D, R^2).  Because h sqrt(R^2) = h R >= max_dist, a node farther than R spacings away cannot
 * change a value: an implementation may search a window of R nodes per axis or the whole grid, and
 * the result does not depend on which.
 *   Distance.  dist(D) = h * sqrt((double)D): the square root correctly rounded, the product
 * rounded once, no fused multiply-add; dist(TGMS_EDT_NONE) = +inf.
 *   mode 0 (unsigned).  value = (float) min(dist(Do), max_dist), d2 = min(Do, R^2).  An occupied
 * node gets exactly 0: the convention of an unsigned field (0 inside), which is what r_free of the
 * occupancy table expects.
 *   mode TGMS_EDT_SIGNED.  A free node gets value = (float) min(dist(Do) - h/2, max_dist) and d2 =
 * min(Do, R^2); an occupied node value = (float) -min(dist(Df) - h/2, max_dist) and d2 =
 * -min(Df, R^2); the difference is rounded once.  d2 is never 0.  The half-spacing offset puts the
 * zero level half-way between an occupied node and its free neighbour, and it keeps the field
 * 1-Lipschitz along the axes: for two neighbours of one kind dist changes by at most h (the
 * triangle inequality on the lattice), and an occupied node and its free neighbour have Do = Df =
 * 1, values h/2 and -h/2, again h apart; the cap and the clamp only reduce a difference.  So every
 * axis edge difference is at most h, G_a <= 1 in the field-clearance call and its L <= sqrt(3)
 * holds.  Without the offset the step across the surface would be 2 h.
 *   Outputs, each nullable, at least one given: d_values [nz][ny][nx] fp32, the tgms_field values
 * of the other map calls; d_d2, the same shape, int32.  d_work holds
 * tgms_field_edt_work_size(field, mode) bytes (two int32 per node: the passes ping-pong in it), is
 * caller-owned, 4-byte aligned and may be reused once the call's work on `stream` is done.
 *   TGMS_ERR_INVALID_ARG: an n_a < 2 or > 16,384 (3 (n - 1)^2 stays inside int32); nx ny nz >
 * 2^31 - 1; h or an origin component not finite; h <= 0; max_dist not finite or <= 0; unknown mode
 * bits; a NULL field, d_occ or d_work; d_values and d_d2 both NULL; d_values, d_d2 or d_work not
 * 4-byte aligned.  tgms_field_edt_work_size returns 0 for a field or mode the call would refuse.
 *   The device call uses no handle scratch and no host plan and may be captured into a HIP graph
 * (three launches, six in the signed mode: the same passes on the complement).  On a multi handle
 * it runs on device 0; on a host handle it returns TGMS_ERR_UNSUPPORTED and tgms_field_edt computes
 * on the calling thread from the same core (tgms_edt_core.h).  On a GPU handle tgms_field_edt
 * uploads the occupancy, runs with a workspace from the handle and downloads: for tests and
 * tools; a planner keeps map and field on the device. */
#define TGMS_EDT_SIGNED 1
#define TGMS_EDT_NONE INT32_MAX
size_t tgms_field_edt_work_size(const tgms_field* field, int32_t mode); /* bytes; 0 on a bad field */
tgms_status tgms_field_edt_device(tgms_handle* h, const tgms_field* field /* host */,
                                  const uint8_t* d_occ /* [nz][ny][nx], x fastest */, double max_dist, int32_t mode,
                                  float* d_values /* [nz][ny][nx], nullable */,
                                  int32_t* d_d2 /* the same shape, nullable */,
                                  void* d_work /* tgms_field_edt_work_size bytes, caller-owned */, void* stream);
tgms_status tgms_field_edt(tgms_handle* h, const tgms_field* field, const uint8_t* occ, double max_dist, int32_t mode,
                           float* values, int32_t* d2);

/* ---- waypoint repair: move map-blocked waypoints to the nearest free node ----
 * What the re-route asks of the planner when it reports TGMS_RRT_ENDS: the waypoint itself sits in
 * a cell with a non-free node, and no detour can fix a waypoint.  Two calls.  The first makes, per
 * map and r_free like the occupancy table, the nearest free node of every node: the argument of the
 * distance transform (a feature transform), not only its value.  The second moves every blocked
 * waypoint of a batch onto the free node nearest to it and rescales the times of the legs it
 * touched.  The results are integers and doubles with stated rounding: the host backend, the device
 * and a brute-force search over all pairs of nodes agree to the bit.
 *
 * The nearest-free map.
 *   Free node.  values[node] >= (float)r_free in fp32; NaN is not free: the occupancy call's rule.
 *   Site of a node p.  Among the free nodes q with D = sum_a (p_a - q_a)^2 <= max_shift^2, in
 * lattice units, the one with the least D; among equal D the lowest k, then the lowest j, then the
 * lowest i, which is the lowest linear index (k ny + j) nx + i.  d_nearest[p] is that linear index,
 * d_dsq[p] is D; both are TGMS_NEAR_NONE when there is no such node.  A free node is its own site
 * with D = 0.  The tie order is the one a separable transform produces (tgms_repair_core.h has the
 * argument), so an implementation may search a window of max_shift nodes per axis or whole lines,
 * and the result does not depend on which.
 *   max_shift lies in 1..32,768.  The grid rules are the distance-field build's: 2..16,384 nodes
 * per axis, nx ny nz <= 2^31 - 1.
 *   d_nearest [nz][ny][nx] int32 is required, d_dsq of the same shape is nullable.  d_work holds
 * tgms_field_nearest_free_work_size bytes (one int32 per node: the middle pass), is caller-owned,
 * 4-byte aligned and may be reused once the call's work on `stream` is done.  The outputs and the
 * workspace must not overlap each other or the values.
 *   TGMS_ERR_INVALID_ARG: the grid rules above; h or an origin component not finite; h <= 0; r_free
 * not finite; max_shift outside 1..32,768; a NULL field, d_values, d_nearest or d_work; a buffer
 * that is not 4-byte aligned.  The work size is 0 for a field the call would refuse.
 *   tgms_field_nearest_free_dev uses no handle scratch and no host plan and may be captured into a
 * HIP graph (three launches).  On a multi handle it runs on device 0; on a host handle it returns
 * TGMS_ERR_UNSUPPORTED and tgms_field_nearest_free computes on the calling thread from the same
 * core.  On a GPU handle tgms_field_nearest_free uploads the values, runs with a workspace from the
 * handle and downloads: for tests and tools.
 *
 * The repair.  seg_offsets do not change: no segment is added.  Waypoint w is row s + b of
 * trajectory b, as everywhere.
 *   Own seed.  The inflation's seed rule applied to the pair (w, w): per axis lo = floor((w_a -
 * origin_a) / h) with its corrective step, hi = ceil of the same with its own: one or two nodes an
 * axis, the corners of the waypoint's cell.
 *   Outcome, exactly one per waypoint, decided in this order.  A coordinate is not finite:
 * TGMS_FEAS_NONFINITE.  The seed leaves the grid: TGMS_RPR_OUTSIDE.  Every node of the seed has
 * d_nearest[node] == node (it is free): the waypoint is clear, flag 0.  `mode` protects it:
 * TGMS_RPR_KEPT; TGMS_RPR_KEEP_FIRST protects a trajectory's first waypoint (where the vehicle is),
 * TGMS_RPR_KEEP_LAST its last (where it must go).  Otherwise the waypoint is blocked and becomes
 * TGMS_RPR_MOVED or TGMS_RPR_STUCK as below.  In every case but TGMS_RPR_MOVED the row is copied
 * bit for bit.
 *   Nearest node.  N(w)_a = floor((w_a - origin_a) / h + 0.5), each operation a separately rounded
 * IEEE fp64 operation, no fused multiply-add, clamped to the grid: the re-route's end-node rule.
 *   Move.  q = d_nearest[N(w)].  TGMS_NEAR_NONE: TGMS_RPR_STUCK, the row is copied; the caller
 * grows max_shift.  Otherwise w'_a = origin_a + h q_a per axis, the product and the sum each
 * rounded (the re-route's point rule), and the flag is TGMS_RPR_MOVED.  d_shift is sum_a (N(w)_a -
 * q_a)^2 for a moved waypoint and TGMS_NEAR_NONE for every other.  A blocked waypoint whose nearest
 * node is free snaps onto it with shift 0.
 *   Times (d_seg_times and d_seg_times_out are NULL together or not at all).  len is the
 * re-route's: sqrt((dx dx + dy dy) + dz dz), every operation rounded once.  A leg with at least one
 * moved end gets T_s (len(w0', w1') / len(w0, w1)), quotient and product each rounded once, when
 * both lengths are finite and positive; otherwise, and for every untouched leg, the time is copied
 * bit for bit.
 *   Outputs.  d_waypoints_out [S+B][3] (required), d_seg_times_out [S], d_wp_flags [S+B], d_shift
 * [S+B] and d_flags [B], the OR of the trajectory's waypoint flags; all but the first nullable.
 * Outputs must not overlap inputs.  A segment count outside 1..TGMS_MAX_SEGMENTS follows the
 * inflation's rule: nothing is read for the trajectory, its rows are not written, and d_flags[b] =
 * TGMS_FEAS_NONFINITE.
 *   Guarantees.  (1) A moved waypoint lies on a free node.  (2) No ENDS after a full repair.  When
 * the lattice arithmetic is exact -- origin + h i and (x - origin) / h carry no rounding, for
 * instance a dyadic origin, h and waypoints -- and both waypoints of a leg are clear or
 * TGMS_RPR_MOVED, tgms_corridor_reroute_batch with the same map and r_free never reports
 * TGMS_RRT_ENDS for the leg.  The reasoning.  The re-route sets ENDS in two places.  First, an end
 * node A or Z is not free.  A moved waypoint is a free node and its own nearest node.  The nearest
 * node of a clear waypoint is a corner of its cell, hence of its own seed, all of whose nodes are
 * free; the re-route clamps to the leg's seed, which contains the waypoint's, so the clamp changes
 * nothing.  Second, the greedy fails at j = a + 1: the seed of an anchor and the very next point
 * holds a non-free node.  From the anchor Q_0 = w0 the next point is Q_1, the point of A, unless it
 * equals Q_0 and is dropped.  For a moved w0, or a clear one that lies on A, it does and is: the
 * next point is then the point of the second path node, a free 6-neighbour of A, and the seed of
 * two neighbouring free nodes is those two nodes.  Any other clear w0 has the seed of (w0, Q_1)
 * inside its own cell, all free.  Every
 * later anchor is a path node, Q_(j-1) of an earlier step, and the point after it is the next path
 * node, again a free neighbour, or w1 itself after the last path node Z: the seed of (Z, w1) lies
 * inside w1's cell when w1 is clear and is the node Z when w1 was moved (w1 = the point of Z, and
 * that point was then dropped as the last-but-one).  So no test at j = a + 1 can fail.  WINDOW,
 * NOPATH and LONG remain possible: they are about the space between the waypoints.  (3) A clear
 * waypoint is never touched.  (4) No result depends on the launch shape, and a repeated call gives
 * the same bits.
 *   The limit.  The nearest free node is nearest in the lattice, not reachable: with a large
 * max_shift a waypoint may land across a thin wall.  The caller bounds that with max_shift; a wall
 * thicker than max_shift spacings cannot be crossed.
 *   TGMS_ERR_INVALID_ARG: the grid rules above; unknown mode bits; a NULL input or d_waypoints_out;
 * exactly one of the two time arrays NULL; an fp64 array that is not 16-byte aligned; in the
 * host-pointer call also r_free not finite and max_shift out of range.  B == 0 is TGMS_OK and
 * launches nothing.
 *   The device entry points end in `_dev` -- deliberately not `_device`, for the re-route's reason:
 * the recorded error-path fixture of the test suite enumerates every export of that ending and must
 * stay as it is.  They behave as the `_device` calls do.  tgms_waypoints_repair_batch_dev is one
 * launch, uses no handle scratch and may be captured; on a multi handle it runs on device 0; on a
 * host handle it returns TGMS_ERR_UNSUPPORTED.  tgms_waypoints_repair_batch takes values, r_free
 * and max_shift and builds the map itself: on a host handle on the calling thread from the same
 * core, on a GPU handle with one upload, the map in the handle's workspace, and one download. */
#define TGMS_RPR_MOVED 1      /* the waypoint was moved onto the site of its nearest node */
#define TGMS_RPR_STUCK 2      /* blocked, and no free node within max_shift of its nearest node */
#define TGMS_RPR_KEPT 4       /* blocked, but mode protects it */
#define TGMS_RPR_OUTSIDE 8    /* the waypoint's own seed leaves the grid */
#define TGMS_RPR_KEEP_FIRST 1 /* mode: never move a trajectory's first waypoint */
#define TGMS_RPR_KEEP_LAST 2  /* mode: never move a trajectory's last waypoint */
/* TGMS_FEAS_NONFINITE (16) and TGMS_NEAR_NONE (-1) are reused */
size_t tgms_field_nearest_free_work_size(const tgms_field* field); /* bytes; 0 for a field the call refuses */
tgms_status tgms_field_nearest_free_dev(tgms_handle* h, const tgms_field* field /* host */, const float* d_values,
                                        double r_free, int32_t max_shift, int32_t* d_nearest /* [nz][ny][nx] */,
                                        int32_t* d_dsq /* the same shape, nullable */,
                                        void* d_work /* tgms_field_nearest_free_work_size bytes, caller-owned */,
                                        void* stream);
tgms_status tgms_field_nearest_free(tgms_handle* h, const tgms_field* field, const float* values, double r_free,
                                    int32_t max_shift, int32_t* nearest, int32_t* dsq);
tgms_status tgms_waypoints_repair_batch_dev(tgms_handle* h, int32_t B, const int32_t* d_seg_offsets,
                                            const double* d_waypoints /* [S+B][3] */,
                                            const double* d_seg_times /* [S], nullable */,
                                            const tgms_field* field /* host */, const int32_t* d_nearest, int32_t mode,
                                            double* d_waypoints_out /* [S+B][3] */,
                                            double* d_seg_times_out /* [S], nullable */,
                                            int32_t* d_wp_flags /* [S+B], nullable */,
                                            int32_t* d_shift /* [S+B], nullable */, int32_t* d_flags /* [B], nullable */,
                                            void* stream);
tgms_status tgms_waypoints_repair_batch(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                        const double* waypoints, const double* seg_times, const tgms_field* field,
                                        const float* values, double r_free, int32_t max_shift, int32_t mode,
                                        double* waypoints_out, double* seg_times_out, int32_t* wp_flags, int32_t* shift,
                                        int32_t* flags);

/* ---- multi-GPU ----
 * One process drives devices 0 .. device_count-1 through one handle that owns one RCCL
 * communicator per device (ncclCommInitAll, rccl.h:236; RCCL is loaded here, not at
 * library load).  The batch is split into contiguous shards of equal cost
 * (tgms_plan_shards), every shard into pieces; device 0 scatters each piece's inputs
 * to its device and gathers its coefficients / statuses back with grouped
 * ncclSend / ncclRecv (rccl.h:700, :722; per-piece counts, so ragged batches need no
 * padding) while the device solves the next piece.  Device 0 solves its own shard in
 * place.  The caller sees one device-0 batch, exactly as tgms_solve_batch_device
 * would produce it (identical coefficients: trajectories are independent).  The single-
 * device entry points applied to a multi handle run on device 0 only; the multi entry
 * points applied to a tgms_create handle run the single-device path.  Replaces nothing
 * in the reference, whose caller (TrajectoryGenerator.hpp:83, src/TrajectoryGenerator.cpp:71)
 * holds one Trajectory; this is the swarm / sampling planner's batch path (configs 4, 5). */
tgms_status tgms_create_multi(tgms_handle** out, int device_count);
int tgms_device_count(const tgms_handle* h); /* 1 for a tgms_create handle, 0 for a host handle */
/* Host-only shard planner: bounds [parts+1] of contiguous trajectory ranges with
 * ~equal cost (reduced / band: 2 + M_b, dense KKT: (14 M_b + 2)^3 per trajectory). */
tgms_status tgms_plan_shards(int32_t B, const int32_t* seg_offsets, int32_t parts, int method,
                             int32_t* bounds);
/* Host-only introspection of the multi-GPU schedule (no device, no RCCL needed): what a
 * tgms_solve_batch_multi_device / tgms_refine_loop_multi_device call over device_count
 * devices would do with this batch -- the shard bounds [device_count+1], every device's
 * piece-workspace size (ws_bytes [device_count], nullable), the pieces (trajectory /
 * segment ranges and the byte offsets of their arrays in the workspace) and every
 * point-to-point transfer in issue order: scatter groups 0..3 (piece k's inputs of every
 * device, device 0 -> dev), then gather groups 4..7 (piece k's results, dev -> device 0);
 * each transfer is one ncclSend on one side and one ncclRecv on the other.  flags:
 * TGMS_SCHED_* below.  Returns TGMS_ERR_INVALID_ARG (with *n_pieces / *n_xfers set to the
 * sizes needed) when piece_cap or xfer_cap is too small.  It does exactly the host work of
 * the call before its first transfer.  With TGMS_SCHED_REFINE: no pass over the offsets
 * (the cuts checked).  Without (a solve): for the reduced method the offsets' ends and a
 * uniform check that stops at the first 4,096-trajectory block holding two different M (a
 * ragged batch is then grouped and checked per trajectory on its devices, as a refinement
 * loop's; round 6); for the band / dense methods the full validation pass. */
#define TGMS_SCHED_REFINE 1
#define TGMS_SCHED_END_DERIVS 2
#define TGMS_SCHED_COEFFS 4
#define TGMS_SCHED_STATUS 8
#define TGMS_SCHED_COST 16
#define TGMS_SCHED_SELF_GATHER 32 /* device 0's shard through the pipeline too (TGMS_MULTI_SELF_GATHER=1) */
typedef struct tgms_piece {
    int32_t dev, piece, lo, hi; /* trajectories [lo, hi) */
    int64_t s0, s1;             /* segments [s0, s1) */
    int64_t ws_off[11];         /* byte offsets: seg_offsets (ragged: rebased for a band / dense solve,
                                   the raw slice for a refinement loop or a reduced solve),
                                   permutation, W, T, T2, ED, C, status, cost, and for a device-planned
                                   piece the device grouping's block counts and its device-side plan
                                   (uniform batches: empty regions) */
} tgms_piece;
typedef struct tgms_xfer {
    int32_t dev, piece, gather; /* gather 0: device 0 -> dev (scatter), 1: dev -> device 0 */
    int32_t array;              /* 0 W, 1 T, 2 end derivs, 3 coeffs, 4 status, 5 cost, 6 seg_offsets
                                   (the slice [lo, hi] of a device-planned piece) */
    int64_t batch_elem;         /* element offset in the device-0 batch array */
    int64_t ws_byte;            /* byte offset in dev's piece workspace */
    int64_t count;              /* elements */
    int32_t elem_bytes;         /* 8 (fp64) or 4 (int32) */
    int32_t group;              /* RCCL group (ncclGroupStart .. ncclGroupEnd) in issue order */
} tgms_xfer;
tgms_status tgms_multi_schedule(int32_t device_count, int32_t B, const int32_t* seg_offsets, int method,
                                int32_t flags, int32_t* bounds, int64_t* ws_bytes, tgms_piece* pieces,
                                int32_t piece_cap, int32_t* n_pieces, tgms_xfer* xfers, int32_t xfer_cap,
                                int32_t* n_xfers);
/* Host pointers, blocking: upload to device 0, the multi-GPU solve, one download. */
tgms_status tgms_solve_batch_multi(tgms_handle* h, int32_t B, const int32_t* seg_offsets,
                                   const double* waypoints, const double* seg_times,
                                   const double* end_derivs, double* coeffs, int32_t* status);
/* Device-0 pointers, asynchronous on `stream` (a device-0 stream).  Reduced method, ragged
 * batch (round 6): the host reads only the offsets' ends and the shard / piece cuts; every
 * device groups and checks its pieces' trajectories (as tgms_refine_loop_multi_device): a
 * trajectory with M outside 1..16 fails its piece -- TGMS_ERR_INVALID_ARG for it,
 * TGMS_ERR_SKIPPED for the piece's others, zero coefficients -- and the call returns
 * TGMS_OK, so check d_status.  Band / dense methods and uniform batches are validated on the
 * host as before (an error return names the first offending trajectory). */
tgms_status tgms_solve_batch_multi_device(tgms_handle* h, int32_t B, const int32_t* h_seg_offsets,
                                          const int32_t* d_seg_offsets, const double* d_waypoints,
                                          const double* d_seg_times, const double* d_end_derivs,
                                          double* d_coeffs, int32_t* d_status, void* stream);
/* tgms_refine_loop_device over the devices (config 5): times (in place), costs,
 * coefficients and statuses gathered back to device 0.  Every batch (uniform ones too) runs
 * the device-grouped loop; the host does no pass over the offsets (see
 * tgms_solve_batch_device above: a piece with bad offsets fails on its device). */
tgms_status tgms_refine_loop_multi_device(tgms_handle* h, int32_t B, const int32_t* h_seg_offsets,
                                          const int32_t* d_seg_offsets, const double* d_waypoints,
                                          double* d_seg_times, const double* d_end_derivs, double k_T,
                                          double eta, int32_t iters, double* d_coeffs, double* d_cost,
                                          int32_t* d_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGMS_H */
