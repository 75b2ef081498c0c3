// tgms_host.h — the explicit host backend of the C ABI (tgms_create_host; tgms_host.cpp).
// Plain C++ (no HIP): compiled by g++ into libtgms.so.
#pragma once

#include <stdint.h>

#include "tgms.h"

namespace tgms {
namespace dilate {
struct Lim;
}
namespace retime {
struct Lim;
}
namespace host {

// One trajectory (include/tgms.h layouts): waypoints [M+1][3], seg_times [M], end_derivs
// NULL or [18], coeffs [M][3][8].  Returns a tgms_status; every failure writes exact zeros.
int solve(int M, const double* waypoints, const double* seg_times, const double* end_derivs, double* coeffs);

// ns samples (tgms_sample_count) of one solved trajectory into out [ns][TGMS_GOAL_STRIDE].
void sample(int M, const double* coeffs, const double* seg_times, const double* waypoints, const double* end_derivs,
            double dt, int yaw_mode, double yaw_const, int64_t ns, double* out);

// Those ns samples reduced to rec [TGMS_EXTREMA_STRIDE] (pmin pmax v_peak a_peak j_peak
// duration) without storing them: the same scan and Horner chains as sample().  Returns the
// TGMS_FEAS_* bits against lim (nullable: nothing checked), TGMS_FEAS_NONFINITE alone (rec
// all NaN) when an input or a result is not finite.
int extrema(int M, const double* coeffs, const double* seg_times, const double* waypoints, const double* end_derivs,
            double dt, const tgms_limits* lim, double* rec);

// The continuous counterpart (include/tgms.h tgms_bounds_batch): the same record and flags from
// the stationary points of the polynomials on every segment's closed interval, no dt.  The
// algorithm is the kernel's (tgms_bounds_core.h), one item after the other.
int bounds(int M, const double* coeffs, const double* seg_times, const tgms_limits* lim, double* rec);

// The continuous thrust and tilt bounds (include/tgms.h tgms_thrust_batch) of one trajectory:
// rec [TGMS_THRUST_STRIDE] = f_min t_fmin f_max t_fmax tilt_max t_tilt of f = p'' + g e_z;
// returns the TGMS_THRUST_* bits against lim (nullable: nothing checked), TGMS_FEAS_NONFINITE
// alone (rec all NaN) for an unusable trajectory.  The algorithm is the kernel's
// (tgms_thrust_core.h), one segment after the other.
int thrust(int M, const double* coeffs, const double* seg_times, double g, const tgms_thrust_limits* lim,
           double* rec);

// The continuous body-rate bound (include/tgms.h tgms_rate_batch) of one trajectory: rec
// [TGMS_RATE_STRIDE] = omega_max t_omega of ||f x p'''|| / ||f||^2, seg_rec [M][TGMS_RATE_STRIDE]
// each segment's own maximum and local time (either nullable); returns TGMS_RATE_HIGH against
// omega_limit (+inf: unchecked), TGMS_FEAS_NONFINITE alone (rec and, for a usable segment count,
// the M rows all NaN) for an unusable trajectory.  The algorithm is the kernel's
// (tgms_rate_core.h), one segment after the other.
int rate(int M, const double* coeffs, const double* seg_times, double g, double omega_limit, double* rec,
         double* seg_rec);

// Time dilation (include/tgms.h tgms_dilate_batch) of one trajectory: the least stretch in
// [s_lo, s_hi] that meets lim (tgms_dilate_core.h, resolved) into *scale, the TGMS_DIL_* code of
// the active limit into *active, the scaled times into T_out [M] and coefficients into C_out
// [M][3][8] (each nullable; T_out / C_out may be seg_times / coeffs); returns the flags.  The
// algorithm is the kernel's (tgms_dilate_core.h), one segment and one evaluation after the other.
int dilate(int M, const double* coeffs, const double* seg_times, double g, const tgms::dilate::Lim& lim, double s_lo,
           double s_hi, double* scale, int* active, double* T_out, double* C_out);

// Segment re-timing (include/tgms.h tgms_retime_batch) of one trajectory (1 <= M <=
// TGMS_MAX_SEGMENTS): the times s_i T_i into T_out [M] (may be seg_times), the rows v a j r into
// seg_rec [M][TGMS_RETIME_STRIDE], r_max D_in D_out into rec [TGMS_RETIME_REC] (each nullable);
// returns the flags.  The rule and the fold are the kernel's (tgms_retime_core.h), one segment
// after the other.
int retime(int M, const double* coeffs, const double* seg_times, const tgms::retime::Lim& lim, double s_lo,
           double s_hi, double* T_out, double* seg_rec, double* rec);

// Closest approach of one pair (include/tgms.h tgms_separation_batch): trajectory i has Mi
// segments (coeffs ci, times Ti) and starts at t0i, likewise j.  Mi or Mj == 0 says that the
// pair's index was out of range.  rec [TGMS_SEP_STRIDE] = d_min t_min; returns the TGMS_SEP_*
// bits.  The algorithm is the kernel's (tgms_separation_core.h), one interval after the other.
int separation(int Mi, const double* ci, const double* Ti, double t0i, int Mj, const double* cj, const double* Tj,
               double t0j, const double* scale, double r_min, double* rec);

// The swarm neighbour search (include/tgms.h tgms_neighbors_batch) of a whole batch, row by
// row: the boxes of every vehicle once, then per row the hull test, the walk over the
// per-segment boxes (tgms_neighbors_core.h) and separation() for what is left.  Every output
// is nullable.
void neighbors(int32_t B, const int32_t* seg_offsets, const double* seg_times, const double* coeffs,
               const double* start_times, const double* scale, double r_min, double* near, int32_t* nbr,
               int32_t* count, int32_t* tested, int32_t* flags);

// The obstacle clearance (include/tgms.h tgms_clearance_batch) of a whole batch, row by row: per
// trajectory its boxes, then per usable obstacle the hull test, the segment-box test and the
// admissible combinations of tgms_clearance_core.h for what is left.  Every output is nullable.
void clearance(int32_t B, const int32_t* seg_offsets, const double* seg_times, const double* coeffs, int32_t K,
               const double* obstacles, const double* scale, double r_min, double* near, int32_t* obs, int32_t* count,
               int32_t* tested, int32_t* flags);

// The distance-field clearance (include/tgms.h tgms_field_clearance_batch) of a whole batch, row by
// row: the knots, then each segment's interval tree of tgms_field_core.h, one after the other
// with the row's least value carried along.  lip == 0: the bound is reduced from the values
// first.  Every output is nullable.
void field_clearance(int32_t B, const int32_t* seg_offsets, const double* seg_times, const double* coeffs,
                     const tgms_field& field, const float* values, double lip, double r_min, double tol,
                     int32_t max_evals, double* near, int32_t* evals, int32_t* flags);

// The corridor inflation (include/tgms.h tgms_corridor_inflate_batch) of a whole batch: the
// summed-volume table of the map first (field_occupancy, [(nz+1)][(ny+1)][(nx+1)]), then segment by
// segment the seed and the growth of tgms_inflate_core.h.  Every output is nullable.
void field_occupancy(const tgms_field& field, const float* values, double r_free, int32_t* table);
void corridor_inflate(int32_t B, const int32_t* seg_offsets, const double* waypoints, const tgms_field& field,
                      const float* values, double r_free, int32_t max_grow, int32_t* box, double* faces,
                      int64_t* face_offsets, int32_t* seg_flags, int32_t* flags);

// The distance-field build (include/tgms.h tgms_field_edt): the row pass and the two
// lower-envelope passes of tgms_edt_core.h over the whole grid, once more on the complement when
// `mode` has TGMS_EDT_SIGNED, then the conversion.  values and d2 are nullable.
void field_edt(const tgms_field& field, const uint8_t* occ, double max_dist, int32_t mode, float* values, int32_t* d2);

// The corridor subdivision (include/tgms.h tgms_corridor_subdivide_batch) of a whole batch,
// trajectory by trajectory: the table first, then per leg the traversal of tgms_subdivide_core.h,
// the trajectory's depth and its leaves.  The offsets are valid (1..TGMS_MAX_SEGMENTS); T and
// T_out are nullable together, parent, seg_flags and flags nullable.
void subdivide(int32_t B, const int32_t* so, const double* W, const double* T, const tgms_field& field,
               const float* values, double r_free, int32_t max_depth, int32_t* so_out, double* W_out, double* T_out,
               int32_t* parent, int32_t* seg_flags, int64_t* totals, int32_t* flags);

// The corridor re-route (include/tgms.h tgms_corridor_reroute_batch) of a whole batch, trajectory
// by trajectory: the table first, then per candidate leg a queue search of its window, the descent
// and the greedy of tgms_reroute_core.h, the trajectory's budget and its rows.  The offsets are
// valid; T and T_out are nullable together, parent, seg_flags, hops and flags nullable.
void reroute(int32_t B, const int32_t* so, const double* W, const double* T, const tgms_field& field,
             const float* values, double r_free, int32_t margin, int32_t max_pieces, int32_t* so_out, double* W_out,
             double* T_out, int32_t* parent, int32_t* seg_flags, int32_t* hops, int64_t* totals, int32_t* flags);

// The waypoint repair (include/tgms.h tgms_field_nearest_free, tgms_waypoints_repair_batch).
// nearest_free: the row pass and the two lower-envelope passes of tgms_repair_core.h over the whole
// grid; dsq is nullable.  waypoints_repair: that map first, then waypoint by waypoint the decision
// of tgms_repair_core.h and leg by leg the time.  The offsets are valid; T and T_out are nullable
// together, wp_flags, shift and flags nullable.
void nearest_free(const tgms_field& field, const float* values, double r_free, int32_t max_shift, int32_t* nearest,
                  int32_t* dsq);
void waypoints_repair(int32_t B, const int32_t* so, const double* W, const double* T, const tgms_field& field,
                      const float* values, double r_free, int32_t max_shift, int32_t mode, double* W_out, double* T_out,
                      int32_t* wp_flags, int32_t* shift, int32_t* flags);

// The corridor containment (include/tgms.h tgms_corridor_batch) of a whole batch, trajectory by
// trajectory: per segment and face the item of tgms_corridor_core.h, the segment's fold in face
// order, the trajectory's fold left to right.  face_offsets NULL: all F faces apply to every
// segment.  Every output is nullable.
void corridor(int32_t B, const int32_t* seg_offsets, const double* seg_times, const double* coeffs, int64_t F,
              const double* faces, const int64_t* face_offsets, double r, double* rec, int32_t* where,
              double* seg_rec, int32_t* seg_face, int32_t* flags);

// The corridor split (include/tgms.h tgms_corridor_split_batch) of a whole batch, trajectory by
// trajectory: the decisions of tgms_corridor_split_core.h, so every integer and every time is
// the device's to the bit.  The offsets are valid (1..TGMS_MAX_SEGMENTS); parent and flags are
// nullable, faces_out and fo_out unused when fo is NULL.
void corridor_split(int32_t B, const int32_t* so, const double* W, const double* T, const double* C, int64_t F,
                    const double* faces, const int64_t* fo, const double* seg_rec, const int32_t* seg_face, double r,
                    int mode, double min_frac, int32_t* so_out, double* W_out, double* T_out, double* faces_out,
                    int64_t* fo_out, int32_t* parent, int64_t* totals, int32_t* flags);

// The replan cut (include/tgms.h tgms_cut_batch) of a whole batch, trajectory by trajectory: the
// decisions of tgms_cut_core.h, so every integer, flag, time and t0 is the device's to the bit.
// The offsets are valid (1..TGMS_MAX_SEGMENTS); ED, C_out, parent, t0_out and flags are nullable.
void cut(int32_t B, const int32_t* so, const double* W, const double* T, const double* ED, const double* C,
         const double* t_cut, double min_frac, int32_t* so_out, double* W_out, double* T_out, double* ED_out,
         double* C_out, int32_t* parent, double* t0_out, int64_t* totals, int32_t* flags);

}  // namespace host
}  // namespace tgms
