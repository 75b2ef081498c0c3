// tgms_capi_analysis.hip — the calls on a solved batch (include/tgms.h): extrema, bounds, thrust,
// rate, dilation, re-timing, corridor containment and split, replan cut, separation, neighbours,
// clearance.  Each call keeps one sequence: enter, offsets, rules, empty batch, pointers, host
// backend, stage, launch, download.
#include "tgms_capi.h"
#include "tgms_dilate_core.h"
#include "tgms_host.h"
#include "tgms_retime_core.h"
#include "tgms_separation_core.h"

#include <algorithm>
#include <cmath>
#include <limits>

using namespace tgms::capi;

extern "C" {

// ---- feasibility check: extents, peaks, limit flags ----

// The limits a launch carries: the caller's, or "nothing checked" (+-inf) for NULL.  A NaN
// entry or an empty box is the caller's error.
static bool resolve_limits(const tgms_limits* in, tgms_limits* out) {
    const double inf = std::numeric_limits<double>::infinity();
    if (!in) {
        *out = tgms_limits{{-inf, -inf, -inf}, {inf, inf, inf}, inf, inf, inf};
        return true;
    }
    *out = *in;
    for (int a = 0; a < 3; ++a)
        if (!(in->pmin[a] <= in->pmax[a])) return false;  // NaN fails too
    return !(std::isnan(in->v_max) || std::isnan(in->a_max) || std::isnan(in->j_max));
}

tgms_status tgms_extrema_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW,
                                      const double* dT, const double* dED, const double* dC, double dt,
                                      const tgms_limits* limits, double* d_extrema, int32_t* d_flags,
                                      void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (B < 0 || !(dt > 0.0) || !std::isfinite(dt)) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or dt");
    tgms_limits lim;
    if (!resolve_limits(limits, &lim)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit or pmin > pmax");
    if (!d_extrema && !d_flags) return set_err(h, TGMS_ERR_INVALID_ARG, "d_extrema and d_flags both NULL");
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC, d_extrema);
    TGMS_HIP(h, tgms::launch_extrema(B, d_so, dW, dT, dED, dC, dt, lim, d_extrema, d_flags,
                                     static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_extrema_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                               const double* seg_times, const double* end_derivs, const double* coeffs, double dt,
                               const tgms_limits* limits, double* extrema, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    if (!(dt > 0.0) || !std::isfinite(dt)) return set_err(h, TGMS_ERR_INVALID_ARG, "bad dt");
    tgms_limits lim;
    if (!resolve_limits(limits, &lim)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit or pmin > pmax");
    if (!extrema && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "extrema and flags both NULL");
    if (B == 0) return TGMS_OK;
    if (!waypoints || !seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            double rec[TGMS_EXTREMA_STRIDE];
            const int fl = tgms::host::extrema(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0,
                                               waypoints + (s0 + b) * 3,
                                               end_derivs ? end_derivs + (int64_t)b * 18 : nullptr, dt, &lim, rec);
            if (extrema) std::copy(rec, rec + TGMS_EXTREMA_STRIDE, extrema + (int64_t)b * TGMS_EXTREMA_STRIDE);
            if (flags) flags[b] = fl;
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B];
    double *dW, *dT, *dED, *dC;
    int32_t* dSo;
    Outputs out;
    const auto oRec = out.add(extrema, (size_t)B * TGMS_EXTREMA_STRIDE);
    const auto oFl = out.add(flags, (size_t)B);
    s = stage(h, {input(&dW, waypoints, (S + B) * 3), input(&dT, seg_times, S), input(&dED, end_derivs, (size_t)B * 18),
                  input(&dC, coeffs, S * 24), input(&dSo, so, (size_t)B + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_extrema(B, dSo, dW, dT, dED, dC, dt, lim, out.dev(oRec), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- continuous feasibility bounds: the same record and flags, no dt ----

tgms_status tgms_bounds_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                     const double* dC, const tgms_limits* limits, double* d_extrema,
                                     int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    tgms_limits lim;
    if (!resolve_limits(limits, &lim)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit or pmin > pmax");
    if (!d_extrema && !d_flags) return set_err(h, TGMS_ERR_INVALID_ARG, "d_extrema and d_flags both NULL");
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_extrema);
    TGMS_HIP(h, tgms::launch_bounds(B, d_so, dT, dC, lim, d_extrema, d_flags, static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_bounds_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                              const double* coeffs, const tgms_limits* limits, double* extrema, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    tgms_limits lim;
    if (!resolve_limits(limits, &lim)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit or pmin > pmax");
    if (!extrema && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "extrema and flags both NULL");
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            double rec[TGMS_EXTREMA_STRIDE];
            const int fl = tgms::host::bounds(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0, &lim, rec);
            if (extrema) std::copy(rec, rec + TGMS_EXTREMA_STRIDE, extrema + (int64_t)b * TGMS_EXTREMA_STRIDE);
            if (flags) flags[b] = fl;
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B];
    double *dT, *dC;
    int32_t* dSo;
    Outputs out;
    const auto oRec = out.add(extrema, (size_t)B * TGMS_EXTREMA_STRIDE);
    const auto oFl = out.add(flags, (size_t)B);
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dSo, so, (size_t)B + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_bounds(B, dSo, dT, dC, lim, out.dev(oRec), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- continuous thrust and tilt bounds from differential flatness ----

// The limits a launch carries: the caller's with an infinite entry of either sign turned into
// "unchecked", or nothing checked for NULL.  A NaN entry is the caller's error.
static bool resolve_thrust_limits(const tgms_thrust_limits* in, tgms_thrust_limits* out) {
    const double inf = std::numeric_limits<double>::infinity();
    *out = tgms_thrust_limits{-inf, inf, inf};
    if (!in) return true;
    if (std::isnan(in->f_min) || std::isnan(in->f_max) || std::isnan(in->tilt_max)) return false;
    if (std::isfinite(in->f_min)) out->f_min = in->f_min;
    if (std::isfinite(in->f_max)) out->f_max = in->f_max;
    if (std::isfinite(in->tilt_max)) out->tilt_max = in->tilt_max;
    return true;
}

tgms_status tgms_thrust_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                     const double* dC, double g, const tgms_thrust_limits* limits, double* d_rec,
                                     int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (B < 0 || !(g >= 0.0) || !std::isfinite(g)) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or g");
    tgms_thrust_limits lim;
    if (!resolve_thrust_limits(limits, &lim)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit");
    if (!d_rec && !d_flags) return set_err(h, TGMS_ERR_INVALID_ARG, "d_rec and d_flags both NULL");
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_rec);
    TGMS_HIP(h, tgms::launch_thrust(B, d_so, dT, dC, g, lim, d_rec, d_flags, static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_thrust_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                              const double* coeffs, double g, const tgms_thrust_limits* limits, double* rec,
                              int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    if (!(g >= 0.0) || !std::isfinite(g)) return set_err(h, TGMS_ERR_INVALID_ARG, "bad g");
    tgms_thrust_limits lim;
    if (!resolve_thrust_limits(limits, &lim)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit");
    if (!rec && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "rec and flags both NULL");
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            double r[TGMS_THRUST_STRIDE];
            const int fl = tgms::host::thrust(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0, g, &lim, r);
            if (rec) std::copy(r, r + TGMS_THRUST_STRIDE, rec + (int64_t)b * TGMS_THRUST_STRIDE);
            if (flags) flags[b] = fl;
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B];
    double *dT, *dC;
    int32_t* dSo;
    Outputs out;
    const auto oRec = out.add(rec, (size_t)B * TGMS_THRUST_STRIDE);
    const auto oFl = out.add(flags, (size_t)B);
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dSo, so, (size_t)B + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_thrust(B, dSo, dT, dC, g, lim, out.dev(oRec), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- continuous body-rate bound: peak roll/pitch rate from differential flatness ----

// The argument rules the two rate entry points share (include/tgms.h); *limit is what a launch
// carries: an infinite omega_limit of either sign is unchecked.
static tgms_status check_rate(tgms_handle* h, int32_t B, double g, double omega_limit, bool any_output,
                              double* limit) {
    if (B < 0 || !(g >= 0.0) || !std::isfinite(g)) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or g");
    if (std::isnan(omega_limit)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit");
    *limit = std::isfinite(omega_limit) ? omega_limit : std::numeric_limits<double>::infinity();
    if (!any_output) return set_err(h, TGMS_ERR_INVALID_ARG, "every output is NULL");
    return TGMS_OK;
}

tgms_status tgms_rate_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                   const double* dC, double g, double omega_limit, double* d_rec,
                                   double* d_seg_rec, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    double lim;
    const tgms_status s = check_rate(h, B, g, omega_limit, d_rec || d_seg_rec || d_flags, &lim);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_rec, d_seg_rec);
    TGMS_HIP(h, tgms::launch_rate(B, d_so, dT, dC, g, lim, d_rec, d_seg_rec, d_flags, static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_rate_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                            const double* coeffs, double g, double omega_limit, double* rec, double* seg_rec,
                            int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    double lim;
    s = check_rate(h, B, g, omega_limit, rec || seg_rec || flags, &lim);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            const int fl = tgms::host::rate(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0, g, lim,
                                            rec ? rec + (int64_t)b * TGMS_RATE_STRIDE : nullptr,
                                            seg_rec ? seg_rec + s0 * TGMS_RATE_STRIDE : nullptr);
            if (flags) flags[b] = fl;
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B];
    double *dT, *dC;
    int32_t* dSo;
    Outputs out;
    const auto oSeg = out.add(seg_rec, S * TGMS_RATE_STRIDE);
    const auto oRec = out.add(rec, (size_t)B * TGMS_RATE_STRIDE);
    const auto oFl = out.add(flags, (size_t)B);
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dSo, so, (size_t)B + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_rate(B, dSo, dT, dC, g, lim, out.dev(oRec), out.dev(oSeg), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- time dilation: the least uniform stretch that meets the dynamic limits ----

// The argument rules the two dilation entry points share (include/tgms.h), and the six limits a
// launch carries: +inf is unchecked (f_lo: <= 0), an infinite entry of either sign or a NULL
// struct likewise.
static tgms_status check_dilate(tgms_handle* h, int32_t B, double g, const tgms_limits* limits,
                                const tgms_thrust_limits* tlimits, double s_lo, double s_hi, bool any_output,
                                tgms::dilate::Lim* out) {
    const double inf = std::numeric_limits<double>::infinity();
    if (B < 0 || !(g >= 0.0) || !std::isfinite(g)) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or g");
    if (!(s_lo > 0.0) || !(s_lo <= s_hi) || !std::isfinite(s_hi))
        return set_err(h, TGMS_ERR_INVALID_ARG, "the scale interval needs 0 < s_lo <= s_hi, both finite");
    *out = tgms::dilate::Lim{inf, inf, inf, 0.0, inf, inf};
    if (limits) {
        if (std::isnan(limits->v_max) || std::isnan(limits->a_max) || std::isnan(limits->j_max))
            return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit");
        if (std::isfinite(limits->v_max)) out->v_max = limits->v_max;
        if (std::isfinite(limits->a_max)) out->a_max = limits->a_max;
        if (std::isfinite(limits->j_max)) out->j_max = limits->j_max;
    }
    tgms_thrust_limits tl;
    if (!resolve_thrust_limits(tlimits, &tl)) return set_err(h, TGMS_ERR_INVALID_ARG, "NaN limit");
    if (std::isfinite(tl.tilt_max) && !(tl.tilt_max < 1.5707963267948966))
        return set_err(h, TGMS_ERR_INVALID_ARG, "a finite tilt_max must be < pi / 2");
    out->f_lo = std::isfinite(tl.f_min) ? tl.f_min : 0.0;
    out->f_hi = tl.f_max;
    out->tilt = tl.tilt_max;
    if (!any_output) return set_err(h, TGMS_ERR_INVALID_ARG, "every output is NULL");
    return TGMS_OK;
}

tgms_status tgms_dilate_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                     const double* dC, double g, const tgms_limits* limits,
                                     const tgms_thrust_limits* tlimits, double s_lo, double s_hi, double* d_scale,
                                     int32_t* d_active, int32_t* d_flags, double* dT_out, double* dC_out,
                                     void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    tgms::dilate::Lim lim;
    const tgms_status s = check_dilate(h, B, g, limits, tlimits, s_lo, s_hi,
                                       d_scale || d_active || d_flags || dT_out || dC_out, &lim);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_scale, dT_out, dC_out);
    TGMS_HIP(h, tgms::launch_dilate(B, d_so, dT, dC, g, lim, s_lo, s_hi, d_scale, d_active, d_flags, dT_out, dC_out,
                                    static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_dilate_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                              const double* coeffs, double g, const tgms_limits* limits,
                              const tgms_thrust_limits* tlimits, double s_lo, double s_hi, double* scale,
                              int32_t* active, int32_t* flags, double* seg_times_out, double* coeffs_out) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    tgms::dilate::Lim lim;
    s = check_dilate(h, B, g, limits, tlimits, s_lo, s_hi, scale || active || flags || seg_times_out || coeffs_out,
                     &lim);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            double sc;
            int act;
            const int fl = tgms::host::dilate(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0, g, lim, s_lo, s_hi,
                                              &sc, &act, seg_times_out ? seg_times_out + s0 : nullptr,
                                              coeffs_out ? coeffs_out + s0 * 24 : nullptr);
            if (scale) scale[b] = sc;
            if (active) active[b] = act;
            if (flags) flags[b] = fl;
        }
        return TGMS_OK;
    }
    // the kernel gets nullptr for every output the caller omitted
    const size_t S = (size_t)so[B], n = (size_t)B;
    Outputs out;
    const auto oC = out.add(coeffs_out, S * 24), oT = out.add(seg_times_out, S), oS = out.add(scale, n);
    const auto oA = out.add(active, n), oF = out.add(flags, n);
    double *dT, *dC;
    int32_t* dSo;
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dSo, so, n + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_dilate(B, dSo, dT, dC, g, lim, s_lo, s_hi, out.dev(oS), out.dev(oA), out.dev(oF), out.dev(oT),
                                    out.dev(oC), h->stream));
    return out.download(h);
}

// ---- segment re-timing: lengthen only the segments that break a limit ----

// The argument rules the two re-timing entry points share (include/tgms.h), and the three limits
// a launch carries (+inf: unchecked).
static tgms_status check_retime(tgms_handle* h, int32_t B, const tgms_limits* limits, double s_lo, double s_hi,
                                bool any_output, tgms::retime::Lim* out) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (!(s_lo > 0.0) || !(s_lo <= 1.0) || !(s_hi >= 1.0) || !std::isfinite(s_hi))
        return set_err(h, TGMS_ERR_INVALID_ARG, "the scale interval needs 0 < s_lo <= 1 <= s_hi, both finite");
    if (!limits) return set_err(h, TGMS_ERR_INVALID_ARG, "limits is NULL");
    *out = tgms::retime::Lim{limits->v_max, limits->a_max, limits->j_max};
    if (!(out->v_max > 0.0) || !(out->a_max > 0.0) || !(out->j_max > 0.0))  // NaN fails too
        return set_err(h, TGMS_ERR_INVALID_ARG, "v_max, a_max and j_max must be > 0");
    if (std::isinf(out->v_max) && std::isinf(out->a_max) && std::isinf(out->j_max))
        return set_err(h, TGMS_ERR_INVALID_ARG, "all three limits are infinite");
    if (!any_output) return set_err(h, TGMS_ERR_INVALID_ARG, "every output is NULL");
    return TGMS_OK;
}

tgms_status tgms_retime_batch_dev(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT, const double* dC,
                                  const tgms_limits* limits, double s_lo, double s_hi, double* dT_out,
                                  double* d_seg_rec, double* d_rec, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    tgms::retime::Lim lim;
    const tgms_status s = check_retime(h, B, limits, s_lo, s_hi, dT_out || d_seg_rec || d_rec || d_flags, &lim);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, dT_out, d_seg_rec, d_rec);
    TGMS_HIP(h, tgms::launch_retime(B, d_so, dT, dC, lim, s_lo, s_hi, dT_out, d_seg_rec, d_rec, d_flags,
                                    static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_retime_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                              const double* coeffs, const tgms_limits* limits, double s_lo, double s_hi,
                              double* seg_times_out, double* seg_rec, double* rec, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    tgms::retime::Lim lim;
    s = check_retime(h, B, limits, s_lo, s_hi, seg_times_out || seg_rec || rec || flags, &lim);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            const int fl = tgms::host::retime(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0, lim, s_lo, s_hi,
                                              seg_times_out ? seg_times_out + s0 : nullptr,
                                              seg_rec ? seg_rec + s0 * TGMS_RETIME_STRIDE : nullptr,
                                              rec ? rec + (int64_t)b * TGMS_RETIME_REC : nullptr);
            if (flags) flags[b] = fl;
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B], n = (size_t)B;
    Outputs out;
    const auto oSeg = out.add(seg_rec, S * TGMS_RETIME_STRIDE), oT = out.add(seg_times_out, S);
    const auto oRec = out.add(rec, n * TGMS_RETIME_REC);
    const auto oF = out.add(flags, n);
    double *dT, *dC;
    int32_t* dSo;
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dSo, so, n + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_retime(B, dSo, dT, dC, lim, s_lo, s_hi, out.dev(oT), out.dev(oSeg), out.dev(oRec),
                                    out.dev(oF), h->stream));
    return out.download(h);
}

// ---- corridor containment: worst excursion from per-segment polytopes ----

// The argument rules the two corridor entry points share (include/tgms.h).
static tgms_status check_corridor(tgms_handle* h, int32_t B, int64_t F, const void* faces, const void* face_offsets,
                                  double r, const void* rec, const void* where, const void* seg_rec,
                                  const void* seg_face, const void* flags) {
    if (B < 0 || F < 0 || F > INT32_MAX) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or F");
    if (!std::isfinite(r)) return set_err(h, TGMS_ERR_INVALID_ARG, "r is not finite");
    if (!rec && !where && !seg_rec && !seg_face && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "every output is NULL");
    if (F > 0 && !faces) return set_err(h, TGMS_ERR_INVALID_ARG, "faces is NULL with F > 0");
    if (!face_offsets && F > TGMS_COR_MAX_FACES)
        return set_err(h, TGMS_ERR_INVALID_ARG, "shared faces: F > TGMS_COR_MAX_FACES");
    return TGMS_OK;
}

tgms_status tgms_corridor_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                       const double* dC, int64_t F, const double* d_faces,
                                       const int64_t* d_face_offsets, double r, double* d_rec, int32_t* d_where,
                                       double* d_seg_rec, int32_t* d_seg_face, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_corridor(h, B, F, d_faces, d_face_offsets, r, d_rec, d_where, d_seg_rec, d_seg_face, d_flags);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_faces, d_face_offsets, d_rec, d_seg_rec);
    TGMS_HIP(h, tgms::launch_corridor(B, d_so, dT, dC, F, d_faces, d_face_offsets, r, d_rec, d_where, d_seg_rec,
                                      d_seg_face, d_flags, static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_corridor_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                                const double* coeffs, int64_t F, const double* faces, const int64_t* face_offsets,
                                double r, double* rec, int32_t* where, double* seg_rec, int32_t* seg_face,
                                int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_corridor(h, B, F, faces, face_offsets, r, rec, where, seg_rec, seg_face, flags);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::corridor(B, so, seg_times, coeffs, F, faces, face_offsets, r, rec, where, seg_rec, seg_face, flags);
        return TGMS_OK;
    }
    // the kernel gets every array; what the caller omitted is dropped on the host
    const size_t S = (size_t)so[B], n = (size_t)B;
    Outputs out;
    const auto oSegRec = out.add(seg_rec, S * TGMS_COR_STRIDE, true), oRec = out.add(rec, n * TGMS_COR_STRIDE, true);
    const auto oSegFace = out.add(seg_face, S, true), oWhere = out.add(where, 2 * n, true), oFl = out.add(flags, n, true);
    double *dT, *dC, *dF;
    int64_t* dFo;
    int32_t* dSo;
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dF, faces, (size_t)F * 4),
                  input(&dFo, face_offsets, S + 1), input(&dSo, so, n + 1), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_corridor(B, dSo, dT, dC, F, dF, dFo, r, out.dev(oRec), out.dev(oWhere), out.dev(oSegRec),
                                      out.dev(oSegFace), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- corridor split: insert waypoints at the worst excursions ----

// The argument rules the two split entry points share (include/tgms.h).
static tgms_status check_split(tgms_handle* h, int32_t B, int64_t F, const void* faces, const void* face_offsets,
                               double r, int mode, double min_frac, const void* so_out, const void* W_out,
                               const void* T_out, const void* faces_out, const void* fo_out, const void* totals) {
    if (B < 0 || F < 0 || F > INT32_MAX) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or F");
    if (!std::isfinite(r)) return set_err(h, TGMS_ERR_INVALID_ARG, "r is not finite");
    if (mode != TGMS_SPLIT_PULL && mode != TGMS_SPLIT_CHORD) return set_err(h, TGMS_ERR_INVALID_ARG, "unknown mode");
    if (!std::isfinite(min_frac) || !(min_frac > 0.0) || !(min_frac <= 0.5))
        return set_err(h, TGMS_ERR_INVALID_ARG, "min_frac must be finite, > 0 and <= 0.5");
    if (!so_out || !totals) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets_out or totals is NULL");
    if (B > 0 && (!W_out || !T_out)) return set_err(h, TGMS_ERR_INVALID_ARG, "waypoints_out or seg_times_out is NULL");
    if (F > 0 && !faces) return set_err(h, TGMS_ERR_INVALID_ARG, "faces is NULL with F > 0");
    if (!face_offsets) {
        if (F > TGMS_COR_MAX_FACES) return set_err(h, TGMS_ERR_INVALID_ARG, "shared faces: F > TGMS_COR_MAX_FACES");
        if (faces_out || fo_out)
            return set_err(h, TGMS_ERR_INVALID_ARG, "shared mode: faces_out and face_offsets_out must be NULL");
    } else if (B > 0 && (!fo_out || (F > 0 && !faces_out))) {
        return set_err(h, TGMS_ERR_INVALID_ARG, "faces_out or face_offsets_out is NULL");
    }
    return TGMS_OK;
}

// The launch of either call, on the handle's scratch.
static tgms_status run_split(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dW,
                             const double* dT, const double* dC, int64_t F, const double* d_faces,
                             const int64_t* d_face_offsets, const double* d_seg_rec, const int32_t* d_seg_face, double r,
                             int mode, double min_frac, int32_t* d_so_out, double* dW_out, double* dT_out,
                             double* d_faces_out, int64_t* d_fo_out, int32_t* d_parent, int64_t* d_totals,
                             int32_t* d_flags) {
    return launch_on_scratch(h, st, "tgms_corridor_split_batch_device", "launch_corridor_split",
                             tgms::corridor_split_scratch_bytes(B), [&](void* ws) {
                                 return tgms::launch_corridor_split(B, d_so, dW, dT, dC, F, d_faces, d_face_offsets, d_seg_rec,
                                                                    d_seg_face, r, mode, min_frac, ws, d_so_out, dW_out, dT_out,
                                                                    d_faces_out, d_fo_out, d_parent, d_totals, d_flags, st);
                             });
}

tgms_status tgms_corridor_split_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW,
                                             const double* dT, const double* dC, int64_t F, const double* d_faces,
                                             const int64_t* d_face_offsets, const double* d_seg_rec,
                                             const int32_t* d_seg_face, double r, int mode, double min_frac,
                                             int32_t* d_so_out, double* dW_out, double* dT_out, double* d_faces_out,
                                             int64_t* d_fo_out, int32_t* d_parent, int64_t* d_totals,
                                             int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_split(h, B, F, d_faces, d_face_offsets, r, mode, min_frac, d_so_out, dW_out, dT_out,
                                      d_faces_out, d_fo_out, d_totals);
    if (s != TGMS_OK) return s;
    if (B > 0 && (!d_so || !dW || !dT || !dC || !d_seg_rec || !d_seg_face))
        return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dC, d_faces, d_face_offsets, d_seg_rec, dW_out, dT_out, d_faces_out, d_fo_out,
                       d_totals);
    return run_split(h, static_cast<hipStream_t>(stream), B, d_so, dW, dT, dC, F, d_faces, d_face_offsets, d_seg_rec,
                     d_seg_face, r, mode, min_frac, d_so_out, dW_out, dT_out, d_faces_out, d_fo_out, d_parent, d_totals,
                     d_flags);
}

tgms_status tgms_corridor_split_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                                      const double* seg_times, const double* coeffs, int64_t F, const double* faces,
                                      const int64_t* face_offsets, const double* seg_rec, const int32_t* seg_face,
                                      double r, int mode, double min_frac, int32_t* so_out, double* waypoints_out,
                                      double* seg_times_out, double* faces_out, int64_t* face_offsets_out,
                                      int32_t* parent, int64_t* totals, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_split(h, B, F, faces, face_offsets, r, mode, min_frac, so_out, waypoints_out, seg_times_out, faces_out,
                    face_offsets_out, totals);
    if (s != TGMS_OK) return s;
    if (B == 0) {
        so_out[0] = 0;
        totals[0] = 0;
        totals[1] = face_offsets ? 0 : F;
        return TGMS_OK;
    }
    if (!waypoints || !seg_times || !coeffs || !seg_rec || !seg_face) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::corridor_split(B, so, waypoints, seg_times, coeffs, F, faces, face_offsets, seg_rec, seg_face, r,
                                   mode, min_frac, so_out, waypoints_out, seg_times_out, faces_out, face_offsets_out,
                                   parent, totals, flags);
        return TGMS_OK;
    }
    // the outputs at the capacities of the header (2 S segments, 2 F faces), of which the first
    // S' / F' rows go to the caller; no face outputs in shared mode, every other array reaches
    // the kernel
    const size_t S = (size_t)so[B], n = (size_t)B;
    const bool per_seg = face_offsets != nullptr;
    Outputs out;
    const auto oW = out.add(waypoints_out, (2 * S + n) * 3), oT = out.add(seg_times_out, 2 * S),
               oF = out.add(faces_out, 2 * (size_t)F * 4, per_seg);
    const auto oFo = out.add(face_offsets_out, 2 * S + 1, per_seg), oTot = out.add(totals, 2);
    const auto oSo = out.add(so_out, n + 1), oPar = out.add(parent, 2 * S, true), oFl = out.add(flags, n, true);
    double *dW, *dT, *dC, *dF, *dRec;
    int64_t* dFo;
    int32_t *dSo, *dFace;
    s = stage(h, {input(&dW, waypoints, (S + n) * 3), input(&dT, seg_times, S), input(&dC, coeffs, S * 24),
                  input(&dF, faces, (size_t)F * 4), input(&dFo, face_offsets, S + 1), input(&dRec, seg_rec, S * 2),
                  input(&dSo, so, n + 1), input(&dFace, seg_face, S), output(&out)});
    if (s != TGMS_OK) return s;
    s = run_split(h, h->stream, B, dSo, dW, dT, dC, F, dF, dFo, dRec, dFace, r, mode, min_frac, out.dev(oSo), out.dev(oW),
                  out.dev(oT), out.dev(oF), out.dev(oFo), out.dev(oPar), out.dev(oTot), out.dev(oFl));
    if (s == TGMS_OK) s = out.fetch(h);
    if (s != TGMS_OK) return s;
    out.take(oTot, 2);
    const size_t S1 = (size_t)totals[0], F1 = (size_t)totals[1];
    out.take(oSo, n + 1);
    out.take(oW, (S1 + n) * 3);
    out.take(oT, S1);
    out.take(oF, F1 * 4);
    out.take(oFo, S1 + 1);
    out.take(oPar, S1);
    out.take(oFl, n);
    return TGMS_OK;
}

// ---- replan cut: restart each trajectory from its state at a given time ----

// The argument rules the two cut entry points share (include/tgms.h).
static tgms_status check_cut(tgms_handle* h, int32_t B, double min_frac, const void* so_out, const void* W_out,
                             const void* T_out, const void* ED_out, const void* totals) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (!std::isfinite(min_frac) || !(min_frac >= 0.0) || !(min_frac < 1.0))
        return set_err(h, TGMS_ERR_INVALID_ARG, "min_frac must be finite, >= 0 and < 1");
    if (!so_out || !totals) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets_out or totals is NULL");
    if (B > 0 && (!W_out || !T_out || !ED_out))
        return set_err(h, TGMS_ERR_INVALID_ARG, "waypoints_out, seg_times_out or end_derivs_out is NULL");
    return TGMS_OK;
}

// The launch of either call, on the handle's scratch.
static tgms_status run_cut(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dW,
                           const double* dT, const double* dED, const double* dC, const double* d_t_cut, double min_frac,
                           int32_t* d_so_out, double* dW_out, double* dT_out, double* dED_out, double* dC_out,
                           int32_t* d_parent, double* d_t0, int64_t* d_totals, int32_t* d_flags) {
    return launch_on_scratch(h, st, "tgms_cut_batch_device", "launch_cut", tgms::cut_scratch_bytes(B), [&](void* ws) {
        return tgms::launch_cut(B, d_so, dW, dT, dED, dC, d_t_cut, min_frac, ws, d_so_out, dW_out, dT_out, dED_out, dC_out,
                                d_parent, d_t0, d_totals, d_flags, st);
    });
}

tgms_status tgms_cut_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW, const double* dT,
                                  const double* dED, const double* dC, const double* d_t_cut, double min_frac,
                                  int32_t* d_so_out, double* dW_out, double* dT_out, double* dED_out, double* dC_out,
                                  int32_t* d_parent, double* d_t0, int64_t* d_totals, int32_t* d_flags,
                                  void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_cut(h, B, min_frac, d_so_out, dW_out, dT_out, dED_out, d_totals);
    if (s != TGMS_OK) return s;
    if (B > 0 && (!d_so || !dW || !dT || !dC || !d_t_cut)) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC, d_t_cut, dW_out, dT_out, dED_out, dC_out, d_t0, d_totals);
    return run_cut(h, static_cast<hipStream_t>(stream), B, d_so, dW, dT, dED, dC, d_t_cut, min_frac, d_so_out, dW_out,
                   dT_out, dED_out, dC_out, d_parent, d_t0, d_totals, d_flags);
}

tgms_status tgms_cut_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                           const double* seg_times, const double* end_derivs, const double* coeffs,
                           const double* t_cut, double min_frac, int32_t* so_out, double* waypoints_out,
                           double* seg_times_out, double* end_derivs_out, double* coeffs_out, int32_t* parent,
                           double* t0_out, int64_t* totals, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_cut(h, B, min_frac, so_out, waypoints_out, seg_times_out, end_derivs_out, totals);
    if (s != TGMS_OK) return s;
    if (B == 0) {
        so_out[0] = 0;
        totals[0] = 0;
        return TGMS_OK;
    }
    if (!waypoints || !seg_times || !coeffs || !t_cut) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::cut(B, so, waypoints, seg_times, end_derivs, coeffs, t_cut, min_frac, so_out, waypoints_out,
                        seg_times_out, end_derivs_out, coeffs_out, parent, t0_out, totals, flags);
        return TGMS_OK;
    }
    // the outputs at the capacities of the header (S segments), of which the first S' rows go to
    // the caller; the kernel gets nullptr for omitted coefficients and every other array
    const size_t S = (size_t)so[B], n = (size_t)B;
    Outputs out;
    const auto oW = out.add(waypoints_out, (S + n) * 3), oT = out.add(seg_times_out, S), oE = out.add(end_derivs_out, n * 18),
               oC = out.add(coeffs_out, S * 24), oT0 = out.add(t0_out, n, true);
    const auto oTot = out.add(totals, 1);
    const auto oSo = out.add(so_out, n + 1), oPar = out.add(parent, S, true), oFl = out.add(flags, n, true);
    double *dW, *dT, *dED, *dC, *dCut;
    int32_t* dSo;
    s = stage(h, {input(&dW, waypoints, (S + n) * 3), input(&dT, seg_times, S), input(&dED, end_derivs, n * 18),
                  input(&dC, coeffs, S * 24), input(&dCut, t_cut, n), input(&dSo, so, n + 1), output(&out)});
    if (s != TGMS_OK) return s;
    s = run_cut(h, h->stream, B, dSo, dW, dT, dED, dC, dCut, min_frac, out.dev(oSo), out.dev(oW), out.dev(oT), out.dev(oE),
                out.dev(oC), out.dev(oPar), out.dev(oT0), out.dev(oTot), out.dev(oFl));
    if (s == TGMS_OK) s = out.fetch(h);
    if (s != TGMS_OK) return s;
    out.take(oTot, 1);
    const size_t S1 = (size_t)totals[0];
    out.take(oSo, n + 1);
    out.take(oW, (S1 + n) * 3);
    out.take(oT, S1);
    out.take(oE, n * 18);
    out.take(oC, S1 * 24);
    out.take(oPar, S1);
    out.take(oT0, n);
    out.take(oFl, n);
    return TGMS_OK;
}

// ---- continuous swarm separation: closest approach of trajectory pairs ----

// The scale a launch carries: the caller's, or 1, 1, 1 for NULL.
static bool resolve_scale(const double* in, double (&out)[3]) {
    for (int a = 0; a < 3; ++a) {
        out[a] = in ? in[a] : 1.0;
        if (!(out[a] > 0.0) || !std::isfinite(out[a])) return false;
    }
    return true;
}

// What both calls check before they look at a pointer.
static tgms_status check_separation(tgms_handle* h, int32_t B, int64_t P, const int32_t* pairs, const double* scale,
                                    double r_min, const void* sep, const void* flags, double (&sc)[3]) {
    if (B < 0 || P < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or P");
    if (!pairs && P != (int64_t)B * ((int64_t)B - 1) / 2)
        return set_err(h, TGMS_ERR_INVALID_ARG, "pairs == NULL needs P == B (B - 1) / 2");
    if (!resolve_scale(scale, sc)) return set_err(h, TGMS_ERR_INVALID_ARG, "scale entries must be finite and > 0");
    if (std::isnan(r_min)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_min is NaN");
    if (!sep && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "sep and flags both NULL");
    return TGMS_OK;
}

tgms_status tgms_separation_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                         const double* dC, const double* d_start_times, int64_t P,
                                         const int32_t* d_pairs, const double* scale, double r_min, double* d_sep,
                                         int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    double sc[3];
    const tgms_status s = check_separation(h, B, P, d_pairs, scale, r_min, d_sep, d_flags, sc);
    if (s != TGMS_OK) return s;
    if (P == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_start_times, d_sep);
    TGMS_HIP(h, tgms::launch_separation(B, d_so, dT, dC, d_start_times, P, d_pairs, sc, r_min, d_sep, d_flags,
                                        static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_separation_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                                  const double* coeffs, const double* start_times, int64_t P, const int32_t* pairs,
                                  const double* scale, double r_min, double* sep, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    double sc[3];
    s = check_separation(h, B, P, pairs, scale, r_min, sep, flags, sc);
    if (s != TGMS_OK) return s;
    if (P == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        for (int64_t n = 0; n < P; ++n) {
            int32_t ij[2];
            if (pairs) {
                ij[0] = pairs[2 * n];
                ij[1] = pairs[2 * n + 1];
            } else {
                tgms::separation::decode_pair(n, B, P, ij[0], ij[1]);
            }
            int M[2] = {0, 0};
            int64_t s0[2] = {0, 0};
            double t0[2] = {0.0, 0.0};
            for (int k = 0; k < 2; ++k)
                if (ij[k] >= 0 && ij[k] < B) {  // else nothing is read: M == 0 rules the pair out
                    s0[k] = so[ij[k]];
                    M[k] = so[ij[k] + 1] - so[ij[k]];
                    t0[k] = start_times ? start_times[ij[k]] : 0.0;
                }
            double rec[TGMS_SEP_STRIDE];
            const int fl = tgms::host::separation(M[0], coeffs + s0[0] * 24, seg_times + s0[0], t0[0], M[1],
                                                  coeffs + s0[1] * 24, seg_times + s0[1], t0[1], sc, r_min, rec);
            if (sep) std::copy(rec, rec + TGMS_SEP_STRIDE, sep + n * TGMS_SEP_STRIDE);
            if (flags) flags[n] = fl;
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B];
    double *dT, *dC, *dT0;
    int32_t *dSo, *dP;
    Outputs out;
    const auto oSep = out.add(sep, (size_t)P * TGMS_SEP_STRIDE);
    const auto oFl = out.add(flags, (size_t)P);
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dT0, start_times, (size_t)B),
                  input(&dSo, so, (size_t)B + 1), input(&dP, pairs, (size_t)P * 2), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_separation(B, dSo, dT, dC, dT0, P, dP, sc, r_min, out.dev(oSep), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- swarm neighbour search: nearest vehicle per vehicle, far pairs culled ----

// What both calls check before they look at a pointer.
static tgms_status check_neighbors(tgms_handle* h, int32_t B, const double* scale, double r_min, const void* near,
                                   const void* nbr, const void* count, const void* flags, double (&sc)[3]) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (!resolve_scale(scale, sc)) return set_err(h, TGMS_ERR_INVALID_ARG, "scale entries must be finite and > 0");
    if (!(r_min > 0.0) || !std::isfinite(r_min)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_min must be finite and > 0");
    if (!near && !nbr && !count && !flags)
        return set_err(h, TGMS_ERR_INVALID_ARG, "near, nbr, count and flags all NULL");
    return TGMS_OK;
}

// The launch of either call, on the handle's scratch.
static tgms_status run_neighbors(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dT,
                                 const double* dC, const double* d_start_times, const double (&sc)[3], double r_min,
                                 double* d_near, int32_t* d_nbr, int32_t* d_count, int32_t* d_tested, int32_t* d_flags) {
    return launch_on_scratch(h, st, "tgms_neighbors_batch_device", "launch_neighbors", tgms::neighbors_scratch_bytes(B),
                             [&](void* ws) {
                                 return tgms::launch_neighbors(B, d_so, dT, dC, d_start_times, sc, r_min, ws, d_near, d_nbr,
                                                               d_count, d_tested, d_flags, st);
                             });
}

tgms_status tgms_neighbors_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                        const double* dC, const double* d_start_times, const double* scale,
                                        double r_min, double* d_near, int32_t* d_nbr, int32_t* d_count,
                                        int32_t* d_tested, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    double sc[3];
    const tgms_status s = check_neighbors(h, B, scale, r_min, d_near, d_nbr, d_count, d_flags, sc);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_start_times, d_near);
    return run_neighbors(h, static_cast<hipStream_t>(stream), B, d_so, dT, dC, d_start_times, sc, r_min, d_near, d_nbr,
                         d_count, d_tested, d_flags);
}

tgms_status tgms_neighbors_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                                 const double* coeffs, const double* start_times, const double* scale, double r_min,
                                 double* near, int32_t* nbr, int32_t* count, int32_t* tested, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    double sc[3];
    s = check_neighbors(h, B, scale, r_min, near, nbr, count, flags, sc);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::neighbors(B, so, seg_times, coeffs, start_times, sc, r_min, near, nbr, count, tested, flags);
        return TGMS_OK;
    }
    // the kernel gets every array; what the caller omitted is dropped on the host
    const size_t S = (size_t)so[B], n = (size_t)B;
    Outputs out;
    const auto oNear = out.add(near, n * TGMS_SEP_STRIDE, true);
    const auto oNbr = out.add(nbr, n, true), oCnt = out.add(count, n, true), oTst = out.add(tested, n, true),
               oFl = out.add(flags, n, true);
    double *dT, *dC, *dT0;
    int32_t* dSo;
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dT0, start_times, n),
                  input(&dSo, so, n + 1), output(&out)});
    if (s != TGMS_OK) return s;
    s = run_neighbors(h, h->stream, B, dSo, dT, dC, dT0, sc, r_min, out.dev(oNear), out.dev(oNbr), out.dev(oCnt),
                      out.dev(oTst), out.dev(oFl));
    return s != TGMS_OK ? s : out.download(h);
}

// ---- obstacle clearance: nearest static box per trajectory, far ones culled ----

// What both calls check before they look at a pointer.
static tgms_status check_clearance(tgms_handle* h, int32_t B, int32_t K, const double* scale, double r_min,
                                   const void* near, const void* obs, const void* count, const void* flags,
                                   double (&sc)[3]) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (K < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad K");
    if (!resolve_scale(scale, sc)) return set_err(h, TGMS_ERR_INVALID_ARG, "scale entries must be finite and > 0");
    if (!(r_min > 0.0) || !std::isfinite(r_min)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_min must be finite and > 0");
    if (!near && !obs && !count && !flags)
        return set_err(h, TGMS_ERR_INVALID_ARG, "near, obs, count and flags all NULL");
    return TGMS_OK;
}

// The launch of either call, on the handle's scratch.
static tgms_status run_clearance(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dT,
                                 const double* dC, int32_t K, const double* d_obstacles, const double (&sc)[3],
                                 double r_min, double* d_near, int32_t* d_obs, int32_t* d_count, int32_t* d_tested,
                                 int32_t* d_flags) {
    return launch_on_scratch(h, st, "tgms_clearance_batch_device", "launch_clearance", tgms::clearance_scratch_bytes(B, K),
                             [&](void* ws) {
                                 return tgms::launch_clearance(B, d_so, dT, dC, K, d_obstacles, sc, r_min, ws, d_near, d_obs,
                                                               d_count, d_tested, d_flags, st);
                             });
}

tgms_status tgms_clearance_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                        const double* dC, int32_t K, const double* d_obstacles, const double* scale,
                                        double r_min, double* d_near, int32_t* d_obs, int32_t* d_count,
                                        int32_t* d_tested, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    double sc[3];
    const tgms_status s = check_clearance(h, B, K, scale, r_min, d_near, d_obs, d_count, d_flags, sc);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC || (K > 0 && !d_obstacles)) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_obstacles, d_near);
    return run_clearance(h, static_cast<hipStream_t>(stream), B, d_so, dT, dC, K, d_obstacles, sc, r_min, d_near, d_obs,
                         d_count, d_tested, d_flags);
}

tgms_status tgms_clearance_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                                 const double* coeffs, int32_t K, const double* obstacles, const double* scale,
                                 double r_min, double* near, int32_t* obs, int32_t* count, int32_t* tested,
                                 int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    double sc[3];
    s = check_clearance(h, B, K, scale, r_min, near, obs, count, flags, sc);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs || (K > 0 && !obstacles)) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::clearance(B, so, seg_times, coeffs, K, obstacles, sc, r_min, near, obs, count, tested, flags);
        return TGMS_OK;
    }
    // the kernel gets every array; what the caller omitted is dropped on the host
    const size_t S = (size_t)so[B], n = (size_t)B;
    Outputs out;
    const auto oNear = out.add(near, n * TGMS_SEP_STRIDE, true);
    const auto oObs = out.add(obs, n, true), oCnt = out.add(count, n, true), oTst = out.add(tested, n, true),
               oFl = out.add(flags, n, true);
    double *dT, *dC, *dOb;
    int32_t* dSo;
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dOb, obstacles, (size_t)K * 6),
                  input(&dSo, so, n + 1), output(&out)});
    if (s != TGMS_OK) return s;
    s = run_clearance(h, h->stream, B, dSo, dT, dC, K, dOb, sc, r_min, out.dev(oNear), out.dev(oObs), out.dev(oCnt),
                      out.dev(oTst), out.dev(oFl));
    return s != TGMS_OK ? s : out.download(h);
}

}  // extern "C"
