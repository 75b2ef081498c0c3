// tgms_capi_map.hip — the voxel-map calls (include/tgms.h): field clearance, occupancy table,
// corridor inflation, subdivision and re-route, distance-field build, waypoint repair.
#include "tgms_capi.h"
#include "tgms_host.h"

#include <algorithm>
#include <cmath>

using namespace tgms::capi;

// The grid rules of a tgms_field (include/tgms.h), per axis in this order: 2..axis_max nodes, a
// finite origin, and the running product of what is counted (the nodes, or with pad = 1 the
// n + 1 table entries) within int32; then the spacing.  The product is < 2^62 after two factors
// and checked before the third.  With axis_max = 16,384 it is at most 2^28 after two axes, so
// the count rule can only fire on the last axis, that is after every per-axis rule.
// `h` may be NULL.
struct GridRules {
    int32_t pad, axis_max;
    const char *axis_msg, *count_msg;
};
constexpr GridRules kFieldGrid{0, INT32_MAX, "a field needs at least 2 nodes per axis", "a field holds at most 2^31 - 1 nodes"};
constexpr GridRules kTableGrid{1, INT32_MAX, "a field needs at least 2 nodes per axis",
                               "the table holds at most 2^31 - 1 entries"};
static_assert((int64_t)16384 * 16384 < INT32_MAX, "with a higher ceiling the transform's count rule could fire before axis 2");
constexpr GridRules kEdtGrid{0, 16384, "the transform takes 2..16,384 nodes per axis", "a field holds at most 2^31 - 1 nodes"};

static tgms_status check_grid(tgms_handle* h, const tgms_field* field, const GridRules& r) {
    int64_t total = 1;
    for (int a = 0; a < 3; ++a) {
        if (field->n[a] < 2 || field->n[a] > r.axis_max) return set_err(h, TGMS_ERR_INVALID_ARG, r.axis_msg);
        if (!std::isfinite(field->origin[a])) return set_err(h, TGMS_ERR_INVALID_ARG, "field origin must be finite");
        total *= (int64_t)field->n[a] + r.pad;
        if (total > INT32_MAX) return set_err(h, TGMS_ERR_INVALID_ARG, r.count_msg);
    }
    if (!(field->h > 0.0) || !std::isfinite(field->h)) return set_err(h, TGMS_ERR_INVALID_ARG, "h must be finite and > 0");
    return TGMS_OK;
}

extern "C" {

// ---- distance-field clearance: certified closest approach to a voxel map ----

// What both calls check before they look at a pointer to the batch.
static tgms_status check_field(tgms_handle* h, int32_t B, const tgms_field* field, const void* values, double lip,
                               double r_min, double tol, int32_t max_evals, const void* near, const void* evals,
                               const void* flags) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (!field || !values) return set_err(h, TGMS_ERR_INVALID_ARG, "field or values NULL");
    if (tgms_status s = check_grid(h, field, kFieldGrid); s != TGMS_OK) return s;
    if (!(tol > 0.0) || !std::isfinite(tol)) return set_err(h, TGMS_ERR_INVALID_ARG, "tol must be finite and > 0");
    if (!(r_min > 0.0)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_min must be > 0 (+inf allowed)");
    if (!(lip >= 0.0) || !std::isfinite(lip)) return set_err(h, TGMS_ERR_INVALID_ARG, "lip must be finite and >= 0");
    if (max_evals < 1) return set_err(h, TGMS_ERR_INVALID_ARG, "max_evals must be >= 1");
    if (!near && !evals && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "near, evals and flags all NULL");
    return TGMS_OK;
}

// The launches of either call: one with a given bound; with lip == 0 the reduction first, on
// the handle's scratch.
static tgms_status run_field(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dT,
                             const double* dC, const tgms_field& field, const float* d_values, double lip, double r_min,
                             double tol, int32_t max_evals, double* d_near, int32_t* d_evals, int32_t* d_flags) {
    if (lip > 0.0) {
        TGMS_HIP(h, hipSetDevice(h->device));
        TGMS_HIP(h, tgms::launch_field(B, d_so, dT, dC, field, d_values, lip, r_min, tol, max_evals, nullptr, d_near,
                                       d_evals, d_flags, st));
        return TGMS_OK;
    }
    return launch_on_scratch(h, st, "tgms_field_clearance_batch_device with lip == 0", "launch_field",
                             tgms::field_scratch_bytes(), [&](void* ws) {
                                 return tgms::launch_field(B, d_so, dT, dC, field, d_values, lip, r_min, tol, max_evals, ws,
                                                           d_near, d_evals, d_flags, st);
                             });
}

tgms_status tgms_field_clearance_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dT,
                                              const double* dC, const tgms_field* field, const float* d_values,
                                              double lip, double r_min, double tol, int32_t max_evals, double* d_near,
                                              int32_t* d_evals, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_field(h, B, field, d_values, lip, r_min, tol, max_evals, d_near, d_evals, d_flags);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dT, dC, d_near);
    if (misaligned({d_values}, 4))
        return set_err(h, TGMS_ERR_INVALID_ARG, "fp32 device buffers must be 4-byte aligned");
    return run_field(h, static_cast<hipStream_t>(stream), B, d_so, dT, dC, *field, d_values, lip, r_min, tol, max_evals,
                     d_near, d_evals, d_flags);
}

tgms_status tgms_field_clearance_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* seg_times,
                                       const double* coeffs, const tgms_field* field, const float* values, double lip,
                                       double r_min, double tol, int32_t max_evals, double* near, int32_t* evals,
                                       int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_field(h, B, field, values, lip, r_min, tol, max_evals, near, evals, flags);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!seg_times || !coeffs) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::field_clearance(B, so, seg_times, coeffs, *field, values, lip, r_min, tol, max_evals, near, evals,
                                    flags);
        return TGMS_OK;
    }
    // the kernel gets every array; what the caller omitted is dropped on the host
    const size_t S = (size_t)so[B], n = (size_t)B;
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oNear = out.add(near, n * TGMS_SEP_STRIDE, true);
    const auto oEv = out.add(evals, n, true), oFl = out.add(flags, n, true);
    double *dT, *dC;
    float* dV;
    int32_t* dSo;
    s = stage(h, {input(&dT, seg_times, S), input(&dC, coeffs, S * 24), input(&dV, values, N), input(&dSo, so, n + 1),
                  output(&out)});
    if (s != TGMS_OK) return s;
    s = run_field(h, h->stream, B, dSo, dT, dC, *field, dV, lip, r_min, tol, max_evals, out.dev(oNear), out.dev(oEv),
                  out.dev(oFl));
    return s != TGMS_OK ? s : out.download(h);
}

// ---- corridor inflation: the largest free box per segment from a voxel map ----

// The grid rules of the occupancy table (include/tgms.h): the field-clearance call's, with the
// table's entries in place of the nodes.
static tgms_status check_inflate_field(tgms_handle* h, const tgms_field* field) {
    if (!field) return set_err(h, TGMS_ERR_INVALID_ARG, "field NULL");
    return check_grid(h, field, kTableGrid);
}

static size_t inflate_table_entries(const tgms_field& f) {
    return ((size_t)f.n[0] + 1) * ((size_t)f.n[1] + 1) * ((size_t)f.n[2] + 1);
}

// What both inflation calls check before they look at a pointer to the batch.
static tgms_status check_inflate(tgms_handle* h, int32_t B, const tgms_field* field, const void* map, int32_t max_grow,
                                 const void* box, const void* faces, const void* fo, const void* seg_flags,
                                 const void* flags) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (tgms_status s = check_inflate_field(h, field); s != TGMS_OK) return s;
    if (!map) return set_err(h, TGMS_ERR_INVALID_ARG, "values or table NULL");
    if (max_grow < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "max_grow must be >= 0");
    if (!box && !faces && !fo && !seg_flags && !flags) return set_err(h, TGMS_ERR_INVALID_ARG, "every output is NULL");
    return TGMS_OK;
}

tgms_status tgms_field_occupancy_device(tgms_handle* h, const tgms_field* field, const float* d_values, double r_free,
                                        int32_t* d_table, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (tgms_status s = check_inflate_field(h, field); s != TGMS_OK) return s;
    if (!std::isfinite(r_free)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_free must be finite");
    if (!d_values || !d_table) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    if (misaligned({d_values, d_table}, 4))
        return set_err(h, TGMS_ERR_INVALID_ARG, "4-byte device buffers must be 4-byte aligned");
    TGMS_HIP(h, hipSetDevice(h->device));
    TGMS_HIP(h, tgms::launch_field_occupancy(*field, d_values, r_free, d_table, static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_corridor_inflate_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW,
                                               const tgms_field* field, const int32_t* d_table, int32_t max_grow,
                                               int32_t* d_box, double* d_faces, int64_t* d_fo, int32_t* d_seg_flags,
                                               int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_inflate(h, B, field, d_table, max_grow, d_box, d_faces, d_fo, d_seg_flags, d_flags);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, d_faces, d_fo);
    TGMS_HIP(h, hipSetDevice(h->device));
    TGMS_HIP(h, tgms::launch_inflate(B, d_so, dW, *field, d_table, max_grow, d_box, d_faces, d_fo, d_seg_flags, d_flags,
                                     static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_corridor_inflate_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                                        const tgms_field* field, const float* values, double r_free, int32_t max_grow,
                                        int32_t* box, double* faces, int64_t* face_offsets, int32_t* seg_flags,
                                        int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_inflate(h, B, field, values, max_grow, box, faces, face_offsets, seg_flags, flags);
    if (s != TGMS_OK) return s;
    if (!std::isfinite(r_free)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_free must be finite");
    if (B == 0) return TGMS_OK;
    if (!waypoints) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::corridor_inflate(B, so, waypoints, *field, values, r_free, max_grow, box, faces, face_offsets,
                                     seg_flags, flags);
        return TGMS_OK;
    }
    // the map goes up with the batch and its table is built beside them, in the workspace
    const size_t S = (size_t)so[B], n = (size_t)B;
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oFaces = out.add(faces, S * 24);
    const auto oFo = out.add(face_offsets, S + 1);
    const auto oBox = out.add(box, S * 6), oSegFl = out.add(seg_flags, S), oFl = out.add(flags, n);
    double* dW;
    float* dV;
    int32_t *dSo, *dTab;
    s = stage(h, {input(&dW, waypoints, (S + n) * 3), input(&dV, values, N), input(&dSo, so, n + 1),
                  output(&dTab, inflate_table_entries(*field)), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_field_occupancy(*field, dV, r_free, dTab, h->stream));
    TGMS_HIP(h, tgms::launch_inflate(B, dSo, dW, *field, dTab, max_grow, out.dev(oBox), out.dev(oFaces), out.dev(oFo),
                                     out.dev(oSegFl), out.dev(oFl), h->stream));
    return out.download(h);
}

// ---- corridor subdivision: split map-blocked legs until their boxes are free ----

// What both subdivision calls check before they look at a pointer to the batch.
static tgms_status check_subdivide(tgms_handle* h, int32_t B, const tgms_field* field, const void* map,
                                   int32_t max_depth, const void* T, const void* so_out, const void* W_out,
                                   const void* T_out, const void* totals) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (tgms_status s = check_inflate_field(h, field); s != TGMS_OK) return s;
    if (!map) return set_err(h, TGMS_ERR_INVALID_ARG, "values or table NULL");
    if (max_depth < 0 || max_depth > 4) return set_err(h, TGMS_ERR_INVALID_ARG, "max_depth must be in 0..4");
    if ((T == nullptr) != (T_out == nullptr))
        return set_err(h, TGMS_ERR_INVALID_ARG, "seg_times and seg_times_out are NULL together or not at all");
    if (!so_out || !totals) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets_out or totals is NULL");
    if (B > 0 && !W_out) return set_err(h, TGMS_ERR_INVALID_ARG, "waypoints_out is NULL");
    return TGMS_OK;
}

// The launch of either call, on the handle's scratch.
static tgms_status run_subdivide(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dW,
                                 const double* dT, const tgms_field& field, const int32_t* d_table, int32_t max_depth,
                                 int32_t* d_so_out, double* dW_out, double* dT_out, int32_t* d_parent,
                                 int32_t* d_seg_flags, int64_t* d_totals, int32_t* d_flags) {
    return launch_on_scratch(h, st, "tgms_corridor_subdivide_batch_device", "launch_subdivide",
                             tgms::subdivide_scratch_bytes(B), [&](void* ws) {
                                 return tgms::launch_subdivide(B, d_so, dW, dT, field, d_table, max_depth, ws, d_so_out, dW_out,
                                                               dT_out, d_parent, d_seg_flags, d_totals, d_flags, st);
                             });
}

tgms_status tgms_corridor_subdivide_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW,
                                                 const double* dT, const tgms_field* field, const int32_t* d_table,
                                                 int32_t max_depth, int32_t* d_so_out, double* dW_out, double* dT_out,
                                                 int32_t* d_parent, int32_t* d_seg_flags, int64_t* d_totals,
                                                 int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_subdivide(h, B, field, d_table, max_depth, dT, d_so_out, dW_out, dT_out, d_totals);
    if (s != TGMS_OK) return s;
    if (B > 0 && (!d_so || !dW)) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dW_out, dT_out, d_totals);
    return run_subdivide(h, static_cast<hipStream_t>(stream), B, d_so, dW, dT, *field, d_table, max_depth, d_so_out,
                         dW_out, dT_out, d_parent, d_seg_flags, d_totals, d_flags);
}

tgms_status tgms_corridor_subdivide_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                                          const double* seg_times, const tgms_field* field, const float* values,
                                          double r_free, int32_t max_depth, int32_t* so_out, double* waypoints_out,
                                          double* seg_times_out, int32_t* parent, int32_t* seg_flags_out,
                                          int64_t* totals, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_subdivide(h, B, field, values, max_depth, seg_times, so_out, waypoints_out, seg_times_out, totals);
    if (s != TGMS_OK) return s;
    if (!std::isfinite(r_free)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_free must be finite");
    if (B == 0) {
        so_out[0] = 0;
        totals[0] = 0;
        return TGMS_OK;
    }
    if (!waypoints) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::subdivide(B, so, waypoints, seg_times, *field, values, r_free, max_depth, so_out, waypoints_out,
                              seg_times_out, parent, seg_flags_out, totals, flags);
        return TGMS_OK;
    }
    // the map goes up with the batch and its table is built beside them, in the workspace; the
    // outputs at the capacity of the header, of which the first S' rows go to the caller
    const size_t S = (size_t)so[B], n = (size_t)B;
    const size_t cap = std::min(S << max_depth, (size_t)TGMS_MAX_SEGMENTS * n);
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oW = out.add(waypoints_out, (cap + n) * 3), oT = out.add(seg_times_out, cap);
    const auto oTot = out.add(totals, 1);
    const auto oSo = out.add(so_out, n + 1), oPar = out.add(parent, cap), oSegFl = out.add(seg_flags_out, cap),
               oFl = out.add(flags, n);
    double *dW, *dT;
    float* dV;
    int32_t *dSo, *dTab;
    s = stage(h, {input(&dW, waypoints, (S + n) * 3), input(&dT, seg_times, S), input(&dV, values, N),
                  input(&dSo, so, n + 1), output(&dTab, inflate_table_entries(*field)), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_field_occupancy(*field, dV, r_free, dTab, h->stream));
    s = run_subdivide(h, h->stream, B, dSo, dW, dT, *field, dTab, max_depth, out.dev(oSo), out.dev(oW), out.dev(oT),
                      out.dev(oPar), out.dev(oSegFl), out.dev(oTot), out.dev(oFl));
    if (s == TGMS_OK) s = out.fetch(h);
    if (s != TGMS_OK) return s;
    out.take(oTot, 1);
    const size_t S1 = (size_t)totals[0];
    out.take(oSo, n + 1);
    out.take(oW, (S1 + n) * 3);
    out.take(oT, S1);
    out.take(oPar, S1);
    out.take(oSegFl, S1);
    out.take(oFl, n);
    return TGMS_OK;
}

// ---- corridor re-route: detour blocked legs through the free nodes of the map ----

// What both re-route calls check before they look at a pointer to the batch.
static tgms_status check_reroute(tgms_handle* h, int32_t B, const tgms_field* field, const void* map, int32_t margin,
                                 int32_t max_pieces, const void* T, const void* so_out, const void* W_out,
                                 const void* T_out, const void* totals) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (tgms_status s = check_inflate_field(h, field); s != TGMS_OK) return s;
    if (!map) return set_err(h, TGMS_ERR_INVALID_ARG, "values or table NULL");
    if (margin < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "margin must be >= 0");
    if (max_pieces < 2 || max_pieces > 8) return set_err(h, TGMS_ERR_INVALID_ARG, "max_pieces must be in 2..8");
    if ((T == nullptr) != (T_out == nullptr))
        return set_err(h, TGMS_ERR_INVALID_ARG, "seg_times and seg_times_out are NULL together or not at all");
    if (!so_out || !totals) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets_out or totals is NULL");
    if (B > 0 && !W_out) return set_err(h, TGMS_ERR_INVALID_ARG, "waypoints_out is NULL");
    return TGMS_OK;
}

// The launch of either call, on the handle's scratch.
static tgms_status run_reroute(tgms_handle* h, hipStream_t st, int32_t B, const int32_t* d_so, const double* dW,
                               const double* dT, const tgms_field& field, const int32_t* d_table, int32_t margin,
                               int32_t max_pieces, int32_t* d_so_out, double* dW_out, double* dT_out, int32_t* d_parent,
                               int32_t* d_seg_flags, int32_t* d_hops, int64_t* d_totals, int32_t* d_flags) {
    return launch_on_scratch(h, st, "tgms_corridor_reroute_batch_dev", "launch_reroute", tgms::reroute_scratch_bytes(B),
                             [&](void* ws) {
                                 if (!h->reroute_ready) {
                                     if (const hipError_t e = tgms::reroute_prepare(); e != hipSuccess) return e;
                                     h->reroute_ready = true;
                                 }
                                 return tgms::launch_reroute(B, d_so, dW, dT, field, d_table, margin, max_pieces, ws,
                                                             d_so_out, dW_out, dT_out, d_parent, d_seg_flags, d_hops,
                                                             d_totals, d_flags, st);
                             });
}

tgms_status tgms_corridor_reroute_batch_dev(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW,
                                            const double* dT, const tgms_field* field, const int32_t* d_table,
                                            int32_t margin, int32_t max_pieces, int32_t* d_so_out, double* dW_out,
                                            double* dT_out, int32_t* d_parent, int32_t* d_seg_flags, int32_t* d_hops,
                                            int64_t* d_totals, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_reroute(h, B, field, d_table, margin, max_pieces, dT, d_so_out, dW_out, dT_out, d_totals);
    if (s != TGMS_OK) return s;
    if (B > 0 && (!d_so || !dW)) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dW_out, dT_out, d_totals);
    return run_reroute(h, static_cast<hipStream_t>(stream), B, d_so, dW, dT, *field, d_table, margin, max_pieces, d_so_out,
                       dW_out, dT_out, d_parent, d_seg_flags, d_hops, d_totals, d_flags);
}

tgms_status tgms_corridor_reroute_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                                        const double* seg_times, const tgms_field* field, const float* values,
                                        double r_free, int32_t margin, int32_t max_pieces, int32_t* so_out,
                                        double* waypoints_out, double* seg_times_out, int32_t* parent,
                                        int32_t* seg_flags_out, int32_t* hops, int64_t* totals, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_reroute(h, B, field, values, margin, max_pieces, seg_times, so_out, waypoints_out, seg_times_out, totals);
    if (s != TGMS_OK) return s;
    if (!std::isfinite(r_free)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_free must be finite");
    if (B == 0) {
        so_out[0] = 0;
        totals[0] = 0;
        return TGMS_OK;
    }
    if (!waypoints) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::reroute(B, so, waypoints, seg_times, *field, values, r_free, margin, max_pieces, so_out, waypoints_out,
                            seg_times_out, parent, seg_flags_out, hops, totals, flags);
        return TGMS_OK;
    }
    // the map goes up with the batch and its table is built beside them, in the workspace; the
    // outputs at the capacity of the header, of which the first S' rows go to the caller
    const size_t S = (size_t)so[B], n = (size_t)B;
    const size_t cap = std::min(S * (size_t)max_pieces, (size_t)TGMS_MAX_SEGMENTS * n);
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oW = out.add(waypoints_out, (cap + n) * 3), oT = out.add(seg_times_out, cap);
    const auto oTot = out.add(totals, 1);
    const auto oSo = out.add(so_out, n + 1), oPar = out.add(parent, cap), oSegFl = out.add(seg_flags_out, cap),
               oHops = out.add(hops, S), oFl = out.add(flags, n);
    double *dW, *dT;
    float* dV;
    int32_t *dSo, *dTab;
    s = stage(h, {input(&dW, waypoints, (S + n) * 3), input(&dT, seg_times, S), input(&dV, values, N),
                  input(&dSo, so, n + 1), output(&dTab, inflate_table_entries(*field)), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_field_occupancy(*field, dV, r_free, dTab, h->stream));
    s = run_reroute(h, h->stream, B, dSo, dW, dT, *field, dTab, margin, max_pieces, out.dev(oSo), out.dev(oW), out.dev(oT),
                    out.dev(oPar), out.dev(oSegFl), out.dev(oHops), out.dev(oTot), out.dev(oFl));
    if (s == TGMS_OK) s = out.fetch(h);
    if (s != TGMS_OK) return s;
    out.take(oTot, 1);
    const size_t S1 = (size_t)totals[0];
    out.take(oSo, n + 1);
    out.take(oW, (S1 + n) * 3);
    out.take(oT, S1);
    out.take(oPar, S1);
    out.take(oSegFl, S1);
    out.take(oHops, S);
    out.take(oFl, n);
    return TGMS_OK;
}

// ---- distance-field build: exact Euclidean transform of a voxel map ----

// The grid and mode rules of the transform (include/tgms.h); `h` may be NULL (the work size).
static tgms_status check_edt_field(tgms_handle* h, const tgms_field* field, int32_t mode) {
    if (!field) return set_err(h, TGMS_ERR_INVALID_ARG, "field NULL");
    if (tgms_status s = check_grid(h, field, kEdtGrid); s != TGMS_OK) return s;
    if (mode & ~TGMS_EDT_SIGNED) return set_err(h, TGMS_ERR_INVALID_ARG, "unknown mode bits");
    return TGMS_OK;
}

// What both calls check before they look at a pointer to the map.
static tgms_status check_edt(tgms_handle* h, const tgms_field* field, const void* occ, double max_dist, int32_t mode,
                             const void* values, const void* d2) {
    if (tgms_status s = check_edt_field(h, field, mode); s != TGMS_OK) return s;
    if (!(max_dist > 0.0) || !std::isfinite(max_dist))
        return set_err(h, TGMS_ERR_INVALID_ARG, "max_dist must be finite and > 0");
    if (!occ) return set_err(h, TGMS_ERR_INVALID_ARG, "occupancy NULL");
    if (!values && !d2) return set_err(h, TGMS_ERR_INVALID_ARG, "values and d2 both NULL");
    return TGMS_OK;
}

size_t tgms_field_edt_work_size(const tgms_field* field, int32_t mode) {
    return check_edt_field(nullptr, field, mode) == TGMS_OK ? tgms::edt_work_bytes(*field) : 0;
}

tgms_status tgms_field_edt_device(tgms_handle* h, const tgms_field* field, const uint8_t* d_occ, double max_dist,
                                  int32_t mode, float* d_values, int32_t* d_d2, void* d_work, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (tgms_status s = check_edt(h, field, d_occ, max_dist, mode, d_values, d_d2); s != TGMS_OK) return s;
    if (!d_work) return set_err(h, TGMS_ERR_INVALID_ARG, "workspace NULL");
    if (misaligned({d_values, d_d2, d_work}, 4))
        return set_err(h, TGMS_ERR_INVALID_ARG, "4-byte device buffers must be 4-byte aligned");
    TGMS_HIP(h, hipSetDevice(h->device));
    TGMS_HIP(h, tgms::launch_edt(*field, d_occ, max_dist, (mode & TGMS_EDT_SIGNED) != 0, d_values, d_d2, d_work,
                                 static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_field_edt(tgms_handle* h, const tgms_field* field, const uint8_t* occ, double max_dist, int32_t mode,
                           float* values, int32_t* d2) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    if (tgms_status s = check_edt(h, field, occ, max_dist, mode, values, d2); s != TGMS_OK) return s;
    if (h->host) {
        tgms::host::field_edt(*field, occ, max_dist, mode, values, d2);
        return TGMS_OK;
    }
    // the map goes up, the passes ping-pong in the handle's workspace, the outputs come down
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oVal = out.add(values, N);
    const auto oD2 = out.add(d2, N);
    uint8_t* dOcc;
    int32_t* dWork;
    const tgms_status s = stage(h, {input(&dOcc, occ, N), output(&dWork, tgms::edt_work_bytes(*field) / sizeof(int32_t)),
                                    output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_edt(*field, dOcc, max_dist, (mode & TGMS_EDT_SIGNED) != 0, out.dev(oVal), out.dev(oD2), dWork,
                                 h->stream));
    return out.download(h);
}

// ---- waypoint repair: move map-blocked waypoints to the nearest free node ----

// The grid, threshold and reach rules of the nearest-free map (include/tgms.h): the transform's
// grid; `h` may be NULL (the work size).
static tgms_status check_near_field(tgms_handle* h, const tgms_field* field) {
    if (!field) return set_err(h, TGMS_ERR_INVALID_ARG, "field NULL");
    return check_grid(h, field, kEdtGrid);
}

static tgms_status check_near(tgms_handle* h, const tgms_field* field, const void* values, double r_free,
                              int32_t max_shift) {
    if (tgms_status s = check_near_field(h, field); s != TGMS_OK) return s;
    if (!std::isfinite(r_free)) return set_err(h, TGMS_ERR_INVALID_ARG, "r_free must be finite");
    if (max_shift < 1 || max_shift > 32768) return set_err(h, TGMS_ERR_INVALID_ARG, "max_shift must be in 1..32,768");
    if (!values) return set_err(h, TGMS_ERR_INVALID_ARG, "values NULL");
    return TGMS_OK;
}

// What both repair calls check before they look at a pointer to the batch.
static tgms_status check_repair(tgms_handle* h, int32_t B, const tgms_field* field, const void* map, int32_t mode,
                                const void* T, const void* W_out, const void* T_out) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B");
    if (tgms_status s = check_near_field(h, field); s != TGMS_OK) return s;
    if (!map) return set_err(h, TGMS_ERR_INVALID_ARG, "values or nearest NULL");
    if (mode & ~(TGMS_RPR_KEEP_FIRST | TGMS_RPR_KEEP_LAST)) return set_err(h, TGMS_ERR_INVALID_ARG, "unknown mode bits");
    if ((T == nullptr) != (T_out == nullptr))
        return set_err(h, TGMS_ERR_INVALID_ARG, "seg_times and seg_times_out are NULL together or not at all");
    if (B > 0 && !W_out) return set_err(h, TGMS_ERR_INVALID_ARG, "waypoints_out is NULL");
    return TGMS_OK;
}

size_t tgms_field_nearest_free_work_size(const tgms_field* field) {
    return check_near_field(nullptr, field) == TGMS_OK ? tgms::nearest_free_work_bytes(*field) : 0;
}

tgms_status tgms_field_nearest_free_dev(tgms_handle* h, const tgms_field* field, const float* d_values, double r_free,
                                        int32_t max_shift, int32_t* d_nearest, int32_t* d_dsq, void* d_work,
                                        void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (tgms_status s = check_near(h, field, d_values, r_free, max_shift); s != TGMS_OK) return s;
    if (!d_nearest || !d_work) return set_err(h, TGMS_ERR_INVALID_ARG, "nearest or workspace NULL");
    if (misaligned({d_values, d_nearest, d_dsq, d_work}, 4))
        return set_err(h, TGMS_ERR_INVALID_ARG, "4-byte device buffers must be 4-byte aligned");
    TGMS_HIP(h, hipSetDevice(h->device));
    TGMS_HIP(h, tgms::launch_nearest_free(*field, d_values, r_free, max_shift, d_nearest, d_dsq, d_work,
                                          static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_field_nearest_free(tgms_handle* h, const tgms_field* field, const float* values, double r_free,
                                    int32_t max_shift, int32_t* nearest, int32_t* dsq) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    if (tgms_status s = check_near(h, field, values, r_free, max_shift); s != TGMS_OK) return s;
    if (!nearest) return set_err(h, TGMS_ERR_INVALID_ARG, "nearest NULL");
    if (h->host) {
        tgms::host::nearest_free(*field, values, r_free, max_shift, nearest, dsq);
        return TGMS_OK;
    }
    // the map goes up, the middle pass runs in the handle's workspace, the outputs come down
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oNear = out.add(nearest, N);
    const auto oDsq = out.add(dsq, N);
    float* dV;
    int32_t* dWork;
    const tgms_status s = stage(h, {input(&dV, values, N), output(&dWork, N), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_nearest_free(*field, dV, r_free, max_shift, out.dev(oNear), out.dev(oDsq), dWork, h->stream));
    return out.download(h);
}

tgms_status tgms_waypoints_repair_batch_dev(tgms_handle* h, int32_t B, const int32_t* d_so, const double* dW,
                                            const double* dT, const tgms_field* field, const int32_t* d_nearest,
                                            int32_t mode, double* dW_out, double* dT_out, int32_t* d_wp_flags,
                                            int32_t* d_shift, int32_t* d_flags, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    const tgms_status s = check_repair(h, B, field, d_nearest, mode, dT, dW_out, dT_out);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dW_out, dT_out);
    TGMS_HIP(h, hipSetDevice(h->device));
    TGMS_HIP(h, tgms::launch_repair(B, d_so, dW, dT, *field, d_nearest, mode, dW_out, dT_out, d_wp_flags, d_shift, d_flags,
                                    static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_waypoints_repair_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                                        const double* seg_times, const tgms_field* field, const float* values,
                                        double r_free, int32_t max_shift, int32_t mode, double* waypoints_out,
                                        double* seg_times_out, int32_t* wp_flags, int32_t* shift, int32_t* flags) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    s = check_repair(h, B, field, values, mode, seg_times, waypoints_out, seg_times_out);
    if (s != TGMS_OK) return s;
    s = check_near(h, field, values, r_free, max_shift);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!waypoints) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer");
    if (h->host) {
        tgms::host::waypoints_repair(B, so, waypoints, seg_times, *field, values, r_free, max_shift, mode, waypoints_out,
                                     seg_times_out, wp_flags, shift, flags);
        return TGMS_OK;
    }
    // the map goes up with the batch and its nearest-free map is built beside them, in the workspace
    const size_t S = (size_t)so[B], n = (size_t)B;
    const size_t N = (size_t)field->n[0] * field->n[1] * field->n[2];
    Outputs out;
    const auto oW = out.add(waypoints_out, (S + n) * 3), oT = out.add(seg_times_out, S);
    const auto oWf = out.add(wp_flags, S + n), oSh = out.add(shift, S + n), oFl = out.add(flags, n);
    double *dW, *dT;
    float* dV;
    int32_t *dSo, *dNear, *dWork;
    s = stage(h, {input(&dW, waypoints, (S + n) * 3), input(&dT, seg_times, S), input(&dV, values, N),
                  input(&dSo, so, n + 1), output(&dNear, N), output(&dWork, N), output(&out)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_nearest_free(*field, dV, r_free, max_shift, dNear, nullptr, dWork, h->stream));
    TGMS_HIP(h, tgms::launch_repair(B, dSo, dW, dT, *field, dNear, mode, out.dev(oW), out.dev(oT), out.dev(oWf),
                                    out.dev(oSh), out.dev(oFl), h->stream));
    return out.download(h);
}

}  // extern "C"
