// tgms_capi.h — private to the C-ABI units (tgms_capi*.hip): the handle, and the helpers that
// more than one of those units uses.  Not installed, and no kernel file includes it.
//
//   tgms_capi.hip           handle life cycle, errors, staging, scratch ordering, offsets; launch
//                           plans, the refinement-loop graphs; solve / refine / sample
//   tgms_capi_multi.hip     RCCL loader and the multi-GPU scheduler
//   tgms_capi_analysis.hip  extrema .. clearance (the calls on a solved batch)
//   tgms_capi_map.hip       the voxel-map calls
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "tgms.h"
#include "tgms_internal.h"

#ifndef TGMS_AUX_STREAMS
#define TGMS_AUX_STREAMS 4
#endif

struct tgms_multi_ctx;  // multi-GPU state of a tgms_create_multi handle (tgms_capi_multi.hip)

struct tgms_handle {
    bool host = false;  // tgms_create_host: the explicit host backend (config 1), no HIP state
    int device = 0;
    tgms_multi_ctx* multi = nullptr;  // non-null: handle over devices 0..n-1 (tgms_create_multi)
    int method = TGMS_METHOD_REDUCED;
    hipStream_t stream = nullptr;  // stream of the blocking (host-pointer) API
    std::string last_error;
    // grow-only device workspace for the host-pointer API and ragged plans
    void* d_ws = nullptr;
    size_t ws_cap = 0;
    int32_t* d_perm = nullptr;  // ragged plan: trajectory ids grouped by M
    size_t perm_cap = 0;
    int32_t* d_perm_hist = nullptr;  // the device-side grouping's per-block counts (refinement loop)
    size_t perm_hist_cap = 0;
    tgms::DevPlan* d_plan = nullptr;  // the device-side plan of a ragged refinement loop
    int32_t* h_perm = nullptr;  // pinned staging of the plan
    size_t h_perm_cap = 0;
    hipEvent_t perm_ev = nullptr;  // guards h_perm reuse until the upload completed
    // Handle-owned device scratch (d_perm, d_loop_ws, d_band, d_nbr_ws) is in use by the work
    // enqueued up to scratch_ev.  Every asynchronous entry point that touches it makes
    // its stream wait for scratch_ev first and records it again after its own work, so
    // calls on different streams are ordered on the GPU (no host blocking).
    hipEvent_t scratch_ev = nullptr;
    bool scratch_pending = false;
    // tgms_refine_loop_device's second time buffer (kept apart from d_ws, which the
    // blocking host API reuses)
    double* d_loop_ws = nullptr;
    size_t loop_ws_cap = 0;
    // tgms_neighbors_batch_device's per-vehicle boxes and knots, also tgms_clearance_batch_device's
    // and the per-trajectory plans of tgms_corridor_split_batch_device and tgms_cut_batch_device
    // (grow-only, ordered by scratch_ev)
    void* d_nbr_ws = nullptr;
    size_t nbr_ws_cap = 0;
    bool reroute_ready = false;  // the re-route search's dynamic LDS limit is raised on this handle's device
    // ragged plans: the per-M group launches fork onto these streams and join back, so
    // the groups (each a few hundred wavefronts) run side by side instead of in series
    hipStream_t aux[TGMS_AUX_STREAMS] = {};
    hipEvent_t fork_ev = nullptr;
    hipEvent_t join_ev[TGMS_AUX_STREAMS] = {};
    bool aux_ready = false;
    // Refinement loops (tgms_refine_loop_device, and every piece of a multi-GPU call on this
    // device) are captured into HIP graphs once and replayed while their arguments are
    // unchanged.  The plan is computed on the device inside the graph, so the key holds
    // only sizes, pointers and parameters: new offsets of the same B and S replay the same
    // graph.  A few graphs are cached (a multi-GPU call keeps one per piece).
    struct LoopKey {
        int32_t B = -1, iters = 0;
        int64_t S = 0;
        const void *d_so, *dW, *dT, *dT2, *dED, *dC, *d_cost, *dSt, *d_perm, *d_hist, *d_plan;
        double k_T, eta;
        int uniform_m;
        bool operator==(const LoopKey& o) const {
            return B == o.B && iters == o.iters && S == o.S && d_so == o.d_so && dW == o.dW && dT == o.dT &&
                   dT2 == o.dT2 && dED == o.dED && dC == o.dC && d_cost == o.d_cost && dSt == o.dSt &&
                   d_perm == o.d_perm && d_hist == o.d_hist && d_plan == o.d_plan && k_T == o.k_T && eta == o.eta &&
                   uniform_m == o.uniform_m;
        }
    };
    struct LoopGraph {
        LoopKey key;
        hipGraphExec_t exec = nullptr;
        uint64_t used = 0;
        hipEvent_t done = nullptr;  // recorded after every replay: eviction waits on it
    };
    std::vector<LoopGraph> loop_graphs;
    uint64_t loop_clock = 0;
    hipStream_t cap_stream = nullptr;
    // band-KKT method: persistent grid and the U slabs of its wavefronts.  d_band serves
    // uncaptured calls (grow-only, ordered by scratch_ev).  A slab a HIP-graph capture has
    // used belongs to graphs from then on (d_band_graph): replays cannot be ordered by the
    // handle's event, so uncaptured calls never touch it again, and it is never freed
    // before tgms_destroy (retired graph slabs stay alive in band_retired).
    int32_t band_grid = 0;
    double* d_band = nullptr;
    size_t band_cap = 0;
    double* d_band_graph = nullptr;
    size_t band_graph_cap = 0;
    std::vector<double*> band_retired;
    // Completion marker of the uncaptured band-KKT calls, for a capture that takes d_band
    // over: each uncaptured band call's scratch_release writes band_seq into this pinned word
    // from its stream (hipStreamWriteValue32); the hand-off waits on the host until the word
    // reaches the last value issued -- no HIP call, so the caller's capture stays valid.
    uint32_t* band_done = nullptr;  // pinned, mapped
    uint32_t band_seq = 0;
    bool band_unmarked = false;  // an uncaptured band call since the last marker
};

namespace tgms::capi {

// ---- errors and the opening of an entry point ----

inline tgms_status set_err(tgms_handle* h, tgms_status st, const std::string& msg) {
    if (h) h->last_error = msg;
    return st;
}

tgms_status hip_err(tgms_handle* h, hipError_t e, const char* where);

#define TGMS_HIP(h, call)                                  \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) return hip_err(h, e_, #call); \
    } while (0)

// Every entry point's opening: a handle, a GPU handle where `gpu_only` names the entry point
// (the host backend has no device path), and no error left over from an earlier call.
inline tgms_status enter(tgms_handle* h, const char* gpu_only = nullptr) {
    if (!h) return TGMS_ERR_INVALID_ARG;
    if (gpu_only && h->host)
        return set_err(h, TGMS_ERR_UNSUPPORTED, std::string(gpu_only) + " needs a GPU handle (tgms_create)");
    h->last_error.clear();
    return TGMS_OK;
}

// Device buffers: the kernels move fp64 data in 16-B pieces (double2 loads/stores,
// buffer_store_b128), so every fp64 device array must be 16-byte aligned (hipMalloc
// and torch allocations are 256-B aligned; a slice at an odd element offset is not).
// 4-byte arrays (fp32 maps, int32 tables) need their natural alignment only.  `align`: a power
// of two; a NULL pointer (an omitted optional array) is never misaligned.
inline bool misaligned(std::initializer_list<const void*> ps, uintptr_t align = 16) {
    for (const void* p : ps)
        if (p && (reinterpret_cast<uintptr_t>(p) & (align - 1))) return true;
    return false;
}
#define TGMS_CHECK_ALIGNED(h, ...)                                                                   \
    do {                                                                                             \
        if (misaligned({__VA_ARGS__}))                                                               \
            return set_err(h, TGMS_ERR_INVALID_ARG, "fp64 device buffers must be 16-byte aligned"); \
    } while (0)

// ---- staging of the host-pointer (blocking) entry points ----
// Such a call lays its device arrays out in the handle's workspace, uploads its inputs on the
// handle's stream, launches, and downloads.  It declares its regions in layout order
// (input / output below, counts in elements) and stage() does the rest.  Every region starts
// 256-byte aligned (the kernels move fp64 data in 16-byte pieces); a region without elements
// takes no space, gets nullptr and no copy.
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

tgms_status ensure_ws(tgms_handle* h, size_t bytes);

struct Region {
    void* slot;                      // the caller's T*: receives the region's device pointer
    void (*set)(void* slot, char*);  // the typed store into it
    const void* src;                 // host data to upload; nullptr: an output or scratch
    size_t bytes;
};
template <class T>
void set_slot(void* slot, char* p) {
    *static_cast<T**>(slot) = reinterpret_cast<T*>(p);
}
template <class T>
Region input(T** dev, const T* src, size_t n) {  // absent when src is NULL
    return {dev, set_slot<T>, src, src ? n * sizeof(T) : 0};
}
template <class T>
Region output(T** dev, size_t n) {
    return {dev, set_slot<T>, nullptr, n * sizeof(T)};
}

tgms_status stage(tgms_handle* h, std::initializer_list<Region> regions);

// Enqueues the download of n elements on the handle's stream.
template <class T>
hipError_t fetch(tgms_handle* h, T* host, const T* dev, size_t n) {
    return hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, h->stream);
}

// The outputs of a host-pointer call, one behind the other in one region so that one copy
// fetches them all.  The call declares them in layout order with add(), stages the region as
// one output(), launches with the typed device pointers dev() and downloads.  Every part
// starts 16-byte aligned (the region itself 256-byte, by stage()); a part without elements or
// one that is not reserved takes no space and has a NULL device pointer.
struct Outputs {
    template <class T>
    struct Part {  // add()'s ticket: it carries the element type to dev() and take()
        size_t i;
    };
    struct Slot {
        void* host;  // the caller's destination; NULL: not asked for, or nothing reserved
        size_t off, bytes;
    };
    std::vector<Slot> slots;
    size_t bytes = 0;
    char* d = nullptr;      // the region (stage)
    std::vector<char> all;  // its downloaded bytes (fetch)

    // `cap` elements for `host` (may be NULL); `reserve`: whether the device array exists, by
    // default only when the caller asked for it (the kernel gets nullptr otherwise).
    template <class T>
    Part<T> add(T* host, size_t cap, bool reserve) {
        const size_t n = reserve ? cap * sizeof(T) : 0, off = (bytes + 15) & ~size_t(15);
        if (n) bytes = off + n;
        slots.push_back({n ? host : nullptr, off, n});
        return {slots.size() - 1};
    }
    template <class T>
    Part<T> add(T* host, size_t cap) {
        return add(host, cap, host != nullptr);
    }
    template <class T>
    T* dev(Part<T> p) const {
        return slots[p.i].bytes ? reinterpret_cast<T*>(d + slots[p.i].off) : nullptr;
    }

    // One copy out of the region and the wait for it.
    tgms_status copy(tgms_handle* h, void* dst, size_t off, size_t n) const {
        TGMS_HIP(h, hipMemcpyAsync(dst, d + off, n, hipMemcpyDeviceToHost, h->stream));
        TGMS_HIP(h, hipStreamSynchronize(h->stream));
        return TGMS_OK;
    }
    // The whole region; then take() hands the first n elements of a part to the caller if asked for.
    tgms_status fetch(tgms_handle* h) {
        all.resize(bytes);
        return copy(h, all.data(), 0, bytes);
    }
    template <class T>
    void take(Part<T> p, size_t n) const {
        if (slots[p.i].host) std::memcpy(slots[p.i].host, all.data() + slots[p.i].off, n * sizeof(T));
    }
    // Every part the caller asked for, whole; a part asked for alone goes straight to the caller.
    tgms_status download(tgms_handle* h) {
        const Slot* only = nullptr;
        int wanted = 0;
        for (const Slot& s : slots)
            if (s.host) {
                only = &s;
                ++wanted;
            }
        if (wanted == 1) return copy(h, only->host, only->off, only->bytes);
        const tgms_status st = fetch(h);
        for (const Slot& s : slots)
            if (st == TGMS_OK && s.host) std::memcpy(s.host, all.data() + s.off, s.bytes);
        return st;
    }
};
inline Region output(Outputs* o) { return output(&o->d, o->bytes); }

// The end of a blocking solve: the statuses go to the caller (or, for status == NULL, into a
// temporary), the stream is drained, and the worst status is the call's result; `message`: the
// first trajectory that has it goes into last_error.
tgms_status finish_status(tgms_handle* h, const int32_t* dSt, int32_t* status, int32_t B, bool message);

// ---- ordering of the handle's device scratch ----

// True while `stream` is being captured into a HIP graph.
bool capturing(hipStream_t stream);
// Order `stream` after every earlier user of the handle's device scratch.
tgms_status scratch_acquire(tgms_handle* h, hipStream_t stream);
// The work just enqueued on `stream` is the scratch's latest user.
tgms_status scratch_release(tgms_handle* h, hipStream_t stream);
// After a dispatch that returned `s`: released on failure too (a band call that launched
// must still write its marker); the first error is the result.
tgms_status scratch_release(tgms_handle* h, hipStream_t stream, tgms_status s);
// TGMS_ERR_UNSUPPORTED, naming `what`, while `stream` is being captured.
tgms_status no_capture(tgms_handle* h, hipStream_t stream, const char* what);
tgms_status ensure_nbr_ws(tgms_handle* h, size_t bytes);

// The launches of a call that uses `bytes` of the handle's scratch (d_nbr_ws), between acquire
// and release: launch(scratch) -> hipError_t.  `entry` names the call where a capture is
// refused, `where` the launch in last_error; a failed launch is still released.
template <class Launch>
tgms_status launch_on_scratch(tgms_handle* h, hipStream_t st, const char* entry, const char* where, size_t bytes,
                              Launch launch) {
    tgms_status s = no_capture(h, st, entry);
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, hipSetDevice(h->device));
    s = ensure_nbr_ws(h, bytes);
    if (s == TGMS_OK) s = scratch_acquire(h, st);
    if (s != TGMS_OK) return s;
    return scratch_release(h, st, hip_err(h, launch(h->d_nbr_ws), where));
}

// ---- CSR offsets ----

// Validates a CSR segment layout on the host; fills per-M counts.
tgms_status check_offsets(tgms_handle* h, int32_t B, const int32_t* so, int max_m, std::vector<int32_t>* counts,
                          int* uniform_m);
inline int max_m_for(const tgms_handle* h) {
    return h->method == TGMS_METHOD_DENSE_KKT ? TGMS_DENSE_MAX_SEGMENTS : TGMS_MAX_SEGMENTS;
}

// ---- the planner of tgms_capi.hip, which the multi-GPU scheduler drives per device and piece ----

// Launch plan of one batch: uniform M, or the trajectories grouped by M (counting
// sort into the device permutation).  Built once per call; a refinement loop
// reuses it for every step.
struct Plan {
    int uniform_m = 0;
    std::vector<int32_t> counts, starts;
    const int32_t* d_perm = nullptr;  // ragged: trajectory ids grouped by M (device)
};

// Device buffers of a ragged refinement loop's device-side plan (handle-owned for one
// device, in the piece workspace for the pieces of a multi-GPU call).
struct DevPlanBufs {
    int32_t* hist = nullptr;
    int32_t* perm = nullptr;
    tgms::DevPlan* plan = nullptr;
};

tgms_status ensure_perm_device(tgms_handle* h, int32_t B);
tgms_status plan_upload(tgms_handle* h, int32_t B, const int32_t* h_so, Plan* p, hipStream_t stream);
tgms_status make_plan(tgms_handle* h, int32_t B, const int32_t* h_so, int max_m, Plan* p, hipStream_t stream);
tgms_status dispatch(tgms_handle* h, const Plan& p, int32_t B, const int32_t* d_so, const double* W, const double* T,
                     const double* ED, double* C, int32_t* st, hipStream_t stream);
tgms_status refine_loop(tgms_handle* h, const Plan& p, int32_t B, int64_t S, const int32_t* d_so, const double* W,
                        double* const T[2], const double* ED, double kT, double eta, int32_t iters, double* C,
                        double* cost, int32_t* st, hipStream_t stream, int* cur, const DevPlanBufs* dp);
tgms_status solve_ragged_dev(tgms_handle* h, int32_t B, int64_t S, const int32_t* d_so, const double* W,
                             const double* T, const double* ED, double* C, int32_t* st, hipStream_t stream,
                             const DevPlanBufs& dp);
tgms_status run_loop_graph(tgms_handle* h, const tgms_handle::LoopKey& key, hipStream_t stream,
                           const std::function<tgms_status(hipStream_t)>& body);
tgms_status check_refine_args(tgms_handle* h, double kT, double eta);
tgms_status loop_on_device(tgms_handle* h, int32_t B, int64_t S, int uniform_m, const int32_t* d_so, const double* dW,
                           double* dT, const double* dED, double k_T, double eta, int32_t iters, double* dC,
                           double* d_cost, int32_t* dSt, hipStream_t st);

// ---- the multi unit's part in the handle's life cycle ----

void destroy_multi(tgms_multi_ctx* m);
void multi_set_method(tgms_multi_ctx* m, int method);

}  // namespace tgms::capi
