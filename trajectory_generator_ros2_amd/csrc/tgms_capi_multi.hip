// tgms_capi_multi.hip — the multi-GPU handle: the RCCL loader, the scatter / solve / gather
// pipeline over the host-only schedule of tgms_plan.h, and the multi entry points of
// include/tgms.h.
#include "tgms_capi.h"
#include "tgms_plan.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace tgms::capi;

static_assert(sizeof(tgms::DevPlan) <= tgms::DEV_PLAN_BYTES, "the planner's region for the device plan is too small");

namespace {

// so[b] == M0 b for every b <= B (so[0] == 0 and so[B] within [B, 16 B] checked by the
// caller): one load per trajectory against an induction variable, in blocks of 4,096 that
// stop at the first block holding a different M.  Modulo 2^32 is exact here: offsets in
// [0, 2^31) congruent to M0 b for every b step by exactly M0.
// (built for AVX2 where the CPU has it, as minmax_m above: the inner loop vectorises)
#define TGMS_UNIFORM_BODY                                                                 \
    const uint32_t m = (uint32_t)M0;                                                      \
    uint32_t diff = 0;                                                                    \
    for (int32_t b0 = 0; b0 <= B && diff == 0; b0 += 4096) {                              \
        const int32_t e = std::min(B + 1, b0 + 4096);                                     \
        for (int32_t b = b0; b < e; ++b) diff |= (uint32_t)so[b] ^ (m * (uint32_t)b);     \
    }                                                                                     \
    return diff == 0;
__attribute__((target("avx2"))) bool uniform_offsets_avx2(int32_t B, const int32_t* so, int32_t M0) {
    TGMS_UNIFORM_BODY
}
bool uniform_offsets_base(int32_t B, const int32_t* so, int32_t M0) { TGMS_UNIFORM_BODY }
#undef TGMS_UNIFORM_BODY
bool uniform_offsets(int32_t B, const int32_t* so, int32_t M0) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    return avx2 ? uniform_offsets_avx2(B, so, M0) : uniform_offsets_base(B, so, M0);
}

// The host check of a multi-GPU ragged solve with the reduced method (round 6, as the
// refinement loop's): the offsets' ends, and uniform detection in blocks of 4,096 that stops
// at the first block holding two different M (a ragged batch leaves after its first block).
// A uniform batch keeps the uniform kernels (its M checked here); a ragged one is grouped
// and checked per trajectory on its devices.
tgms_status scan_multi_offsets(tgms_handle* h, int32_t B, const int32_t* so, int max_m, int* uniform_m) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "B < 0");
    if (!so) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets is NULL");
    if (so[0] != 0) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets[0] != 0");
    *uniform_m = 0;
    if (B == 0) return TGMS_OK;
    if (so[B] < B || (int64_t)so[B] > (int64_t)TGMS_MAX_SEGMENTS * B)
        return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets[B] outside [B, 16 B]");
    const int32_t M0 = so[1] - so[0];
    if (!uniform_offsets(B, so, M0)) return TGMS_OK;
    if (M0 < 1 || M0 > max_m) return set_err(h, TGMS_ERR_INVALID_ARG, "uniform batch with M outside the method's range");
    *uniform_m = M0;
    return TGMS_OK;
}

// ---------------------------------------------------------------------------
// Multi-GPU handle: one process drives devices 0..n-1 through
// one communicator per device (ncclCommInitAll, rccl.h:236).  A batch is split into
// contiguous cost-balanced shards (plan_shards: the same rule as shard.ragged_bounds);
// every shard is cut into pieces; device 0 scatters each piece's inputs to its device
// over RCCL (grouped ncclSend/ncclRecv, rccl.h:700/722: per-piece byte counts, so
// ragged batches need no padding), the device solves the piece on its compute stream,
// and the piece's coefficients (+ statuses, and for the refinement loop its times and
// costs) go back to device 0 on the device's communication stream while the next
// piece is being solved.  Device 0's own shard is solved in place on the caller's
// stream, beside the gathers.  RCCL is loaded at tgms_create_multi (dlopen), so
// single-device users never load it.

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;

    bool load(std::string* err) {
        // librccl.so.1 is torch's bundled copy when torch is loaded (same soname), else ROCm's
        for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) {
            *err = std::string("cannot load RCCL (librccl.so.1): ") + dlerror();
            return false;
        }
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(lib, name));
            return fn != nullptr;
        };
        if (sym(comm_init_all, "ncclCommInitAll") && sym(comm_destroy, "ncclCommDestroy") && sym(send, "ncclSend") &&
            sym(recv, "ncclRecv") && sym(group_start, "ncclGroupStart") && sym(group_end, "ncclGroupEnd") &&
            sym(error_string, "ncclGetErrorString"))
            return true;
        *err = "RCCL library lacks a needed entry point";
        return false;
    }
};

// Contiguous cost-balanced shards of a CSR batch: the rule of shard.ragged_bounds
// (trajectory_generator_ros2_amd/shard.py), step for step in the same fp64 arithmetic,
// so the C++ and Python planners give identical bounds (tests/test_multi_host.py).
enum class MultiJob { Solve, Refine };

struct MultiArgs {
    MultiJob job = MultiJob::Solve;
    int32_t B = 0;
    const int32_t* h_so = nullptr;
    const int32_t* d_so = nullptr;  // device 0
    const double *dW = nullptr, *dED = nullptr;
    double* dT = nullptr;  // refine: updated in place
    double *dC = nullptr, *d_cost = nullptr;
    int32_t* dSt = nullptr;
    double k_T = 0.0, eta = 0.0;
    int32_t iters = 0;
    const Plan* checked = nullptr;  // the whole batch's validated counts / uniform M
};

}  // namespace

struct tgms_multi_ctx {
    int n = 0;
    RcclApi r;
    std::vector<ncclComm_t> comm;
    std::vector<tgms_handle*> sub;    // sub[0] is the root handle itself
    std::vector<hipStream_t> sm;      // per device: RCCL stream (sm[0]: device 0's scatter/gather stream)
    std::vector<hipStream_t> sc;      // per device: compute stream of its pieces
    std::vector<char*> dws;           // per device: piece workspace (device)
    std::vector<size_t> dws_cap;
    std::vector<char*> pin;           // per device: pinned staging of the pieces' plans
    std::vector<size_t> pin_cap;
    std::vector<hipEvent_t> ev_up;
    std::vector<std::vector<hipEvent_t>> ev_in;  // per device and piece: the piece's inputs have landed
    std::vector<bool> up_pending;
    std::vector<std::vector<hipEvent_t>> ev_piece;
    hipEvent_t ev_start = nullptr, ev_end = nullptr;
    bool self_gather = false;  // device 0's shard through the RCCL pipeline too (tests on one GPU)
    // error-path test hook (TGMS_MULTI_FAIL="piece:k" or "group:k", read at
    // tgms_create_multi, fires once): the dispatch of piece k, or the gather group of
    // piece k right after ncclGroupStart, reports a device error
    int fail_kind = 0, fail_piece = -1;  // kind 1: piece dispatch, 2: inside the gather group
};

namespace tgms::capi {

void destroy_multi(tgms_multi_ctx* m) {
    if (!m) return;
    for (int d = 0; d < m->n; ++d) {
        (void)hipSetDevice(d);
        (void)hipDeviceSynchronize();
    }
    for (int d = 0; d < m->n; ++d) {
        if (d < (int)m->comm.size() && m->comm[d] && m->r.comm_destroy) (void)m->r.comm_destroy(m->comm[d]);
        (void)hipSetDevice(d);
        if (d < (int)m->sm.size() && m->sm[d]) (void)hipStreamDestroy(m->sm[d]);
        if (d == 0 && d < (int)m->sc.size() && m->sc[d]) (void)hipStreamDestroy(m->sc[d]);
        if (d < (int)m->dws.size() && m->dws[d]) (void)hipFree(m->dws[d]);
        if (d < (int)m->pin.size() && m->pin[d]) (void)hipHostFree(m->pin[d]);
        if (d < (int)m->ev_up.size() && m->ev_up[d]) (void)hipEventDestroy(m->ev_up[d]);
        if (d < (int)m->ev_in.size())
            for (hipEvent_t e : m->ev_in[d])
                if (e) (void)hipEventDestroy(e);
        if (d < (int)m->ev_piece.size())
            for (hipEvent_t e : m->ev_piece[d])
                if (e) (void)hipEventDestroy(e);
        if (d >= 1 && d < (int)m->sub.size() && m->sub[d]) tgms_destroy(m->sub[d]);
    }
    (void)hipSetDevice(0);
    if (m->ev_start) (void)hipEventDestroy(m->ev_start);
    if (m->ev_end) (void)hipEventDestroy(m->ev_end);
    delete m;
}

void multi_set_method(tgms_multi_ctx* m, int method) {
    for (tgms_handle* sub : m->sub)
        if (sub) sub->method = method;
}

}  // namespace tgms::capi

namespace {

tgms_status nccl_err(tgms_handle* h, ncclResult_t e, const char* where) {
    if (e == ncclSuccess) return TGMS_OK;
    const char* msg = h->multi && h->multi->r.error_string ? h->multi->r.error_string(e) : "RCCL error";
    return set_err(h, TGMS_ERR_DEVICE, std::string(where) + ": " + msg);
}
#define TGMS_NCCL(h, call)                                    \
    do {                                                      \
        ncclResult_t n_ = (call);                             \
        if (n_ != ncclSuccess) return nccl_err(h, n_, #call); \
    } while (0)

// An RCCL group opened by start() is closed on every exit of the scope: an early
// return from inside ncclGroupStart() .. ncclGroupEnd() would otherwise leave the
// thread's group depth raised, and every later RCCL call of the thread deferred into
// a group that never ends.  (After a failed send/recv, ncclGroupEnd reports the
// group's error and launches none of its operations.)
struct NcclGroup {
    const RcclApi& r;
    bool open = false;
    explicit NcclGroup(const RcclApi& api) : r(api) {}
    ncclResult_t start() {
        const ncclResult_t e = r.group_start();
        open = e == ncclSuccess;
        return e;
    }
    ncclResult_t end() {
        open = false;
        return r.group_end();
    }
    ~NcclGroup() {
        if (open) (void)r.group_end();
    }
    NcclGroup(const NcclGroup&) = delete;
    NcclGroup& operator=(const NcclGroup&) = delete;
};

// The calling thread's HIP device, restored on every exit of a multi-device call.
struct DeviceRestore {
    int dev = 0;
    bool ok = false;
    DeviceRestore() { ok = hipGetDevice(&dev) == hipSuccess; }
    ~DeviceRestore() {
        if (ok) (void)hipSetDevice(dev);
    }
};

// Counting sort of one piece's trajectories by M into `perm` (host); fills the plan's
// counts / starts / uniform_m (as check_offsets + upload_plan do for a whole batch).
void piece_plan(const int32_t* so_rebased, int32_t n, int max_m, Plan* p, int32_t* perm) {
    p->counts.assign(max_m + 1, 0);
    int um = -1;
    for (int32_t b = 0; b < n; ++b) {
        const int32_t M = so_rebased[b + 1] - so_rebased[b];
        p->counts[M]++;
        um = (b == 0) ? M : (um == M ? M : 0);
    }
    p->uniform_m = n > 0 ? um : 0;
    p->starts.assign(p->counts.size() + 1, 0);
    for (size_t m = 1; m < p->counts.size(); ++m) p->starts[m + 1] = p->starts[m] + p->counts[m];
    if (p->uniform_m > 0) return;
    std::vector<int32_t> fill(p->starts.begin(), p->starts.end());
    for (int32_t b = 0; b < n; ++b) perm[fill[so_rebased[b + 1] - so_rebased[b]]++] = b;
}

// The multi-GPU pipeline (see the section comment).  Arrays in `a` live on device 0
// and are ordered on `ustream` (a device-0 stream).  Stream roles per device d:
//   sm[d]  plan upload, scatter receive (d = 0: every send too), gathers
//   sc[d]  the pieces' solves (waits for the scatter; the gathers wait for it)
// The plan upload goes on sm[d], so it is ordered after the previous call's gathers,
// which read the same workspace (a later call's plan block may overlap the previous
// call's piece outputs).
tgms_status multi_enqueue(tgms_handle* h, const MultiArgs& a, hipStream_t ustream);

// Drain every stream of the pipeline: after a failure nothing the call already queued
// may still write into the caller's buffers once the error has been returned.
void multi_drain(tgms_multi_ctx* m) {
    for (int d = 0; d < m->n; ++d) {
        if (hipSetDevice(d) != hipSuccess) continue;
        if (m->sm[d]) (void)hipStreamSynchronize(m->sm[d]);
        if (m->sc[d]) (void)hipStreamSynchronize(m->sc[d]);
    }
}

tgms_status multi_run(tgms_handle* h, const MultiArgs& a, hipStream_t ustream) {
    DeviceRestore restore;  // the caller's device on every return
    const tgms_status s = multi_enqueue(h, a, ustream);
    if (s != TGMS_OK) {
        multi_drain(h->multi);
        (void)hipSetDevice(0);
        (void)hipStreamSynchronize(ustream);
    }
    return s;
}

tgms_status multi_enqueue(tgms_handle* h, const MultiArgs& a, hipStream_t ustream) {
    using tgms::MULTI_PIECES;
    tgms_multi_ctx* m = h->multi;
    const int n = m->n;
    const bool refine = a.job == MultiJob::Refine;
    const int max_m = refine ? TGMS_MAX_SEGMENTS : max_m_for(h);
    const int um = a.checked ? a.checked->uniform_m : 0;
    // a ragged solve with the reduced method: every piece (and device 0's shard) grouped on
    // its device, as the refinement loop's (round 6)
    const bool dev_solve = !refine && h->method == TGMS_METHOD_REDUCED && um <= 0;
    // the whole schedule (shards, pieces, workspace layout, transfers) from the host-only
    // planner (tgms_plan.cpp, CPU-tested through tgms_multi_schedule)
    tgms::MultiFlags fl;
    fl.refine = refine;
    fl.has_ed = a.dED != nullptr;
    fl.has_c = a.dC != nullptr;
    fl.has_st = a.dSt != nullptr;
    fl.has_cost = a.d_cost != nullptr;
    fl.self_gather = m->self_gather;
    tgms::MultiPlan P;
    tgms::plan_multi(n, a.B, a.h_so, h->method, um, fl, &P);
    const std::vector<int32_t>& bounds = P.bounds;
    // the refinement loop's offsets were not scanned on the host: a cut where they decrease
    // or a piece whose span no M in 1..16 can give is the caller's error (the workspaces are
    // sized from these spans)
    if (!tgms::cuts_valid(P, a.h_so))
        return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets: a shard or piece cut where they decrease");
    std::vector<std::vector<Plan>> plans(n);  // per piece: its launch plan (M groups)
    for (int d = 0; d < n; ++d) {
        if (P.pieces[d].empty()) continue;
        const size_t plan_bytes = P.plan_bytes[d], off = P.ws_bytes[d];
        // workspaces (grow-only; a regrow waits for the device's previous work)
        TGMS_HIP(h, hipSetDevice(d));
        if (off > m->dws_cap[d]) {
            TGMS_HIP(h, hipDeviceSynchronize());
            if (m->dws[d]) TGMS_HIP(h, hipFree(m->dws[d]));
            m->dws[d] = nullptr;
            m->dws_cap[d] = 0;
            TGMS_HIP(h, hipMalloc(reinterpret_cast<void**>(&m->dws[d]), off));
            m->dws_cap[d] = off;
        }
        plans[d].resize(P.pieces[d].size());
        if (!plan_bytes) {
            // uniform batches need no plan; a ragged refinement loop plans each piece on its
            // device (the piece's offsets arrive with its inputs, grouped in the loop's graph)
            for (auto& pl : plans[d]) pl.uniform_m = um;
            continue;
        }
        // a ragged solve: each piece's rebased offsets and M grouping from the host, one upload
        if (m->up_pending[d]) TGMS_HIP(h, hipEventSynchronize(m->ev_up[d]));  // staging free again
        m->up_pending[d] = false;
        if (plan_bytes > m->pin_cap[d]) {
            if (m->pin[d]) TGMS_HIP(h, hipHostFree(m->pin[d]));
            m->pin[d] = nullptr;
            m->pin_cap[d] = 0;
            TGMS_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&m->pin[d]), plan_bytes));
            m->pin_cap[d] = plan_bytes;
        }
        for (size_t k = 0; k < P.pieces[d].size(); ++k) {
            const tgms::PiecePlan& p = P.pieces[d][k];
            int32_t* so_p = reinterpret_cast<int32_t*>(m->pin[d] + p.oSo);
            for (int32_t b = p.lo; b <= p.hi; ++b) so_p[b - p.lo] = a.h_so[b] - a.h_so[p.lo];
            piece_plan(so_p, p.n(), max_m, &plans[d][k], reinterpret_cast<int32_t*>(m->pin[d] + p.oPerm));
            plans[d][k].d_perm = reinterpret_cast<const int32_t*>(m->dws[d] + p.oPerm);
        }
        {
            // on sm[d]: after the previous call's gathers out of this workspace
            TGMS_HIP(h, hipMemcpyAsync(m->dws[d], m->pin[d], plan_bytes, hipMemcpyHostToDevice, m->sm[d]));
            TGMS_HIP(h, hipEventRecord(m->ev_up[d], m->sm[d]));
            m->up_pending[d] = true;
        }
    }
    // Everything a send/recv below is given was planned above: the pieces' ranges lie
    // inside the batch, their workspaces are allocated, and the peers are 0..n-1.  (The
    // refinement loop's offsets were not scanned on the host: cuts where they decrease are
    // the caller's error.)
    for (int d = 0; d < n; ++d)
        for (const tgms::PiecePlan& p : P.pieces[d]) {
            if (!m->dws[d] || p.lo < 0 || p.hi > a.B || p.s0 < 0 || p.s1 > a.h_so[a.B] ||
                tgms::perm_hist_bytes(p.n()) != tgms::dev_hist_bytes(p.n()))
                return set_err(h, TGMS_ERR_DEVICE, "internal: multi-GPU piece plan out of range");
        }
    // the device-0 batch array and the workspace region a transfer moves between
    auto batch_ptr = [&](const tgms::Xfer& x) -> char* {
        switch (x.array) {
            case tgms::XA_W: return (char*)(a.dW + x.batch_elem);
            case tgms::XA_T: return (char*)(a.dT + x.batch_elem);
            case tgms::XA_ED: return (char*)(a.dED + x.batch_elem);
            case tgms::XA_C: return (char*)(a.dC + x.batch_elem);
            case tgms::XA_ST: return (char*)(a.dSt + x.batch_elem);
            case tgms::XA_SO: return (char*)(a.d_so + x.batch_elem);
            default: return (char*)(a.d_cost + x.batch_elem);
        }
    };
    // one RCCL group of transfers: scatter groups send from device 0 (its stream sm[0])
    // and receive on the piece's device (sm[d]); gather groups the other way round
    size_t xi = 0;
    auto run_group = [&](int g) -> tgms_status {
        NcclGroup grp(m->r);
        TGMS_NCCL(h, grp.start());
        if (g >= MULTI_PIECES && m->fail_kind == 2 && m->fail_piece == g - MULTI_PIECES) {
            m->fail_kind = 0;  // fires once: leaves the (still empty) group to the guard
            return set_err(h, TGMS_ERR_DEVICE, "injected failure inside a gather group (TGMS_MULTI_FAIL)");
        }
        for (; xi < P.xfers.size() && P.xfers[xi].group == g; ++xi) {
            const tgms::Xfer& x = P.xfers[xi];
            const ncclDataType_t dt = x.elem_bytes == 4 ? ncclInt32 : ncclFloat64;
            char* ws = m->dws[x.dev] + x.ws_byte;
            char* bp = batch_ptr(x);
            if (!x.gather) {
                TGMS_NCCL(h, m->r.send(bp, (size_t)x.count, dt, x.dev, m->comm[0], m->sm[0]));
                TGMS_NCCL(h, m->r.recv(ws, (size_t)x.count, dt, 0, m->comm[x.dev], m->sm[x.dev]));
            } else {
                TGMS_NCCL(h, m->r.send(ws, (size_t)x.count, dt, 0, m->comm[x.dev], m->sm[x.dev]));
                TGMS_NCCL(h, m->r.recv(bp, (size_t)x.count, dt, x.dev, m->comm[0], m->sm[0]));
            }
        }
        TGMS_NCCL(h, grp.end());
        return TGMS_OK;
    };
    // device 0: the caller's inputs are ready on ustream
    TGMS_HIP(h, hipSetDevice(0));
    TGMS_HIP(h, hipEventRecord(m->ev_start, ustream));
    TGMS_HIP(h, hipStreamWaitEvent(m->sm[0], m->ev_start, 0));
    // scatter, one group per piece index; the event marks piece k's inputs on its device
    // (its solve waits for that event alone, below: piece k of a device starts once its own
    // inputs have landed, not after the whole shard's)
    for (int k = 0; k < MULTI_PIECES; ++k) {
        tgms_status s = run_group(k);
        if (s != TGMS_OK) return s;
        for (int d = 0; d < n; ++d) {
            if (k >= (int)P.pieces[d].size()) continue;
            TGMS_HIP(h, hipSetDevice(d));
            TGMS_HIP(h, hipEventRecord(m->ev_in[d][k], m->sm[d]));
        }
        TGMS_HIP(h, hipSetDevice(0));
    }
    // device 0's own shard, in place on the caller's stream (beside the gathers)
    TGMS_HIP(h, hipSetDevice(0));
    if (!m->self_gather && bounds[1] > 0) {
        const int32_t b1 = bounds[1];
        tgms_status s = scratch_acquire(h, ustream);
        if (s != TGMS_OK) return s;
        if (refine) {
            // the shard's loop as one cached graph, planned on the device (its offsets
            // start at 0: shard 0 is the batch's first trajectories)
            s = loop_on_device(h, b1, (int64_t)a.h_so[b1], um, a.d_so, a.dW, a.dT, a.dED, a.k_T, a.eta, a.iters,
                               a.dC, a.d_cost, a.dSt, ustream);
        } else if (dev_solve) {
            s = ensure_perm_device(h, b1);
            if (s == TGMS_OK)
                s = solve_ragged_dev(h, b1, (int64_t)a.h_so[b1], a.d_so, a.dW, a.dT, a.dED, a.dC, a.dSt, ustream,
                                     DevPlanBufs{h->d_perm_hist, h->d_perm, h->d_plan});
        } else {
            Plan p0;
            if (a.checked && b1 == a.B) {  // the whole batch on device 0: validated already
                p0.counts = a.checked->counts;
                p0.uniform_m = a.checked->uniform_m;
                s = plan_upload(h, b1, a.h_so, &p0, ustream);
            } else {
                s = make_plan(h, b1, a.h_so, max_m, &p0, ustream);
            }
            if (s != TGMS_OK) return s;
            s = dispatch(h, p0, b1, a.d_so, a.dW, a.dT, a.dED, a.dC, a.dSt, ustream);
        }
        {  // released on failure too: a band call that launched must still write its marker
            const tgms_status r_ = scratch_release(h, ustream);
            if (s == TGMS_OK) s = r_;
        }
        if (s != TGMS_OK) return s;
    }
    // pieces: solve on the device, then gather to device 0 beside the next piece's solve
    for (int k = 0; k < MULTI_PIECES; ++k) {
        bool any = false;
        for (int d = 0; d < n; ++d) {
            if (k >= (int)P.pieces[d].size()) continue;
            any = true;
            const tgms::PiecePlan& p = P.pieces[d][k];
            char* w = m->dws[d];
            tgms_handle* hd = m->sub[d];
            TGMS_HIP(h, hipSetDevice(d));
            const int32_t* so_p = reinterpret_cast<const int32_t*>(w + p.oSo);
            double* Wp = reinterpret_cast<double*>(w + p.oW);
            double* Tp = reinterpret_cast<double*>(w + p.oT);
            const double* EDp = a.dED ? reinterpret_cast<const double*>(w + p.oED) : nullptr;
            double* Cp = a.dC ? reinterpret_cast<double*>(w + p.oC) : nullptr;
            int32_t* Stp = reinterpret_cast<int32_t*>(w + p.oSt);
            TGMS_HIP(h, hipStreamWaitEvent(m->sc[d], m->ev_in[d][k], 0));  // this piece's inputs only
            tgms_status s;
            if (refine) {
                // the piece's loop as one cached graph of its device's handle, planned on the
                // device from the raw offsets slice that arrived with its inputs
                const Plan& pl = plans[d][k];
                double* T[2] = {Tp, reinterpret_cast<double*>(w + p.oT2)};
                const DevPlanBufs dp{reinterpret_cast<int32_t*>(w + p.oHist), reinterpret_cast<int32_t*>(w + p.oPerm),
                                     reinterpret_cast<tgms::DevPlan*>(w + p.oPlan)};
                double* costp = reinterpret_cast<double*>(w + p.oCost);
                const int32_t np = p.n();
                const int64_t Sp = p.S();
                auto body = [&](hipStream_t q) -> tgms_status {
                    int cur = 0;
                    tgms_status r = refine_loop(hd, pl, np, Sp, so_p, Wp, T, EDp, a.k_T, a.eta, a.iters, Cp, costp,
                                                Stp, q, &cur, &dp);
                    if (r == TGMS_OK && cur == 1)
                        TGMS_HIP(hd, hipMemcpyAsync(Tp, T[1], (size_t)Sp * 8, hipMemcpyDeviceToDevice, q));
                    return r;
                };
                const tgms_handle::LoopKey key{np, a.iters, Sp, so_p, Wp, Tp, T[1], EDp, Cp, costp, Stp, dp.perm,
                                               dp.hist, dp.plan, a.k_T, a.eta, pl.uniform_m};
                s = run_loop_graph(hd, key, m->sc[d], body);
            } else if (dev_solve) {
                // planned on the device from the raw offsets slice that arrived with its inputs
                s = solve_ragged_dev(hd, p.n(), p.S(), so_p, Wp, Tp, EDp, Cp, Stp, m->sc[d],
                                     DevPlanBufs{reinterpret_cast<int32_t*>(w + p.oHist),
                                                 reinterpret_cast<int32_t*>(w + p.oPerm),
                                                 reinterpret_cast<tgms::DevPlan*>(w + p.oPlan)});
            } else {
                s = dispatch(hd, plans[d][k], p.n(), so_p, Wp, Tp, EDp, Cp, Stp, m->sc[d]);
            }
            if (s == TGMS_OK && m->fail_kind == 1 && m->fail_piece == k) {
                m->fail_kind = 0;  // fires once
                s = set_err(hd, TGMS_ERR_DEVICE, "injected failure of a piece's dispatch (TGMS_MULTI_FAIL)");
            }
            if (s != TGMS_OK) return hd == h ? s : set_err(h, s, std::string("device ") + std::to_string(d) + ": " +
                                                                 tgms_last_error(hd));
            TGMS_HIP(h, hipEventRecord(m->ev_piece[d][k], m->sc[d]));
            TGMS_HIP(h, hipStreamWaitEvent(m->sm[d], m->ev_piece[d][k], 0));
        }
        if (!any) break;
        TGMS_HIP(h, hipSetDevice(0));
        tgms_status s = run_group(MULTI_PIECES + k);
        if (s != TGMS_OK) return s;
    }
    TGMS_HIP(h, hipSetDevice(0));
    TGMS_HIP(h, hipEventRecord(m->ev_end, m->sm[0]));
    TGMS_HIP(h, hipStreamWaitEvent(ustream, m->ev_end, 0));
    return TGMS_OK;
}

tgms_status create_multi_ctx(tgms_handle* h, int n) {
    tgms_multi_ctx* m = new tgms_multi_ctx();
    h->multi = m;
    m->n = n;
    const char* sg = std::getenv("TGMS_MULTI_SELF_GATHER");
    m->self_gather = sg && sg[0] == '1';
    if (const char* f = std::getenv("TGMS_MULTI_FAIL")) {  // error-path test hook
        int k = -1;
        if (sscanf(f, "piece:%d", &k) == 1) m->fail_kind = 1;
        else if (sscanf(f, "group:%d", &k) == 1) m->fail_kind = 2;
        m->fail_piece = k;
    }
    std::string err;
    if (!m->r.load(&err)) return set_err(h, TGMS_ERR_DEVICE, err);
    m->comm.assign(n, nullptr);
    m->sub.assign(n, nullptr);
    m->sm.assign(n, nullptr);
    m->sc.assign(n, nullptr);
    m->dws.assign(n, nullptr);
    m->dws_cap.assign(n, 0);
    m->pin.assign(n, nullptr);
    m->pin_cap.assign(n, 0);
    m->ev_up.assign(n, nullptr);
    m->ev_in.assign(n, std::vector<hipEvent_t>(tgms::MULTI_PIECES, nullptr));
    m->up_pending.assign(n, false);
    m->ev_piece.assign(n, std::vector<hipEvent_t>(tgms::MULTI_PIECES, nullptr));
    std::vector<int> devs(n);
    for (int d = 0; d < n; ++d) devs[d] = d;
    TGMS_NCCL(h, m->r.comm_init_all(m->comm.data(), n, devs.data()));
    m->sub[0] = h;
    for (int d = 0; d < n; ++d) {
        if (d >= 1) {
            const tgms_status s = tgms_create(&m->sub[d], d);
            if (s != TGMS_OK) return set_err(h, s, "tgms_create on device " + std::to_string(d));
            m->sub[d]->method = h->method;
        }
        TGMS_HIP(h, hipSetDevice(d));
        TGMS_HIP(h, hipStreamCreateWithFlags(&m->sm[d], hipStreamNonBlocking));
        if (d == 0)
            TGMS_HIP(h, hipStreamCreateWithFlags(&m->sc[0], hipStreamNonBlocking));
        else
            m->sc[d] = m->sub[d]->stream;
        TGMS_HIP(h, hipEventCreateWithFlags(&m->ev_up[d], hipEventDisableTiming));
        for (auto& e : m->ev_in[d]) TGMS_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto& e : m->ev_piece[d]) TGMS_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    TGMS_HIP(h, hipSetDevice(0));
    TGMS_HIP(h, hipEventCreateWithFlags(&m->ev_start, hipEventDisableTiming));
    TGMS_HIP(h, hipEventCreateWithFlags(&m->ev_end, hipEventDisableTiming));
    return TGMS_OK;
}

}  // namespace


extern "C" {

// ---- multi-GPU ----

tgms_status tgms_create_multi(tgms_handle** out, int device_count) {
    if (!out) return TGMS_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TGMS_ERR_NO_DEVICE;
    if (device_count < 1 || device_count > n) return TGMS_ERR_INVALID_ARG;
    tgms_handle* h = nullptr;
    tgms_status s = tgms_create(&h, 0);
    if (s != TGMS_OK) return s;
    s = create_multi_ctx(h, device_count);
    if (s != TGMS_OK) {
        fprintf(stderr, "tgms_create_multi: %s\n", h->last_error.c_str());
        tgms_destroy(h);
        return s;
    }
    *out = h;
    return TGMS_OK;
}

int tgms_device_count(const tgms_handle* h) { return !h || h->host ? 0 : (h->multi ? h->multi->n : 1); }

tgms_status tgms_plan_shards(int32_t B, const int32_t* so, int32_t parts, int method, int32_t* bounds) {
    if (parts < 1 || !bounds || B < 0 || !so || so[0] != 0) return TGMS_ERR_INVALID_ARG;
    if (method != TGMS_METHOD_REDUCED && method != TGMS_METHOD_DENSE_KKT && method != TGMS_METHOD_BAND_KKT)
        return TGMS_ERR_INVALID_ARG;
    int32_t M0 = B > 0 ? so[1] - so[0] : 0, diff = 0;
    for (int32_t b = 0; b < B; ++b) {
        if (so[b + 1] - so[b] < 1) return TGMS_ERR_INVALID_ARG;
        diff |= (so[b + 1] - so[b]) ^ M0;
    }
    tgms::plan_shards(B, so, parts, method, bounds, diff == 0 ? M0 : 0);
    return TGMS_OK;
}

tgms_status tgms_multi_schedule(int32_t device_count, int32_t B, const int32_t* so, int method, int32_t flags,
                                int32_t* bounds, int64_t* ws_bytes, tgms_piece* pieces, int32_t piece_cap,
                                int32_t* n_pieces, tgms_xfer* xfers, int32_t xfer_cap, int32_t* n_xfers) {
    if (device_count < 1 || B < 0 || !so || so[0] != 0 || !bounds || !n_pieces || !n_xfers || piece_cap < 0 ||
        xfer_cap < 0)
        return TGMS_ERR_INVALID_ARG;
    if (method != TGMS_METHOD_REDUCED && method != TGMS_METHOD_DENSE_KKT && method != TGMS_METHOD_BAND_KKT)
        return TGMS_ERR_INVALID_ARG;
    int32_t M0 = 0;
    if (flags & TGMS_SCHED_REFINE) {
        // as tgms_refine_loop_multi_device: no pass over the offsets (the devices check each
        // trajectory's M), every batch on the device-grouped loop; the cuts are checked below
        if (B > 0 && (so[B] < B || (int64_t)so[B] > (int64_t)TGMS_MAX_SEGMENTS * B)) return TGMS_ERR_INVALID_ARG;
    } else if (method == TGMS_METHOD_REDUCED) {
        // as tgms_solve_batch_multi_device (scan_multi_offsets): the ends, and uniform
        // detection that stops at the first block with two different M
        if (B > 0 && (so[B] < B || (int64_t)so[B] > (int64_t)TGMS_MAX_SEGMENTS * B)) return TGMS_ERR_INVALID_ARG;
        const int32_t m0 = B > 0 ? so[1] - so[0] : 0;
        const bool uni = B > 0 && uniform_offsets(B, so, m0);
        if (uni && (m0 < 1 || m0 > TGMS_MAX_SEGMENTS)) return TGMS_ERR_INVALID_ARG;
        M0 = uni ? m0 : 0;
    } else {
        int32_t lo = INT32_MAX, hi = INT32_MIN;  // one vectorised pass (as scan_offsets)
        for (int32_t b = 0; b < B; ++b) {
            const int32_t M = so[b + 1] - so[b];
            lo = std::min(lo, M);
            hi = std::max(hi, M);
        }
        if (B > 0 && (lo < 1 || hi > TGMS_MAX_SEGMENTS)) return TGMS_ERR_INVALID_ARG;
        M0 = (B > 0 && lo == hi) ? lo : 0;
    }
    tgms::MultiFlags f;
    f.refine = flags & TGMS_SCHED_REFINE;
    f.has_ed = flags & TGMS_SCHED_END_DERIVS;
    f.has_c = flags & TGMS_SCHED_COEFFS;
    f.has_st = flags & TGMS_SCHED_STATUS;
    f.has_cost = flags & TGMS_SCHED_COST;
    f.self_gather = flags & TGMS_SCHED_SELF_GATHER;
    tgms::MultiPlan P;
    tgms::plan_multi(device_count, B, so, method, M0, f, &P);
    if (!tgms::cuts_valid(P, so)) return TGMS_ERR_INVALID_ARG;  // (as multi_enqueue)
    for (int d = 0; d <= device_count; ++d) bounds[d] = P.bounds[d];
    int32_t np = 0;
    for (int d = 0; d < device_count; ++d) {
        if (ws_bytes) ws_bytes[d] = (int64_t)P.ws_bytes[d];
        for (size_t k = 0; k < P.pieces[d].size(); ++k, ++np) {
            if (np >= piece_cap || !pieces) continue;
            const tgms::PiecePlan& p = P.pieces[d][k];
            tgms_piece& q = pieces[np];
            q.dev = d;
            q.piece = (int32_t)k;
            q.lo = p.lo;
            q.hi = p.hi;
            q.s0 = p.s0;
            q.s1 = p.s1;
            const size_t o[11] = {p.oSo, p.oPerm, p.oW, p.oT, p.oT2, p.oED, p.oC, p.oSt, p.oCost, p.oHist, p.oPlan};
            for (int j = 0; j < 11; ++j) q.ws_off[j] = (int64_t)o[j];
        }
    }
    *n_pieces = np;
    *n_xfers = (int32_t)P.xfers.size();
    for (size_t i = 0; i < P.xfers.size() && (int32_t)i < xfer_cap && xfers; ++i) {
        const tgms::Xfer& x = P.xfers[i];
        xfers[i] = tgms_xfer{x.dev, x.piece, x.gather, x.array, x.batch_elem, x.ws_byte, x.count, x.elem_bytes,
                             x.group};
    }
    return (np > piece_cap || *n_xfers > xfer_cap) ? TGMS_ERR_INVALID_ARG : TGMS_OK;
}

tgms_status tgms_solve_batch_multi_device(tgms_handle* h, int32_t B, const int32_t* h_so, const int32_t* d_so,
                                          const double* dW, const double* dT, const double* dED, double* dC,
                                          int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (!h->multi) return tgms_solve_batch_device(h, B, h_so, d_so, dW, dT, dED, dC, dSt, stream);
    Plan checked;
    // reduced method: no pass over a ragged batch's offsets on the host (its devices group and
    // check it, include/tgms.h); band / dense: the host-planned pieces need the validated counts
    tgms_status s = h->method == TGMS_METHOD_REDUCED
                        ? scan_multi_offsets(h, B, h_so, max_m_for(h), &checked.uniform_m)
                        : check_offsets(h, B, h_so, max_m_for(h), &checked.counts, &checked.uniform_m);
    if (s != TGMS_OK || B == 0) return s;
    if (!d_so || !dW || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC);
    s = no_capture(h, static_cast<hipStream_t>(stream), "a multi-GPU call");
    if (s != TGMS_OK) return s;
    MultiArgs a;
    a.checked = &checked;
    a.job = MultiJob::Solve;
    a.B = B;
    a.h_so = h_so;
    a.d_so = d_so;
    a.dW = dW;
    a.dT = const_cast<double*>(dT);  // read only for a solve
    a.dED = dED;
    a.dC = dC;
    a.dSt = dSt;
    return multi_run(h, a, static_cast<hipStream_t>(stream));
}

tgms_status tgms_refine_loop_multi_device(tgms_handle* h, int32_t B, const int32_t* h_so, const int32_t* d_so,
                                          const double* dW, double* dT, const double* dED, double k_T, double eta,
                                          int32_t iters, double* dC, double* d_cost, int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    // one device and no self-gather: the whole batch is device 0's shard, solved in place,
    // so the single-device loop (its captured graph, the M grouping on the device) is that
    // shard's path
    if (!h->multi || (h->multi->n == 1 && !h->multi->self_gather))
        return tgms_refine_loop_device(h, B, h_so, d_so, dW, dT, dED, k_T, eta, iters, dC, d_cost, dSt, stream);
    tgms_status s = check_refine_args(h, k_T, eta);
    if (s != TGMS_OK) return s;
    if (iters < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "iters < 0");
    // No pass over the offsets on the host (round 5, VERDICT r04 item 2: the host work before
    // the first transfer stays O(devices x pieces x log B)).  The host checks what its schedule
    // rests on -- so[0], the span, the shard and piece cuts (multi_enqueue) -- and every
    // piece's device plan checks each trajectory's M (k_plan_scatter: a piece whose offsets are
    // bad runs nothing and returns TGMS_ERR_INVALID_ARG statuses and zeros).  Every batch,
    // uniform ones too, runs the device-grouped loop.
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "B < 0");
    if (!h_so) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets is NULL");
    if (h_so[0] != 0) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets[0] != 0");
    if (B == 0) return TGMS_OK;
    if (h_so[B] < B || (int64_t)h_so[B] > (int64_t)TGMS_MAX_SEGMENTS * B)
        return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets[B] outside [B, 16 B]");
    Plan checked;  // uniform_m = 0: the ragged (device-planned) loop
    if (!d_so || !dW || !dT) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC, d_cost);
    s = no_capture(h, static_cast<hipStream_t>(stream), "a multi-GPU call");
    if (s != TGMS_OK) return s;
    MultiArgs a;
    a.checked = &checked;
    a.job = MultiJob::Refine;
    a.B = B;
    a.h_so = h_so;
    a.d_so = d_so;
    a.dW = dW;
    a.dT = dT;
    a.dED = dED;
    a.dC = dC;
    a.d_cost = d_cost;
    a.dSt = dSt;
    a.k_T = k_T;
    a.eta = eta;
    a.iters = iters;
    return multi_run(h, a, static_cast<hipStream_t>(stream));
}

tgms_status tgms_solve_batch_multi(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                                   const double* seg_times, const double* end_derivs, double* coeffs,
                                   int32_t* status) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (!h->multi) return tgms_solve_batch(h, B, so, waypoints, seg_times, end_derivs, coeffs, status);
    Plan checked;
    tgms_status s = check_offsets(h, B, so, max_m_for(h), &checked.counts, &checked.uniform_m);
    if (s != TGMS_OK || B == 0) return s;
    if (!waypoints || !seg_times || !coeffs)
        return set_err(h, TGMS_ERR_INVALID_ARG, "NULL waypoints/seg_times/coeffs");
    const size_t S = (size_t)so[B];
    double *dW, *dT, *dED, *dC;
    int32_t *dSt, *dSo;
    s = stage(h, {input(&dW, waypoints, (S + B) * 3), input(&dT, seg_times, S), input(&dED, end_derivs, (size_t)B * 18),
                  output(&dC, S * 24), output(&dSt, (size_t)B), input(&dSo, so, (size_t)B + 1)});
    if (s != TGMS_OK) return s;
    MultiArgs a;
    a.checked = &checked;
    a.B = B;
    a.h_so = so;
    a.d_so = dSo;
    a.dW = dW;
    a.dT = dT;
    a.dED = dED;
    a.dC = dC;
    a.dSt = dSt;
    s = multi_run(h, a, h->stream);
    (void)hipSetDevice(h->device);
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, fetch(h, coeffs, dC, S * 24));
    return finish_status(h, dSt, status, B, true);
}

}  // extern "C"
