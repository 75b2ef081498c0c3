// tgms_capi.hip — C ABI of libtgms (include/tgms.h): handles, validation of the CSR offsets,
// host<->device staging, ragged-batch planning and the solve / refine / sample entry points.
// The multi-GPU scheduler, the analysis calls and the map calls have units of their own
// (tgms_capi_multi.hip, tgms_capi_analysis.hip, tgms_capi_map.hip); tgms_capi.h is what they share.
//
// Error conventions mirror the reference's boundary: no C++
// exceptions cross the ABI, every entry point returns a tgms_status, and the
// MinSnap adapter maps a failure to the reference's RCLCPP_ERROR + exit(1)
// (Line.cpp:77-78).  There is deliberately NO CPU fallback: without a HIP
// device tgms_create() fails with TGMS_ERR_NO_DEVICE.
#include <chrono>
#include <thread>

#include "tgms_capi.h"
#include "tgms_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

// File-local helpers are `static`; the rest is declared in tgms_capi.h for the other units.
namespace tgms::capi {

tgms_status hip_err(tgms_handle* h, hipError_t e, const char* where) {
    if (e == hipSuccess) return TGMS_OK;
    return set_err(h, TGMS_ERR_DEVICE, std::string(where) + ": " + hipGetErrorString(e));
}

tgms_status ensure_ws(tgms_handle* h, size_t bytes) {
    if (bytes <= h->ws_cap) return TGMS_OK;
    if (h->d_ws) {
        TGMS_HIP(h, hipStreamSynchronize(h->stream));
        TGMS_HIP(h, hipFree(h->d_ws));
        h->d_ws = nullptr;
        h->ws_cap = 0;
    }
    TGMS_HIP(h, hipMalloc(&h->d_ws, bytes));
    h->ws_cap = bytes;
    return TGMS_OK;
}

tgms_status stage(tgms_handle* h, std::initializer_list<Region> regions) {
    TGMS_HIP(h, hipSetDevice(h->device));
    size_t off = 0;
    for (const Region& r : regions) off = align256(off + r.bytes);
    const tgms_status s = ensure_ws(h, off);
    if (s != TGMS_OK) return s;
    char* const base = static_cast<char*>(h->d_ws);
    off = 0;
    for (const Region& r : regions) {
        char* const d = r.bytes ? base + off : nullptr;
        r.set(r.slot, d);
        if (d && r.src) TGMS_HIP(h, hipMemcpyAsync(d, r.src, r.bytes, hipMemcpyHostToDevice, h->stream));
        off = align256(off + r.bytes);
    }
    return TGMS_OK;
}

// The worst per-trajectory status of a batch; `message`: the first trajectory that has it
// goes into last_error.
static tgms_status worst_status(tgms_handle* h, const int32_t* st, int32_t B, bool message) {
    int worst = TGMS_OK;
    for (int32_t b = 0; b < B; ++b) worst = std::max(worst, (int)st[b]);
    if (worst != TGMS_OK && message) {
        for (int32_t b = 0; b < B; ++b)
            if (st[b] == worst) {
                char buf[160];
                snprintf(buf, sizeof buf, "trajectory %d: %s", b, tgms_status_string(worst));
                h->last_error = buf;
                break;
            }
    }
    return (tgms_status)worst;
}

// The end of a blocking solve: the statuses go to the caller (or, for status == NULL, into a
// temporary), the stream is drained, and the worst status is the call's result.
tgms_status finish_status(tgms_handle* h, const int32_t* dSt, int32_t* status, int32_t B, bool message) {
    std::vector<int32_t> tmp;
    if (!status) {
        tmp.resize(B);
        status = tmp.data();
    }
    TGMS_HIP(h, fetch(h, status, dSt, (size_t)B));
    TGMS_HIP(h, hipStreamSynchronize(h->stream));
    return worst_status(h, status, B, message);
}

// True while `stream` is being captured into a HIP graph.
bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// Order `stream` after every earlier user of the handle's device scratch.  Inside a
// caller's stream capture the handshake is skipped (an event recorded outside the
// capture cannot order a graph's replays): a graph that holds band-KKT launches must
// be replayed in stream order with the handle's other scratch users (include/tgms.h).
tgms_status scratch_acquire(tgms_handle* h, hipStream_t stream) {
    if (h->scratch_pending && !capturing(stream)) TGMS_HIP(h, hipStreamWaitEvent(stream, h->scratch_ev, 0));
    return TGMS_OK;
}

// The work just enqueued on `stream` is the scratch's latest user.
tgms_status scratch_release(tgms_handle* h, hipStream_t stream) {
    if (capturing(stream)) return TGMS_OK;
    TGMS_HIP(h, hipEventRecord(h->scratch_ev, stream));
    h->scratch_pending = true;
    if (h->band_unmarked) {
        TGMS_HIP(h, hipStreamWriteValue32(stream, h->band_done, ++h->band_seq, 0));
        h->band_unmarked = false;
    }
    return TGMS_OK;
}

// After a dispatch that returned `s`: released on failure too (a band call that launched
// must still write its marker); the first error is the result.
tgms_status scratch_release(tgms_handle* h, hipStream_t stream, tgms_status s) {
    const tgms_status r = scratch_release(h, stream);
    return s != TGMS_OK ? s : r;
}

tgms_status no_capture(tgms_handle* h, hipStream_t stream, const char* what) {
    if (!capturing(stream)) return TGMS_OK;
    return set_err(h, TGMS_ERR_UNSUPPORTED,
                   std::string(what) + " cannot be captured into a HIP graph: it uploads a launch plan from the "
                                       "handle's host staging (or grows device scratch) at call time; capture "
                                       "uniform solves, or issue this call outside the capture");
}

static tgms_status ensure_loop_ws(tgms_handle* h, size_t bytes) {
    if (bytes <= h->loop_ws_cap) return TGMS_OK;
    if (h->d_loop_ws) {
        TGMS_HIP(h, hipDeviceSynchronize());
        TGMS_HIP(h, hipFree(h->d_loop_ws));
        h->d_loop_ws = nullptr;
        h->loop_ws_cap = 0;
    }
    TGMS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->d_loop_ws), bytes));
    h->loop_ws_cap = bytes;
    return TGMS_OK;
}

tgms_status ensure_nbr_ws(tgms_handle* h, size_t bytes) {
    if (bytes <= h->nbr_ws_cap) return TGMS_OK;
    if (h->d_nbr_ws) {
        TGMS_HIP(h, hipDeviceSynchronize());
        TGMS_HIP(h, hipFree(h->d_nbr_ws));
        h->d_nbr_ws = nullptr;
        h->nbr_ws_cap = 0;
    }
    TGMS_HIP(h, hipMalloc(&h->d_nbr_ws, bytes));
    h->nbr_ws_cap = bytes;
    return TGMS_OK;
}

// The device-side grouping of the refinement loop: the permutation buffer (shared with the
// host-planned paths) and the per-block counts.
tgms_status ensure_perm_device(tgms_handle* h, int32_t B) {
    if ((size_t)B > h->perm_cap) {
        if (h->d_perm) {
            TGMS_HIP(h, hipDeviceSynchronize());
            TGMS_HIP(h, hipFree(h->d_perm));
            h->d_perm = nullptr;
        }
        TGMS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->d_perm), sizeof(int32_t) * B));
        h->perm_cap = B;
    }
    const size_t need = tgms::perm_hist_bytes(B);
    if (need > h->perm_hist_cap) {
        if (h->d_perm_hist) {
            TGMS_HIP(h, hipDeviceSynchronize());
            TGMS_HIP(h, hipFree(h->d_perm_hist));
            h->d_perm_hist = nullptr;
        }
        TGMS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->d_perm_hist), need));
        h->perm_hist_cap = need;
    }
    if (!h->d_plan) TGMS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->d_plan), sizeof(tgms::DevPlan)));
    return TGMS_OK;
}

// One pass over the offsets: the smallest and largest M (a vectorised min/max), all the
// device-planned paths need from the host (validation and uniform detection); the slow
// scan of check_offsets runs only to name the first offending trajectory.
// min and max of M = so[b+1] - so[b] over the batch: the per-call host pass of the
// device-pointer entry points (1,048,576 offsets at config 5's full size).  The loop
// vectorises; the AVX2 build of it (8 differences per instruction) runs where the CPU has
// AVX2 -- the baseline x86-64 target has no packed 32-bit min/max (round 6: 0.37 ms of host
// time per full-size refinement call, most of it this scan).
#define TGMS_MINMAX_M_BODY                          \
    int32_t l = INT32_MAX, u = INT32_MIN;           \
    for (int32_t b = 0; b < B; ++b) {               \
        const int32_t m = so[b + 1] - so[b];        \
        l = m < l ? m : l;                          \
        u = m > u ? m : u;                          \
    }                                               \
    lo = l;                                         \
    hi = u;
__attribute__((target("avx2"))) static void minmax_m_avx2(int32_t B, const int32_t* so, int32_t& lo, int32_t& hi) {
    TGMS_MINMAX_M_BODY
}
static void minmax_m_base(int32_t B, const int32_t* so, int32_t& lo, int32_t& hi) { TGMS_MINMAX_M_BODY }
#undef TGMS_MINMAX_M_BODY

static tgms_status scan_offsets(tgms_handle* h, int32_t B, const int32_t* so, int max_m, int* uniform_m) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "B < 0");
    if (!so) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets is NULL");
    if (so[0] != 0) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets[0] != 0");
    static const bool avx2 = __builtin_cpu_supports("avx2");
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    if (avx2)
        minmax_m_avx2(B, so, lo, hi);
    else
        minmax_m_base(B, so, lo, hi);
    if (B > 0 && (lo < 1 || hi > max_m)) {
        const tgms_status st = check_offsets(h, B, so, max_m, nullptr, nullptr);
        return st != TGMS_OK ? st : set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets out of range");
    }
    *uniform_m = (B > 0 && lo == hi) ? lo : 0;
    return TGMS_OK;
}

// Validates a CSR segment layout on the host; fills per-M counts.
// Host planning of ragged batches (a config-5 batch of 1,048,576 trajectories has to be
// validated and grouped by M on every call): the offsets are scanned in PLAN_CHUNKS
// contiguous chunks interleaved in one loop, so the per-chunk histogram updates (and the
// counting-sort cursors below) form independent dependency chains instead of one.
constexpr int PLAN_CHUNKS = 4;
constexpr int PLAN_BINS = TGMS_MAX_SEGMENTS + 2;  // M clamped into 0..MAX+1: 0 and MAX+1 are "out of range"
struct ChunkHist {
    int32_t B = -1;
    const int32_t* so = nullptr;
    int32_t h[PLAN_CHUNKS][PLAN_BINS];
};
static thread_local ChunkHist t_hist;  // the last ragged check_offsets of this thread, reused by upload_plan

static void chunk_hist(int32_t B, const int32_t* so, ChunkHist& ch) {
    std::memset(ch.h, 0, sizeof ch.h);
    const int32_t L = B / PLAN_CHUNKS;
    auto bin = [](int32_t M) { return M < 0 ? 0 : (M > TGMS_MAX_SEGMENTS ? TGMS_MAX_SEGMENTS + 1 : M); };
    for (int32_t i = 0; i < L; ++i)
        for (int c = 0; c < PLAN_CHUNKS; ++c) {
            const int32_t b = c * L + i;
            ch.h[c][bin(so[b + 1] - so[b])]++;
        }
    for (int32_t b = PLAN_CHUNKS * L; b < B; ++b) ch.h[PLAN_CHUNKS - 1][bin(so[b + 1] - so[b])]++;
    ch.B = B;
    ch.so = so;
}

tgms_status check_offsets(tgms_handle* h, int32_t B, const int32_t* so, int max_m,
                          std::vector<int32_t>* counts, int* uniform_m) {
    if (B < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "B < 0");
    if (!so) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets is NULL");
    if (so[0] != 0) return set_err(h, TGMS_ERR_INVALID_ARG, "seg_offsets[0] != 0");
    if (counts) counts->assign(max_m + 1, 0);
    // uniform batches (the common large case): one vectorisable pass over the offsets,
    // in blocks so a ragged batch leaves it after its first block
    if (B > 0) {
        const int32_t M0 = so[1] - so[0];
        int32_t diff = 0;
        for (int32_t b0 = 0; b0 < B && diff == 0; b0 += 4096) {
            const int32_t e = std::min(B, b0 + 4096);
            for (int32_t b = b0; b < e; ++b) diff |= (so[b + 1] - so[b]) ^ M0;
        }
        if (diff == 0 && M0 >= 1 && M0 <= TGMS_MAX_SEGMENTS && M0 <= max_m) {
            if (counts) (*counts)[M0] = B;
            if (uniform_m) *uniform_m = M0;
            return TGMS_OK;
        }
    }
    ChunkHist& ch = t_hist;
    chunk_hist(B, so, ch);
    int32_t tot[PLAN_BINS] = {};
    for (int c = 0; c < PLAN_CHUNKS; ++c)
        for (int m = 0; m < PLAN_BINS; ++m) tot[m] += ch.h[c][m];
    bool bad = tot[0] || tot[TGMS_MAX_SEGMENTS + 1];
    for (int m = max_m + 1; m <= TGMS_MAX_SEGMENTS; ++m) bad = bad || tot[m];
    if (bad) {  // rare: report the first offending trajectory, as a sequential scan would
        ch.B = -1;
        for (int32_t b = 0; b < B; ++b) {
            const int32_t M = so[b + 1] - so[b];
            if (M < 1 || M > TGMS_MAX_SEGMENTS) {
                char buf[128];
                snprintf(buf, sizeof buf, "trajectory %d has %d segments (allowed 1..%d)", b, M,
                         TGMS_MAX_SEGMENTS);
                return set_err(h, TGMS_ERR_INVALID_ARG, buf);
            }
            if (M > max_m) {
                char buf[128];
                snprintf(buf, sizeof buf, "trajectory %d has %d segments; method supports <= %d", b, M, max_m);
                return set_err(h, TGMS_ERR_UNSUPPORTED, buf);
            }
        }
    }
    int um = 0;
    for (int m = 1; m <= max_m; ++m) {
        if (counts) (*counts)[m] = tot[m];
        if (B > 0 && tot[m] == B) um = m;
    }
    if (uniform_m) *uniform_m = (B > 0) ? um : -1;
    return TGMS_OK;
}

// Groups trajectories by M (counting sort) and uploads the permutation.
static tgms_status upload_plan(tgms_handle* h, int32_t B, const int32_t* so,
                        const std::vector<int32_t>& counts, std::vector<int32_t>* starts,
                        hipStream_t stream) {
    starts->assign(counts.size() + 1, 0);
    for (size_t m = 1; m < counts.size(); ++m) (*starts)[m + 1] = (*starts)[m] + counts[m];
    if ((size_t)B > h->h_perm_cap) {
        if (h->h_perm) {
            TGMS_HIP(h, hipEventSynchronize(h->perm_ev));
            TGMS_HIP(h, hipHostFree(h->h_perm));
        }
        TGMS_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_perm), sizeof(int32_t) * B));
        h->h_perm_cap = B;
    }
    if ((size_t)B > h->perm_cap) {
        if (h->d_perm) {
            TGMS_HIP(h, hipDeviceSynchronize());
            TGMS_HIP(h, hipFree(h->d_perm));
        }
        TGMS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->d_perm), sizeof(int32_t) * B));
        h->perm_cap = B;
    }
    TGMS_HIP(h, hipEventSynchronize(h->perm_ev));  // previous upload must have drained
    // stable counting sort: chunk c's trajectories of each M follow chunk c-1's, and the
    // PLAN_CHUNKS cursors advance independently
    ChunkHist& ch = t_hist;
    if (!(ch.B == B && ch.so == so)) chunk_hist(B, so, ch);
    int32_t cur[PLAN_CHUNKS][PLAN_BINS];
    for (int m = 0; m < PLAN_BINS; ++m) {
        int32_t base = (m >= 1 && (size_t)m < counts.size()) ? (*starts)[m] : 0;
        for (int c = 0; c < PLAN_CHUNKS; ++c) {
            cur[c][m] = base;
            base += ch.h[c][m];
        }
    }
    const int32_t L = B / PLAN_CHUNKS;
    int32_t* const perm = h->h_perm;
    for (int32_t i = 0; i < L; ++i)
        for (int c = 0; c < PLAN_CHUNKS; ++c) {
            const int32_t b = c * L + i;
            perm[cur[c][so[b + 1] - so[b]]++] = b;
        }
    for (int32_t b = PLAN_CHUNKS * L; b < B; ++b) perm[cur[PLAN_CHUNKS - 1][so[b + 1] - so[b]]++] = b;
    ch.B = -1;  // the offsets may change before the next call
    TGMS_HIP(h, hipMemcpyAsync(h->d_perm, h->h_perm, sizeof(int32_t) * B, hipMemcpyHostToDevice, stream));
    TGMS_HIP(h, hipEventRecord(h->perm_ev, stream));
    return TGMS_OK;
}

// The plan of a batch whose offsets check_offsets already validated into p->counts /
// p->uniform_m (one host pass per call): uploads the grouping of a ragged batch.
tgms_status plan_upload(tgms_handle* h, int32_t B, const int32_t* h_so, Plan* p, hipStream_t stream) {
    if (B == 0 || p->uniform_m > 0) return TGMS_OK;
    tgms_status s = no_capture(h, stream, "a ragged batch");
    if (s != TGMS_OK) return s;
    s = upload_plan(h, B, h_so, p->counts, &p->starts, stream);
    p->d_perm = h->d_perm;
    return s;
}

tgms_status make_plan(tgms_handle* h, int32_t B, const int32_t* h_so, int max_m, Plan* p, hipStream_t stream) {
    tgms_status s = check_offsets(h, B, h_so, max_m, &p->counts, &p->uniform_m);
    if (s != TGMS_OK) return s;
    return plan_upload(h, B, h_so, p, stream);
}

static tgms_status ensure_aux(tgms_handle* h) {
    if (h->aux_ready) return TGMS_OK;
    TGMS_HIP(h, hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
    for (int j = 0; j < TGMS_AUX_STREAMS; ++j) {
        TGMS_HIP(h, hipStreamCreateWithFlags(&h->aux[j], hipStreamNonBlocking));
        TGMS_HIP(h, hipEventCreateWithFlags(&h->join_ev[j], hipEventDisableTiming));
    }
    h->aux_ready = true;
    return TGMS_OK;
}

// Run independent launches (each `hipError_t(hipStream_t)`): one goes on `stream`;
// several fork onto the auxiliary streams and join back, so `stream` order is kept
// for the caller.
static tgms_status run_parallel(tgms_handle* h, hipStream_t stream,
                         const std::vector<std::function<hipError_t(hipStream_t)>>& jobs) {
    if (jobs.size() <= 1 || TGMS_AUX_STREAMS <= 1) {
        for (auto& j : jobs) TGMS_HIP(h, j(stream));
        return TGMS_OK;
    }
    tgms_status s = ensure_aux(h);
    if (s != TGMS_OK) return s;
    const int used = (int)std::min<size_t>(jobs.size(), TGMS_AUX_STREAMS);
    TGMS_HIP(h, hipEventRecord(h->fork_ev, stream));
    for (int j = 0; j < used; ++j) TGMS_HIP(h, hipStreamWaitEvent(h->aux[j], h->fork_ev, 0));
    for (size_t g = 0; g < jobs.size(); ++g) TGMS_HIP(h, jobs[g](h->aux[g % used]));
    for (int j = 0; j < used; ++j) {
        TGMS_HIP(h, hipEventRecord(h->join_ev[j], h->aux[j]));
        TGMS_HIP(h, hipStreamWaitEvent(stream, h->join_ev[j], 0));
    }
    return TGMS_OK;
}

// Reduced method, ragged plan: every M group in one launch per occupancy class
// (M <= 11 / M >= 12), the longest groups' wavefronts first.
static void class_tables(const Plan& p, bool has_ed, tgms::GroupTable (&tab)[2]) {
    tab[0] = tgms::GroupTable{};
    tab[1] = tgms::GroupTable{};
    const int max2 = tgms::two_wave_max_m(has_ed);
    for (size_t m = p.counts.size(); m-- > 1;) {
        if (!p.counts[m]) continue;
        tgms::GroupTable& t = tab[(int)m > max2 ? 1 : 0];
        const int g = t.ngroups++;
        t.m[g] = (int32_t)m;
        t.n[g] = p.counts[m];
        t.perm[g] = p.d_perm + p.starts[m];
        t.blk_end[g] = (g ? t.blk_end[g - 1] : 0) + (p.counts[m] + tgms::RAGGED_TPW - 1) / tgms::RAGGED_TPW;
    }
}

static tgms_status run_ragged_multi(tgms_handle* h, const Plan& p, hipStream_t stream, bool refine, const int32_t* d_so,
                             const double* W, const double* T, const double* ED, double kT, double eta,
                             double* Tout, double* cost, double* C, int32_t* st) {
    tgms::GroupTable tab[2];
    class_tables(p, ED != nullptr, tab);
    std::vector<std::function<hipError_t(hipStream_t)>> jobs;
    for (int c = 1; c >= 0; --c)
        if (tab[c].ngroups)
            jobs.push_back([&, c](hipStream_t q) {
                return tgms::launch_ragged_multi(c, tab[c], refine, d_so, W, T, ED, kT, eta, Tout, cost, C, st, q);
            });
    return run_parallel(h, stream, jobs);
}

// Band-KKT scratch for largest M `m_max`; the slabs are per wavefront of one launch, so
// launches sharing them are serialised (uncaptured: by the scratch event; captured: the
// graph slab, whose replays the caller keeps in stream order, include/tgms.h).  *slab
// receives the slab this launch must use.
static tgms_status ensure_band(tgms_handle* h, int m_max, hipStream_t stream, double** slab) {
    if (h->band_grid == 0) {
        int cus = 0;
        TGMS_HIP(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        h->band_grid = std::max(1, cus) * tgms::BAND_WAVES_PER_CU;
    }
    const size_t need = tgms::band_scratch_bytes(m_max, h->band_grid);
    if (capturing(stream)) {
        if (!(h->d_band_graph && need <= h->band_graph_cap)) {
            // hand the uncaptured slab to the graphs (no allocation inside a capture)
            if (!(h->d_band && need <= h->band_cap))
                return no_capture(h, stream, "a band-KKT call that grows the handle's slab");
            // An uncaptured call may still be running on that slab (on any stream): nothing
            // orders the graphs' replays after it, so the host waits for it here -- on the
            // pinned completion word, not a HIP call (hipEventSynchronize inside a capture
            // invalidates it, round 5)
            if (h->band_unmarked)  // cannot happen since every uncaptured band call releases
                return set_err(h, TGMS_ERR_DEVICE,
                               "an uncaptured band-KKT call ended without its completion marker; the capture "
                               "cannot tell when the slab it takes over is free");
            if (h->band_done) {
                const auto t0 = std::chrono::steady_clock::now();
                while ((int32_t)(__atomic_load_n(h->band_done, __ATOMIC_ACQUIRE) - h->band_seq) < 0) {
                    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
                        return set_err(h, TGMS_ERR_DEVICE,
                                       "a band-KKT capture waited 60 s for an uncaptured call on the slab it takes over");
                    std::this_thread::sleep_for(std::chrono::microseconds(20));
                }
            }
            if (h->d_band_graph) h->band_retired.push_back(h->d_band_graph);  // an older graph may use it
            h->d_band_graph = h->d_band;
            h->band_graph_cap = h->band_cap;
            h->d_band = nullptr;
            h->band_cap = 0;
        }
        *slab = h->d_band_graph;
        return TGMS_OK;
    }
    if (!h->band_done) {
        TGMS_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->band_done), sizeof(uint32_t),
                                  hipHostMallocMapped | hipHostMallocCoherent));
        *h->band_done = h->band_seq;
    }
    h->band_unmarked = true;  // this call's release writes the marker
    if (need > h->band_cap) {
        if (h->d_band) {
            TGMS_HIP(h, hipStreamSynchronize(stream));
            TGMS_HIP(h, hipDeviceSynchronize());
            TGMS_HIP(h, hipFree(h->d_band));
            h->d_band = nullptr;
            h->band_cap = 0;
        }
        TGMS_HIP(h, hipMalloc(&h->d_band, need));
        h->band_cap = need;
    }
    *slab = h->d_band;
    return TGMS_OK;
}

tgms_status dispatch(tgms_handle* h, const Plan& p, int32_t B, const int32_t* d_so, const double* W,
                     const double* T, const double* ED, double* C, int32_t* st, hipStream_t stream) {
    if (B == 0) return TGMS_OK;
    if (h->method == TGMS_METHOD_BAND_KKT) {
        int m_max = p.uniform_m;
        for (size_t m = 1; m < p.counts.size(); ++m)
            if (p.counts[m]) m_max = std::max(m_max, (int)m);
        double* slab = nullptr;
        tgms_status s = ensure_band(h, m_max, stream, &slab);
        if (s != TGMS_OK) return s;
        if (p.uniform_m > 0) {
            TGMS_HIP(h, tgms::launch_band_kkt(p.uniform_m, B, nullptr, nullptr, W, T, ED, C, st, slab,
                                              h->band_grid, stream));
            return TGMS_OK;
        }
        for (size_t m = p.counts.size(); m-- > 1;)
            if (p.counts[m])
                TGMS_HIP(h, tgms::launch_band_kkt((int)m, p.counts[m], p.d_perm + p.starts[m], d_so, W, T, ED, C,
                                                  st, slab, h->band_grid, stream));
        return TGMS_OK;
    }
    if (p.uniform_m > 0) {
        if (h->method == TGMS_METHOD_REDUCED)
            TGMS_HIP(h, tgms::launch_reduced_uniform(p.uniform_m, B, W, T, ED, C, st, stream));
        else
            TGMS_HIP(h, tgms::launch_dense_kkt(p.uniform_m, B, nullptr, nullptr, W, T, ED, C, st, stream));
        return TGMS_OK;
    }
    if (h->method == TGMS_METHOD_REDUCED)
        return run_ragged_multi(h, p, stream, false, d_so, W, T, ED, 0.0, 0.0, nullptr, nullptr, C, st);
    std::vector<std::function<hipError_t(hipStream_t)>> jobs;
    for (size_t m = p.counts.size(); m-- > 1;)
        if (p.counts[m])
            jobs.push_back([&, m](hipStream_t q) {
                return tgms::launch_dense_kkt((int)m, p.counts[m], p.d_perm + p.starts[m], d_so, W, T, ED, C, st, q);
            });
    return run_parallel(h, stream, jobs);
}

// One refinement step over a batch (uniform or ragged), reduced method only.
static tgms_status dispatch_refine(tgms_handle* h, const Plan& p, int32_t B, const int32_t* d_so, const double* W,
                            const double* T, const double* ED, double kT, double eta, double* Tout, double* cost,
                            int32_t* st, hipStream_t stream) {
    if (B == 0) return TGMS_OK;
    if (p.uniform_m > 0) {
        TGMS_HIP(h, tgms::launch_refine_uniform(p.uniform_m, B, W, T, ED, kT, eta, Tout, cost, st, stream));
        return TGMS_OK;
    }
    return run_ragged_multi(h, p, stream, true, d_so, W, T, ED, kT, eta, Tout, cost, nullptr, st);
}

// `iters` steps ping-ponging between T[0] and T[1] (the final times end in T[*cur]),
// the cost at the final times (a step with eta = 0 leaves them unchanged), and the
// final solve into C when it is not NULL.  S: the batch's segment count (so[B] - so[0]).
tgms_status refine_loop(tgms_handle* h, const Plan& p, int32_t B, int64_t S, const int32_t* d_so, const double* W,
                        double* const T[2], const double* ED, double kT, double eta, int32_t iters, double* C,
                        double* cost, int32_t* st, hipStream_t stream, int* cur, const DevPlanBufs* dp) {
    if (B > 0 && p.uniform_m == 0) {
        // Ragged: every step of a trajectory only involves that trajectory, so each
        // occupancy class runs its whole loop (steps, cost, final solve) in ONE launch,
        // times kept in LDS between steps and updated in place in T[0]; the two classes'
        // launches run side by side.  The grouping by M and both classes' tables are
        // computed on the device first (k_perm_hist, k_plan_scatter).
        if (!dp || !dp->hist || !dp->perm || !dp->plan)
            return set_err(h, TGMS_ERR_DEVICE, "internal: ragged refinement loop without plan buffers");
        TGMS_HIP(h, tgms::launch_group_plan_dev(B, S, d_so, ED != nullptr, dp->hist, dp->perm, dp->plan, st, C, cost,
                                                stream));
        std::vector<std::function<hipError_t(hipStream_t)>> jobs;
        // the one-wave class first (launching the longer two-wave class first, or both
        // without the loop's graph, measured 0.58-0.60 ms against 0.52-0.53)
        for (int k = 1; k >= 0; --k)
            jobs.push_back([&, k](hipStream_t q) {
                return tgms::launch_refine_loop_dev(k, B, dp->plan, d_so, W, T[0], ED, kT, eta, iters, cost, C, st, q);
            });
        tgms_status s = run_parallel(h, stream, jobs);
        if (s != TGMS_OK) return s;
        *cur = 0;
        return TGMS_OK;
    }
    int c = 0;
    for (int32_t k = 0; k < iters; ++k, c ^= 1) {
        tgms_status s = dispatch_refine(h, p, B, d_so, W, T[c], ED, kT, eta, T[c ^ 1], nullptr, st, stream);
        if (s != TGMS_OK) return s;
    }
    if (cost) {
        tgms_status s = dispatch_refine(h, p, B, d_so, W, T[c], ED, kT, 0.0, T[c ^ 1], cost, st, stream);
        if (s != TGMS_OK) return s;
    }
    if (C) {
        tgms_status s = dispatch(h, p, B, d_so, W, T[c], ED, C, st, stream);
        if (s != TGMS_OK) return s;
    }
    *cur = c;
    return TGMS_OK;
}

// A ragged solve (reduced method) grouped on the device (round 6): k_perm_hist ->
// k_plan_scatter, then both occupancy classes from the device plan, so
// the host makes no pass over the offsets.  A bad M fails the batch on the device
// (TGMS_ERR_INVALID_ARG where M is outside 1..16, TGMS_ERR_SKIPPED elsewhere, zeros).
tgms_status solve_ragged_dev(tgms_handle* h, int32_t B, int64_t S, const int32_t* d_so, const double* W,
                             const double* T, const double* ED, double* C, int32_t* st, hipStream_t stream,
                             const DevPlanBufs& dp) {
    if (B <= 0) return TGMS_OK;
    if (!dp.hist || !dp.perm || !dp.plan) return set_err(h, TGMS_ERR_DEVICE, "internal: ragged solve without plan buffers");
    TGMS_HIP(h, tgms::launch_group_plan_dev(B, S, d_so, ED != nullptr, dp.hist, dp.perm, dp.plan, st, C, nullptr,
                                            stream));
    std::vector<std::function<hipError_t(hipStream_t)>> jobs;
    for (int k = 1; k >= 0; --k)
        jobs.push_back([&, k](hipStream_t q) {
            return tgms::launch_reduced_multi_dev(k, B, dp.plan, d_so, W, T, ED, C, st, q);
        });
    return run_parallel(h, stream, jobs);
}

// Replay the handle's graph for `key`, capturing `body` into it first if there is none
// (at most kLoopGraphs cached per handle, least recently used evicted).  Runs on the
// handle's device (the caller has selected it).
constexpr size_t kLoopGraphs = 16;
tgms_status run_loop_graph(tgms_handle* h, const tgms_handle::LoopKey& key, hipStream_t stream,
                           const std::function<tgms_status(hipStream_t)>& body) {
    tgms_handle::LoopGraph* hit = nullptr;
    for (auto& g : h->loop_graphs)
        if (g.exec && g.key == key) hit = &g;
    if (!hit) {
        if (!h->cap_stream) TGMS_HIP(h, hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
        tgms_status s = ensure_aux(h);  // no stream/event creation inside the capture
        if (s != TGMS_OK) return s;
        TGMS_HIP(h, hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
        const tgms_status r = body(h->cap_stream);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(h->cap_stream, &g);
        if (r != TGMS_OK) {
            if (g) (void)hipGraphDestroy(g);
            return r;
        }
        if (e != hipSuccess) return hip_err(h, e, "hipStreamEndCapture");
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ei != hipSuccess) return hip_err(h, ei, "hipGraphInstantiate");
        hipEvent_t done = nullptr;
        const hipError_t ee = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (ee != hipSuccess) {
            (void)hipGraphExecDestroy(exec);
            return hip_err(h, ee, "hipEventCreateWithFlags");
        }
        if (h->loop_graphs.size() >= kLoopGraphs) {
            auto lru = std::min_element(h->loop_graphs.begin(), h->loop_graphs.end(),
                                        [](const auto& a, const auto& b) { return a.used < b.used; });
            // the evicted graph may still be running (a replay on another stream, e.g. a
            // multi-GPU piece on sc[d]): wait for its last replay before destroying it
            TGMS_HIP(h, hipEventSynchronize(lru->done));
            TGMS_HIP(h, hipGraphExecDestroy(lru->exec));
            TGMS_HIP(h, hipEventDestroy(lru->done));
            h->loop_graphs.erase(lru);
        }
        h->loop_graphs.push_back({key, exec, 0, done});
        hit = &h->loop_graphs.back();
    }
    hit->used = ++h->loop_clock;
    TGMS_HIP(h, hipGraphLaunch(hit->exec, stream));
    TGMS_HIP(h, hipEventRecord(hit->done, stream));
    return TGMS_OK;
}

tgms_status check_refine_args(tgms_handle* h, double kT, double eta) {
    if (h->method != TGMS_METHOD_REDUCED)
        return set_err(h, TGMS_ERR_UNSUPPORTED, "time refinement needs the reduced method");
    if (!(kT >= 0.0) || !std::isfinite(kT) || !(eta >= 0.0) || !std::isfinite(eta))
        return set_err(h, TGMS_ERR_INVALID_ARG, "k_T and eta must be finite and >= 0");
    return TGMS_OK;
}

// The whole loop of one device's batch (or shard) as one cached graph: the plan of a
// ragged batch is computed inside it on the device, so per call the host scans the offsets
// once (validation, uniform detection) and replays.
tgms_status loop_on_device(tgms_handle* h, int32_t B, int64_t S, int uniform_m, const int32_t* d_so, const double* dW,
                           double* dT, const double* dED, double k_T, double eta, int32_t iters, double* dC,
                           double* d_cost, int32_t* dSt, hipStream_t st) {
    Plan plan;
    plan.uniform_m = uniform_m;
    // the uniform path ping-pongs through a second time buffer; the ragged one works in place
    tgms_status s = uniform_m > 0 ? ensure_loop_ws(h, align256((size_t)S * 8)) : ensure_perm_device(h, B);
    if (s != TGMS_OK) return s;
    double* T[2] = {dT, uniform_m > 0 ? h->d_loop_ws : nullptr};
    const DevPlanBufs dp{h->d_perm_hist, h->d_perm, h->d_plan};
    auto body = [&](hipStream_t q) -> tgms_status {
        int cur = 0;
        tgms_status r = refine_loop(h, plan, B, S, d_so, dW, T, dED, k_T, eta, iters, dC, d_cost, dSt, q, &cur, &dp);
        if (r != TGMS_OK) return r;
        if (cur == 1) TGMS_HIP(h, hipMemcpyAsync(dT, T[1], (size_t)S * 8, hipMemcpyDeviceToDevice, q));
        return TGMS_OK;
    };
    static const bool no_graph = std::getenv("TGMS_NO_GRAPH") != nullptr;
    if (no_graph) return body(st);
    // launch-bound (a few small kernels per step for uniform batches): capture once,
    // replay while nothing changed
    const tgms_handle::LoopKey key{B, iters, S, d_so, dW, dT, T[1], dED, dC, d_cost, dSt,
                                   uniform_m > 0 ? nullptr : h->d_perm, uniform_m > 0 ? nullptr : h->d_perm_hist,
                                   uniform_m > 0 ? nullptr : h->d_plan, k_T, eta, uniform_m};
    return run_loop_graph(h, key, st, body);
}

}  // namespace tgms::capi

using namespace tgms::capi;

extern "C" {

int tgms_abi_version(void) { return TGMS_ABI_VERSION; }

const char* tgms_status_string(int status) {
    switch (status) {
        case TGMS_OK: return "TGMS_OK";
        case TGMS_ERR_INVALID_ARG: return "TGMS_ERR_INVALID_ARG";
        case TGMS_ERR_SINGULAR: return "TGMS_ERR_SINGULAR";
        case TGMS_ERR_NONFINITE: return "TGMS_ERR_NONFINITE";
        case TGMS_ERR_NO_DEVICE: return "TGMS_ERR_NO_DEVICE";
        case TGMS_ERR_DEVICE: return "TGMS_ERR_DEVICE";
        case TGMS_ERR_UNSUPPORTED: return "TGMS_ERR_UNSUPPORTED";
        case TGMS_ERR_SKIPPED: return "TGMS_ERR_SKIPPED";
        default: return "TGMS_ERR_UNKNOWN";
    }
}

tgms_status tgms_create(tgms_handle** out, int device) {
    if (!out) return TGMS_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TGMS_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return TGMS_ERR_INVALID_ARG;
    tgms_handle* h = new tgms_handle();
    h->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->perm_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->scratch_ev, hipEventDisableTiming) != hipSuccess) {
        delete h;
        return TGMS_ERR_DEVICE;
    }
    *out = h;
    return TGMS_OK;
}

tgms_status tgms_create_host(tgms_handle** out) {
    if (!out) return TGMS_ERR_INVALID_ARG;
    tgms_handle* h = new tgms_handle();
    h->host = true;
    *out = h;
    return TGMS_OK;
}

void tgms_destroy(tgms_handle* h) {
    if (!h) return;
    if (h->host) {
        delete h;
        return;
    }
    if (h->multi) {
        destroy_multi(h->multi);
        h->multi = nullptr;
    }
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipDeviceSynchronize();
    if (h->d_ws) (void)hipFree(h->d_ws);
    if (h->d_perm_hist) (void)hipFree(h->d_perm_hist);
    if (h->d_band) (void)hipFree(h->d_band);
    if (h->d_band_graph) (void)hipFree(h->d_band_graph);
    for (double* p : h->band_retired) (void)hipFree(p);
    if (h->d_perm) (void)hipFree(h->d_perm);
    if (h->h_perm) (void)hipHostFree(h->h_perm);
    if (h->perm_ev) (void)hipEventDestroy(h->perm_ev);
    if (h->scratch_ev) (void)hipEventDestroy(h->scratch_ev);
    if (h->band_done) (void)hipHostFree(h->band_done);
    if (h->d_loop_ws) (void)hipFree(h->d_loop_ws);
    if (h->d_nbr_ws) (void)hipFree(h->d_nbr_ws);
    for (int j = 0; j < TGMS_AUX_STREAMS; ++j) {
        if (h->aux[j]) (void)hipStreamDestroy(h->aux[j]);
        if (h->join_ev[j]) (void)hipEventDestroy(h->join_ev[j]);
    }
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    for (auto& g : h->loop_graphs) {
        if (g.done) (void)hipEventSynchronize(g.done);
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.done) (void)hipEventDestroy(g.done);
    }
    if (h->d_plan) (void)hipFree(h->d_plan);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    // destroy reports nothing: leave no error of these calls behind for the caller's next
    // HIP call to pick up (hipGetLastError is per thread)
    (void)hipGetLastError();
    delete h;
}

const char* tgms_last_error(const tgms_handle* h) { return h ? h->last_error.c_str() : ""; }

tgms_status tgms_set_method(tgms_handle* h, int method) {
    if (!h) return TGMS_ERR_INVALID_ARG;
    if (method != TGMS_METHOD_REDUCED && method != TGMS_METHOD_DENSE_KKT && method != TGMS_METHOD_BAND_KKT)
        return set_err(h, TGMS_ERR_INVALID_ARG, "unknown method");
    if (h->host && method != TGMS_METHOD_REDUCED)
        return set_err(h, TGMS_ERR_UNSUPPORTED, "the host backend solves the reduced formulation only");
    h->method = method;
    if (h->multi) multi_set_method(h->multi, method);
    return TGMS_OK;
}

tgms_status tgms_solve_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                             const double* seg_times, const double* end_derivs, double* coeffs,
                             int32_t* status) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    Plan plan;
    tgms_status s = check_offsets(h, B, so, max_m_for(h), &plan.counts, &plan.uniform_m);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!waypoints || !seg_times || !coeffs)
        return set_err(h, TGMS_ERR_INVALID_ARG, "NULL waypoints/seg_times/coeffs");
    if (h->host) {  // the explicit host backend (config 1), on the calling thread
        int worst = TGMS_OK;
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            const int st = tgms::host::solve(so[b + 1] - so[b], waypoints + (s0 + b) * 3, seg_times + s0,
                                             end_derivs ? end_derivs + (int64_t)b * 18 : nullptr, coeffs + s0 * 24);
            if (status) status[b] = st;
            if (st > worst) {
                worst = st;
                h->last_error = "trajectory " + std::to_string(b) + ": " + tgms_status_string(st);
            }
        }
        return (tgms_status)worst;
    }
    const size_t S = (size_t)so[B];
    double *dW, *dT, *dED, *dC;
    int32_t *dSt, *dSo;
    s = stage(h, {input(&dW, waypoints, (S + B) * 3), input(&dT, seg_times, S), input(&dED, end_derivs, (size_t)B * 18),
                  output(&dC, S * 24), output(&dSt, (size_t)B), input(&dSo, so, (size_t)B + 1)});
    if (s != TGMS_OK) return s;
    hipStream_t st = h->stream;
    s = scratch_acquire(h, st);
    if (s != TGMS_OK) return s;
    s = plan_upload(h, B, so, &plan, st);
    if (s != TGMS_OK) return s;
    s = scratch_release(h, st, dispatch(h, plan, B, dSo, dW, dT, dED, dC, dSt, st));
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, fetch(h, coeffs, dC, S * 24));
    return finish_status(h, dSt, status, B, true);
}

tgms_status tgms_solve_uniform_device(tgms_handle* h, int32_t B, int32_t M, const double* dW,
                                      const double* dT, const double* dED, double* dC,
                                      int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (B < 0 || M < 1 || M > max_m_for(h))
        return set_err(h, M > TGMS_MAX_SEGMENTS || M < 1 || B < 0 ? TGMS_ERR_INVALID_ARG : TGMS_ERR_UNSUPPORTED,
                       "bad B or M for this method");
    if (B == 0) return TGMS_OK;
    if (!dW || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (h->method == TGMS_METHOD_BAND_KKT) {
        double* slab = nullptr;
        tgms_status s = ensure_band(h, M, st, &slab);
        if (s == TGMS_OK) s = scratch_acquire(h, st);
        if (s != TGMS_OK) {
            if (!capturing(st)) (void)scratch_release(h, st);  // ensure_band may have armed the marker
            return s;
        }
        const hipError_t e = tgms::launch_band_kkt(M, B, nullptr, nullptr, dW, dT, dED, dC, dSt, slab, h->band_grid, st);
        const tgms_status r = scratch_release(h, st);
        return e != hipSuccess ? hip_err(h, e, "launch_band_kkt") : r;
    } else if (h->method == TGMS_METHOD_REDUCED)
        TGMS_HIP(h, tgms::launch_reduced_uniform(M, B, dW, dT, dED, dC, dSt, st));
    else
        TGMS_HIP(h, tgms::launch_dense_kkt(M, B, nullptr, nullptr, dW, dT, dED, dC, dSt, st));
    return TGMS_OK;
}

tgms_status tgms_solve_batch_device(tgms_handle* h, int32_t B, const int32_t* h_so,
                                    const int32_t* d_so, const double* dW, const double* dT,
                                    const double* dED, double* dC, int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    Plan plan;
    tgms_status s = check_offsets(h, B, h_so, max_m_for(h), &plan.counts, &plan.uniform_m);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW || !dT || !dC) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC);
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = scratch_acquire(h, st);
    if (s != TGMS_OK) return s;
    s = plan_upload(h, B, h_so, &plan, st);
    if (s != TGMS_OK) return s;
    s = dispatch(h, plan, B, d_so, dW, dT, dED, dC, dSt, st);
    if (s != TGMS_OK) return s;
    return scratch_release(h, st);
}

tgms_status tgms_refine_uniform_device(tgms_handle* h, int32_t B, int32_t M, const double* dW, const double* dT,
                                       const double* dED, double k_T, double eta, double* dT_out, double* d_cost,
                                       int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    tgms_status s = check_refine_args(h, k_T, eta);
    if (s != TGMS_OK) return s;
    if (B < 0 || M < 1 || M > TGMS_MAX_SEGMENTS) return set_err(h, TGMS_ERR_INVALID_ARG, "bad B or M");
    if (B == 0) return TGMS_OK;
    if (!dW || !dT || !dT_out || dT_out == dT) return set_err(h, TGMS_ERR_INVALID_ARG, "bad device pointers");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dT_out, d_cost);
    TGMS_HIP(h, tgms::launch_refine_uniform(M, B, dW, dT, dED, k_T, eta, dT_out, d_cost, dSt,
                                            static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_refine_batch_device(tgms_handle* h, int32_t B, const int32_t* h_so, const int32_t* d_so,
                                     const double* dW, const double* dT, const double* dED, double k_T, double eta,
                                     double* dT_out, double* d_cost, int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    tgms_status s = check_refine_args(h, k_T, eta);
    if (s != TGMS_OK) return s;
    Plan plan;
    s = check_offsets(h, B, h_so, TGMS_MAX_SEGMENTS, &plan.counts, &plan.uniform_m);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW || !dT || !dT_out || dT_out == dT) return set_err(h, TGMS_ERR_INVALID_ARG, "bad device pointers");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dT_out, d_cost);
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = scratch_acquire(h, st);
    if (s != TGMS_OK) return s;
    s = plan_upload(h, B, h_so, &plan, st);
    if (s != TGMS_OK) return s;
    s = dispatch_refine(h, plan, B, d_so, dW, dT, dED, k_T, eta, dT_out, d_cost, dSt, st);
    if (s != TGMS_OK) return s;
    return scratch_release(h, st);
}

tgms_status tgms_refine_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                              double* seg_times, const double* end_derivs, double k_T, double eta, int32_t iters,
                              double* coeffs, double* cost, int32_t* status) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    tgms_status s = check_refine_args(h, k_T, eta);
    if (s != TGMS_OK) return s;
    if (iters < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "iters < 0");
    Plan plan;
    s = scan_offsets(h, B, so, TGMS_MAX_SEGMENTS, &plan.uniform_m);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!waypoints || !seg_times) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL waypoints/seg_times");
    const size_t S = (size_t)so[B];
    double *dW, *dT[2], *dED, *dC, *dCost;  // dT: the loop's two time buffers; dC: only if asked for
    int32_t *dSt, *dSo;
    s = stage(h, {input(&dW, waypoints, (S + B) * 3), input(&dT[0], seg_times, S), output(&dT[1], S),
                  input(&dED, end_derivs, (size_t)B * 18), output(&dC, coeffs ? S * 24 : 0), output(&dCost, (size_t)B),
                  output(&dSt, (size_t)B), input(&dSo, so, (size_t)B + 1)});
    if (s != TGMS_OK) return s;
    hipStream_t st = h->stream;
    s = scratch_acquire(h, st);
    if (s == TGMS_OK && plan.uniform_m == 0) s = ensure_perm_device(h, B);
    if (s != TGMS_OK) return s;
    const DevPlanBufs dp{h->d_perm_hist, h->d_perm, h->d_plan};
    int cur = 0;
    s = scratch_release(h, st, refine_loop(h, plan, B, (int64_t)S, dSo, dW, dT, dED, k_T, eta, iters, dC, dCost, dSt,
                                           st, &cur, &dp));
    if (s != TGMS_OK) return s;
    if (coeffs) TGMS_HIP(h, fetch(h, coeffs, dC, S * 24));
    TGMS_HIP(h, fetch(h, seg_times, dT[cur], S));
    if (cost) TGMS_HIP(h, fetch(h, cost, dCost, (size_t)B));
    return finish_status(h, dSt, status, B, false);  // the worst status, no message
}

tgms_status tgms_refine_loop_device(tgms_handle* h, int32_t B, const int32_t* h_so, const int32_t* d_so,
                                    const double* dW, double* dT, const double* dED, double k_T, double eta,
                                    int32_t iters, double* dC, double* d_cost, int32_t* dSt, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    tgms_status s = check_refine_args(h, k_T, eta);
    if (s != TGMS_OK) return s;
    if (iters < 0) return set_err(h, TGMS_ERR_INVALID_ARG, "iters < 0");
    int um = 0;
    s = scan_offsets(h, B, h_so, TGMS_MAX_SEGMENTS, &um);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW || !dT) return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC, d_cost);
    hipStream_t st = static_cast<hipStream_t>(stream);
    s = no_capture(h, st, "tgms_refine_loop_device (it captures and replays its own graph)");
    if (s == TGMS_OK) s = scratch_acquire(h, st);
    if (s != TGMS_OK) return s;
    return scratch_release(h, st, loop_on_device(h, B, (int64_t)h_so[B], um, d_so, dW, dT, dED, k_T, eta, iters, dC,
                                                 d_cost, dSt, st));
}

int64_t tgms_sample_count(double total_T, double dt) {
    if (!(dt > 0.0) || !(total_T >= 0.0) || !std::isfinite(total_T)) return 0;
    const double x = std::ceil(total_T / dt - 1e-9);
    int64_t n = (int64_t)x;
    if (n < 1) n = 1;
    return n + 1;
}

tgms_status tgms_sample_offsets(int32_t B, const int32_t* so, const double* T, double dt,
                                int64_t* sample_offsets) {
    if (B < 0 || !so || !sample_offsets || (B > 0 && !T) || !(dt > 0.0)) return TGMS_ERR_INVALID_ARG;
    sample_offsets[0] = 0;
    for (int32_t b = 0; b < B; ++b) {
        double tot = 0.0;
        for (int32_t i = so[b]; i < so[b + 1]; ++i) tot += T[i];
        const int64_t n = tgms_sample_count(tot, dt);
        if (n <= 0) return TGMS_ERR_INVALID_ARG;
        sample_offsets[b + 1] = sample_offsets[b] + n;
    }
    return TGMS_OK;
}

tgms_status tgms_sample_batch_device(tgms_handle* h, int32_t B, const int32_t* d_so,
                                     const double* dW, const double* dT, const double* dED,
                                     const double* dC, double dt, int yaw_mode, double yaw_const,
                                     const int64_t* d_sample_offsets, double* d_out, void* stream) {
    if (tgms_status e = enter(h, __func__); e != TGMS_OK) return e;
    if (B < 0 || !(dt > 0.0) || (yaw_mode != TGMS_YAW_CONSTANT && yaw_mode != TGMS_YAW_VELOCITY))
        return set_err(h, TGMS_ERR_INVALID_ARG, "bad B, dt or yaw_mode");
    if (B == 0) return TGMS_OK;
    if (!d_so || !dW || !dT || !dC || !d_sample_offsets || !d_out)
        return set_err(h, TGMS_ERR_INVALID_ARG, "NULL device pointer");
    TGMS_CHECK_ALIGNED(h, dW, dT, dED, dC, d_out);
    TGMS_HIP(h, tgms::launch_sample(B, d_so, dW, dT, dED, dC, dt, yaw_mode, yaw_const, d_sample_offsets,
                                    d_out, static_cast<hipStream_t>(stream)));
    return TGMS_OK;
}

tgms_status tgms_sample_batch(tgms_handle* h, int32_t B, const int32_t* so, const double* waypoints,
                              const double* seg_times, const double* end_derivs, const double* coeffs,
                              double dt, int yaw_mode, double yaw_const,
                              const int64_t* sample_offsets, double* out) {
    if (tgms_status e = enter(h); e != TGMS_OK) return e;
    tgms_status s = check_offsets(h, B, so, TGMS_MAX_SEGMENTS, nullptr, nullptr);
    if (s != TGMS_OK) return s;
    if (B == 0) return TGMS_OK;
    if (!waypoints || !seg_times || !coeffs || !sample_offsets || !out || !(dt > 0.0))
        return set_err(h, TGMS_ERR_INVALID_ARG, "NULL pointer or dt <= 0");
    if (yaw_mode != TGMS_YAW_CONSTANT && yaw_mode != TGMS_YAW_VELOCITY)
        return set_err(h, TGMS_ERR_INVALID_ARG, "bad yaw_mode");
    if (h->host) {
        for (int32_t b = 0; b < B; ++b) {
            const int64_t s0 = so[b];
            tgms::host::sample(so[b + 1] - so[b], coeffs + s0 * 24, seg_times + s0, waypoints + (s0 + b) * 3,
                               end_derivs ? end_derivs + (int64_t)b * 18 : nullptr, dt, yaw_mode, yaw_const,
                               sample_offsets[b + 1] - sample_offsets[b], out + sample_offsets[b] * TGMS_GOAL_STRIDE);
        }
        return TGMS_OK;
    }
    const size_t S = (size_t)so[B], nOut = (size_t)sample_offsets[B] * TGMS_GOAL_STRIDE;
    double *dW, *dT, *dED, *dC, *dOut;
    int32_t* dSo;
    int64_t* dSmp;
    s = stage(h, {input(&dW, waypoints, (S + B) * 3), input(&dT, seg_times, S), input(&dED, end_derivs, (size_t)B * 18),
                  input(&dC, coeffs, S * 24), input(&dSo, so, (size_t)B + 1),
                  input(&dSmp, sample_offsets, (size_t)B + 1), output(&dOut, nOut)});
    if (s != TGMS_OK) return s;
    TGMS_HIP(h, tgms::launch_sample(B, dSo, dW, dT, dED, dC, dt, yaw_mode, yaw_const, dSmp, dOut, h->stream));
    TGMS_HIP(h, fetch(h, out, dOut, nOut));
    TGMS_HIP(h, hipStreamSynchronize(h->stream));
    return TGMS_OK;
}

}  // extern "C"
