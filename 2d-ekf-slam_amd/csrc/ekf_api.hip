// ekf_api.hip -- host side of libekfslam_hip.so: the C ABI of include/ekfslam_c.h.
//
// Owns the HBM layout (ekf_device.h), one HIP stream per handle, the immediate-mode input ring
// (host-mapped pinned memory, so an API call is kernel launches only), device-resident step
// scripts and their HIP-graph replay.  There is no CPU fallback: without a gfx950 device
// ekf_create fails with EKF_ERR_NO_DEVICE.
//
// This file is the hot layer -- streaming command ring, the enqueuer of the window scheduler (issue_pass, OpsSink, close_set,
// launch_ops), the graph path -- and the accessors.  What every launch and every dense pass looks like is decided by pure code in
// ekf_window_plan.h (WindowState, plan_close, plan_ops, route_call); this file resolves its roles to streams and events and makes
// the HIP calls.  The map operations (removal, frame change, joining, extraction, consistency, duplicate search, fusion), which run once
// per call on a handle at rest, are in ekf_map_api.hip, included below where they use this file's helpers; their list checks and
// tables are pure code in ekf_map_plan.h.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <string>
#include <atomic>
#include <mutex>
#include <vector>
#include <algorithm>

#include "ekf_device.h"
#include "ekf_geometry.h"
#include "ekf_map_plan.h"
#include "ekf_map_scratch.h"
#include "ekf_window_plan.h"

// single translation unit: the kernels are compiled together with their launch sites
#include "ekf_kernels.hip"
#include "ekf_solo.hip"
#include "ekf_rewrite.hip"
#include "ekf_factor.hip"
#include "ekf_pairs.hip"
#include "ekf_fuse.hip"
#include "ekf_match.hip"
#include "ekf_match_iter.hip"
#include "ekf_fix.hip"
#include "ekf_polar.hip"
#include "ekf_extract.hip"
#include "ekf_gate.hip"
#include "ekf_locate.hip"
#include "ekf_assoc.hip"

static thread_local std::string g_last_error;

// (format_text: ekf_map_plan.h, whose checks format the same way without this file: the CPU check program includes that header alone)
__attribute__((format(printf, 2, 3))) static int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    g_last_error = format_text(fmt, ap);
    va_end(ap);
    return code;
}
static int set_error(const PlanStatus &st) { return st.code ? set_error(st.code, "%s", st.text.c_str()) : EKF_OK; }  // (a check of ekf_map_plan.h)

int ekf_set_last_error(int code, const char *what) { return set_error(code, "%s", what ? what : ""); }  // for the library's other translation units (feat_api.hip)

#define HIP_TRY(expr)                                                                                                                     \
    do {                                                                                                                                  \
        hipError_t e_ = (expr);                                                                                                           \
        if (e_ != hipSuccess) return set_error(EKF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);   \
    } while (0)

// ... and for the library's own int status chains (the callee has set the error text)
#define EKF_TRY(expr)        \
    do {                     \
        int rc_ = (expr);    \
        if (rc_) return rc_; \
    } while (0)

// A transient device allocation that frees itself, so that HIP_TRY / EKF_TRY may return past it.
template <typename T>
struct DevTmp {
    T *p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() {
        if (p) hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
    // ... of at least one element, filled with `count` of the host's: on stream s, or (async = false) by a synchronous copy
    hipError_t upload(const T *src, size_t count, hipStream_t s, bool async = true) {
        const hipError_t e = alloc(count > 0 ? count : 1);
        if (e != hipSuccess || count == 0) return e;
        return async ? hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s) : hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
};

// Asynchronous copies between the device and pageable host memory -- a local std::vector, a caller's buffer -- on one stream.  Every
// enqueue goes through the guard and arms it; wait() is stream_wait and disarms; a return with a copy still in flight (HIP_TRY /
// EKF_TRY past a later failure) waits for the stream in the destructor, before the buffers go.  Declare it BEHIND the buffers it
// guards.  A success path pays nothing: it ends disarmed, by wait() or, where something else has waited for the stream, by waited().
static hipError_t stream_wait(hipStream_t s);
struct HostCopies {
    hipStream_t s;
    bool armed = false;
    explicit HostCopies(hipStream_t stream) : s(stream) {}
    HostCopies(const HostCopies &) = delete;
    HostCopies &operator=(const HostCopies &) = delete;
    ~HostCopies() {
        if (armed) (void)hipStreamSynchronize(s);
    }
    hipError_t copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        armed = true;
        return hipMemcpyAsync(dst, src, bytes, kind, s);
    }
    hipError_t copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind) {
        armed = true;
        return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, s);
    }
    template <typename T>
    hipError_t upload(DevTmp<T> *tmp, const T *src, size_t count) {
        armed = true;
        return tmp->upload(src, count, s);
    }
    hipError_t wait() {
        const hipError_t e = stream_wait(s);
        armed = false;
        return e;
    }
    void waited() { armed = false; }  // the stream has been waited for behind the last enqueue (finish_rewrite, read_back_dense)
};

// Device scratch that a handle keeps from the first call of an operation on (ekf_map_api.hip), counted in ekf_device_bytes while it
// lives: block_alloc; ekf_destroy releases every block, ekf_reserve has those that existed built again.
struct DevBlock {
    void *p = nullptr;
    size_t bytes = 0;
};
enum { BLK_FACTOR, BLK_DUP, BLK_DUP_LIST, BLK_FUSE, BLK_MATCH, BLK_ITER, BLK_GATE, BLK_GATE_LIST, BLK_ASSOC, BLK_ADD, BLK_LOC, BLK_LOC_LIST, BLK_COUNT };

// Everything the map operations keep on a handle: the scratch structs their kernels take (ekf_map_scratch.h: arrays and layout) and
// the allocations behind them.  A block is built by the first call that needs it (block_build in ekf_map_api.hip) and kept.
//
//   block          struct  built by the first                          follows                               zeroed
//   BLK_FACTOR     fac     ekf_joint_consistency                       the capacity                          yes
//   BLK_DUP        dup     ekf_find_duplicates                         the capacity                          yes
//   BLK_DUP_LIST   dup     ekf_find_duplicates                         the pairs asked for or found (cap,    no
//                                                                      from 256)
//   BLK_FUSE       fuse    ekf_fuse_landmarks, ekf_update_matched,     the capacity                          yes
//                          ekf_update_fixes
//   BLK_MATCH      match   ekf_update_matched, ekf_joint_compat,       the longest list brought (zcap,       yes
//                          ekf_associate_joint that searches,          from 64)
//                          ekf_update_fixes, ekf_fix_compat
//   BLK_ITER       iter    ekf_update_matched_iter                     the longest list brought (zcap,       yes
//                                                                      from 64)
//   BLK_GATE       gate    ekf_gate_candidates with a valid entry      the longest scan brought (zcap, from  yes
//                                                                      64) and the capacity (npart)
//   BLK_GATE_LIST  gate    ekf_gate_candidates that hands pairs out,   the pairs asked for or found (ccap,   no
//                          ekf_associate_joint                         from 256)
//   BLK_ASSOC      assoc   ekf_associate_joint that searches           the batch alone                       yes
//   BLK_ADD        add     ekf_add_landmarks that adds                 the longest list brought (zcap,       yes
//                                                                      from 64)
//   BLK_LOC        loc     ekf_locate_scan that searches               the batch alone                       yes
//   BLK_LOC_LIST   loc     ekf_locate_scan that searches               the candidates found (ccap, from      no
//                                                                      4096)
// A capacity that a call outgrows is doubled until it fits (plan_grown_cap) and the block replaced.
// ekf_reserve (map_scratch_rebuild) builds again, for the new capacity and as large as it was, every block the old buffers had --
// with one irregularity: BLK_DUP and BLK_DUP_LIST are built together, when the old handle had the LIST (a base whose list never
// got allocated is not rebuilt); BLK_GATE_LIST follows BLK_GATE's presence with the old ccap (0: no list); BLK_LOC and BLK_LOC_LIST
// are built together by every call, with the old ccap.
struct MapKept {
    FactorScratch fac = {};
    DupScratch dup = {};
    FuseScratch fuse = {};
    MatchScratch match = {};
    IterScratch iter = {};
    GateScratch gate = {};
    AssocScratch assoc = {};
    AddScratch add = {};
    LocScratch loc = {};
    DevBlock blk[BLK_COUNT];
};

struct GraphEntry {
    int steps, M, has_truth;
    hipGraphExec_t exec;
};

struct ekf_batch {
    EkfDev dv;
    ekf_params params;
    int device;
    hipStream_t s_chain;  // chain kernels (and, without overlap, the dense passes too)
    hipStream_t s_flush;  // overlap: the dense passes; == s_chain otherwise
    bool overlap;         // a window's dense pass runs beside the next window's chain kernels (two slot sets, two Bm buffers)
    hipEvent_t ev_chain, ev_flush[2];
    hipEvent_t prof_stop[2] = {nullptr, nullptr};  // EV_PROFi: the stop event of the profiling pair that the pass of slot i took
    WindowCfg wcfg;       // what the window scheduler (ekf_window_plan.h) knows of this handle: read_debug_hooks fills it
    WindowState win;      // which window is open and what it waits for
    bool inkernel_wait;   // chain kernels wait for their pass in-kernel (kernels of two streams run side by side), else by event
    long long chain_seq;  // chain launches so far; the kernel stores it into the host mirror when it is done
    int ncu = 0;                            // CUs of the device
    bool persist = true;                    // scripted runs in overlap mode: one chain launch for several windows (EKF_PERSIST=0 switches it off)
    bool stats_in_mirror = false;  // mirror.stats is current (a chain launch ran since the last ekf_reset_stats)
    bool mirror_by_chain; // the newest writer of the host mirror is chain launch number chain_seq (else: some other kernel, synchronise)
    int flush_keep;       // pool key of s_flush: CUs kept free for the chain, -1 = unmasked
    bool solo = false;    // one workgroup per filter and one slot set (phase groups are possible)
    bool solo_fuse = false;    // ... and k_solo folds the windows it fills itself (ChainSeg::self_pass; EKF_SOLO_FUSE=0: k_flush_rb launches between the windows)
    long long prof_fused_passes = 0;  // dense passes executed inside profiled k_solo launches since the last ekf_flush_profile_read
    long long prof_solo_pairs = 0;    // ... and the number of those launches (event pairs that bracket a k_solo launch, not a k_flush_rb)
    bool solo_long = false;    // ... with a window longer than its own-row cache (k_solo<true>: the first half in accumulation registers)
    bool solo_kernel = false;  // ... run by k_solo (ekf_solo.hip: maps of up to 256 landmarks, one landmark per thread, one barrier per measurement)
    // Phase groups (solo batches): the filters are cut into ngroups ranges, each with a stream of its own on which its chain
    // launches and its dense passes alternate; the groups run out of phase, so that at any moment some groups are in their
    // (latency-bound) chain kernels while another streams its pass through HBM.  s_grp[0] == s_chain.
    int ngroups = 1;
    std::vector<hipStream_t> s_grp;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;  // (tn.solo_stagger_ticks: the phase shift between consecutive groups at the start of a grouped run)
    int chain_wgs;       // k_chain workgroups per filter
    int chain_filters;    // filters per k_chain launch (all of the batch when its workgroups are resident together)
    int claimed_cus;      // CUs this handle's chain workgroups occupy when they run (residency registry, below)
    int solo_cus = 0;     // one-workgroup handles: CUs their launches occupy while they run (they claim none: g_cus_solo)
    bool flush_masked;    // s_flush is a dedicated CU-masked queue
    size_t chain_lds;     // dynamic LDS of a k_chain launch: the own-row cache
    bool chain_one = false;  // k_chain<true>: several workgroups per filter, at most one landmark per worker thread (EKF_CHAIN_ONE=0: the general kernel)
    double *bm1_base;     // allocation behind dv.Bm[1] (overlap mode)
    std::vector<int *> tile_maps;  // [nT]: XCD-aware wave -> tile tables of the row-block dense pass, built on demand (tn.xcd_map)
    size_t device_bytes;
    int chain_threads;
    // host-side tracking
    int n_lm_hi;    // upper bound on max_b n_lm[b]
    // Product tunables and experiment variables (read from the environment at ekf_*_create by read_tunables, listed in
    // include/ekfslam_c.h "Tunables" and INTEGRATION.md; every one of them changes scheduling only, never results) -- bench.py
    // records every EKF_* variable it saw.
    Tunables tn;
    // Test / experiment hooks.  They exist only in the debug variant of the library (make debug: -DEKF_DEBUG_HOOKS,
    // libekfslam_hip_debug.so); in the product build the fields keep these values and no environment variable can change them.
    bool dbg_skip_flush = false;        // EKF_DEBUG_SKIP_FLUSH=1: timing experiments only, results are wrong
    int dbg_drop_marks_from = 0;        // EKF_DEBUG_DROP_MARKS_FROM=k (and ..._TO=m, exclusive): dense passes k .. m-1 never report completion (tests of the bounded waits)
    int dbg_drop_marks_to = 0x7fffffff;
    long dbg_stream_idle_ticks = 0;     // EKF_DEBUG_STREAM_IDLE_TICKS=t: a streaming launch leaves by itself after t ticks of the 100 MHz clock without a command (default 10 000)
    bool dbg_stream_no_recheck = false; // EKF_DEBUG_STREAM_NO_RECHECK=1: ... and WITHOUT looking at the command slot once more: commands get lost on purpose (tests of the host's safety net)
    // streaming immediate-mode calls (one-filter handles run by k_chain<true>; EKF_STREAM=0 switches them off): a resident launch consumes
    // the calls' operations from a host-mapped command ring (ekf_device.h: StreamCtl)
    StreamCtl *sctl_h = nullptr;  // host view of dv.sctl
    StreamCtl *sring_h = nullptr; // host view of dv.sring: sctl_h, or the device allocation itself (written through the BAR; never read by the host)
    bool sring_in_hbm = false;
    bool stream_calls = false;    // the handle streams its immediate-mode calls
    bool stream_alive = false;    // a streaming launch has been started and not been told (or seen) to leave
    int stream_launch = 0;        // number of the newest streaming launch (ChainPlan::stream)
    long long stream_starts = 0, stream_ops = 0;  // (diagnostics: ekf_debug_stream)
    long long stream_last_seq = 0;  // sequence number of the newest streamed command
    int stream_slot_before[EKF_STREAM_RING] = {};  // slots of the open window filled BEFORE streamed command seq (index seq % ring): where a replacement launch resumes
    // immediate-mode input ring (host-mapped pinned)
    double *ring_h;
    double *ring_d;
    int ring_ops;  // records in the ring; a record is B*8 doubles
    int ring_pos;
    hipEvent_t ring_ev[2];
    bool ring_ev_valid[2];
    // script
    double *script_d;
    int *cursor_d;
    int script_steps, script_M, script_has_truth;
    std::vector<GraphEntry> graphs;
    // timing
    hipEvent_t t0, t1;
    bool prof_flush;
    std::vector<hipEvent_t> prof_pool;
    size_t prof_used;
    long long prof_launches;
    double prof_ms;
    EkfMirror *mirror_h;  // host view of dv.mirror
    ekf_params params_requested;
    // scratch
    std::vector<int> h_int;
    MapKept map;  // the map operations' kept scratch
    long long state_edits = 0;     // rewrites, broadcasts and scripted runs so far: with chain_seq and stream_ops, "has the state changed?"
    long long fac_stamp[3] = {-1, -1, -1};  // those three when map.fac was last filled (ekf_debug_joint_factor)
    int fac_b0 = 0;                // ... by a call over filters [fac_b0, fac_b0 + fac_n.size()) with fac_n landmarks each
    std::vector<int> fac_n;
};

static int sticky_status(ekf_batch *h, bool include_capacity);
static int stream_stop(ekf_batch *h);
static bool filter_ok(const ekf_batch *h, int index) { return h && index >= 0 && index < h->dv.B; }  // a handle and one of its filters

extern "C" const char *ekf_last_error(void) { return g_last_error.c_str(); }

extern "C" void ekf_default_params(ekf_params *p) {
    if (!p) return;
    p->sigma_v = 0.01;
    p->sigma_w = 0.04;
    p->gamma_max = 50.0;
    p->gamma_min = 10.0;
    p->cond_limit = 80.0;
    p->max_pending = 16;
    p->log_capacity = 4096;
    p->overlap = -1;
}

// ---- the environment ----------------------------------------------------------------------------------------------------------
// Read here and nowhere else: once per process (process_tunables), at every ekf_*_create (read_tunables, into the handle's
// Tunables) and, in the debug variant, at create and ekf_set_state (read_debug_hooks, below).
static EnvInt env_int(const char *name) {
    EnvInt e;
    if (const char *s = getenv(name)) e.set = true, e.v = atoi(s);
    return e;
}

struct ProcessTunables {
    bool trace;       // EKF_TRACE=1: progress marks of handle creation / destruction on stderr (diagnostic)
    bool inline_rec;  // EKF_INLINE_REC=0: an immediate-mode call's record always travels through the ring
};
static const ProcessTunables &process_tunables() {
    static const ProcessTunables t = {env_int("EKF_TRACE").v != 0, env_int("EKF_INLINE_REC").flag(true)};
    return t;
}
static bool trace_on() { return process_tunables().trace; }

static Tunables read_tunables() {
    Tunables t;
    t.overlap = env_int("EKF_OVERLAP");
    t.solo = env_int("EKF_SOLO");
    t.chain_wgs = env_int("EKF_CHAIN_WGS");
    t.solo_long_window = env_int("EKF_SOLO_LONG_WINDOW");
    t.solo_fuse = env_int("EKF_SOLO_FUSE");
    t.chain_one = env_int("EKF_CHAIN_ONE");
    t.chain_helpers = env_int("EKF_CHAIN_HELPERS");
    t.solo_stagger_ticks = env_int("EKF_SOLO_STAGGER_US").set ? env_int("EKF_SOLO_STAGGER_US").v * 100 : 3500;
    t.bm_skew_bytes = getenv("EKF_BM_SKEW") ? atol(getenv("EKF_BM_SKEW")) : 4096;
    t.stream_ring_host = env_int("EKF_STREAM_RING_HOST").flag(false);
    t.balanced_tail = env_int("EKF_BALANCED_TAIL").flag(true);
    t.chain_cus = env_int("EKF_CHAIN_CUS");
    t.inkernel_wait = env_int("EKF_INKERNEL_WAIT").flag(true);
    t.solo_groups = env_int("EKF_SOLO_GROUPS").or_else(1);
    t.flush_alternate = env_int("EKF_FLUSH_ALTERNATE").flag(true);
    t.persist = env_int("EKF_PERSIST").flag(true);
    t.stream = env_int("EKF_STREAM").flag(true);
    t.xcd_map = env_int("EKF_XCD_MAP").flag(true);
    t.batch_interleave = env_int("EKF_BATCH_INTERLEAVE").flag(true);
    t.overlap_serial = getenv("EKF_OVERLAP_SERIAL") != nullptr;
    t.solo_fuse_stagger_ticks = env_int("EKF_SOLO_FUSE_STAGGER_US").v * 100;
    t.inline_rec = process_tunables().inline_rec;
    return t;
}
#define TRACE(msg)                                          \
    do {                                                    \
        if (trace_on()) {                                   \
            fprintf(stderr, "[ekf] %s\n", msg);             \
            fflush(stderr);                                 \
        }                                                   \
    } while (0)

// Streams are recycled through a process-wide pool and never destroyed: hipStreamCreateWithFlags and
// hipExtStreamCreateWithCUMask were seen to block forever once in a few thousand create/destroy cycles (ROCm 7.2;
// scripts/stress_create.py), which a test suite that opens hundreds of handles does reach.  A handle takes an
// idle stream of the right kind (device, CUs kept free: -1 = unmasked) or creates one; ekf_destroy returns it
// after synchronising.
// The price, and a known limit: the pool only grows.  pool_take matches (device, keep) exactly, so the process keeps one CU-masked
// stream per `keep` value and per handle of that value that was ever open AT THE SAME TIME, and the runtime gives every masked stream
// a hardware queue of its own (unmasked ones share GPU_MAX_HW_QUEUES).  OPEN: a 256-filter overlap-mode handle (256 chain workgroups
// that wait in-kernel for a dense pass which only runs on CUs without a chain workgroup, residency_ok) has run out its bounded wait
// (EKF_ERR_TIMEOUT) when it was created late in a process that had opened many handles -- behind test modules with four handles open
// at once, behind the ekf_gate_candidates tests with two, and behind the ekf_add_landmarks tests with two (window 16 of the 256-filter
// test that time, window 32 before; that test passes when its module is collected first or runs alone, on this and on the previous
// commit's library).  Neither call can hold anything back itself: gate_impl and add_impl enqueue on s_chain alone, wait for it before
// they return, and create no stream, event or queue; what those test modules share is dozens of handles opened and closed in both
// pipeline modes ahead of the 256-filter one, i.e. the pool's contents.  The cause is not found; that the pool's state (how many queues, which
// stream the handle is given) decides whether the pass reaches the CUs ahead of the spinning launch is a supposition.
// INTEGRATION.md §3.
struct PooledStream {
    int device, keep;
    hipStream_t s;
};
static std::mutex g_pool_mu;
static std::vector<PooledStream> g_pool;

static bool pool_take(int device, int keep, hipStream_t *out) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); i++)
        if (g_pool[i].device == device && g_pool[i].keep == keep) {
            *out = g_pool[i].s;
            g_pool.erase(g_pool.begin() + i);
            return true;
        }
    return false;
}

// Idle streams are destroyed when the process exits, before the HIP runtime's own teardown (atexit handlers run in
// reverse order of registration, and the runtime was loaded first): streams left alive crashed rocprofv3's finalisation.
static void pool_drain() {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto &p : g_pool) {
        if (hipSetDevice(p.device) == hipSuccess) hipStreamDestroy(p.s);
    }
    g_pool.clear();
}

static void pool_give(int device, int keep, hipStream_t s) {
    static bool registered = false;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!registered) {
        atexit(pool_drain);
        registered = true;
    }
    g_pool.push_back({device, keep, s});
}

// Do kernels on two streams of this process really run side by side?  The overlapped pipeline lets a chain kernel wait
// IN-KERNEL for the dense pass it depends on (cheaper than a cross-stream event by 6 us per window), which is only safe
// when that pass can run while the chain kernel spins.  Tools that serialise kernel execution (rocprofv3 --pmc) break
// the assumption; then the pipeline keeps the event.  Probed once per process and device.
static int concurrent_kernels_ok(int device, hipStream_t a, hipStream_t b) {
    static std::mutex mu;
    static std::vector<int> cache(64, -1);
    std::lock_guard<std::mutex> lk(mu);
    if (device >= 0 && device < (int)cache.size() && cache[device] >= 0) return cache[device];
    int h[2] = {0, 0}, ok = 0;
    {
        DevTmp<int> d;
        if (d.alloc(2) == hipSuccess && hipMemset(d.p, 0, 2 * sizeof(int)) == hipSuccess) {
            hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(64), 0, a, d.p, d.p + 1);
            hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(64), 0, b, d.p);
            if (hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess &&
                hipMemcpy(h, d.p, 2 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
                ok = h[1] == 1;
        }
    }
    (void)hipGetLastError();
    if (device >= 0 && device < (int)cache.size()) cache[device] = ok;
    return ok;
}

static hipError_t dev_alloc_zero_bytes(void **p, size_t count, size_t elem, size_t *total, hipStream_t s) {
    size_t bytes = count * elem;
    if (bytes == 0) bytes = elem;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return e;
    *total += bytes;
    return hipMemsetAsync(*p, 0, bytes, s);
}
template <typename T>
static hipError_t dev_alloc_zero(T **p, size_t count, size_t *total, hipStream_t s) {
    return dev_alloc_zero_bytes((void **)p, count, sizeof(T), total, s);
}

// Residency registry.  The workgroups of a filter's chain kernel exchange their arg-min candidates while they run, so all
// of them must be resident at once; a workgroup that cannot be placed until another one exits would leave the others
// polling until their bound runs out (EKF_ERR_TIMEOUT).  Every live handle therefore claims the CUs its chain launch needs
// (workgroups / workgroups-per-CU from the occupancy query), and a handle that does not fit beside the live ones is
// refused at creation.  Per process and device; other processes on the GPU are out of sight.
static std::mutex g_res_mu;
static int g_cus_claimed[64];
// CUs the launches of one-workgroup ("solo") handles occupy while they run.  Those handles wait for nobody, so they need no
// co-residency and claim nothing above -- but a 256-filter k_solo launch does fill the GPU, and a multi-segment chain launch of
// ANOTHER handle, whose gated dense passes need free CUs, must know (launch_ops: persist).
static int g_cus_solo[64];

// ---- the device arrays of a handle, named once ----------------------------------------------------------------------------------
// Allocation (create_impl), release (ekf_destroy), "clear filter b" (ekf_set_state) and "copy filter 0 to filter b"
// (ekf_broadcast_state) walk this table; a new buffer is one more row.  Not in it, and handled where they are used: Bm[1] (an alias
// of Bm[0] in place; in overlap mode an allocation of its own behind a skewed base, bm1_base, cleared with Bm[0] and zeroed by a
// broadcast), the tile maps, a loaded script and the host-mapped blocks.
enum : unsigned { AR_CLEAR = 1, AR_COPY = 2 };  // ekf_set_state clears the filter's part; ekf_broadcast_state copies filter 0's
struct DevArray {
    void **slot;    // the pointer in EkfDev (or the handle)
    size_t elem;    // bytes per element
    size_t stride;  // elements per filter; 0: one array per handle
    size_t tail;    // elements behind the per-filter part
    unsigned ops;
    size_t count(int B) const { return (size_t)B * stride + tail; }
    size_t filter_bytes() const { return stride * elem; }
    char *at(size_t b) const { return (char *)*slot + b * stride * elem; }
};
static std::vector<DevArray> device_arrays(ekf_batch *h) {
    EkfDev &dv = h->dv;
#define EKF_ARRAY(ptr, stride, tail, ops) DevArray{(void **)&(ptr), sizeof(*(ptr)), (size_t)(stride), (size_t)(tail), ops}
#ifdef EKF_CHAIN_STAMPS
    const size_t dbg_words = 32 + 65 * 2048;  // + publish times of every workgroup, 2048 exchanges (scripts/history/r04_skew.py)
#else
    const size_t dbg_words = 32;
#endif
    return {
        EKF_ARRAY(dv.x, dv.xs, 0, AR_CLEAR | AR_COPY),
        EKF_ARRAY(dv.R, 3 * dv.xs, 0, AR_CLEAR | AR_COPY),
        EKF_ARRAY(dv.D, 3 * dv.dn, 0, AR_CLEAR | AR_COPY),
        EKF_ARRAY(dv.Bm[0], dv.bm_stride, 0, AR_CLEAR | AR_COPY),  // (a broadcast copies Bm[buf_in]: the settled buffer)
        EKF_ARRAY(dv.FA, 2 * dv.f_stride, 0, AR_CLEAR | AR_COPY),
        EKF_ARRAY(dv.FB, 2 * dv.f_stride, 0, AR_CLEAR | AR_COPY),
        EKF_ARRAY(dv.slot_active, 2 * dv.maxp, EKF_MAX_PENDING, AR_COPY),  // (+ EKF_MAX_PENDING: k_flush_rb reads that many entries of a row unconditionally)
        EKF_ARRAY(dv.n_lm, 1, 0, AR_COPY),
        EKF_ARRAY(dv.n_lm_sweep, 1, 0, AR_COPY),
        EKF_ARRAY(dv.n_lm_flush, 2, 0, AR_COPY),
        EKF_ARRAY(dv.status, 1, 0, AR_COPY),
        EKF_ARRAY(dv.slot_meta, 2 * dv.maxp, 0, 0),
        EKF_ARRAY(dv.pass_flag, 0, 1, 0),
        EKF_ARRAY(dv.seg_count, 0, EKF_PLAN_MAX, 0),
        EKF_ARRAY(dv.bar, 2, 0, 0),
        EKF_ARRAY(dv.dbg, 0, dbg_words, 0),
        EKF_ARRAY(dv.part, 2 * dv.nrec * EKF_REC_DOUBLES, 0, 0),
        EKF_ARRAY(dv.log, dv.logcap, 0, 0),
        EKF_ARRAY(dv.log_count, 1, 0, AR_COPY),
        EKF_ARRAY(dv.stats, 1, 0, 0),
        EKF_ARRAY(h->cursor_d, 0, 1, 0),
        EKF_ARRAY(dv.sfw, 0, 40, 0),
    };
#undef EKF_ARRAY
}

// ---- one launcher per kernel family ---------------------------------------------------------------------------------------------
// The chain kernel of a handle: k_solo<LONG, STREAM> for one-workgroup maps of up to 256 landmarks, k_chain<ONE, STREAM> otherwise.
// The only place that names an instantiation.
typedef void (*ChainKernel)(EkfDev, const double *, const int *, ChainPlan, int);
static ChainKernel chain_kernel(bool solo_kernel, bool long_or_one, bool streaming) {
    static const ChainKernel table[2][2][2] = {{{k_chain<false, false>, k_chain<false, true>}, {k_chain<true, false>, k_chain<true, true>}},
                                               {{k_solo<false, false>, k_solo<false, true>}, {k_solo<true, false>, k_solo<true, true>}}};
    return table[solo_kernel][long_or_one][streaming];
}
static ChainKernel chain_kernel(const ekf_batch *h, bool streaming) {
    return chain_kernel(h->solo_kernel, h->solo_kernel ? h->solo_long : h->chain_one, streaming);
}

// One chain launch over filters [b0, b0 + nb) on stream s.  on_packet: the hipExt form, whose start / stop events (either may be null)
// ride on the dispatch packet itself; else the plain form.
static void launch_chain(const ekf_batch *h, hipStream_t s, bool streaming, bool on_packet, hipEvent_t ev0, hipEvent_t ev1, const double *in, const int *cursor,
                         const ChainPlan &plan, int b0, int nb) {
    const ChainKernel k = chain_kernel(h, streaming);
    const dim3 grid(h->chain_wgs, nb), block(h->chain_threads);
    if (on_packet) hipExtLaunchKernelGGL(k, grid, block, h->chain_lds, s, ev0, ev1, 0, h->dv, in, cursor, plan, b0);
    else hipLaunchKernelGGL(k, grid, block, h->chain_lds, s, h->dv, in, cursor, plan, b0);
}

// One dense pass (k_flush_rb) over nslots slots of slot set `set` of filters [b0, b0 + nb), Bm[fin] -> Bm[fout], on stream s; e0 / e1
// ride on the dispatch packet (no extra barrier packets).  interleave: a filter's workgroups on one XCD (batches); else tmap, if any.
static void launch_pass(const EkfDev &dv, hipStream_t s, hipEvent_t e0, hipEvent_t e1, bool interleave, int nT_hi, int set, int nslots, int fin, int fout,
                        const int *tmap, int rev, int b0, int nb) {
    const int nwg = (nT_hi * (nT_hi + 1) / 2 + 3) / 4;
    if (interleave)
        hipExtLaunchKernelGGL(k_flush_rb, dim3((unsigned)((nb + 7) / 8 * 8 * nwg), 1), dim3(256), 0, s, e0, e1, 0, dv, nT_hi, set, nslots, fin, fout, (const int *)nullptr, nwg, rev, b0, nb);
    else
        hipExtLaunchKernelGGL(k_flush_rb, dim3(nwg, nb), dim3(256), 0, s, e0, e1, 0, dv, nT_hi, set, nslots, fin, fout, tmap, 0, rev, b0, nb);
}

static int create_impl(ekf_batch *h, int batch, int capacity_landmarks, int device_id, const ekf_params *params, const hipDeviceProp_t &prop);

// The debug variant reads its hooks when a handle is created and again at ekf_set_state (a test switches them off between the
// two); the product build reads none.
static void read_debug_hooks(ekf_batch *h) {
#ifdef EKF_DEBUG_HOOKS
    h->dv.spin_limit = getenv("EKF_DEBUG_SPIN_LIMIT") ? atoll(getenv("EKF_DEBUG_SPIN_LIMIT")) : (1LL << 24);
    h->dbg_skip_flush = getenv("EKF_DEBUG_SKIP_FLUSH") && atoi(getenv("EKF_DEBUG_SKIP_FLUSH")) != 0;
    h->dbg_drop_marks_from = getenv("EKF_DEBUG_DROP_MARKS_FROM") ? atoi(getenv("EKF_DEBUG_DROP_MARKS_FROM")) : 0;
    h->dbg_drop_marks_to = getenv("EKF_DEBUG_DROP_MARKS_TO") ? atoi(getenv("EKF_DEBUG_DROP_MARKS_TO")) : 0x7fffffff;
    h->dbg_stream_idle_ticks = getenv("EKF_DEBUG_STREAM_IDLE_TICKS") ? atol(getenv("EKF_DEBUG_STREAM_IDLE_TICKS")) : 0;
    h->dbg_stream_no_recheck = getenv("EKF_DEBUG_STREAM_NO_RECHECK") && atoi(getenv("EKF_DEBUG_STREAM_NO_RECHECK")) != 0;
#endif
    // ... and the window scheduler's view of the handle (ekf_window_plan.h) is written here, once the geometry, the streams and the hooks are known
    WindowCfg &c = h->wcfg;
    const Tunables &tn = h->tn;
    c.B = h->dv.B, c.maxp = h->dv.maxp, c.overlap = h->overlap, c.inkernel_wait = h->inkernel_wait, c.chain_wgs = h->chain_wgs, c.chain_filters = h->chain_filters;
    c.solo = h->solo, c.solo_kernel = h->solo_kernel, c.solo_fuse = h->solo_fuse, c.ngroups = h->ngroups, c.persist = h->persist;
    c.balanced_tail = tn.balanced_tail, c.flush_alternate = tn.flush_alternate, c.batch_interleave = tn.batch_interleave, c.overlap_serial = tn.overlap_serial;
    c.xcd_map = tn.xcd_map, c.inline_rec = tn.inline_rec, c.solo_fuse_stagger_ticks = tn.solo_fuse_stagger_ticks;
    c.dbg_skip_flush = h->dbg_skip_flush, c.dbg_drop_marks_from = h->dbg_drop_marks_from, c.dbg_drop_marks_to = h->dbg_drop_marks_to;
}

extern "C" int ekf_destroy(ekf_handle h);

extern "C" int ekf_batch_create(ekf_handle *out, int batch, int capacity_landmarks, int device_id, const ekf_params *params) {
    if (!out || batch < 1 || capacity_landmarks < 1 || capacity_landmarks > EKF_MAX_CAPACITY) return set_error(EKF_ERR_BAD_ARG, "bad batch/capacity");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(EKF_ERR_NO_DEVICE, "no HIP device: libekfslam_hip has no CPU fallback");
    if (device_id < 0 || device_id >= ndev || device_id >= 64) return set_error(EKF_ERR_BAD_ARG, "bad device_id");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        return set_error(EKF_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code objects only", device_id, prop.gcnArchName);
    }
    HIP_TRY(hipSetDevice(device_id));
    ekf_batch *h = new ekf_batch();  // value-initialised: every pointer null, every count zero
    h->device = device_id;
    int rc = create_impl(h, batch, capacity_landmarks, device_id, params, prop);
    if (rc != EKF_OK) {
        std::string keep = g_last_error;
        ekf_destroy(h);  // frees whatever was allocated before the failure (tolerates the null members)
        (void)hipGetLastError();
        g_last_error = keep;
        return rc;
    }
    *out = h;
    return EKF_OK;
}

static int create_impl(ekf_batch *h, int batch, int capacity_landmarks, int device_id, const ekf_params *params, const hipDeviceProp_t &prop) {
    ekf_default_params(&h->params);
    if (params) h->params = *params;
    h->params_requested = h->params;  // (ekf_reserve builds the larger handle from what the caller asked for, not from what this capacity allowed)
    if (h->params.log_capacity < 16) h->params.log_capacity = 16;

    // ---- tunables -> geometry (ekf_geometry.h: the whole decision, checked on the CPU) ----
    h->tn = read_tunables();
    const Tunables &tn = h->tn;
    const ChainGeometry geo = plan_geometry(batch, capacity_landmarks, h->params, prop.sharedMemPerBlock, tn);
    if (geo.error) return set_error(geo.error, "%s", geo.what);
    h->params.max_pending = geo.max_pending;  // the effective window, see ekf_window()
    h->params.overlap = geo.overlap ? 1 : 0;
    h->overlap = geo.overlap;
    h->solo = geo.solo, h->solo_kernel = geo.solo_kernel, h->solo_long = geo.solo_long, h->solo_fuse = geo.solo_fuse;
    h->chain_wgs = geo.chain_wgs, h->chain_filters = geo.chain_filters, h->chain_threads = geo.chain_threads;
    h->chain_lds = geo.chain_lds, h->chain_one = geo.chain_one;
    EkfDev &dv = h->dv;
    memset(&dv, 0, sizeof dv);
    dv.B = batch;
    dv.Ncap = capacity_landmarks;
    dv.T = geo.T, dv.xs = geo.xs, dv.dn = geo.dn, dv.rows = geo.rows, dv.bm_stride = geo.bm_stride;
    dv.maxp = geo.max_pending, dv.maxpairs = geo.maxpairs, dv.f_stride = geo.f_stride, dv.vs_cap = geo.cache_slots;
    dv.gmax = geo.chain_wgs, dv.lpw = geo.lpw, dv.hpw = geo.hpw, dv.nrec = geo.nrec;
    dv.logcap = h->params.log_capacity;
    dv.gamma_max = h->params.gamma_max;
    dv.gamma_min = h->params.gamma_min;
    dv.spin_limit = 1LL << 24;
    dv.cond_limit = h->params.cond_limit;
    {
        // cond >= L  <=>  q r >= kappa (q^2 + r^2); kappa = 1/2 - 1/(L^2 + 1) (-> 1/2 for L = inf: only q = r is skipped).
        // L <= 1: every finite S is skipped (cond >= 1 always): kappa = 0.  NaN stays NaN: nothing is skipped.
        const long double L = h->params.cond_limit;
        long double kappa = L <= 1.0L ? 0.0L : 0.5L - 1.0L / (L * L + 1.0L);
        dv.cond_k2 = (double)(kappa * kappa);
    }

    // ---- residency claim ----
    for (int k = 0; k < 8; k++)  // one setting for every handle and every chain kernel
        HIP_TRY(hipFuncSetAttribute((const void *)chain_kernel((k & 4) != 0, (k & 2) != 0, (k & 1) != 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)chain_lds_budget(prop.sharedMemPerBlock)));
    {
        const int G = h->chain_wgs;
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)chain_kernel(h, false), h->chain_threads, h->chain_lds));
        if (per_cu < 1) return set_error(EKF_ERR_STATE, "the chain kernel does not fit a CU with this capacity / window");
        // (one-workgroup filters wait for nobody: they need no co-residency and claim nothing)
        const int need = h->solo ? 0 : (G * h->chain_filters + per_cu - 1) / per_cu;
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (g_cus_claimed[device_id] + need > prop.multiProcessorCount)
            return set_error(EKF_ERR_STATE, "this handle's %d chain workgroups need %d CUs, %d of %d are claimed by live handles: they could not all be resident at once",
                             G * h->chain_filters, need, g_cus_claimed[device_id], prop.multiProcessorCount);
        g_cus_claimed[device_id] += need;
        h->claimed_cus = need;
        h->solo_cus = h->solo ? (h->chain_filters + per_cu - 1) / per_cu : 0;
        if (h->solo_cus > prop.multiProcessorCount) h->solo_cus = prop.multiProcessorCount;
        g_cus_solo[device_id] += h->solo_cus;
        h->ncu = prop.multiProcessorCount;
    }

    // ---- buffers ----
    if (!pool_take(device_id, -1, &h->s_chain)) {
        TRACE("create: stream");
        HIP_TRY(hipStreamCreateWithFlags(&h->s_chain, hipStreamNonBlocking));
        TRACE("create: stream done");
    }
    const size_t B = batch;
    hipStream_t s = h->s_chain;
    for (const DevArray &a : device_arrays(h)) {
        HIP_TRY(dev_alloc_zero_bytes(a.slot, a.count(batch), a.elem, &h->device_bytes, s));
        if (a.slot != (void **)&dv.Bm[0]) continue;
        if (h->overlap) {  // the dense pass goes buffer to buffer
            // The second buffer is shifted by 4 KB against the first so that a tile's source and destination differ in DRAM
            // channel/bank phase: 107-108 us per pass instead of 110-111 (scripts/history/exp_skew.sh; EKF_BM_SKEW overrides, bytes)
            const size_t skew = (size_t)tn.bm_skew_bytes / sizeof(double);
            HIP_TRY(dev_alloc_zero(&h->bm1_base, B * dv.bm_stride + skew, &h->device_bytes, s));
            dv.Bm[1] = h->bm1_base + skew;
        }
        else dv.Bm[1] = dv.Bm[0];  // one buffer: the dense pass runs in place
    }
    TRACE("create: device buffers queued");
    HIP_TRY(hipHostMalloc((void **)&h->mirror_h, B * sizeof(EkfMirror), hipHostMallocMapped));
    memset(h->mirror_h, 0, B * sizeof(EkfMirror));
    HIP_TRY(hipHostGetDevicePointer((void **)&dv.mirror, h->mirror_h, 0));
    HIP_TRY(hipHostMalloc((void **)&h->sctl_h, sizeof(StreamCtl), hipHostMallocMapped));
    memset(h->sctl_h, 0, sizeof(StreamCtl));
    HIP_TRY(hipHostGetDevicePointer((void **)&dv.sctl, h->sctl_h, 0));
    {
        // the command ring in device memory where the host can write it (large BAR; EKF_STREAM_RING_HOST=1 keeps it in host memory)
        int large_bar = 0;
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, h->device) != hipSuccess) large_bar = 0, (void)hipGetLastError();
        dv.sring = dv.sctl, h->sring_h = h->sctl_h;
        if (large_bar && !tn.stream_ring_host) {
            StreamCtl *d = nullptr;
            if (hipExtMallocWithFlags((void **)&d, sizeof(StreamCtl), hipDeviceMallocFinegrained) == hipSuccess) {
                HIP_TRY(hipMemsetAsync(d, 0, sizeof(StreamCtl), s));
                h->device_bytes += sizeof(StreamCtl);
                dv.sring = d, h->sring_h = d, h->sring_in_hbm = true;
            } else {
                (void)hipGetLastError();
            }
        }
    }
    const size_t rec_bytes = B * 8 * sizeof(double);
    long ring_ops = (long)((16u << 20) / rec_bytes);
    if (ring_ops > 1024) ring_ops = 1024;
    if (ring_ops < 2 * EKF_CHAIN_MAX_OPS) ring_ops = 2 * EKF_CHAIN_MAX_OPS;
    h->ring_ops = (int)ring_ops;
    HIP_TRY(hipHostMalloc((void **)&h->ring_h, rec_bytes * h->ring_ops, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void **)&h->ring_d, h->ring_h, 0));

    // ---- streams and events (the handle was value-initialised: every count, flag and cursor of the pipeline starts at zero) ----
    for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreateWithFlags(&h->ring_ev[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&h->t0));
    HIP_TRY(hipEventCreate(&h->t1));
    h->s_flush = h->s_chain;
    if (h->overlap) {
        // The chain kernel needs its workgroups' CUs the moment it is launched; a dense pass that owns every CU
        // would make it queue behind whole tiles.  The dense pass therefore gets a stream restricted to the CUs
        // the chain does not need (EKF_CHAIN_CUS overrides the number kept free).
        int keep = tn.chain_cus.or_else(h->chain_wgs * batch < 32 ? h->chain_wgs * batch : 32);  // (measured: 32 beats 64 even for 64 workgroups)
        int ncu = prop.multiProcessorCount;
        if (keep > ncu / 2) keep = ncu / 2;
        h->flush_keep = keep > 0 ? keep : -1;
        if (!pool_take(device_id, h->flush_keep, &h->s_flush)) {
            hipError_t em = hipErrorUnknown;
            if (keep > 0) {
                std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
                // CU i sits on XCD i % 8 (round-robin numbering): free the same share of every XCD
                int per_xcd = (keep + 7) / 8, xcds = 8, freed[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int i = 0; i < ncu; i++) {
                    int xc = i % xcds;
                    bool chain_cu = freed[xc] < per_xcd;
                    if (chain_cu) freed[xc]++;
                    else mask[i / 32] |= 1u << (i % 32);
                }
                TRACE("create: cu-mask stream");
                em = hipExtStreamCreateWithCUMask(&h->s_flush, (uint32_t)mask.size(), mask.data());
                TRACE("create: cu-mask stream done");
            }
            if (em != hipSuccess) {
                (void)hipGetLastError();
                h->flush_keep = -1;  // an ordinary stream (and that is the pool it goes back to)
                if (!pool_take(device_id, -1, &h->s_flush)) HIP_TRY(hipStreamCreateWithFlags(&h->s_flush, hipStreamNonBlocking));
            }
        }
        h->flush_masked = h->flush_keep > 0;
        // In-kernel waiting only where the pass has a queue of its own CUs and kernels of the two streams were seen to run
        // side by side; everywhere else (unmasked fallback stream, serialising tools) the chain stream waits for the
        // pass's event.
        h->inkernel_wait = tn.inkernel_wait && h->flush_masked && concurrent_kernels_ok(device_id, h->s_chain, h->s_flush) != 0;
        HIP_TRY(hipEventCreate(&h->ev_chain));  // (stop events of dispatch packets)
        for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreate(&h->ev_flush[i]));
    }
    if (h->solo) {
        int ng = tn.solo_groups;
        if (ng > 8) ng = 8;
        if (ng < 1 || batch < 16 * ng) ng = 1;  // (small batches: one launch for all filters)
        h->ngroups = ng;
        h->s_grp.assign(ng, nullptr);
        h->s_grp[0] = h->s_chain;
        h->ev_join.assign(ng, nullptr);
        if (ng > 1) HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        for (int g = 1; g < ng; g++) {
            if (!pool_take(device_id, -1, &h->s_grp[g])) HIP_TRY(hipStreamCreateWithFlags(&h->s_grp[g], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&h->ev_join[g], hipEventDisableTiming));
        }
    }
    {
        int can_wait_value = 0;
        (void)hipDeviceGetAttribute(&can_wait_value, hipDeviceAttributeCanUseStreamWaitValue, device_id);
        h->persist = tn.persist && can_wait_value != 0;
    }
    read_debug_hooks(h);
    // streaming immediate-mode calls: every handle of ONE filter (k_chain above 256 landmarks, k_solo up to 256)
    h->stream_calls = batch == 1 && tn.stream;
    h->h_int.resize(B);
    TRACE("create: final sync");
    HIP_TRY(hipStreamSynchronize(h->s_chain));
    TRACE("create: done");
    return EKF_OK;
}

extern "C" int ekf_create(ekf_handle *out, int capacity_landmarks, int device_id, const ekf_params *params) {
    return ekf_batch_create(out, 1, capacity_landmarks, device_id, params);
}

// Bounds-checking variant (make check: -DEKF_CHAIN_CHECK, libekfslam_hip_check.so): every data-dependent global index of k_chain
// is range-checked on the device and the first violation of a handle is left in dv.dbg[8..11]; a handle that is destroyed with one
// reports it on stderr and counts it here (tests/test_safety_builds.py runs part of the suite against that library and wants 0).
static std::atomic<long> g_check_violations{0};
extern "C" long ekf_debug_check_violations(void) { return g_check_violations.load(); }

extern "C" int ekf_destroy(ekf_handle h) {
    if (!h) return EKF_OK;
    hipSetDevice(h->device);
    TRACE("destroy: sync");
    if (h->sctl_h && h->s_chain) (void)stream_stop(h);  // (a resident streaming launch leaves first)
    if (h->s_chain) hipStreamSynchronize(h->s_chain);
#ifdef EKF_CHAIN_CHECK
    if (h->dv.dbg) {
        long long d[12] = {0};
        if (hipMemcpy(d, h->dv.dbg, sizeof d, hipMemcpyDeviceToHost) == hipSuccess && d[8] != 0) {
            g_check_violations++;
            fprintf(stderr, "EKF_CHAIN_CHECK: index %lld outside [0, %lld) at ekf_kernels.hip:%lld (workgroup * 100000 + thread = %lld)\n", d[9], d[10], d[8], d[11]);
        }
    }
#endif
    if (h->s_flush && h->s_flush != h->s_chain) {
        hipStreamSynchronize(h->s_flush);
        pool_give(h->device, h->flush_keep, h->s_flush);
    }
    for (size_t g = 1; g < h->s_grp.size(); g++)
        if (h->s_grp[g]) {
            hipStreamSynchronize(h->s_grp[g]);
            pool_give(h->device, -1, h->s_grp[g]);
        }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    for (auto e : h->ev_join)
        if (e) hipEventDestroy(e);
    if (h->ev_chain) hipEventDestroy(h->ev_chain);
    for (int i = 0; i < 2; i++)
        if (h->ev_flush[i]) hipEventDestroy(h->ev_flush[i]);
    if (h->bm1_base) hipFree(h->bm1_base);
    for (DevBlock &blk : h->map.blk)
        if (blk.p) hipFree(blk.p);
    for (auto &g : h->graphs) hipGraphExecDestroy(g.exec);
    for (const DevArray &a : device_arrays(h))
        if (*a.slot) hipFree(*a.slot);
    for (int *m : h->tile_maps)
        if (m) hipFree(m);
    if (h->script_d) hipFree(h->script_d);
    if (h->ring_h) hipHostFree(h->ring_h);
    if (h->sring_in_hbm) hipFree(h->dv.sring);
    if (h->sctl_h) hipHostFree(h->sctl_h);
    if (h->mirror_h) hipHostFree(h->mirror_h);
    for (int i = 0; i < 2; i++)
        if (h->ring_ev[i]) hipEventDestroy(h->ring_ev[i]);
    if (h->t0) hipEventDestroy(h->t0);
    if (h->t1) hipEventDestroy(h->t1);
    for (auto e : h->prof_pool) hipEventDestroy(e);
    TRACE("destroy: streams");
    if (h->s_chain) pool_give(h->device, -1, h->s_chain);
    if (h->claimed_cus > 0 || h->solo_cus > 0) {
        std::lock_guard<std::mutex> lk(g_res_mu);
        g_cus_claimed[h->device] -= h->claimed_cus;
        g_cus_solo[h->device] -= h->solo_cus;
    }
    delete h;
    (void)hipGetLastError();
    TRACE("destroy: done");
    return EKF_OK;
}

extern "C" int ekf_batch_size(ekf_handle h) { return h ? h->dv.B : EKF_ERR_BAD_ARG; }
extern "C" int ekf_window(ekf_handle h) { return h ? h->dv.maxp : EKF_ERR_BAD_ARG; }
extern "C" int ekf_overlap(ekf_handle h) { return h ? (h->overlap ? 1 : 0) : EKF_ERR_BAD_ARG; }

extern "C" int ekf_capacity(ekf_handle h) { return h ? h->dv.Ncap : EKF_ERR_BAD_ARG; }
extern "C" void *ekf_stream(ekf_handle h) {
    if (!h) return nullptr;
    (void)stream_stop(h);  // (the caller is about to order its own work on this stream: nothing resident may hold it)
    return (void *)h->s_chain;
}
extern "C" size_t ekf_device_bytes(ekf_handle h) { return h ? h->device_bytes : 0; }

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Low-latency waits: a blocking hipStreamSynchronize / hipEventSynchronize costs 20-50 us of wake-up latency, which is a
// sizeable part of a run of a few hundred microseconds.  The host polls the stream / event for up to two milliseconds
// (about a microsecond per query) and only then blocks.
// ... and a blocking wait in the runtime is never entered at all: once in a few dozen waits of several milliseconds the wake-up
// came 4-10 ms late on the gpurun boxes (scripts/history/r04_stall_hunt.py: hipEventSynchronize returned 10-16 ms after the start of a
// 6.9 ms region; the driver's box showed 54 ms once), which is what a robot loop must not see.  So: spin on the query for 2 ms
// (short waits: no system call), then keep querying between naps (one core mostly asleep, wake-up bounded by the nap).
// The naps back off with the length of the wait -- 20 us up to 10 ms (with the kernel's default 50 us timer slack a nap really lasts
// about 70 us), 100 us up to 100 ms, 1 ms beyond: with eight ranks on a host and waits of many milliseconds (ekf_sync at the end of a
// timed region, ekf_reserve) a rank wakes its host thread a few thousand times per second at most instead of tens of thousands, a
// wait of a second costs about a thousand queries, and a hung GPU is polled a thousand times per second, not spun on.
template <typename Query>
static hipError_t poll_wait(Query query) {
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long spin = 0;; spin++) {
        hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        if ((spin & 63) == 63) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 2000000L) break;
        }
        __builtin_ia32_pause();
    }
    for (;;) {
        hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const long waited_us = (t1.tv_sec - t0.tv_sec) * 1000000L + (t1.tv_nsec - t0.tv_nsec) / 1000L;
        const timespec nap = {0, waited_us < 10000L ? 20000L : (waited_us < 100000L ? 100000L : 1000000L)};
        nanosleep(&nap, nullptr);
    }
}
static hipError_t stream_wait(hipStream_t s) {
    return poll_wait([s]() { return hipStreamQuery(s); });
}

static hipError_t event_wait(hipEvent_t ev) {
    return poll_wait([ev]() { return hipEventQuery(ev); });
}

static int check_launch() {
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? set_error(EKF_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e)) : EKF_OK;
}

// Wave -> tile table of the row-block dense pass for nT live tile rows: workgroup w (4 waves) gets tiles of class
// (I mod 2, J mod 4) = w mod 8, consecutive tiles of a class sharing their tile row; a class that runs dry takes from the
// fullest one.  Built once per nT (the map only grows), uploaded synchronously.
static const int *tile_map_for(ekf_batch *h, int nT) {
    if (!h->tn.xcd_map || nT < 8) return nullptr;  // small maps: nothing to share
    if ((int)h->tile_maps.size() <= nT) h->tile_maps.resize(nT + 1, nullptr);
    if (h->tile_maps[nT]) return h->tile_maps[nT];
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->s_chain, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;  // no allocation or copy while a graph is being captured: this pass uses the arithmetic order
    }
    std::vector<std::vector<int>> cls(8);
    for (int I = 0; I < nT; I++)
        for (int J = I; J < nT; J++) cls[(I & 1) * 4 + (J & 3)].push_back((I << 16) | J);
    std::vector<size_t> pos(8, 0);
    const int total = nT * (nT + 1) / 2, nwg = (total + 3) / 4;
    std::vector<int> map((size_t)nwg * 4, -1);
    for (int w = 0; w < nwg; w++)
        for (int k = 0; k < 4; k++) {
            int c = w & 7;
            if (pos[c] >= cls[c].size()) {  // this class is used up: take from the class with most tiles left
                size_t best = 0;
                c = -1;
                for (int q = 0; q < 8; q++)
                    if (cls[q].size() - pos[q] > best) best = cls[q].size() - pos[q], c = q;
                if (c < 0) break;
            }
            map[(size_t)w * 4 + k] = cls[c][pos[c]++];
        }
    int *d = nullptr;
    if (hipMalloc((void **)&d, map.size() * sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return nullptr;
    }
    h->device_bytes += map.size() * sizeof(int);
    h->tile_maps[nT] = d;
    return d;
}

// ---- chain / dense-pass alternation ------------------------------------------------------------------
// The decisions are ekf_window_plan.h's (plan_close, plan_ops, ...); what follows carries them out.

// The profiling events (a start / stop pair per dense pass, or per k_solo launch that folds its own windows) are created where
// profiling is switched on and where a script is loaded -- enough pairs for every window the script can close between two reads --
// never on the enqueue path: four hipEventCreate calls inside a timed region of 0.85 ms were part of what the round-5 driver
// run paid.  The enqueue path still grows the pool when a caller outruns it (immediate-mode traffic without a read).
static int prof_reserve(ekf_batch *h, size_t pairs) {
    if (pairs > 4096) pairs = 4096;
    while (h->prof_pool.size() < h->prof_used + 2 * pairs) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->prof_pool.push_back(e);
    }
    return EKF_OK;
}
// A start / stop pair from the pool (recycled after a read, which leaves both streams idle), growing it for a caller that outran
// the pool of ekf_flush_profile / ekf_script_load.
static int prof_take_pair(ekf_batch *h, hipEvent_t *e0, hipEvent_t *e1) {
    if (h->prof_pool.size() < h->prof_used + 2) EKF_TRY(prof_reserve(h, 8));
    *e0 = h->prof_pool[h->prof_used++], *e1 = h->prof_pool[h->prof_used++];
    return EKF_OK;
}
static size_t prof_pairs_for_script(const ekf_batch *h) {
    if (!h->script_d) return 8;
    // a window closes after at least maxp / 2 measurements (the balanced tail) -- and once more per call (terminal passes)
    const size_t slots = (size_t)h->script_steps * (size_t)(h->script_M > 0 ? h->script_M : 0);
    const size_t half = (size_t)(h->dv.maxp > 1 ? h->dv.maxp / 2 : 1);
    return (slots / half + 8) * (size_t)(h->ngroups > 1 ? h->ngroups : 1);
}

// ---- streaming immediate-mode calls (ekf_device.h: StreamCtl; k_chain<ONE, true>) -------------------------------------------------
// Start a streaming launch on the open window: one segment without operations, consuming commands from consumed0 + 1 on.
static int stream_start(ekf_batch *h, long long consumed0, int slot0) {
    ChainPlan plan;
    memset(&plan, 0, sizeof plan);
    plan.s[0] = stream_segment(h->wcfg, h->win, consumed0, slot0);
    plan.nseg = 1, plan.signal = 0, plan.inl_n = 0;
    if (h->dbg_stream_idle_ticks > 0 || h->dbg_stream_no_recheck) {  // (debug library only: a streaming launch has no inline record, the fields carry the test hooks)
        plan.inl_n = 1 | (h->dbg_stream_no_recheck ? 2 : 0);
        plan.inl[0] = h->dbg_stream_idle_ticks > 0 ? (double)h->dbg_stream_idle_ticks : (double)EKF_STREAM_IDLE_TICKS;
    }
    h->stream_launch = h->stream_launch >= 0xffff ? 1 : h->stream_launch + 1;  // (16 bits of it tag the forwards)
    plan.stream = h->stream_launch;
    __atomic_store_n(&h->sctl_h->state, ((unsigned long long)(unsigned)plan.stream << 2) | EKF_STREAM_RUNNING, __ATOMIC_SEQ_CST);
    launch_chain(h, h->s_chain, /*streaming*/ true, /*on_packet*/ true, nullptr, nullptr, (const double *)h->ring_d, nullptr, plan, 0, 1);
    h->stream_alive = true;
    h->stream_starts++;
    return check_launch();
}

// Wait until the streamed command `seq` has been executed (the mirror's sequence number reaches it).  This is also the safety net under
// the leave-by-itself handshake: a launch that has LEFT without consuming what was posted (state EXITED, consumed < seq) is replaced by a
// new one that starts behind what the old one did consume -- the commands are still in the ring -- so that no posted command can be lost
// whatever the order in which the two sides' accesses to host memory were served.  Bounded.
static int stream_wait_consumed(ekf_batch *h, long long seq) {
    StreamCtl *c = h->sctl_h;
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    int relaunches = 0;
    for (long spin = 0;; spin++) {
        if (__atomic_load_n(&h->mirror_h[0].seq, __ATOMIC_ACQUIRE) >= seq) return EKF_OK;
        const unsigned long long launch = (unsigned long long)(unsigned)h->stream_launch;
        if (__atomic_load_n(&c->state, __ATOMIC_ACQUIRE) == ((launch << 2) | EKF_STREAM_EXITED)) {
            const long long consumed = (long long)__atomic_load_n(&c->consumed, __ATOMIC_ACQUIRE);
            if (__atomic_load_n(&h->mirror_h[0].seq, __ATOMIC_ACQUIRE) >= seq) return EKF_OK;
            if (h->mirror_h[0].status == EKF_ERR_TIMEOUT) return sticky_status(h, false);  // the launch gave up: the state is invalid, say so
            if (consumed >= seq || ++relaunches > 4) return set_error(EKF_ERR_STATE, "a streaming launch left without publishing what it consumed");
            // (queued behind the old launch; it resumes at the slot the first unconsumed command was posted at -- the window has not changed:
            // a window only closes behind a command that is known to have been executed)
            EKF_TRY(stream_start(h, consumed, h->stream_slot_before[(unsigned long long)(consumed + 1) % EKF_STREAM_RING]));
        }
        if ((spin & 255) == 255) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 4000000000L) return set_error(EKF_ERR_TIMEOUT, "a streamed command was not executed within 4 s");
        }
        __builtin_ia32_pause();
    }
}

// The resident launch is told to leave and waited for (its epilogue writes the state back that later launches and copies read).  Every
// entry point that enqueues on the chain stream, reads device memory or hands the stream out comes through here first; the
// immediate-mode operations themselves and the mirror's readers (pose, landmark count, robot block, newest decisions, counters) do not.
static int stream_stop(ekf_batch *h) {
    if (!h->stream_alive) return EKF_OK;
    // what has been posted is executed first (the launch looks at the command slot before it looks at the stop word, but two reads of
    // host memory may be served in either order: a stop seen without the command posted in front of it would leave that command behind)
    int rc = stream_wait_consumed(h, h->stream_last_seq);
    h->stream_alive = false;
    // (a plain store: the word may live in device memory behind the BAR, where a sequentially consistent store -- an xchg on x86 -- would be a
    // locked read-modify-write across PCIe; the mapping is write-combining: the fence sends it out now)
    __atomic_store_n(&h->sring_h->stop, (unsigned long long)(unsigned)h->stream_launch, __ATOMIC_RELAXED);
    __builtin_ia32_sfence();
    HIP_TRY(stream_wait(h->s_chain));
    return rc;
}

static hipEvent_t role_event(const ekf_batch *h, EvRole r) {
    switch (r) {
    case EV_CHAIN: return h->ev_chain;
    case EV_FLUSH0: case EV_FLUSH1: return h->ev_flush[r - EV_FLUSH0];
    case EV_PROF0: case EV_PROF1: return h->prof_stop[r - EV_PROF0];
    default: return nullptr;
    }
}

// A pass that goes out later, behind a launch that is made first: its tile map is built (a synchronous copy) while nothing is resident.
static int prepare_pass(ekf_batch *h, const PassOrder &o) {
    if (o.want_tile_map) (void)tile_map_for(h, o.nT_hi);
    return EKF_OK;
}

// The only place that turns a PassOrder into calls.
static int issue_pass(ekf_batch *h, const PassOrder &o) {
    if (o.nslots == 0) return EKF_OK;
    const EkfDev &dv = h->dv;
    const hipStream_t sc = h->s_chain, sf = o.on == ON_CHAIN ? h->s_chain : h->s_flush;
    hipEvent_t e0 = nullptr, e1 = role_event(h, o.stop);
    if (o.prof) {
        EKF_TRY(prof_take_pair(h, &e0, &e1));
        if (o.done == EV_PROF0 || o.done == EV_PROF1) h->prof_stop[o.done - EV_PROF0] = e1;
    }
    const int *tmap = o.want_tile_map ? tile_map_for(h, o.nT_hi) : (const int *)nullptr;
    const hipEvent_t wait_prev = role_event(h, o.wait_prev), done_ev = role_event(h, o.done);
    if (o.terminal) {
        if (wait_prev) HIP_TRY(hipStreamWaitEvent(sc, wait_prev, 0));
    } else {
        if (o.gate_seq) HIP_TRY(hipStreamWaitValue64(sf, dv.seg_count + o.gate_idx, o.gate_seq, hipStreamWaitValueGte, 0xffffffffffffffffull));
        if (o.record_chain) HIP_TRY(hipEventRecord(h->ev_chain, sc));
        if (o.wait_chain) HIP_TRY(hipStreamWaitEvent(sf, h->ev_chain, 0));
    }
    if (o.do_pass) launch_pass(dv, sf, e0, e1, o.interleave, o.nT_hi, o.set, o.nslots, o.fin, o.fout, tmap, o.rev, 0, dv.B);
    if (!o.terminal && wait_prev) HIP_TRY(hipStreamWaitEvent(sc, wait_prev, 0));
    if (o.mark) hipLaunchKernelGGL(k_mark, dim3(1), dim3(64), 0, sf, dv.pass_flag, o.mark_value);
    if (o.record_done) HIP_TRY(hipEventRecord(done_ev, sf));
    if (o.wait_done_on_chain) HIP_TRY(hipStreamWaitEvent(sc, done_ev, 0));
    HIP_TRY(hipGetLastError());
    return EKF_OK;
}

// Close the slot set being filled and hand it to a dense pass (plan_close); the chain continues into the other set.
static int close_set(ekf_batch *h, bool terminal = false) {
    EKF_TRY(stream_stop(h));
    return issue_pass(h, plan_close(h->wcfg, h->win, terminal, h->n_lm_hi, h->prof_flush));
}

// One immediate-mode operation through the streaming launch: post the command, make sure somebody consumes it, keep the host's
// window bookkeeping (launch_ops' for a one-operation launch).  rec: the operation's record; consumes: it takes a slot.
// n_slots: slots of the open window the command consumes (an operation: 0 or 1; a scripted chunk: its measurements -- the caller cuts
// chunks so that none passes the end of the window).
static int stream_op(ekf_batch *h, const double *rec, int n_slots) {
    StreamCtl *c = h->sctl_h;
    const bool consumes = n_slots > 0;
    const bool closes = stream_closes(h->wcfg, h->win, n_slots);
    const long long seq = ++h->chain_seq;
    StreamCmd *cmd = &h->sring_h->cmd[(unsigned long long)seq % EKF_STREAM_RING];
    if (h->stream_alive && seq - EKF_STREAM_RING > 0) {  // the slot's previous command (seq - ring) must have been executed: a caller that posts without ever reading
        int rc = stream_wait_consumed(h, seq - EKF_STREAM_RING);
        if (rc) {
            h->chain_seq--;
            return rc;
        }
    }
    {
        // seventeen granules {32 payload bits, the sequence number's low half}; the flags (g[0]) last: the launch polls them, and re-reads
        // every other granule until it carries the tag
        const unsigned long long tg = ((unsigned long long)seq & 0xffffffffull) << 32;
        for (int i = 0; i < 8; i++) {
            unsigned long long bits;
            memcpy(&bits, rec + i, sizeof bits);
            __atomic_store_n(&cmd->g[1 + 2 * i], (bits & 0xffffffffull) | tg, __ATOMIC_RELAXED);
            __atomic_store_n(&cmd->g[2 + 2 * i], (bits >> 32) | tg, __ATOMIC_RELAXED);
        }
        __atomic_store_n(&cmd->g[0], (unsigned long long)(closes ? EKF_STREAM_END_AFTER : 0) | tg, __ATOMIC_RELEASE);
        __builtin_ia32_sfence();  // (a ring in device memory is written through a write-combining mapping: the command leaves the write buffers now)
    }
    h->stream_ops++;
    h->stream_last_seq = seq;
    h->stream_slot_before[(unsigned long long)seq % EKF_STREAM_RING] = h->win.pending;
    if (!h->stream_alive) {
        // (every earlier streamed command has been executed: a launch is only written off behind stream_wait_consumed -- stream_stop, a closing command)
        EKF_TRY(stream_start(h, seq - 1, h->win.pending));
    } else {
        // "write mine, fence, read yours": the launch does the same with its state word and this command slot before it leaves by itself, so
        // normally one of the two sees the other.  RUNNING: the launch will find the command.  Anything else: wait for the outcome (the
        // operation done, or the launch gone without it and replaced).
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
        const unsigned long long launch = (unsigned long long)(unsigned)h->stream_launch;
        if (__atomic_load_n(&c->state, __ATOMIC_ACQUIRE) != ((launch << 2) | EKF_STREAM_RUNNING)) {
            EKF_TRY(stream_wait_consumed(h, seq));
        }
    }
    h->mirror_by_chain = true;
    h->stats_in_mirror = true;
    if (consumes) h->win.pending += n_slots;
    if (closes) {
        // the launch leaves behind this operation by itself (EKF_STREAM_END_AFTER); the window's dense pass is enqueued behind it once the
        // closing command is known to have been executed (a synchronising caller would wait for it next anyway)
        int rc = stream_wait_consumed(h, seq);
        h->stream_alive = false;
        if (rc) return rc;
        // the window turns over (plan_stream_turn: with overlap the pass goes out behind the next streaming launch, a k_solo launch has folded
        // the window itself, in place the pass runs on the chain's stream and the next launch behind it)
        const StreamTurn t = plan_stream_turn(h->wcfg, h->win, h->n_lm_hi, h->prof_flush);
        if (t.record_chain) HIP_TRY(hipEventRecord(h->ev_chain, h->s_chain));  // (behind the launch that filled the window)
        if (!t.pass_after_start) EKF_TRY(issue_pass(h, t.pass));
        else EKF_TRY(prepare_pass(h, t.pass));
        rc = stream_start(h, seq, h->win.pending);
        if (t.pass_after_start) {
            const int rc_pass = issue_pass(h, t.pass);
            if (rc == EKF_OK) rc = rc_pass;
        }
        return rc;
    }
    return EKF_OK;
}

// Everything folded into Bm[buf_in], streams idle.
static int settle(ekf_batch *h) {
    EKF_TRY(close_set(h, true));
    HIP_TRY(stream_wait(h->s_chain));
    if (h->overlap) HIP_TRY(stream_wait(h->s_flush));
    land_last_pass(h->wcfg, h->win);
    return EKF_OK;
}

// What plan_ops' decisions are carried out on: one call's input, and the handle.
struct OpsSink {
    ekf_batch *h;
    const double *in;
    const int *cursor;
    int segment(const ChainSeg &) {
        h->mirror_by_chain = true;
        h->stats_in_mirror = true;
        return EKF_OK;
    }
    int pass(const PassOrder &o) { return issue_pass(h, o); }
    int prepare(const PassOrder &o) { return prepare_pass(h, o); }
    // One plan goes out: a launch per chain_filters filters.
    int launch(ChainPlan &plan, const LaunchOrder &lo) {
        if (plan.inl_n) memcpy(plan.inl, h->ring_h + (size_t)plan.s[0].k0 * 8, 8 * sizeof(double));
        hipEvent_t pe0 = nullptr, pe1 = nullptr;
        if (lo.prof) {  // the passes live inside this launch: time the launch, count the passes
            EKF_TRY(prof_take_pair(h, &pe0, &pe1));
            h->prof_fused_passes += lo.fused_passes;
            h->prof_solo_pairs++;
        }
        for (ChainLaunch l = chain_launch(h->wcfg, lo, 0); l.nb > 0; l = chain_launch(h->wcfg, lo, l.b0 + l.nb))
            launch_chain(h, h->s_chain, /*streaming*/ false, /*on_packet*/ true, l.start_prof ? pe0 : nullptr, l.stop_prof ? pe1 : role_event(h, l.stop), in, cursor, plan, l.b0, l.nb);
        return check_launch();
    }
};

// One-workgroup filters in phase groups: a call that closes several windows (a scripted run) is cut by filter range instead of
// running the whole batch in lock step.  Group g's stream carries chain launch, dense pass (in place), chain launch, ... for its
// filters only; nothing orders the groups against each other (filters are independent), and a one-off delay in front of each
// group's first launch spreads their phases, so that the passes take turns in HBM while the other groups' chain kernels -- which
// are latency-bound and leave the memory system idle -- run.  Fork from and join into s_chain, so that every other entry point
// keeps seeing one stream.
static int launch_ops_grouped(ekf_batch *h, const double *in, const OpsCall &call) {
    const int ng = h->ngroups, B = h->dv.B;
    const int per = (B + ng - 1) / ng;
    hipError_t e;
    if ((e = hipEventRecord(h->ev_fork, h->s_chain)) != hipSuccess) return set_error(EKF_ERR_HIP, "%s", hipGetErrorString(e));
    for (int g = 1; g < ng; g++) {
        if ((e = hipStreamWaitEvent(h->s_grp[g], h->ev_fork, 0)) != hipSuccess) return set_error(EKF_ERR_HIP, "%s", hipGetErrorString(e));  // (nothing has been launched on a group stream yet)
        if (h->tn.solo_stagger_ticks > 0) hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, h->s_grp[g], (long long)g * h->tn.solo_stagger_ticks);
    }
    const bool interleave = h->tn.batch_interleave;
    // The group streams have been forked off s_chain: whatever happens from here on, they are joined back before this function
    // returns -- later work on s_chain (ring reuse, memsets of ekf_set_state, the hipFree of a staging buffer) must not run beside
    // chain and pass kernels still queued on a group stream.  An error on the way is remembered, the join still happens (where even
    // the join's event calls fail the group stream is drained on the host).
    int rc_pending = EKF_OK;
    // (event creation can fail: do it in front of the first launch, not between a fork and its join)
    if (h->prof_flush) rc_pending = prof_reserve(h, (size_t)ng * (size_t)grouped_passes(h->wcfg, h->win, call));
    ChainPlan plan;
    memset(&plan, 0, sizeof plan);
    plan.nseg = 1;
    GroupedWindow w;
    for (int i = 0; rc_pending == EKF_OK && plan_ops_grouped(h->wcfg, h->win, call, &i, &h->chain_seq, &w);) {
        plan.s[0] = w.seg;
        h->mirror_by_chain = true;
        h->stats_in_mirror = true;
        for (int g = 0; g < ng; g++) {
            const int b0 = g * per, nb = B - b0 < per ? B - b0 : per;
            if (nb <= 0) break;
            launch_chain(h, h->s_grp[g], /*streaming*/ false, /*on_packet*/ false, nullptr, nullptr, in, nullptr, plan, b0, nb);
            if (!w.do_pass) continue;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (h->prof_flush && h->prof_used + 2 <= h->prof_pool.size()) (void)prof_take_pair(h, &e0, &e1);  // (reserved above: never grows here, between a fork and its join)
            launch_pass(h->dv, h->s_grp[g], e0, e1, interleave, w.nT_hi, w.set, w.nslots, w.buf, w.buf, nullptr, w.rev, b0, nb);
        }
    }
    for (int g = 1; g < ng; g++) {
        if ((e = hipEventRecord(h->ev_join[g], h->s_grp[g])) == hipSuccess) e = hipStreamWaitEvent(h->s_chain, h->ev_join[g], 0);
        if (e != hipSuccess) {
            (void)stream_wait(h->s_grp[g]);  // no event to order the streams with: drain this one here
            if (rc_pending == EKF_OK) rc_pending = set_error(EKF_ERR_HIP, "%s", hipGetErrorString(e));
        }
    }
    if (rc_pending != EKF_OK) return rc_pending;
    return check_launch();
}

// CUs on which a gated pass can run while the chain workgroups of a multi-segment launch stay resident: a chain wave leaves too few
// registers on its SIMD for a pass wave, so a pass only runs on CUs without a chain workgroup.  Multi-segment launches are used
// while the chain workgroups of ALL live handles hold at most half of the GPU (256 filters of one workgroup each would
// wait forever for a pass that cannot start: that batch keeps one launch per segment).
static bool residency_ok(const ekf_batch *h) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    return (g_cus_claimed[h->device] + g_cus_solo[h->device] - h->solo_cus) * 2 <= h->ncu;  // (everybody else's chain workgroups, solo launches included)
}

// Run ops [k0, k0 + nops) of `in` (the input ring, or the loaded script: at *cursor while a graph is captured) on the route that
// route_call chooses.  consumes, defer_last_close: OpsCall.
static int launch_ops(ekf_batch *h, const double *in, const int *cursor, int k0, const unsigned char *consumes, int nops, bool defer_last_close = false) {
    const WindowCfg &cfg = h->wcfg;
    if (nops > 0 && h->win.pending == cfg.maxp) EKF_TRY(close_set(h));  // a set whose close the previous call deferred: more work follows, regular pass
    const CallSource src = cursor ? FROM_CURSOR : (in == h->ring_d ? FROM_RING : FROM_SCRIPT);
    const CallPlan cp = route_call(cfg, h->win, h->stream_calls, src, consumes, nops, defer_last_close, persist_possible(cfg, src, defer_last_close) && residency_ok(h));
    if (cp.route == ROUTE_STREAM_OPS) {
        for (int q = 0; q < nops; q++) EKF_TRY(stream_op(h, h->ring_h + (size_t)(k0 + q) * 8, consumes[q] ? 1 : 0));
        return EKF_OK;
    }
    if (cp.route == ROUTE_STREAM_SCRIPT) {
        for (int q0 = 0, q1 = 0; q0 < nops; q0 = q1) {
            const int used = take_ops(consumes, nops, &q1, h->win.pending, cfg.maxp) - h->win.pending;  // (up to, and including, the measurement that fills the window)
            double rec[8] = {0, 0, 0, 0, 0, 0, 0, (double)OP_SCRIPT};
            const long long bits = (long long)(size_t)h->script_d;
            memcpy(&rec[0], &bits, sizeof bits);
            rec[1] = (double)(k0 + q0), rec[2] = (double)(q1 - q0);
            EKF_TRY(stream_op(h, rec, used));
        }
        return EKF_OK;
    }
    EKF_TRY(stream_stop(h));
    const OpsCall call = {src, k0, nops, consumes, defer_last_close, h->n_lm_hi, h->prof_flush};
    if (cp.route == ROUTE_GROUPED) return launch_ops_grouped(h, in, call);
    OpsSink sink = {h, in, cursor};
    return plan_ops(cfg, h->win, cp, call, &h->chain_seq, sink);
}

static void bump_bound(ekf_batch *h, int measurements) {
    h->n_lm_hi += measurements;
    if (h->n_lm_hi > h->dv.Ncap) h->n_lm_hi = h->dv.Ncap;
}

// ---- input ring ---------------------------------------------------------------------------------
// Reserve `count` consecutive records (never straddling the wrap); *rec points at the first.
static int ring_reserve(ekf_batch *h, int count, double **rec, int *k_out) {
    int half = h->ring_ops / 2;
    if (count > half) return set_error(EKF_ERR_BAD_ARG, "too many operations in one call");
    int pos = h->ring_pos;
    int which = pos < half ? 0 : 1;
    if (h->stream_calls && pos + count > (which + 1) * half) {
        // (a streaming handle's records are copied into the command ring when they are posted: no launch ever reads this ring)
        which ^= 1;
        pos = which * half;
    } else if (pos + count > (which + 1) * half) {  // does not fit the rest of this half: move to the next half
        HIP_TRY(hipEventRecord(h->ring_ev[which], h->s_chain));
        h->ring_ev_valid[which] = true;
        which ^= 1;
        pos = which * half;
        if (h->ring_ev_valid[which]) HIP_TRY(event_wait(h->ring_ev[which]));  // its readers from one lap ago
    }
    *rec = h->ring_h + (size_t)pos * h->dv.B * 8;
    *k_out = pos;
    h->ring_pos = pos + count;
    return EKF_OK;
}

// Wait until the newest chain launch has written the host-mapped mirror, then read it.  When that launch is the
// newest writer the host spins on the mirror's sequence number (stored last by the kernel, system scope) for up to
// a millisecond -- a stream synchronise costs 10-20 us of wake-up latency per call, which is most of an
// immediate-mode call -- and falls back to the synchronise.  full = true always synchronises (callers that go on to
// read device memory written by the whole launch).
static int refresh_bounds(ekf_batch *h, bool full = true) {
    bool done = false;
    if (!full && h->mirror_by_chain && h->chain_seq > 0) {
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (long spin = 0;; spin++) {
            bool all = true;
            for (int b = 0; b < h->dv.B; b++)
                if (__atomic_load_n(&h->mirror_h[b].seq, __ATOMIC_ACQUIRE) < h->chain_seq) {
                    all = false;
                    break;
                }
            if (all) {
                done = true;
                break;
            }
            if ((spin & 255) == 255) {
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 1000000L) break;
            }
            __builtin_ia32_pause();
        }
    }
    if (!done) {
        EKF_TRY(stream_stop(h));  // (a resident streaming launch leaves first: the stream would not drain before its idle time is over)
        HIP_TRY(stream_wait(h->s_chain));
    }
    int mx = 0;
    for (int b = 0; b < h->dv.B; b++) {
        h->h_int[b] = h->mirror_h[b].n_lm;
        mx = h->h_int[b] > mx ? h->h_int[b] : mx;
    }
    h->n_lm_hi = mx;
    return sticky_status(h, false);  // a timed-out launch left an invalid state: say so wherever state is handed out
}

// ---- propagate --------------------------------------------------------------------------------------
static void make_Q(const ekf_params &p, double v, double Q[4]) {
    // kalmanfilter.cpp:35-37: Q << sv,0,0,sw; Q = (v*v)*Q*Q  ->  ((v*v)*Q)*Q, column-major out
    double a = (v * v) * p.sigma_v, d = (v * v) * p.sigma_w;
    Q[0] = a * p.sigma_v;
    Q[1] = 0.0;
    Q[2] = 0.0;
    Q[3] = d * p.sigma_w;
}

extern "C" int ekf_batch_propagate_q(ekf_handle h, const double *v, const double *w, const double *Q, const double *dt) {
    if (!h || !v || !w || !Q || !dt) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    double *rec;
    int k;
    EKF_TRY(ring_reserve(h, 1, &rec, &k));
    for (int b = 0; b < h->dv.B; b++) {
        double *r = rec + (size_t)b * 8;
        r[0] = v[b], r[1] = w[b], r[2] = dt[b];
        r[3] = Q[4 * b], r[4] = Q[4 * b + 1], r[5] = Q[4 * b + 2], r[6] = Q[4 * b + 3];
        r[7] = OP_PROP;
    }
    unsigned char consumes = 0;
    return launch_ops(h, h->ring_d, nullptr, k, &consumes, 1);
}

extern "C" int ekf_batch_propagate(ekf_handle h, const double *v, const double *w, const double *dt) {
    if (!h || !v || !w || !dt) return set_error(EKF_ERR_BAD_ARG, "null argument");
    std::vector<double> Q((size_t)4 * h->dv.B);
    for (int b = 0; b < h->dv.B; b++) make_Q(h->params, v[b], &Q[4 * (size_t)b]);
    return ekf_batch_propagate_q(h, v, w, Q.data(), dt);
}

extern "C" int ekf_propagate_q(ekf_handle h, double v, double w, const double Q[4], double dt) {
    if (!h || h->dv.B != 1) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    return ekf_batch_propagate_q(h, &v, &w, Q, &dt);
}

extern "C" int ekf_propagate(ekf_handle h, double v, double w, double dt) {
    if (!h || h->dv.B != 1) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    return ekf_batch_propagate(h, &v, &w, &dt);
}

// ---- update ---------------------------------------------------------------------------------------
static int fetch_decisions(ekf_batch *h, int n_z, ekf_decision *out);

extern "C" int ekf_batch_update(ekf_handle h, const double *z, const double *R, const unsigned char *valid, int n_z, ekf_decision *decisions_out) {
    if (!h || n_z < 0 || (n_z > 0 && (!z || !R))) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    int B = h->dv.B;
    int half = h->ring_ops / 2;
    std::vector<unsigned char> consumes;
    for (int j0 = 0; j0 < n_z; j0 += half) {  // a chunk larger than half the ring goes out in pieces
        int cnt = n_z - j0 < half ? n_z - j0 : half;
        double *rec;
        int k;
        EKF_TRY(ring_reserve(h, cnt, &rec, &k));
        for (int jj = 0; jj < cnt; jj++) {
            int j = j0 + jj;
            for (int b = 0; b < B; b++) {
                double *r = rec + ((size_t)jj * B + b) * 8;
                const double *zz = z + ((size_t)b * n_z + j) * 2;
                const double *RR = R + ((size_t)b * n_z + j) * 4;
                r[0] = zz[0], r[1] = zz[1];
                r[2] = RR[0], r[3] = RR[1], r[4] = RR[2], r[5] = RR[3];
                r[6] = (j == n_z - 1) ? 2.0 : 1.0;  // 2 = last measurement of the chunk (Update.cpp:26 quirk)
                r[7] = (!valid || valid[(size_t)b * n_z + j]) ? OP_MEAS : OP_SKIP_SLOT;
            }
        }
        consumes.assign(cnt, 1);
        bump_bound(h, cnt);
        EKF_TRY(launch_ops(h, h->ring_d, nullptr, k, consumes.data(), cnt));
    }
    if (decisions_out) return fetch_decisions(h, n_z, decisions_out);
    return EKF_OK;
}

extern "C" int ekf_update(ekf_handle h, const double *z_chunk, const double *R_chunk, int n_z, ekf_decision *decisions_out) {
    if (!h || h->dv.B != 1) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    return ekf_batch_update(h, z_chunk, R_chunk, nullptr, n_z, decisions_out);
}

extern "C" int ekf_batch_update_compass(ekf_handle h, const double *z, const double *R, const unsigned char *valid) {
    if (!h || !z || !R) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    double *rec;
    int k;
    EKF_TRY(ring_reserve(h, 1, &rec, &k));
    for (int b = 0; b < h->dv.B; b++) {
        double *r = rec + (size_t)b * 8;
        r[0] = z[b], r[1] = R[b];
        r[2] = r[3] = r[4] = r[5] = r[6] = 0;
        r[7] = (!valid || valid[b]) ? OP_COMPASS : OP_SKIP_SLOT;
    }
    unsigned char consumes = 1;
    return launch_ops(h, h->ring_d, nullptr, k, &consumes, 1);
}

extern "C" int ekf_update_compass(ekf_handle h, double z, double R) {
    if (!h || h->dv.B != 1) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    return ekf_batch_update_compass(h, &z, &R, nullptr);
}

extern "C" int ekf_record_truth(ekf_handle h, const double *truth) {
    if (!h || !truth) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    double *rec;
    int k;
    EKF_TRY(ring_reserve(h, 1, &rec, &k));
    for (int b = 0; b < h->dv.B; b++) {
        double *r = rec + (size_t)b * 8;
        r[0] = truth[3 * b], r[1] = truth[3 * b + 1], r[2] = truth[3 * b + 2];
        r[3] = r[4] = r[5] = r[6] = 0;
        r[7] = OP_TRUTH;
    }
    unsigned char consumes = 0;
    return launch_ops(h, h->ring_d, nullptr, k, &consumes, 1);
}

// ---- synchronising accessors ------------------------------------------------------------------------
// The sticky per-filter status the kernels leave in the host mirror (valid after a synchronising read).  A timeout means
// the filter's state is invalid, and every accessor that hands out state reports it; a capacity overflow leaves a valid
// state (the landmark was simply not added) and is reported by ekf_sync only.
static int sticky_status(ekf_batch *h, bool include_capacity) {
    for (int b = 0; b < h->dv.B; b++) {
        const int st = h->mirror_h[b].status;
        if (st == EKF_ERR_TIMEOUT)
            return set_error(EKF_ERR_TIMEOUT, "filter %d: a device-side wait ran out (the %d chain workgroups of a filter were not all resident -- another tenant on the GPU? -- "
                                              "or the dense pass a launch depends on did not complete); the filter's state is invalid until ekf_set_state", b, h->chain_wgs);
        if (st == EKF_ERR_CAPACITY && include_capacity)
            return set_error(EKF_ERR_CAPACITY, "filter %d: a New landmark did not fit capacity_landmarks = %d (Update.cpp:152-178 would have grown the state)", b, h->dv.Ncap);
        if (st != 0 && st != EKF_ERR_CAPACITY) return set_error(st, "a kernel reported an error status");
    }
    return EKF_OK;
}

// ---- bringing a handle to rest --------------------------------------------------------------------------------------------------
// Every entry point that enqueues on the chain stream behind the launches, reads device memory or rewrites state comes through
// quiesce() first (the immediate-mode operations themselves and the host mirror's readers do not).  It selects the device and has
// the resident streaming launch leave; then, in this order:
//   rule  != ST_NONE       the chain stream is drained and the host's bounds (h_int[], n_lm_hi) are refreshed; a sticky
//                          EKF_ERR_TIMEOUT (the state is invalid) ends the call -- ST_INVALID_OR_FULL: a sticky EKF_ERR_CAPACITY too
//   level == QUIET_SETTLED everything is folded into Bm[buf_in] by a terminal pass, both streams idle
//
//   entry point                                        level          rule                 what follows
//   ekf_sync, ekf_flush_profile_read                   QUIET_STREAM   ST_NONE              wait for both streams (ekf_sync: any sticky status)
//   ekf_get_decisions, ekf_stats_means_device,
//   ekf_script_load, ekf_debug_stamps                  QUIET_STREAM   ST_NONE              own work on the chain stream, waited for
//   ekf_reset_stats, ekf_timer_start, ekf_timer_stop   QUIET_STREAM   ST_NONE              own work on the chain stream, not waited for
//   ekf_get_x                                          QUIET_STREAM   ST_INVALID           copy
//   ekf_get_state                                      QUIET_STREAM   ST_INVALID           size only: returns; else settle(), export
//   ekf_joint_consistency (and the batch form)         QUIET_STREAM   ST_INVALID           settle(), factor in the scratch; the state is only read
//   ekf_find_duplicates (and the batch form)           QUIET_STREAM   ST_INVALID           settle(), the pairwise gate over Bm; the state is only read
//   ekf_set_state                                      QUIET_SETTLED  ST_NONE              (the way out of a timed-out handle: no status ends it)
//   ekf_broadcast_state                                QUIET_SETTLED  ST_NONE
//   ekf_reserve                                        QUIET_SETTLED  ST_NONE              refreshes the bounds AFTER the settle; only EKF_ERR_TIMEOUT ends it
//   ekf_remove_landmarks, ekf_transform_frame,
//   ekf_anchor_at_robot (and the batch forms)          QUIET_SETTLED  ST_INVALID_OR_FULL   the state stays as it is under either status
//   ekf_join_map, ekf_batch_join_map                   QUIET_SETTLED  ST_INVALID_OR_FULL   BOTH handles, the source first (a join without room fails after the settle)
//   ekf_fuse_landmarks (and the batch form)            QUIET_SETTLED  ST_INVALID_OR_FULL   the pair list is checked first, against the mirror's counts; no pair: returns
//   ekf_update_matched (and the batch form)            QUIET_SETTLED  ST_INVALID_OR_FULL   values checked first, ids against the mirror's counts; no measurement: returns
//   ekf_joint_compat (and the batch form)              QUIET_STREAM   ST_INVALID           ids checked; no measurement: returns; else settle(); the state is only read
//   ekf_update_fixes (and the batch form)              QUIET_SETTLED  ST_INVALID_OR_FULL   as ekf_update_matched: values checked first, landmark ids against the mirror's counts; no entry: returns
//   ekf_fix_compat (and the batch form)                QUIET_STREAM   ST_INVALID           as ekf_joint_compat
//   ekf_add_landmarks (and the batch form)             QUIET_SETTLED  ST_INVALID_OR_FULL   values checked first; nothing selected: returns (an add without room fails after the settle)
//   ekf_update_joint (and the batch form)              ekf_associate_joint's, then ekf_update_matched's, then ekf_add_landmarks' (the room is checked between the first two)
//   ekf_extract_map, ekf_batch_extract_map             source: QUIET_STREAM, ST_INVALID, ids checked, settle(); then the destination:
//                                                      QUIET_SETTLED  ST_NONE              as ekf_set_state (the source is only read)
//   ekf_get_submap                                     QUIET_STREAM   ST_INVALID           ids checked; size only: returns; else settle(), the dense gather
//   ekf_associate_joint (and the batch form)           QUIET_STREAM   ST_INVALID           values checked first; the sweep of ekf_gate_candidates; no candidate: returns;
//                                                                                          else settle(), the search; the state is only read
//   ekf_locate_scan (and the batch form)               refresh_bounds alone, as ekf_gate_candidates: values checked first; nothing to search: returns; only x is read
//   ekf_reset_pose (and the batch form)                QUIET_SETTLED  ST_INVALID_OR_FULL   as ekf_transform_frame
//   ekf_relocalize (and the batch form)                ekf_locate_scan's; refused: returns; then ekf_reset_pose's, then ekf_update_matched's
//   ekf_gate_candidates (and the batch form)           refresh_bounds alone (as ekf_get_landmark_covs): values checked first; no measurement: returns;
//                                                      the chain stream drained, a sticky EKF_ERR_TIMEOUT ends it, EKF_ERR_CAPACITY does not; NO settle():
//                                                      the open window stays open, x / robot rows / D are only read, the flush stream is untouched
// (ekf_get_landmark_covs and the mirror's readers go through refresh_bounds alone; ekf_flush / ekf_close_window through close_set.)
enum QuietLevel { QUIET_STREAM, QUIET_SETTLED };
enum StatusRule { ST_NONE, ST_INVALID, ST_INVALID_OR_FULL };
static int quiesce(ekf_batch *h, QuietLevel level, StatusRule rule) {
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(stream_stop(h));
    if (rule != ST_NONE) EKF_TRY(refresh_bounds(h));
    if (rule == ST_INVALID_OR_FULL) EKF_TRY(sticky_status(h, true));
    if (level == QUIET_SETTLED) EKF_TRY(settle(h));
    return EKF_OK;
}

// The end of a state rewrite on the settled handle (ekf_set_state, removal, frame change), behind the caller's own kernels on the
// chain stream.  rearm: clear the slot rows (FA / FB) of filters [b0, b0 + nb) and, in overlap mode, store the host's pass count
// into dv.pass_flag (ekf_set_state has done both itself, in front of its import).  counts: the new landmark count of filter
// b0 + k at counts[k * count_stride] for k_set_meta (counts, slots, host mirror), or null: the counts did not change.  Then: wait,
// report a failed launch, flip_buf: the rewrite went into the other Bm buffer; the mirror is no chain launch's; refresh the bounds.
static int finish_rewrite(ekf_batch *h, int b0, int nb, bool rearm, const int *counts, int count_stride, bool flip_buf) {
    EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    if (rearm) {
        HIP_TRY(hipMemsetAsync(dv.FA + (size_t)b0 * 2 * dv.f_stride, 0, sizeof(double) * (size_t)nb * 2 * dv.f_stride, s));
        HIP_TRY(hipMemsetAsync(dv.FB + (size_t)b0 * 2 * dv.f_stride, 0, sizeof(double) * (size_t)nb * 2 * dv.f_stride, s));
        if (h->overlap) hipLaunchKernelGGL(k_mark, dim3(1), dim3(64), 0, s, dv.pass_flag, h->win.pass_seq);
    }
    if (counts)
        for (int k = 0; k < nb; k++) hipLaunchKernelGGL(k_set_meta, dim3(1), dim3(64), 0, s, dv, b0 + k, counts[(size_t)k * count_stride]);
    HIP_TRY(stream_wait(s));
    EKF_TRY(check_launch());
    if (flip_buf) h->win.buf_in ^= 1;
    h->mirror_by_chain = false;
    h->state_edits++;
    return refresh_bounds(h);
}

extern "C" int ekf_sync(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(stream_wait(h->s_chain));
    if (h->overlap) HIP_TRY(stream_wait(h->s_flush));
    // Every bounded wait that runs out stores EKF_ERR_TIMEOUT into the host-mapped mirror itself, at once (and nothing but
    // k_set_meta ever writes a zero there): the mirror is complete when the streams are idle -- no device-to-host copy here.
    h->h_int.resize(h->dv.B);
    for (int b = 0; b < h->dv.B; b++) h->h_int[b] = h->mirror_h[b].n_lm;
    return sticky_status(h, true);
}

extern "C" int ekf_flush(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    return close_set(h, true);
}

extern "C" int ekf_close_window(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    return close_set(h, false);
}

extern "C" int ekf_batch_get_pose(ekf_handle h, double *pose_out) {
    if (!h || !pose_out) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h, false));
    for (int b = 0; b < h->dv.B; b++)
        for (int i = 0; i < 3; i++) pose_out[3 * b + i] = h->mirror_h[b].pose[i];
    return EKF_OK;
}

extern "C" int ekf_get_pose(ekf_handle h, double pose_out[3]) {
    if (!h || h->dv.B != 1) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    return ekf_batch_get_pose(h, pose_out);
}

extern "C" int ekf_batch_num_landmarks(ekf_handle h, int *n_out) {
    if (!h || !n_out) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h, false));
    for (int b = 0; b < h->dv.B; b++) n_out[b] = h->h_int[b];
    return EKF_OK;
}

extern "C" int ekf_num_landmarks(ekf_handle h) {
    if (!h || h->dv.B != 1) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    int n;
    int rc = ekf_batch_num_landmarks(h, &n);
    return rc ? rc : n;
}

extern "C" int ekf_get_robot_cov(ekf_handle h, double P_RR_out[9]) {
    if (!h || h->dv.B != 1 || !P_RR_out) return set_error(EKF_ERR_BAD_ARG, "single-filter call on a batch handle");
    HIP_TRY(hipSetDevice(h->device));
    // The chain kernels leave the robot block in the host-mapped mirror beside the pose (round 4: a device-to-host copy here cost the
    // compat shim's doPropagation 15-25 us of every step).  The copy stays for what does not write the mirror last (graph replays).
    if (h->mirror_by_chain && h->chain_seq > 0) {
        int rc = refresh_bounds(h, false);  // waits until the newest launch has written the mirror; sticky EKF_ERR_TIMEOUT
        if (rc == EKF_ERR_TIMEOUT) return rc;
        if (h->mirror_by_chain) {
            for (int i = 0; i < 9; i++) P_RR_out[i] = h->mirror_h[0].Prr[i];
            return EKF_OK;
        }
    }
    HIP_TRY(hipMemcpy2DAsync(P_RR_out, 3 * sizeof(double), h->dv.R, (size_t)h->dv.xs * sizeof(double), 3 * sizeof(double), 3,
                             hipMemcpyDeviceToHost, h->s_chain));
    HIP_TRY(stream_wait(h->s_chain));
    return EKF_OK;
}

extern "C" int ekf_get_x(ekf_handle h, int index, double *x_out, int n_max) {
    if (!filter_ok(h, index) || !x_out || n_max < 0) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    int n = 3 + 2 * h->h_int[index];
    int cnt = n < n_max ? n : n_max;
    HIP_TRY(hipMemcpy(x_out, h->dv.x + (size_t)index * h->dv.xs, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return n;
}

static int fetch_decisions(ekf_batch *h, int n_z, ekf_decision *out) {
    // [batch][n_z]: the last entries of every filter's log.  Masked measurements leave no entry, so a
    // filter with fewer real entries gets zeroed records in front.
    int B = h->dv.B;
    EKF_TRY(refresh_bounds(h, false));  // synchronises
    for (int b = 0; b < B; b++) {
        long long cnt = h->mirror_h[b].log_count;
        long long have = cnt < n_z ? cnt : n_z;
        for (int j = 0; j < n_z - have; j++) {
            ekf_decision *dst = out + (size_t)b * n_z + j;
            dst->decision = 0, dst->matched = 0, dst->mahal = 0;
        }
        for (long long j = 0; j < have; j++) {
            long long idx = cnt - have + j;
            ekf_decision *dst = out + (size_t)b * n_z + (n_z - have + j);
            if (cnt - idx <= EKF_MIRROR_DECISIONS) *dst = h->mirror_h[b].last[idx % EKF_MIRROR_DECISIONS];  // still in the host mirror
            else HIP_TRY(hipMemcpy(dst, h->dv.log + (size_t)b * h->dv.logcap + (idx % h->dv.logcap), sizeof(ekf_decision), hipMemcpyDeviceToHost));
        }
    }
    return EKF_OK;
}

extern "C" int ekf_get_decisions(ekf_handle h, int index, ekf_decision *out, int count) {
    if (!filter_ok(h, index) || !out || count < 0) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    long long cnt;
    HIP_TRY(hipMemcpyAsync(&cnt, h->dv.log_count + index, sizeof cnt, hipMemcpyDeviceToHost, h->s_chain));
    HIP_TRY(stream_wait(h->s_chain));
    long long avail = cnt < h->dv.logcap ? cnt : h->dv.logcap;
    long long n = count < avail ? count : avail;
    std::vector<ekf_decision> ring(h->dv.logcap);
    HIP_TRY(hipMemcpy(ring.data(), h->dv.log + (size_t)index * h->dv.logcap, sizeof(ekf_decision) * h->dv.logcap, hipMemcpyDeviceToHost));
    for (long long j = 0; j < n; j++) out[j] = ring[(size_t)((cnt - n + j) % h->dv.logcap)];
    return (int)n;
}

extern "C" int ekf_get_stats(ekf_handle h, ekf_stats *out) {
    if (!h || !out) return set_error(EKF_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    if (h->mirror_by_chain && h->stats_in_mirror && h->chain_seq > 0) {
        // the newest chain launch copies every filter's counters into the host-mapped mirror: no device-to-host copy
        // (a copy into pageable memory costs 40-100 us, a sizeable part of a short run)
        EKF_TRY(refresh_bounds(h, false));
        for (int b = 0; b < h->dv.B; b++) out[b] = h->mirror_h[b].stats;
        return EKF_OK;
    }
    HIP_TRY(hipMemcpyAsync(out, h->dv.stats, sizeof(ekf_stats) * h->dv.B, hipMemcpyDeviceToHost, h->s_chain));
    HIP_TRY(stream_wait(h->s_chain));
    return EKF_OK;
}

extern "C" int ekf_stats_means_device(ekf_handle h, double *out_device) {
    if (!h || !out_device) return set_error(EKF_ERR_BAD_ARG, "null argument");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, out_device) != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
        (void)hipGetLastError();
        return set_error(EKF_ERR_BAD_ARG, "ekf_stats_means_device wants device memory");
    }
    hipLaunchKernelGGL(k_stats_means, dim3(cdiv(h->dv.B, 256)), dim3(256), 0, h->s_chain, (const ekf_stats *)h->dv.stats, h->dv.B, out_device);
    HIP_TRY(stream_wait(h->s_chain));
    return check_launch();
}

extern "C" int ekf_reset_stats(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(hipMemsetAsync(h->dv.stats, 0, sizeof(ekf_stats) * h->dv.B, h->s_chain));
    h->stats_in_mirror = false;  // until the next chain launch writes the mirror
    return EKF_OK;
}

// ---- dense state injection / extraction -----------------------------------------------------------
// The end of a staged dense read-back, behind the export kernel on the chain stream: stage = an n x n matrix and, behind it, n
// entries of x.  x_out (null: there is no x) and P_out, with the caller's leading dimension, are filled and waited for.
static int read_back_dense(ekf_batch *h, const double *stage, int n, double *x_out, double *P_out, int ld) {
    hipStream_t s = h->s_chain;
    if (x_out) HIP_TRY(hipMemcpyAsync(x_out, stage + (size_t)n * n, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpy2DAsync(P_out, (size_t)ld * sizeof(double), stage, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(s));
    return EKF_OK;
}

extern "C" int ekf_get_state(ekf_handle h, int index, double *x_out, double *P_out, int ld) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    int n = 3 + 2 * h->h_int[index];
    if (!x_out && !P_out) return n;  // (the size alone: nothing is folded)
    if (!x_out || !P_out || ld < n) return set_error(EKF_ERR_BAD_ARG, "bad output buffers");
    EKF_TRY(settle(h));
    DevTmp<double> stage;  // transient staging: dense n x n + x
    HIP_TRY(stage.alloc((size_t)n * n + n));
    hipLaunchKernelGGL(k_export, dim3(cdiv(n, 256), n), dim3(256), 0, h->s_chain, h->dv, index, h->win.buf_in, stage.p + (size_t)n * n, stage.p, n, n);
    EKF_TRY(read_back_dense(h, stage.p, n, x_out, P_out, ld));
    return n;  // (a failed launch of k_export is not looked for here, as it is in ekf_get_submap)
}

// Both streams are idle here (quiesce(QUIET_SETTLED)).  A launch that gave up (EKF_ERR_TIMEOUT) leaves the segment counters ahead
// of the host's bases (workgroups that had not aborted kept counting, open_gates raised the rest) and possibly a pass that never
// reported: every later stream gate would open early, every later in-kernel wait would run out again.  Start both from zero / from
// the host's own count, so that a handle is usable again after ekf_set_state (and ekf_extract_map into it), as the sticky status
// promises.
static int restart_waits(ekf_batch *h) {
    EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    read_debug_hooks(h);
    HIP_TRY(hipMemsetAsync(dv.seg_count, 0, sizeof(unsigned long long) * EKF_PLAN_MAX, s));
    for (int q = 0; q < EKF_PLAN_MAX; q++) h->win.seg_count_base[q] = 0;
    h->win.open_set_gate = 0;
    if (h->overlap) hipLaunchKernelGGL(k_mark, dim3(1), dim3(64), 0, s, dv.pass_flag, h->win.pass_seq);
    return EKF_OK;
}

extern "C" int ekf_set_state(ekf_handle h, int index, const double *x, const double *P, int ld, int n) {
    if (!filter_ok(h, index) || !x || !P || n < 3 || ((n - 3) & 1) || ld < n) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    int N = (n - 3) / 2;
    if (N > h->dv.Ncap) return set_error(EKF_ERR_CAPACITY, "state larger than capacity_landmarks");
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_NONE));
    EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    EKF_TRY(restart_waits(h));
    DevTmp<double> stage;
    HIP_TRY(stage.alloc((size_t)n * n + n));
    double *xd = stage.p + (size_t)n * n;
    HIP_TRY(hipMemcpyAsync(xd, x, sizeof(double) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpy2DAsync(stage.p, (size_t)n * sizeof(double), P, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, s));
    for (const DevArray &a : device_arrays(h)) {
        if (!(a.ops & AR_CLEAR)) continue;
        HIP_TRY(hipMemsetAsync(a.at(index), 0, a.filter_bytes(), s));
        if (a.slot == (void **)&dv.Bm[0] && h->overlap) HIP_TRY(hipMemsetAsync(dv.Bm[1] + (size_t)index * dv.bm_stride, 0, sizeof(double) * dv.bm_stride, s));
    }
    hipLaunchKernelGGL(k_import, dim3(cdiv(n, 256), n), dim3(256), 0, s, dv, index, h->win.buf_in, (const double *)xd, (const double *)stage.p, n, n);
    if (N > h->n_lm_hi) h->n_lm_hi = N;
    return finish_rewrite(h, index, 1, /*rearm*/ false, &N, 1, /*flip_buf*/ false);
}

// Grow a handle's landmark capacity (the reference grows x and P with every New landmark, Update.cpp:158-177 /
// kalmanfilter.cpp:78-84, and never fails).  A second set of device buffers of the larger capacity is built, every filter's state
// moves over on the device (k_export into a dense staging matrix, k_import from it: the tile numbering depends on the capacity),
// the counters, the decision log and a loaded script move with it, and the handle keeps its address.
static int reserve_move_state(ekf_batch *h, ekf_batch *nh, const std::vector<int> &n_lm);
static int map_scratch_rebuild(ekf_batch *h, const MapKept &old);  // (ekf_map_api.hip)

extern "C" int ekf_reserve(ekf_handle h, int capacity_landmarks) {
    if (!h || capacity_landmarks < 1 || capacity_landmarks > EKF_MAX_CAPACITY) return set_error(EKF_ERR_BAD_ARG, "bad handle / capacity (EKF_MAX_CAPACITY)");
    if (capacity_landmarks <= h->dv.Ncap) return EKF_OK;
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_NONE));  // every deferred slot folded, both streams idle
    int rc = refresh_bounds(h);  // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT (invalid state) ends it here
    if (rc == EKF_ERR_TIMEOUT) return rc;
    const int B = h->dv.B;
    std::vector<int> n_lm(h->h_int.begin(), h->h_int.begin() + B);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, h->device));
    // the old buffers are idle from here on and will not launch again: their CUs are free for the new handle's residency check
    const int had_claimed = h->claimed_cus, had_solo = h->solo_cus;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        g_cus_claimed[h->device] -= had_claimed;
        g_cus_solo[h->device] -= had_solo;  // (not counted twice while both sets of buffers are alive)
        h->claimed_cus = 0, h->solo_cus = 0;
    }
    ekf_batch *nh = new ekf_batch();
    nh->device = h->device;
    rc = create_impl(nh, B, capacity_landmarks, h->device, &h->params_requested, prop);
    if (rc == EKF_OK) rc = reserve_move_state(h, nh, n_lm);
    if (rc != EKF_OK) {  // the handle stays as it was, with its claim
        std::string keep = g_last_error;
        ekf_destroy(nh);
        (void)hipGetLastError();
        g_last_error = keep;
        std::lock_guard<std::mutex> lk(g_res_mu);
        g_cus_claimed[h->device] += had_claimed, g_cus_solo[h->device] += had_solo;
        h->claimed_cus = had_claimed, h->solo_cus = had_solo;
        return rc;
    }
    for (int b = 0; b < B; b++) {  // the host mirror's newest decisions and counters (ekf_get_stats / the compat shim read them there)
        memcpy(nh->mirror_h[b].last, h->mirror_h[b].last, sizeof nh->mirror_h[b].last);
        nh->mirror_h[b].stats = h->mirror_h[b].stats;
    }
    nh->stats_in_mirror = h->stats_in_mirror;
    nh->n_lm_hi = h->n_lm_hi;
    nh->prof_flush = h->prof_flush;
    // What a caller may hold across the growth keeps working: an open timer (events are time stamps: t0 recorded on the old buffers'
    // stream pairs with a t1 recorded later), the dense-pass profile collected so far (event pairs and sums), and the stream
    // ekf_stream() handed out -- both chain streams are idle here, so the two handles simply trade them (and every alias of them).
    std::swap(nh->t0, h->t0);
    std::swap(nh->t1, h->t1);
    nh->prof_pool.swap(h->prof_pool);
    nh->prof_used = h->prof_used, h->prof_used = 0;
    nh->prof_ms = h->prof_ms, nh->prof_launches = h->prof_launches;
    nh->prof_fused_passes = h->prof_fused_passes, nh->prof_solo_pairs = h->prof_solo_pairs;
    nh->win.windows_closed = h->win.windows_closed, nh->win.last_window_slots = h->win.last_window_slots;  // (ekf_debug_windows counts since create, across growths)
    {
        const hipStream_t s_new = nh->s_chain, s_old = h->s_chain;
        if (nh->s_flush == s_new) nh->s_flush = s_old;
        if (h->s_flush == s_old) h->s_flush = s_new;
        if (!nh->s_grp.empty() && nh->s_grp[0] == s_new) nh->s_grp[0] = s_old;
        if (!h->s_grp.empty() && h->s_grp[0] == s_old) h->s_grp[0] = s_new;
        nh->s_chain = s_old, h->s_chain = s_new;
    }
    // a loaded script is laid out per (operation, filter): independent of the capacity
    std::swap(nh->script_d, h->script_d);
    nh->script_steps = h->script_steps, nh->script_M = h->script_M, nh->script_has_truth = h->script_has_truth;
    h->script_steps = 0;
    const MapKept old = h->map;  // the scratch the map operations keep follows the capacity (only which blocks it had, and how large, is read)
    std::swap(*h, *nh);  // the caller's handle now owns the larger buffers ...
    ekf_destroy(nh);     // ... and the old ones go
    EKF_TRY(map_scratch_rebuild(h, old));
    return refresh_bounds(h);
}

// ekf_reserve: every filter's state from h's settled buffers into nh's, through a dense staging matrix.
static int reserve_move_state(ekf_batch *h, ekf_batch *nh, const std::vector<int> &n_lm) {
    const int B = h->dv.B;
    int n_max = 3;
    for (int b = 0; b < B; b++) n_max = 3 + 2 * n_lm[b] > n_max ? 3 + 2 * n_lm[b] : n_max;
    {
        DevTmp<double> stage;
        HIP_TRY(stage.alloc((size_t)n_max * n_max + n_max));
        for (int b = 0; b < B; b++) {
            const int n = 3 + 2 * n_lm[b];
            double *xd = stage.p + (size_t)n * n;
            hipLaunchKernelGGL(k_export, dim3(cdiv(n, 256), n), dim3(256), 0, h->s_chain, h->dv, b, h->win.buf_in, xd, stage.p, n, n);
            HIP_TRY(stream_wait(h->s_chain));
            hipLaunchKernelGGL(k_import, dim3(cdiv(n, 256), n), dim3(256), 0, nh->s_chain, nh->dv, b, nh->win.buf_in, (const double *)xd, (const double *)stage.p, n, n);
            HIP_TRY(stream_wait(nh->s_chain));
        }
    }
    // counters, decision log (entries name state indices, which do not depend on the capacity), then the bookkeeping kernel
    // (landmark counts, host mirror: pose, count, log position; it also clears the sticky capacity status -- there is room now)
    const bool same_log = nh->dv.logcap == h->dv.logcap;
    HIP_TRY(hipMemcpyAsync(nh->dv.stats, h->dv.stats, sizeof(ekf_stats) * B, hipMemcpyDeviceToDevice, nh->s_chain));
    if (same_log) {
        HIP_TRY(hipMemcpyAsync(nh->dv.log, h->dv.log, sizeof(ekf_decision) * (size_t)B * h->dv.logcap, hipMemcpyDeviceToDevice, nh->s_chain));
        HIP_TRY(hipMemcpyAsync(nh->dv.log_count, h->dv.log_count, sizeof(long long) * B, hipMemcpyDeviceToDevice, nh->s_chain));
    }
    for (int b = 0; b < B; b++) hipLaunchKernelGGL(k_set_meta, dim3(1), dim3(64), 0, nh->s_chain, nh->dv, b, n_lm[b]);
    HIP_TRY(stream_wait(nh->s_chain));
    return check_launch();
}

extern "C" int ekf_broadcast_state(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_NONE));
    EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    const std::vector<DevArray> arrays = device_arrays(h);
    for (int b = 1; b < dv.B; b++)
        for (const DevArray &a : arrays) {
            if (!(a.ops & AR_COPY)) continue;
            if (a.slot != (void **)&dv.Bm[0]) {
                HIP_TRY(hipMemcpyAsync(a.at(b), a.at(0), a.filter_bytes(), hipMemcpyDeviceToDevice, s));
                continue;
            }
            // (the covariance tiles: the settled buffer, whichever of the two it is)
            HIP_TRY(hipMemcpyAsync(dv.Bm[h->win.buf_in] + (size_t)b * dv.bm_stride, dv.Bm[h->win.buf_in], sizeof(double) * dv.bm_stride, hipMemcpyDeviceToDevice, s));
            if (h->overlap) HIP_TRY(hipMemsetAsync(dv.Bm[h->win.buf_in ^ 1] + (size_t)b * dv.bm_stride, 0, sizeof(double) * dv.bm_stride, s));  // no stale tiles beyond the copied map
        }
    HIP_TRY(stream_wait(s));
    for (int b = 1; b < dv.B; b++) hipLaunchKernelGGL(k_set_meta, dim3(1), dim3(64), 0, s, dv, b, h->mirror_h[0].n_lm);  // also refreshes the host mirror
    h->mirror_by_chain = false;
    h->state_edits++;
    return refresh_bounds(h);
}

#include "ekf_map_api.hip"

// ---- scripts --------------------------------------------------------------------------------------
static inline int ops_per_step(const ekf_batch *h) { return 1 + h->script_M + (h->script_has_truth ? 1 : 0); }

extern "C" int ekf_script_load(ekf_handle h, int steps, int M, const double *ctrl, const double *z, const double *R,
                               const unsigned char *valid, const double *truth) {
    if (!h || steps < 1 || M < 0 || !ctrl || (M > 0 && (!z || !R))) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(stream_wait(h->s_chain));
    for (auto &g : h->graphs) hipGraphExecDestroy(g.exec);
    h->graphs.clear();
    if (h->script_d) {
        HIP_TRY(hipFree(h->script_d));
        h->script_d = nullptr;
    }
    int B = h->dv.B;
    h->script_steps = steps;
    h->script_M = M;
    h->script_has_truth = truth ? 1 : 0;
    int ops = ops_per_step(h);
    size_t count = (size_t)steps * ops * B * 8;
    std::vector<double> host(count, 0.0);
    for (int s = 0; s < steps; s++) {
        double *base = host.data() + (size_t)s * ops * B * 8;
        for (int b = 0; b < B; b++) {
            double *r = base + (size_t)b * 8;
            const double *c = ctrl + ((size_t)s * B + b) * 3;
            double Q[4];
            make_Q(h->params, c[0], Q);
            r[0] = c[0], r[1] = c[1], r[2] = c[2], r[3] = Q[0], r[4] = Q[1], r[5] = Q[2], r[6] = Q[3];
            r[7] = OP_PROP;
        }
        for (int m = 0; m < M; m++)
            for (int b = 0; b < B; b++) {
                double *r = base + ((size_t)(1 + m) * B + b) * 8;
                const double *zz = z + (((size_t)s * M + m) * B + b) * 2;
                const double *RR = R + (((size_t)s * M + m) * B + b) * 4;
                r[0] = zz[0], r[1] = zz[1], r[2] = RR[0], r[3] = RR[1], r[4] = RR[2], r[5] = RR[3];
                r[6] = 2.0;  // every scripted measurement is its own doUpdate call (slam.cpp:150-171)
                r[7] = (!valid || valid[((size_t)s * M + m) * B + b]) ? OP_MEAS : OP_SKIP_SLOT;
            }
        if (truth)
            for (int b = 0; b < B; b++) {
                double *r = base + ((size_t)(1 + M) * B + b) * 8;
                const double *t = truth + ((size_t)s * B + b) * 3;
                r[0] = t[0], r[1] = t[1], r[2] = t[2];
                r[7] = OP_TRUTH;
            }
    }
    HIP_TRY(hipMalloc((void **)&h->script_d, count * sizeof(double)));
    HIP_TRY(hipMemcpy(h->script_d, host.data(), count * sizeof(double), hipMemcpyHostToDevice));
    if (h->prof_flush) return prof_reserve(h, prof_pairs_for_script(h));
    return EKF_OK;
}

// enqueue scripted steps [s0, s0 + ns): op index = (cursor ? *cursor : 0) + k
static int enqueue_script_steps(ekf_batch *h, const int *cursor, int k_first, int ns) {
    int ops = ops_per_step(h), M = h->script_M;
    std::vector<unsigned char> consumes((size_t)ns * ops, 0);
    for (int q = 0; q < ns; q++)
        for (int m = 0; m < M; m++) consumes[(size_t)q * ops + 1 + m] = 1;
    return launch_ops(h, h->script_d, cursor, k_first, consumes.data(), ns * ops, /*defer_last_close*/ cursor == nullptr && h->overlap);
}

static int graph_block_steps(const ekf_batch *h) {
    // smallest S >= 8 whose slot count is an even multiple of maxp, so that a graph ends with an
    // empty slot set and with cur_set / buf_in back where they started
    int M = h->script_M, maxp = h->dv.maxp;
    if (M == 0) return 8;
    for (int S = 8; S <= 8 + 4 * maxp; S++)
        if ((S * M) % (2 * maxp) == 0) return S;
    return 2 * maxp;
}

extern "C" int ekf_script_run(ekf_handle h, int first_step, int n_steps, int use_graph) {
    if (!h || !h->script_d) return set_error(EKF_ERR_STATE, "no script loaded");
    if (first_step < 0 || n_steps < 0 || first_step + n_steps > h->script_steps) return set_error(EKF_ERR_BAD_ARG, "step range outside the script");
    HIP_TRY(hipSetDevice(h->device));
    h->state_edits++;
    // (a resident streaming launch takes a short run itself -- launch_ops, OP_SCRIPT -- and leaves first for everything else)
    int ops = ops_per_step(h);
    int s = first_step, end = first_step + n_steps;
    if (use_graph && !h->overlap) {  // (the two-stream pipeline is not captured: plain launches)
        int S = graph_block_steps(h);
        if (end - s >= S) {
            // a graph starts from the settled state (its predecessor in the stream has fully finished)
            EKF_TRY(close_set(h));  // (a resident streaming launch leaves here)
            GraphEntry *ge = nullptr;
            for (auto &g : h->graphs)
                if (g.steps == S && g.M == h->script_M && g.has_truth == h->script_has_truth) ge = &g;
            int save_set = h->win.cur_set, save_buf = h->win.buf_in;
            if (!ge) {
                bool prof_saved = h->prof_flush;
                int hi_saved = h->n_lm_hi;
                h->prof_flush = false;    // event pairs are not captured into graphs
                h->n_lm_hi = h->dv.Ncap;  // graphs bake grid sizes: size the dense pass for the capacity
                (void)tile_map_for(h, (2 * h->n_lm_hi + 63) / 64);  // built before the capture: the captured passes find it ready
                HIP_TRY(hipStreamBeginCapture(h->s_chain, hipStreamCaptureModeThreadLocal));
                int rc2 = enqueue_script_steps(h, h->cursor_d, 0, S);
                if (rc2 == EKF_OK && h->win.pending != 0) rc2 = set_error(EKF_ERR_STATE, "graph block does not end on an empty slot set");
                hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, h->s_chain, h->cursor_d, S * ops);
                hipGraph_t graph = nullptr;
                hipError_t e = hipStreamEndCapture(h->s_chain, &graph);
                h->prof_flush = prof_saved;
                h->n_lm_hi = hi_saved;
                if (rc2 == EKF_OK && e != hipSuccess) rc2 = set_error(EKF_ERR_HIP, "graph capture failed");
                if (rc2 == EKF_OK && (h->win.cur_set != save_set || h->win.buf_in != save_buf)) rc2 = set_error(EKF_ERR_STATE, "graph block does not restore the ping-pong state");
                GraphEntry g;
                g.steps = S, g.M = h->script_M, g.has_truth = h->script_has_truth;
                g.exec = nullptr;
                if (rc2 == EKF_OK && hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) != hipSuccess) rc2 = set_error(EKF_ERR_HIP, "hipGraphInstantiate failed");
                if (graph) hipGraphDestroy(graph);
                if (rc2) {
                    (void)hipGetLastError();
                    return rc2;
                }
                h->graphs.push_back(g);
                ge = &h->graphs.back();
            }
            int start_op = s * ops;
            HIP_TRY(hipMemcpyAsync(h->cursor_d, &start_op, sizeof(int), hipMemcpyHostToDevice, h->s_chain));
            HIP_TRY(stream_wait(h->s_chain));  // start_op is a stack variable
            while (end - s >= S) {
                HIP_TRY(hipGraphLaunch(ge->exec, h->s_chain));
                s += S;
            }
            // The captured chain launches carry the sequence numbers of the capture: a replay stores those into the host
            // mirror, so mirror.seq says nothing about which replay has finished.  Readers fall back to a stream synchronise.
            h->mirror_by_chain = false;
            h->win.pending = 0;
            h->n_lm_hi = h->dv.Ncap;  // landmarks may have been appended inside the graphs; unknown until a sync
        }
    }
    if (s < end) {
        bump_bound(h, (end - s) * h->script_M);
        EKF_TRY(enqueue_script_steps(h, nullptr, s * ops, end - s));
    }
    return check_launch();
}

// Diagnostic tick counters of EKF_CHAIN_STAMPS builds (not declared in the public header).
// (tests) windows closed since create and the slot count of the last one: how launch_ops cut a scripted run
extern "C" int ekf_debug_windows(ekf_handle h, long long *closed, int *last_slots) {
    if (!h || !closed || !last_slots) return set_error(EKF_ERR_BAD_ARG, "null argument");
    *closed = h->win.windows_closed;
    *last_slots = h->win.last_window_slots;
    return EKF_OK;
}

// (tests, bench) streaming launches started and operations posted to them since create
extern "C" int ekf_debug_stream(ekf_handle h, long long *starts, long long *ops) {
    if (!h || !starts || !ops) return set_error(EKF_ERR_BAD_ARG, "null argument");
    *starts = h->stream_starts;
    *ops = h->stream_ops;
    return h->stream_calls ? 1 : 0;
}

extern "C" int ekf_debug_stream_ring(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null argument");
    return h->sring_in_hbm ? 1 : 0;
}

extern "C" int ekf_debug_stamps(ekf_handle h, long long *out16, int reset) {
    if (!h || !out16) return EKF_ERR_BAD_ARG;
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(stream_wait(h->s_chain));
    HIP_TRY(hipMemcpy(out16, h->dv.dbg, 32 * sizeof(long long), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dv.dbg, 0, 32 * sizeof(long long)));
    return EKF_OK;
}

#ifdef EKF_CHAIN_STAMPS
// Diagnostic: wall-clock ticks (100 MHz) at which every workgroup of filter 0 published its head in each of the first 2048
// exchanges of the handle, row 64 = the moment workgroup 0's poll saw all of them.  out: [65][2048].
extern "C" int ekf_debug_exchange_trace(ekf_handle h, long long *out) {
    if (!h || !out) return EKF_ERR_BAD_ARG;
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(stream_wait(h->s_chain));
    HIP_TRY(hipMemcpy(out, h->dv.dbg + 32, (size_t)65 * 2048 * sizeof(long long), hipMemcpyDeviceToHost));
    return EKF_OK;
}
#endif

// ---- timing ---------------------------------------------------------------------------------------
extern "C" int ekf_timer_start(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(hipEventRecord(h->t0, h->s_chain));
    return EKF_OK;
}

extern "C" int ekf_timer_stop(ekf_handle h, double *ms_out) {
    if (!h || !ms_out) return set_error(EKF_ERR_BAD_ARG, "null argument");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    if (h->overlap && h->win.prev_pending > 0) HIP_TRY(hipStreamWaitEvent(h->s_chain, role_event(h, h->win.pass_done[h->win.ev_idx]), 0));  // the pass in flight counts
    HIP_TRY(hipEventRecord(h->t1, h->s_chain));
    HIP_TRY(event_wait(h->t1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->t0, h->t1));
    *ms_out = ms;
    return EKF_OK;
}

extern "C" int ekf_flush_profile(ekf_handle h, int enable) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    h->prof_flush = enable != 0;
    if (h->prof_flush) {
        HIP_TRY(hipSetDevice(h->device));
        return prof_reserve(h, prof_pairs_for_script(h));  // the pool is sized here and in ekf_script_load, not while launches are enqueued
    }
    return EKF_OK;
}

extern "C" int ekf_fused_pass(ekf_handle h) { return h && h->solo_fuse ? 1 : 0; }

extern "C" int ekf_flush_profile_read(ekf_handle h, long long *launches_out, double *total_ms_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_NONE));
    HIP_TRY(stream_wait(h->s_chain));
    if (h->overlap) HIP_TRY(stream_wait(h->s_flush));
    for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->prof_pool[i], h->prof_pool[i + 1]));
        h->prof_ms += ms;
        h->prof_launches++;
    }
    if (h->prof_fused_passes > 0) {
        // k_solo launches were timed whole: report dense passes, not launches -- the time per pass then includes the measurement
        // loop of its window (the pass is not a kernel of its own there; ekf_fused_pass() tells the caller)
        h->prof_launches = h->prof_launches - h->prof_solo_pairs + h->prof_fused_passes;
        h->prof_fused_passes = h->prof_solo_pairs = 0;
    }
    h->prof_used = 0;
    if (launches_out) *launches_out = h->prof_launches;
    if (total_ms_out) *total_ms_out = h->prof_ms;
    h->prof_launches = 0;
    h->prof_ms = 0;
    return EKF_OK;
}
