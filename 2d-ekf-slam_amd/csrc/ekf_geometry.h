// ekf_geometry.h -- the chain geometry of a handle as one pure host function.
//
// Given batch, capacity, the requested window and overlap, the LDS a workgroup may use and the tunables read from the
// environment, plan_geometry() decides how many workgroups run a filter, with how many threads and how much LDS, which kernel
// runs them and how long the window really is.  No HIP runtime call and no getenv in here: tests/cpp/geometry_check.cpp evaluates
// the function on the CPU against tests/golden/chain_geometry.csv.
#pragma once
#include <stddef.h>

#include "ekf_device.h"

// A variable of the environment that may be unset: most tunables only override a default when they are present.
struct EnvInt {
    bool set = false;
    int v = 0;
    int or_else(int dflt) const { return set ? v : dflt; }
    bool flag(bool dflt) const { return set ? v != 0 : dflt; }
};

// Everything a handle takes from the environment at ekf_*_create (ekf_api.hip: read_tunables; include/ekfslam_c.h "Tunables" and
// INTEGRATION.md list them).  Every one of them changes scheduling only, never results.
struct Tunables {
    // ---- read by plan_geometry ----
    EnvInt overlap;           // EKF_OVERLAP: overrides params.overlap
    EnvInt solo;              // EKF_SOLO=0: k_chain also for maps of up to 256 landmarks
    EnvInt chain_wgs;         // EKF_CHAIN_WGS: workgroups per filter (its presence alone keeps k_solo out)
    EnvInt solo_long_window;  // EKF_SOLO_LONG_WINDOW=0: no window longer than k_solo's cache
    EnvInt solo_fuse;         // EKF_SOLO_FUSE=0: k_flush_rb between k_solo's windows
    EnvInt chain_one;         // EKF_CHAIN_ONE=0: the general k_chain
    EnvInt chain_helpers;     // EKF_CHAIN_HELPERS: force / forbid the two helper waves
    // ---- read by the rest of the host layer (resolved: the default where the variable is unset) ----
    int solo_stagger_ticks = 3500;    // EKF_SOLO_STAGGER_US, in ticks of the 100 MHz clock
    long bm_skew_bytes = 4096;        // EKF_BM_SKEW
    bool stream_ring_host = false;    // EKF_STREAM_RING_HOST
    bool balanced_tail = true;        // EKF_BALANCED_TAIL=0: windows always close at max_pending (launch_ops)
    EnvInt chain_cus;                 // EKF_CHAIN_CUS (the default depends on the geometry)
    bool inkernel_wait = true;        // EKF_INKERNEL_WAIT
    int solo_groups = 1;              // EKF_SOLO_GROUPS
    bool flush_alternate = true;      // EKF_FLUSH_ALTERNATE: dense passes walk the tiles alternately first-to-last and last-to-first
    bool persist = true;              // EKF_PERSIST
    bool stream = true;               // EKF_STREAM
    bool xcd_map = true;              // EKF_XCD_MAP
    bool batch_interleave = true;     // EKF_BATCH_INTERLEAVE: batches run a filter's dense-pass workgroups on one XCD
    bool overlap_serial = false;      // EKF_OVERLAP_SERIAL present (experiment: no concurrency between pass and chain)
    int solo_fuse_stagger_ticks = 0;  // EKF_SOLO_FUSE_STAGGER_US (experiment)
    bool inline_rec = true;           // EKF_INLINE_REC (read once per process)
};

struct ChainGeometry {
    int error = 0;                // EKF_OK, or the status ekf_*_create returns ...
    const char *what = nullptr;   // ... with this text
    bool overlap = false;         // a window's dense pass runs beside the next window's chain kernels
    int max_pending = 0;          // the effective window (ekf_window())
    int cache_slots = 0;          // slots of own rows in LDS (EkfDev::vs_cap)
    bool solo = false, solo_kernel = false, solo_long = false, solo_fuse = false;  // (ekf_batch, ekf_api.hip)
    int chain_wgs = 0;            // workgroups per filter (EkfDev::gmax)
    int chain_filters = 0;        // filters per chain launch
    int chain_threads = 0;
    size_t chain_lds = 0;         // dynamic LDS of a chain launch: the own-row cache
    bool chain_one = false;       // k_chain<true>
    int lpw = 0, hpw = 0, nrec = 0;                      // EkfDev fields of the same names
    int T = 0, xs = 0, dn = 0, rows = 0, maxpairs = 0;
    size_t bm_stride = 0, f_stride = 0;
};

// LDS the chain kernels may use for their own-row cache (k_chain's static LDS: 16.2 KB); also what
// hipFuncAttributeMaxDynamicSharedMemorySize is set to for every chain kernel.
static inline long chain_lds_budget(size_t lds_per_block) { return (long)lds_per_block - 16384; }

static inline ChainGeometry plan_geometry(int batch, int capacity_landmarks, const ekf_params &params, size_t lds_per_block, const Tunables &tn) {
    ChainGeometry g;
    int maxp = params.max_pending;
    if (maxp < 1) maxp = 1;
    if (maxp > EKF_MAX_PENDING) maxp = EKF_MAX_PENDING;
    g.T = (2 * capacity_landmarks + 63) / 64;
    g.xs = ((3 + 64 * g.T) + 63) / 64 * 64;
    g.dn = 32 * g.T;
    g.bm_stride = (size_t)g.T * (g.T + 1) / 2 * 4096;
    g.rows = 64 * g.T;
    // k_chain geometry.  About one landmark per worker thread, at most 32 workgroups per filter, and few
    // enough workgroups in total (<= 256) that all of them are resident at once: the cross-workgroup
    // barrier needs every workgroup of a filter running.  Every workgroup keeps its landmarks' rows of every
    // slot of the open window in LDS (64 bytes per landmark and slot), so landmarks-per-workgroup x window
    // must fit the CU's LDS next to the kernel's static 16 KB: more workgroups first, then a shorter window.
    const int max_workers = EKF_CHAIN_MAX_THREADS - 64;
    const long lds_budget = chain_lds_budget(lds_per_block);
    if (lds_budget < 64 * 64) {
        g.error = EKF_ERR_NO_DEVICE, g.what = "device reports too little LDS per workgroup";
        return g;
    }
    // overlap (params.overlap, EKF_OVERLAP overrides): automatic = on when two windows of every landmark's slot rows fit
    // the LDS of at most 64 resident workgroups per filter, i.e. when it does not cost window length
    int want_overlap = tn.overlap.or_else(params.overlap);
    if (want_overlap < 0) {
        int g_max = batch >= 256 ? 1 : (EKF_CHAIN_MAX_WGS < 256 / batch ? EKF_CHAIN_MAX_WGS : 256 / batch);
        if (g_max < 1) g_max = 1;
        long lpw_min = ((capacity_landmarks + g_max - 1) / g_max + 63) / 64 * 64;  // (the LDS cache is laid out in chunks of 64 landmarks)
        want_overlap = (lpw_min * maxp * 2 * 32 <= lds_budget) ? 1 : 0;
        // ... and when there is a dense pass worth hiding.  Round 4 (scripts/history/r04_geometry.py): with several windows per chain launch
        // the overlapped pipeline also saves the launch boundaries between chain kernel and pass, and wins from P_LL = 10 MB on
        // (N = 768: 39.2 k against 35.3 k steps/s in place; N = 1024: 38.5 k against 35.3 k; N = 2048: 37.8 k against 32.3 k; N = 512,
        // 4 MB: 37.6 k against 36.9 k -- a draw; the threshold is 8 MB).  The threshold was 128 MB in rounds 1-3, measured on one-window launches.
        size_t T = (2 * (size_t)capacity_landmarks + 63) / 64;
        if ((size_t)batch * (T * (T + 1) / 2) * 4096 * sizeof(double) < ((size_t)8 << 20)) want_overlap = 0;
    }
    g.overlap = want_overlap != 0;
    const int sets_in_lds = g.overlap ? 2 : 1;  // overlap: the set being folded by the dense pass in flight is still needed
    int G = (capacity_landmarks + max_workers - 1) / max_workers;
    int G_lds = (int)((((long)capacity_landmarks + 63) / 64 * 64 * maxp * sets_in_lds * 32 + lds_budget - 1) / lds_budget);
    if (G_lds > G) G = G_lds;
    // Round 4: about 64 landmarks -- ONE worker wave -- per workgroup is the fastest shape wherever the GPU has the CUs for it, up to
    // 32 workgroups per filter (fewer waves to keep in step at every barrier; N = 512: 8 workgroups 36.9 k against 3 workgroups
    // 34.4 k steps/s, N = 1024: 16 against 6: 35.3 k against 32.5 k in place, N = 2048: 32 against 16: 37.8 k against 36.3 k
    // overlapped; at N = 4096 the rule gives the 32 workgroups of 128 landmarks the LDS budget asked for already, and 64
    // workgroups of 64 were slower there: 29.7 k against 31.6 k, the dense pass loses too many CUs)
    {
        int G_pref = (capacity_landmarks + 63) / 64;
        if (G_pref > 32) G_pref = 32;
        if (G_pref > G) G = G_pref;
    }
    if (G > EKF_CHAIN_MAX_WGS) G = EKF_CHAIN_MAX_WGS;
    if (G * batch > 256) G = 256 / batch;  // (batches of more than 256 filters: one workgroup per filter, several launches)
    if (G < 1) G = 1;
    // the cache holds whole chunks of 64 landmarks per workgroup: a few more workgroups can save a whole chunk each
    // (N = 4096, window 16, two sets: 28 workgroups of 147 landmarks would need 3 chunks, 32 of 128 need 2)
    {
        auto lds_need = [&](int wgs) { return ((long)(capacity_landmarks + wgs - 1) / wgs + 63) / 64 * 64 * maxp * sets_in_lds * 32; };
        const int g_cap = batch >= 256 ? 1 : (EKF_CHAIN_MAX_WGS < 256 / batch ? EKF_CHAIN_MAX_WGS : 256 / batch);
        while (G < g_cap && lds_need(G) > lds_budget) G++;
    }
    // One workgroup per filter and one slot set ("solo").  Maps of up to 256 landmarks whose window fits one CU's LDS are run by
    // k_solo (ekf_solo.hip): one landmark per thread, no control wave, no exchange, one barrier per measurement.  EKF_SOLO=0
    // keeps k_chain for them (A/B comparisons, tests of k_chain's one-workgroup path).
    const bool want_solo_kernel = !g.overlap && tn.solo.flag(true) && !tn.chain_wgs.set;
    // (k_solo runs windows of up to twice what its cache holds -- ekf_solo.hip, SOLO_HALF -- so 16 slots of cache are enough for any window)
    if (want_solo_kernel && capacity_landmarks <= 256 &&
        ((long)capacity_landmarks + 63) / 64 * 64 * (maxp > 2 * 16 ? maxp : (maxp > 16 ? 16 : maxp)) * 32 <= lds_budget) G = 1;
    if (tn.chain_wgs.set && tn.chain_wgs.v > 0) G = tn.chain_wgs.v;
    if (G > EKF_CHAIN_MAX_WGS) G = EKF_CHAIN_MAX_WGS;
    if (G * batch > 256) G = 256 / batch > 0 ? 256 / batch : 1;
    g.solo = !g.overlap && G == 1;
    g.solo_kernel = g.solo && want_solo_kernel && capacity_landmarks <= 256;
    g.chain_wgs = G;
    g.chain_filters = batch * G <= 256 ? batch : 256 / G;  // every workgroup of a launch resident at once
    g.lpw = (capacity_landmarks + G - 1) / G;
    const long lpw64 = ((long)g.lpw + 63) / 64 * 64;  // the own-row cache holds whole chunks of 64 landmarks
    int cache_slots = maxp * sets_in_lds;  // slots of own rows in LDS
    if (lpw64 * maxp * sets_in_lds * 32 > lds_budget) {
        const bool two_halves = g.solo_kernel && lds_budget / (lpw64 * 32) >= 16 && tn.solo_long_window.flag(true);
        if (two_halves) {
            // k_solo: the window's first 16 slots move into registers when the cache is full (ekf_solo.hip: SOLO_HALF): a window of
            // up to 32 with 16 slots of cache -- one dense pass per 32 measurements for a map of 256 landmarks
            if (maxp > 32) maxp = 32;
            cache_slots = 16;
        } else {
            maxp = (int)(lds_budget / (lpw64 * sets_in_lds * 32));
            if (maxp > 1) maxp &= ~1;  // whole slot pairs
            cache_slots = maxp * sets_in_lds;
        }
    }
    if (maxp < 1) {
        g.error = EKF_ERR_BAD_ARG, g.what = "capacity too large for this batch size (one window slot does not fit LDS)";
        return g;
    }
    g.max_pending = maxp;
    g.maxpairs = (maxp + 1) / 2;
    g.f_stride = (size_t)(g.maxpairs + 1) * g.rows * 4;
    g.cache_slots = cache_slots;
    g.solo_long = g.solo_kernel && maxp > cache_slots;
    // (the tile of the in-kernel pass lives in a128..a255 -- the registers of a long window's first half, free otherwise --, the A operands of
    // a tile row in the own-row cache, dead while the pass runs: 2 KiB per pair and wave -- 8 or 16 pairs -- against 2 KiB per cached slot)
    g.solo_fuse = g.solo_kernel && cache_slots >= ((((maxp + 1) >> 1) + 7) & ~7) && tn.solo_fuse.flag(true);
    g.chain_lds = (size_t)lpw64 * cache_slots * 32;
    int workers = (g.lpw + 63) / 64 * 64;
    if (workers > max_workers) workers = max_workers;
    if (g.lpw > 64 && g.lpw <= 128) workers = 192;  // two owner waves and a third that shares their fold (k_chain: helper_on)
    // one owner wave and two that take a third of its fold each (round 4: N = 768 / 12 workgroups 39.2 k -> 40.5 k steps/s, N = 1024 / 16:
    // 38.0 k -> 39.5 k; with 32 workgroups -- N = 2048 -- the two extra waves at every barrier cost more than the shorter fold gives:
    // 37.0 k -> 35.8 k, so only up to 16 workgroups)
    if (g.lpw <= 64 && G > 1 && G <= 16) workers = 192;
    // ... and, whatever the number of workgroups, where the fold is long: 48 virtual slots and more (round 5: N = 4096 as 64 workgroups of 64 landmarks
    // with two windows of 32 in LDS: 36.6 k steps/s with the helper waves, 32.9 k without)
    if (g.lpw <= 64 && G > 1 && cache_slots >= 48) workers = 192;
    if (tn.chain_helpers.set && g.lpw <= 64 && G > 1) workers = tn.chain_helpers.v != 0 ? 192 : (g.lpw + 63) / 64 * 64;  // (experiments: force / forbid the two helper waves)
    g.chain_threads = 64 + workers;  // wave 0 is the control wave
    if (g.solo_kernel) g.chain_threads = (capacity_landmarks + 63) / 64 * 64;  // k_solo: one landmark per thread, no control wave
    g.hpw = (g.lpw + 63) / 64;
    g.chain_one = !g.solo_kernel && G > 1 && g.lpw <= g.chain_threads - 64 && G * g.hpw <= EKF_CHAIN_MAX_WGS && tn.chain_one.flag(true);
    if (!g.chain_one) g.hpw = 1;
    g.nrec = G * g.hpw;
    return g;
}
