// ekf_window_plan.h -- the window scheduler of the host layer as pure code: which window is open and what it waits for
// (WindowState), what a dense pass looks like and what it is ordered against (plan_close -> PassOrder), what a segment of a chain
// launch carries (make_segment), which route a call takes (route_call) and how a call is cut into segments, launches and passes
// (plan_ops, plan_ops_grouped, plan_stream_turn).  No HIP runtime call, no getenv and no handle in here: events and streams are
// named by role, ekf_api.hip resolves the roles and makes the calls (issue_pass, OpsSink).
// tests/cpp/window_plan_check.cpp drives all of it on the CPU against tests/golden/window_plans.txt.gz.
#pragma once
#include <assert.h>
#include <string.h>

#include "ekf_device.h"
#include "ekf_geometry.h"

// What is fixed when a handle is created or reserved (read_debug_hooks in ekf_api.hip fills it, nothing else does).
struct WindowCfg {
    int B = 1, maxp = 1;
    bool overlap = false;        // a window's dense pass runs beside the next window's chain kernels (two slot sets, two Bm buffers)
    bool inkernel_wait = false;  // chain kernels wait for their pass in-kernel, else the chain's stream waits for the pass's event
    int chain_wgs = 1, chain_filters = 1;
    bool solo = false, solo_kernel = false, solo_fuse = false;
    int ngroups = 1;
    bool persist = false;        // EKF_PERSIST and the device can gate a stream on a value: multi-segment launches are possible
    bool balanced_tail = true, flush_alternate = true, batch_interleave = true, overlap_serial = false, xcd_map = true, inline_rec = true;
    int solo_fuse_stagger_ticks = 0;
    bool dbg_skip_flush = false;  // (debug variant only, as the next two)
    int dbg_drop_marks_from = 0, dbg_drop_marks_to = 0x7fffffff;
};

enum EvRole { EV_NONE, EV_CHAIN, EV_FLUSH0, EV_FLUSH1, EV_PROF0, EV_PROF1 };  // EV_PROFi: the stop event of the profiling pair taken by the pass that stands in slot i
enum StreamRole { ON_CHAIN, ON_FLUSH };

// Which window is open and what it waits for.
struct WindowState {
    int cur_set = 0;       // slot set being filled
    int pending = 0;       // slots used in cur_set
    int buf_in = 0;        // Bm buffer the chain kernels read (complete up to the sets still open or in flight)
    int prev_pending = 0;  // overlap: slots of the other set whose dense pass has been launched but is not in Bm[buf_in]
    int need_pass = 0;     // the pass the next chain launches have to wait for in-kernel, 0 = none
    int pass_seq = 0;      // dense passes launched so far (overlap mode); k_mark stores it into dv.pass_flag behind each pass
    int ev_idx = 0;        // slot ev_idx belongs to the dense pass launched last
    EvRole pass_done[2] = {EV_NONE, EV_NONE};  // completion of the pass of slot i: ev_flush[i] itself, or, while passes are profiled, that pass's stop event
    bool chain_signalled = false;          // the last chain launch carried ev_chain as its stop event
    unsigned long long open_set_gate = 0;  // != 0: the open set was filled by segment open_gate_idx of a multi-segment launch: dv.seg_count[open_gate_idx] >= this opens its pass
    int open_gate_idx = 0;
    int flush_dir = 0;  // direction of the next dense pass (0 = first to last; flush_alternate)
    unsigned long long seg_count_base[EKF_PLAN_MAX] = {};  // value dv.seg_count[i] reaches when every multi-segment launch enqueued so far has finished
    long long windows_closed = 0;  // windows counted by turn_window since create (ekf_debug_windows)
    int last_window_slots = 0;     // ... and the slots of the last one
};

// A window turns over: the chain continues into the other slot set.  The only text that flips cur_set and zeroes pending.
// counted: the window shows in windows_closed / last_window_slots; pass_ran: a dense pass consumed a direction.
// As found, and kept value for value: every window handed to a pass by plan_close is counted, and so is a window that a STREAMING
// k_solo launch folds itself (plan_stream_turn) -- but a window folded by a segment of a fused k_solo launch (plan_ops) and a
// window of the grouped path (plan_ops_grouped) is not.  Whether that difference is meant is not known.
inline void turn_window(WindowState &st, bool counted, bool pass_ran) {
    if (pass_ran) st.flush_dir ^= 1;
    if (counted) st.windows_closed++, st.last_window_slots = st.pending;
    st.cur_set ^= 1;
    st.pending = 0;
}

// Everything one dense pass needs, and what it is ordered against.  nslots == 0: there is no order (the window was empty).
struct PassOrder {
    bool terminal, do_pass;  // do_pass false: no kernel (an empty map in overlap mode leaves a marker event; a skipped pass)
    StreamRole on;           // the pass's stream (the chain's own for a terminal pass)
    int set, nslots, fin, fout, nT_hi, rev;
    bool interleave, want_tile_map;
    unsigned long long gate_seq;  // != 0: the pass's stream waits until dv.seg_count[gate_idx] >= gate_seq
    int gate_idx;
    bool record_chain, wait_chain;  // ev_chain is recorded on the chain's stream; the pass's stream waits for it
    EvRole wait_prev;               // the chain's stream waits for this (terminal: in front of the pass, else behind it)
    bool prof;                      // the pass takes a profiling pair (the pair's stop event then is its stop event)
    EvRole stop;                    // ... else the stop event on its dispatch packet
    bool mark;                      // k_mark stores mark_value into dv.pass_flag behind the pass
    int mark_value;
    bool record_done, wait_done_on_chain;  // `done` is recorded behind the pass (a marker: no kernel carries it); the chain's stream waits for it
    EvRole done;
};

// Close the slot set being filled and hand it to a dense pass; the chain continues into the other set.
//  * without overlap: the pass folds the set into Bm in place, in stream order behind the chain kernels.
//  * with overlap: pass k runs on its own stream, Bm[fin] -> Bm[fin ^ 1], while the chain kernels of window
//    k+1 read Bm[fin] and fold set k themselves (n_prev).  Pass k starts after the chain kernels of window k
//    (ev_chain) and, by stream order, after pass k-1 whose output it reads; the chain kernels of window k+1
//    start after pass k-1 (they read its output and overwrite the slot rows it read).
inline PassOrder plan_close(const WindowCfg &cfg, WindowState &st, bool terminal, int n_lm_hi, bool profiling) {
    PassOrder o;
    memset(&o, 0, sizeof o);
    if (st.pending == 0) return o;
    int nT_hi = (2 * n_lm_hi + 63) / 64;
    const int fin = (cfg.overlap && st.prev_pending > 0) ? st.buf_in ^ 1 : st.buf_in;
    // terminal: the caller asked for everything to be folded (ekf_flush, settle), so no chain kernel will run beside this
    // pass.  It then goes out on the chain's own stream (no cross-stream event hop: ~16 us, no k_mark: ~9 us), on all CUs,
    // and in place (the faster form when nothing else uses the memory system); the pipeline restarts empty afterwards.
    terminal = terminal && cfg.overlap;
    o.terminal = terminal;
    o.on = terminal ? ON_CHAIN : ON_FLUSH;
    o.fin = fin, o.fout = (cfg.overlap && !terminal) ? fin ^ 1 : fin;
    // What the pass waits for.  A set filled by a segment of a multi-segment chain launch: the value dv.seg_count shows when
    // every workgroup has finished that segment (a stream gate: the kernel is still running).  Otherwise the chain launch's event.
    o.gate_seq = terminal ? 0 : st.open_set_gate;
    o.gate_idx = st.open_gate_idx;
    st.open_set_gate = 0;
    if (terminal) {
        if (st.prev_pending > 0) o.wait_prev = st.pass_done[st.ev_idx];  // pass k-1 wrote Bm[fin]
    } else if (cfg.overlap) {
        if (!o.gate_seq) o.record_chain = !st.chain_signalled, o.wait_chain = true;
    }
    if (cfg.overlap) st.chain_signalled = false;
    o.do_pass = !cfg.dbg_skip_flush && (nT_hi > 0 || cfg.overlap);
    o.nT_hi = nT_hi < 1 ? 1 : nT_hi;
    if (o.do_pass && cfg.overlap && !terminal) o.stop = st.ev_idx ? EV_FLUSH0 : EV_FLUSH1;  // pass k's completion, signalled by its own dispatch packet
    o.prof = o.do_pass && profiling;  // (the pair's stop event doubles as the pass's completion event)
    // Passes alternate direction: a pass starts on the tiles the previous pass touched last, which are the ones the
    // 256 MB Infinity Cache still holds (P_LL of N=4096 is 270 MB per buffer: walked the same way every time, the
    // cache has evicted a tile long before the next pass comes back to it).
    o.rev = cfg.flush_alternate ? st.flush_dir : 0;
    o.interleave = cfg.B > 1 && cfg.batch_interleave;  // a filter's workgroups on one XCD
    o.want_tile_map = o.do_pass && !o.interleave && cfg.B == 1 && cfg.xcd_map && o.nT_hi >= 8;  // (small maps: nothing to share)
    o.set = st.cur_set, o.nslots = st.pending;
    if (terminal) {
        st.need_pass = 0;
        st.buf_in = fin;
        st.prev_pending = 0;
    } else if (cfg.overlap) {
        // the chain kernels of the next window depend on pass k-1 (they read its output and overwrite the slot rows it
        // read): they wait for its number in dv.pass_flag themselves
        // ... or, where kernels of two streams do not run side by side, the stream waits for the pass's event
        if (cfg.inkernel_wait) {
            st.need_pass = st.prev_pending > 0 ? st.pass_seq : 0;  // pass_seq still names pass k-1 here
        } else {
            st.need_pass = 0;
            if (st.prev_pending > 0) o.wait_prev = st.pass_done[st.ev_idx];  // pass k-1, awaited by the chain's stream
        }
        o.mark = true, o.mark_value = ++st.pass_seq;  // pass k
        if (cfg.dbg_drop_marks_from > 0 && o.mark_value >= cfg.dbg_drop_marks_from && o.mark_value < cfg.dbg_drop_marks_to) o.mark = false;  // (test hook of the debug variant: a pass that never reports)
        st.ev_idx ^= 1;  // pass_done[ev_idx] is pass k's completion: ev_flush[ev_idx] as its stop event, or the profiling pair's stop event
        o.done = o.prof ? (st.ev_idx ? EV_PROF1 : EV_PROF0) : (st.ev_idx ? EV_FLUSH1 : EV_FLUSH0);
        o.record_done = !o.do_pass;  // (no pass kernel to carry the event: a marker)
        st.pass_done[st.ev_idx] = o.done;
        o.wait_done_on_chain = cfg.overlap_serial;  // experiment: no concurrency
        st.buf_in = fin;
        st.prev_pending = st.pending;
    }
    turn_window(st, /*counted*/ true, /*pass_ran*/ o.do_pass);
    return o;
}

// settle, behind the terminal pass and with both streams idle: the last overlapped pass's output is the settled buffer.
inline void land_last_pass(const WindowCfg &cfg, WindowState &st) {
    if (cfg.overlap && st.prev_pending > 0) st.buf_in ^= 1, st.prev_pending = 0;
}

// One segment of a chain launch on the open window.  n_prev, need_pass: the state's (st.prev_pending, st.need_pass), or zeros for
// launches that run in place behind their passes (the grouped path).
inline ChainSeg make_segment(const WindowState &st, int k0, int nops, long long seq, int n_prev, int need_pass, int drop, unsigned long long gate, bool self_pass) {
    ChainSeg sg;
    memset(&sg, 0, sizeof sg);
    sg.k0 = k0, sg.nops = nops, sg.slot0 = st.pending, sg.set = st.cur_set, sg.buf_read = st.buf_in;
    sg.n_prev = n_prev, sg.need_pass = need_pass, sg.drop = drop;
    sg.seq = seq, sg.gate = gate, sg.self_pass = self_pass ? 1 : 0, sg.stagger = 0;
    return sg;
}
// a one-workgroup filter run by k_solo folds the windows it fills itself (ChainSeg::self_pass), in a streaming launch too
inline bool folds_itself(const WindowCfg &cfg) { return cfg.solo_kernel && cfg.solo_fuse && !cfg.dbg_skip_flush; }

// Advance *i over operations until the window holds `limit` slots or EKF_CHAIN_MAX_OPS operations have been taken; `used` slots are
// taken already.  Returns the slots used afterwards (consumes[q] != 0: operation q takes a slot).
inline int take_ops(const unsigned char *consumes, int nops, int *i, int used, int limit) {
    const int start = *i;
    while (*i < nops && *i - start < EKF_CHAIN_MAX_OPS) {
        if (consumes[*i]) {
            if (used == limit) break;
            used++;
        }
        (*i)++;
    }
    return used;
}
inline int count_slots(const unsigned char *consumes, int nops) {
    int slots = 0;
    for (int q = 0; q < nops; q++) slots += consumes[q] ? 1 : 0;
    return slots;
}

// Where a window that begins closes, slots_left slot-consuming operations of the call ahead.
// Balanced tail (round 5; multi-workgroup filters in the overlapped multi-segment mode, EKF_BALANCED_TAIL=0 switches it off): when between one
// and two windows' worth of measurements are left in this call, the window that begins is closed at HALF of them (rounded up to a whole
// slot pair) instead of at max_pending.  A scripted run of 20 steps x 4 measurements at a window of 32 ran 32 | 32 | 16: the pass of the
// second window (16 pairs, 165 us beside the chain kernel) outlasted the 16 measurements after it (100 us) and the last window's pass
// waited behind it -- 170 us exposed after the chain kernel's end; 32 | 24 | 24 hides the second pass under the third segment and leaves
// one 12-pair pass exposed.  Nothing changes for a run whose length is a multiple of the window, nor in the steady state of a long one.
inline int window_limit(const WindowCfg &cfg, bool persist, int slots_left) {
    int limit = cfg.maxp;
    if (cfg.balanced_tail && persist && !cfg.solo_kernel && slots_left > cfg.maxp && slots_left < 2 * cfg.maxp) {
        limit = ((slots_left + 1) / 2 + 1) & ~1;
        if (limit > cfg.maxp) limit = cfg.maxp;  // (an odd max_pending: rounding up to a slot pair must not pass the window -- slot_meta rows, the own-row cache and the pass are sized for maxp)
    }
    return limit;
}

// ---- which route a call takes ---------------------------------------------------------------------------------------------------
enum CallRoute { ROUTE_STREAM_OPS, ROUTE_STREAM_SCRIPT, ROUTE_GROUPED, ROUTE_LAUNCHES };
enum CallSource { FROM_RING, FROM_SCRIPT, FROM_CURSOR };  // the input ring; the loaded script; the script at the device-side cursor (graph capture)
struct CallPlan {
    CallRoute route;
    bool persist, fuse, multi;  // ROUTE_LAUNCHES: multi-segment launches with gated passes; k_solo folds its windows itself; either
};
// Scripted runs in overlap mode: the launches of one call become the segments of one launch (up to EKF_PLAN_MAX at a
// time).  The workgroups stay resident across window boundaries -- no launch gap (5 us), no refill of the LDS caches
// from memory (7 us per 16-measurement window at N = 4096) -- and the dense passes are enqueued behind stream gates that
// the running kernel opens (dv.seg_count).  Needs kernels of two streams side by side (the in-kernel pass wait's probe).
// ... and CUs on which a pass can run while the chain workgroups stay resident (the caller's residency test: only asked for where
// this says yes).
inline bool persist_possible(const WindowCfg &cfg, CallSource src, bool defer_last_close) {
    return cfg.persist && defer_last_close && src != FROM_CURSOR && cfg.overlap && cfg.inkernel_wait && cfg.chain_filters == cfg.B;
}
// streams: the handle streams its immediate-mode calls.  A window whose close an earlier call deferred has been closed by now.
inline CallPlan route_call(const WindowCfg &cfg, const WindowState &st, bool streams, CallSource src, const unsigned char *consumes, int nops, bool defer_last_close,
                           bool residency_ok) {
    CallPlan c = {ROUTE_LAUNCHES, false, false, false};
    // an immediate-mode call of a one-filter handle: its operations go to the resident streaming launch, one command each
    if (streams && src == FROM_RING && nops > 0) return c.route = ROUTE_STREAM_OPS, c;
    // A SHORT scripted chunk of a one-filter handle (ekf_script_run of a step or two: the per-step call pattern of BASELINE.json config 2's
    // latency figure): one OP_SCRIPT command to the resident launch per stretch that stays inside the open window -- at most HALF a window
    // of measurements in all: a step or two.  Whole windows and longer runs keep the multi-segment launches (their windows turn over
    // without the launch leaving, a window they fill exactly stays open for the next call -- what bench.py's timed regions and its
    // one-window `alone` runs rely on).
    if (streams && src == FROM_SCRIPT && nops > 0 && nops <= EKF_CHAIN_MAX_OPS && 2 * count_slots(consumes, nops) <= cfg.maxp) return c.route = ROUTE_STREAM_SCRIPT, c;
    c.persist = persist_possible(cfg, src, defer_last_close) && residency_ok;
    // k_solo folds a window it fills itself (ChainSeg::self_pass): the launches of one call are the segments of one launch, with
    // no dense-pass launch between them (EKF_SOLO_FUSE=0: one launch per window and k_flush_rb, for comparisons)
    c.fuse = cfg.solo_kernel && cfg.solo_fuse;
    c.multi = c.persist || c.fuse;
    // phase groups: the call closes at least two windows (scripted runs, and immediate-mode chunks that long)
    if (!c.fuse && cfg.solo && cfg.ngroups > 1 && src != FROM_CURSOR && (long)st.pending + count_slots(consumes, nops) >= 2L * cfg.maxp) c.route = ROUTE_GROUPED;
    return c;
}

// ---- a call as segments, launches and passes ------------------------------------------------------------------------------------
// How one plan goes out: a launch per chain_filters filters; the stop event rides on the last launch's dispatch packet, a fused
// k_solo launch that is profiled is bracketed by its profiling pair instead.
struct LaunchOrder {
    EvRole stop;
    bool prof;         // takes a profiling pair (the passes live inside the launch: time the launch, count the passes)
    int fused_passes;  // ... this many
};
struct ChainLaunch {
    int b0, nb;  // nb == 0: no more launches
    bool start_prof, stop_prof;  // the pair's start / stop event on this launch's packet
    EvRole stop;
};
inline ChainLaunch chain_launch(const WindowCfg &cfg, const LaunchOrder &lo, int b0) {
    ChainLaunch l = {b0, 0, false, false, EV_NONE};
    if (b0 >= cfg.B) return l;
    l.nb = cfg.B - b0 < cfg.chain_filters ? cfg.B - b0 : cfg.chain_filters;
    const bool last = b0 + l.nb >= cfg.B;
    l.start_prof = lo.prof && b0 == 0, l.stop_prof = lo.prof && last;
    l.stop = last && !lo.prof ? lo.stop : EV_NONE;
    return l;
}

// Deferred passes (multi-segment launches: a pass goes out behind the launch whose segment fills its window): at most one close per
// segment between two flushes of the plan, and the close of a window found full at the head of the loop, which can only come first.
enum { EKF_DEFER_MAX = EKF_PLAN_MAX + 1 };

struct OpsCall {
    CallSource src;
    int k0, nops;
    const unsigned char *consumes;  // consumes[i] != 0 when op i takes a slot (measurement, masked measurement, compass)
    bool defer_last_close;  // when the last segment of the call fills the set, leave the set closed-to-be: the next call closes it (regular
                            // pass) or ekf_flush / a state read does (terminal pass).  Scripted runs use it; never while capturing.
    int n_lm_hi;
    bool profiling;
};

// Cut a call into segments at slot-set boundaries.  The sink carries the decisions out (ekf_api.hip) or prints them (the check):
//   int segment(const ChainSeg &)                          a segment has been appended to the plan
//   int launch(ChainPlan &, const LaunchOrder &)           the plan goes out now
//   int pass(const PassOrder &)                            a dense pass goes out now (a deferred one: behind the launch just made)
//   int prepare(const PassOrder &)                         a pass has been deferred: what it needs built synchronously (its tile map) is built now, in front of the launch
// each returns 0 or a status that ends the call.  *chain_seq: the handle's launch counter (one number per segment: every filter's mirror reaches it).
template <typename Sink>
inline int plan_ops(const WindowCfg &cfg, WindowState &st, const CallPlan &cp, const OpsCall &c, long long *chain_seq, Sink &sink) {
    const bool persist = cp.persist, fuse = cp.fuse, multi = cp.multi;
    ChainPlan plan;
    memset(&plan, 0, sizeof plan);
    PassOrder deferred[EKF_DEFER_MAX];
    int ndeferred = 0, next_drop = 0, rc = 0;
    auto close = [&]() -> int {
        const PassOrder o = plan_close(cfg, st, false, c.n_lm_hi, c.profiling);
        if (o.nslots == 0) return 0;
        if (!persist) return sink.pass(o);
        assert(ndeferred < EKF_DEFER_MAX);
        deferred[ndeferred++] = o;
        return sink.prepare(o);
    };
    auto launch = [&](EvRole stop) -> int {
        if (plan.nseg == 0) return 0;
        // one filter, one segment of one operation, its record in the host-mapped ring (an immediate-mode call, slam.cpp:136-170): the
        // record rides in the kernel arguments -- the kernel's first trip to host memory brings it along, the ring costs a second one
        plan.inl_n = (cfg.inline_rec && cfg.B == 1 && plan.nseg == 1 && plan.s[0].nops == 1 && c.src == FROM_RING) ? 1 : 0;
        LaunchOrder lo = {stop, false, 0};
        if (fuse) {
            for (int q = 0; q < plan.nseg; q++) lo.fused_passes += plan.s[q].self_pass;
            // EKF_SOLO_FUSE_STAGGER_US: a one-off phase shift between the filters of a batch (four groups), so that their own passes take
            // turns in HBM.  Measured: nothing to gain (6.53 M filter-steps/s without, 6.51 / 6.42 / 6.35 M with 35 / 67 / 90 us: one wave
            // per SIMD is latency-bound on its own tile, not bandwidth-bound), so the default is none.
            plan.s[0].stagger = (lo.fused_passes >= 4 && cfg.B >= 16) ? cfg.solo_fuse_stagger_ticks : 0;
            lo.prof = c.profiling && lo.fused_passes > 0;
        }
        if (int r = sink.launch(plan, lo)) return r;
        if (plan.signal)
            for (int q = 0; q < plan.nseg; q++) st.seg_count_base[q] = plan.s[q].gate;
        plan.nseg = 0;
        next_drop = 0;
        const int n = ndeferred;
        ndeferred = 0;
        for (int q = 0; q < n; q++)
            if (int r = sink.pass(deferred[q])) return r;
        return 0;
    };
    int i = 0, slots_left = count_slots(c.consumes, c.nops);  // slot-consuming operations of this call from op i on
    int limit = cfg.maxp;  // where the window being filled closes (a window carried over from an earlier call: max_pending)
    while (i < c.nops) {
        const int start = i;
        if (st.pending == 0) limit = window_limit(cfg, persist, slots_left);
        const int used = take_ops(c.consumes, c.nops, &i, st.pending, limit);
        slots_left -= used - st.pending;
        if (i == start) {  // set already full (cannot happen: full sets are closed before the call is planned, and below)
            if ((rc = close())) return rc;
            continue;
        }
        if (next_drop > 0 && next_drop < st.prev_pending && (rc = launch(EV_NONE))) return rc;  // (the LDS shift moves whole windows: start a new launch instead)
        const bool fills = used == limit;
        // every workgroup of the launch has finished this segment: gate
        const ChainSeg sg = make_segment(st, c.k0 + start, i - start, ++*chain_seq, st.prev_pending, st.need_pass, next_drop,
                                         st.seg_count_base[plan.nseg] + (unsigned long long)cfg.chain_wgs * cfg.B, fuse && fills && !cfg.dbg_skip_flush);
        next_drop = 0;
        plan.s[plan.nseg++] = sg;
        plan.signal = persist ? 1 : 0;
        plan.stream = 0;
        if ((rc = sink.segment(sg))) return rc;
        st.pending = used;
        if (!multi) {
            // overlap: the launch that fills the set signals ev_chain from its own dispatch packet (no marker packet)
            const bool closes = cfg.overlap && fills;
            if ((rc = launch(closes ? EV_CHAIN : EV_NONE))) return rc;
            st.chain_signalled = closes;
        } else {
            st.chain_signalled = false;
            if (persist && fills) st.open_set_gate = sg.gate, st.open_gate_idx = plan.nseg - 1;
        }
        if (sg.self_pass) {
            turn_window(st, /*counted*/ false, /*pass_ran*/ false);  // folded by the launch itself: the next segment starts an empty window
        } else if (fills && !(c.defer_last_close && i == c.nops)) {
            if ((rc = close())) return rc;
            next_drop = sg.n_prev;  // the next segment starts a window: the set whose pass has finished leaves the LDS caches
        }
        if (multi && plan.nseg == EKF_PLAN_MAX && (rc = launch(EV_NONE))) return rc;
    }
    return launch(EV_NONE);
}

// One-workgroup filters in phase groups: every window of the call is one single-segment launch per group and, where the window
// fills, an in-place pass per group behind it (ekf_api.hip: launch_ops_grouped has the fork and the join).
struct GroupedWindow {
    ChainSeg seg;
    bool do_pass;
    int set, nslots, buf, nT_hi, rev;  // the pass: slot set, slots, Bm[buf] in place
};
// The next window of a grouped call from operation *i on; false: the call is done.
inline bool plan_ops_grouped(const WindowCfg &cfg, WindowState &st, const OpsCall &c, int *i, long long *chain_seq, GroupedWindow *w) {
    if (*i >= c.nops) return false;
    const int start = *i, used = take_ops(c.consumes, c.nops, i, st.pending, cfg.maxp);
    w->seg = make_segment(st, c.k0 + start, *i - start, ++*chain_seq, /*n_prev*/ 0, /*need_pass*/ 0, /*drop*/ 0, /*gate*/ 0, /*self_pass*/ false);
    st.pending = used;
    const bool fold = used == cfg.maxp;
    w->nT_hi = (2 * c.n_lm_hi + 63) / 64;
    w->do_pass = fold && !cfg.dbg_skip_flush && w->nT_hi > 0;
    w->rev = cfg.flush_alternate ? st.flush_dir : 0;
    w->set = st.cur_set, w->nslots = cfg.maxp, w->buf = st.buf_in;
    if (fold) turn_window(st, /*counted*/ false, /*pass_ran*/ w->do_pass);
    return true;
}
// profiling pairs a grouped call may take per group: a pass per window it fills, and one
inline long grouped_passes(const WindowCfg &cfg, const WindowState &st, const OpsCall &c) {
    long passes = 0, used = st.pending;
    for (int q = 0; q < c.nops; q++)
        if (c.consumes[q] && ++used == cfg.maxp) passes++, used = 0;
    return passes + 1;
}

// ---- streamed commands ----------------------------------------------------------------------------------------------------------
// A streaming launch on the open window: one segment without operations, consuming commands from consumed0 + 1 on.
inline ChainSeg stream_segment(const WindowCfg &cfg, WindowState &st, long long consumed0, int slot0) {
    ChainSeg sg = make_segment(st, 0, 0, /*seq: the last command consumed before this launch*/ consumed0, st.prev_pending, st.need_pass, 0, 0, folds_itself(cfg));
    sg.slot0 = slot0;
    st.chain_signalled = false;  // (the launch carries no stop event)
    return sg;
}
inline bool stream_closes(const WindowCfg &cfg, const WindowState &st, int n_slots) { return n_slots > 0 && st.pending + n_slots >= cfg.maxp; }

// The window turns over behind a streamed command that filled it (the launch has left by itself); the next window's streaming launch
// follows.  overlap: that launch goes out at once, IN FRONT of the pass's launch: a pass that is already streaming holds every CU
// its mask allows with a queue of workgroups behind them, and a chain launch that arrives later gets its 64 CUs one by one as tiles
// finish -- the first exchange then waits for the last workgroup, 100 us (seen as a bimodal p90).  Launched first, it is resident when
// the next call comes (within the idle time) and the pass takes what is left.  The event the pass waits for sits between the two.
struct StreamTurn {
    bool record_chain;     // ev_chain is recorded on the chain's stream first (behind the launch that filled the window)
    bool pass_after_start; // the pass goes out behind the next streaming launch, else in front of it (in place: on the chain's stream)
    PassOrder pass;        // nslots == 0: none (folded by the launch itself, behind the closing command)
};
inline StreamTurn plan_stream_turn(const WindowCfg &cfg, WindowState &st, int n_lm_hi, bool profiling) {
    StreamTurn t;
    memset(&t, 0, sizeof t);
    if (cfg.overlap) {
        t.record_chain = t.pass_after_start = true;
        st.chain_signalled = true;
        t.pass = plan_close(cfg, st, false, n_lm_hi, profiling);  // the state now describes the next window
    } else if (folds_itself(cfg)) {
        turn_window(st, /*counted*/ true, /*pass_ran*/ false);
    } else {
        t.pass = plan_close(cfg, st, false, n_lm_hi, profiling);
    }
    return t;
}
