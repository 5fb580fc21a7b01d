// The handle shapes and call sequences of the window-plan check, and the format of its lines.  Written against a small interface
// (Sim: one scheduler under test) so that the same sequences could be run over the text of the host layer as it was before
// csrc/ekf_window_plan.h existed -- which is how tests/golden/window_plans.txt.gz was recorded -- and are run over the header by
// window_plan_check.cpp.  A Sim has: Sim(const Shape &), ops(src, k0, consumes, nops, defer_last_close), close(terminal), settle(),
// n_lm_hi (int member) and state(); it reports through the emit_* functions below.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_device.h"

struct Shape {
    const char *name;
    int B, maxp;
    bool overlap, inkernel_wait;
    int chain_wgs, chain_filters;
    bool solo, solo_kernel, solo_fuse;
    int ngroups;
    bool persist, streams;
    bool overlap_serial, profiling, dbg_skip_flush;
    int drop_from, drop_to;
    bool residency_ok;
};
enum { SRC_RING, SRC_SCRIPT, SRC_CURSOR };  // the input ring; the loaded script; the script at the device-side cursor

static std::vector<std::string> g_lines;
__attribute__((format(printf, 1, 2))) static void emit(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_lines.push_back(buf);
}

// ---- the lines: a kind and its fields by position; these tables name them ----
static const char *const SEG_FIELDS[] = {"index", "k0", "nops", "slot0", "set", "buf_read", "n_prev", "need_pass", "drop", "seq", "gate", "self_pass", "stagger", nullptr};
static const char *const LAUNCH_FIELDS[] = {"stream", "streaming", "on_packet", "source", "nseg", "signal", "inl_n", "is_stream_plan", "b0", "nb", "start_event", "stop_event", nullptr};
static const char *const PASS_FIELDS[] = {"terminal", "do_pass", "stream", "set", "nslots", "fin", "fout", "nT_hi", "rev", "interleave", "tile_map", "gate_seq", "gate_idx", "record_chain",
                                          "wait_chain", "wait_prev", "prof", "stop", "mark", "mark_value", "record_done", "wait_done_on_chain", "done", nullptr};
static const char *const GPASS_FIELDS[] = {"stream", "set", "nslots", "fin", "fout", "nT_hi", "rev", "interleave", "b0", "nb", "prof", nullptr};
static const char *const STATE_FIELDS[] = {"cur_set", "pending", "buf_in", "prev_pending", "need_pass", "pass_seq", "ev_idx", "pass_done0", "pass_done1", "chain_signalled", "open_set_gate",
                                           "open_gate_idx", "flush_dir", "windows_closed", "last_window_slots", "chain_seq", "seg_count_base", nullptr};
static const char *const *fields_of(const std::string &kind) {
    if (kind == "seg") return SEG_FIELDS;
    if (kind == "launch") return LAUNCH_FIELDS;
    if (kind == "pass") return PASS_FIELDS;
    if (kind == "gpass") return GPASS_FIELDS;
    if (kind == "state") return STATE_FIELDS;
    return nullptr;
}

// One chain launch and, in front of it, the segments of its plan.
static void emit_launch(const char *stream, bool streaming, bool on_packet, int source, const ChainPlan &plan, int b0, int nb, const char *ev0, const char *ev1) {
    if (b0 == 0)  // (the plan once: in front of the first of its launches)
        for (int q = 0; q < plan.nseg; q++) {
            const ChainSeg &s = plan.s[q];
            emit("seg %d %d %d %d %d %d %d %d %d %lld %llu %d %d", q, s.k0, s.nops, s.slot0, s.set, s.buf_read, s.n_prev, s.need_pass, s.drop, s.seq, s.gate, s.self_pass, s.stagger);
        }
    emit("launch %s %d %d %d %d %d %d %d %d %d %s %s", stream, streaming, on_packet, source, plan.nseg, plan.signal, plan.inl_n, plan.stream != 0, b0, nb, ev0, ev1);
}
static void emit_pass(bool terminal, bool do_pass, const char *stream, int set, int nslots, int fin, int fout, int nT_hi, int rev, bool interleave, bool tile_map, unsigned long long gate_seq,
                      int gate_idx, bool record_chain, bool wait_chain, const char *wait_prev, bool prof, const char *stop, bool mark, int mark_value, bool record_done,
                      bool wait_done_on_chain, const char *done) {
    emit("pass %d %d %s %d %d %d %d %d %d %d %d %llu %d %d %d %s %d %s %d %d %d %d %s", terminal, do_pass, stream, set, nslots, fin, fout, nT_hi, rev, interleave, tile_map, gate_seq, gate_idx,
         record_chain, wait_chain, wait_prev, prof, stop, mark, mark_value, record_done, wait_done_on_chain, done);
}
static void emit_group_pass(const char *stream, int set, int nslots, int fin, int fout, int nT_hi, int rev, bool interleave, int b0, int nb, bool prof) {
    emit("gpass %s %d %d %d %d %d %d %d %d %d %d", stream, set, nslots, fin, fout, nT_hi, rev, interleave, b0, nb, prof);
}
static void emit_state(int cur_set, int pending, int buf_in, int prev_pending, int need_pass, int pass_seq, int ev_idx, const char *done0, const char *done1, bool chain_signalled,
                       unsigned long long open_set_gate, int open_gate_idx, int flush_dir, long long windows_closed, int last_window_slots, long long chain_seq,
                       const unsigned long long *seg_count_base) {
    std::string bases;
    for (int q = 0; q < EKF_PLAN_MAX; q++) bases += (q ? "," : "") + std::to_string(seg_count_base[q]);
    emit("state %d %d %d %d %d %d %d %s %s %d %llu %d %d %lld %d %lld %s", cur_set, pending, buf_in, prev_pending, need_pass, pass_seq, ev_idx, done0, done1, chain_signalled, open_set_gate,
         open_gate_idx, flush_dir, windows_closed, last_window_slots, chain_seq, bases.c_str());
}

// ---- the shapes: the smallest at which each branch exists ----
static std::vector<Shape> all_shapes() {
    std::vector<Shape> v;
    //            name                 B  maxp  ovl    ikw  wgs filt  solo   solok  fuse   ng persist streams serial prof   skip  drop     residency
    v.push_back({"inplace_multiwg",    1,  4, false, false,  8,  1, false, false, false, 1, true,  true,  false, false, false, 0, 0x7fffffff, true});
    v.push_back({"inplace_no_stream",  1,  4, false, false,  8,  1, false, false, false, 1, true,  false, false, false, false, 0, 0x7fffffff, true});
    const int windows[4] = {2, 3, 16, 32};  // (3: the odd-window clamp of the balanced tail)
    static const char *const wnames[4] = {"overlap_persist_w2", "overlap_persist_w3", "overlap_persist_w16", "overlap_persist_w32"};
    for (int k = 0; k < 4; k++) v.push_back({wnames[k], 1, windows[k], true, true, 32, 1, false, false, false, 1, true, true, false, false, false, 0, 0x7fffffff, true});
    v.push_back({"overlap_event_wait",  1,  4, true,  false, 32,  1, false, false, false, 1, true,  true,  false, false, false, 0, 0x7fffffff, true});
    v.push_back({"overlap_serial",      1,  4, true,  true,  32,  1, false, false, false, 1, true,  true,  true,  false, false, 0, 0x7fffffff, true});
    v.push_back({"solo_fused_batch",   16,  4, false, false,  1, 16, true,  true,  true,  1, true,  false, false, false, false, 0, 0x7fffffff, true});
    v.push_back({"solo_fused_one",      1,  4, false, false,  1,  1, true,  true,  true,  1, true,  true,  false, false, false, 0, 0x7fffffff, true});
    v.push_back({"solo_grouped",       16,  4, false, false,  1, 16, true,  true,  false, 4, true,  false, false, false, false, 0, 0x7fffffff, true});
    v.push_back({"one_wg_chain",        4,  4, false, false,  1,  4, true,  false, false, 1, true,  false, false, false, false, 0, 0x7fffffff, true});
    v.push_back({"several_launches",    8,  4, false, false,  4,  3, false, false, false, 1, true,  false, false, false, false, 0, 0x7fffffff, true});
    v.push_back({"overlap_batch_split", 8,  4, true,  true,   4,  3, false, false, false, 1, true,  false, false, false, false, 0, 0x7fffffff, true});
    v.push_back({"overlap_profiled",    1,  4, true,  true,  32,  1, false, false, false, 1, true,  true,  false, true,  false, 0, 0x7fffffff, true});
    v.push_back({"event_wait_profiled", 1,  4, true,  false, 32,  1, false, false, false, 1, true,  true,  false, true,  false, 0, 0x7fffffff, true});
    v.push_back({"solo_fused_profiled",16,  4, false, false,  1, 16, true,  true,  true,  1, true,  false, false, true,  false, 0, 0x7fffffff, true});
    v.push_back({"solo_grouped_profiled",16,4, false, false,  1, 16, true,  true,  false, 4, true,  false, false, true,  false, 0, 0x7fffffff, true});
    v.push_back({"overlap_skip_flush",  1,  4, true,  true,  32,  1, false, false, false, 1, true,  true,  false, false, true,  0, 0x7fffffff, true});
    v.push_back({"inplace_skip_flush",  1,  4, false, false,  8,  1, false, false, false, 1, true,  true,  false, false, true,  0, 0x7fffffff, true});
    v.push_back({"solo_fused_skip_flush",16,4, false, false,  1, 16, true,  true,  true,  1, true,  false, false, false, true,  0, 0x7fffffff, true});
    v.push_back({"overlap_drop_marks",  1,  4, true,  true,  32,  1, false, false, false, 1, true,  true,  false, false, false, 3, 6, true});
    v.push_back({"overlap_no_wait_value",1, 4, true,  true,  32,  1, false, false, false, 1, false, true,  false, false, false, 0, 0x7fffffff, true});
    // each overlap shape where the other handles' chain workgroups hold more than half of the GPU: persist refused
    const size_t n = v.size();
    static std::vector<std::string> names;
    names.reserve(n);
    for (size_t k = 0; k < n; k++)
        if (v[k].overlap) {
            Shape s = v[k];
            names.push_back(std::string(s.name) + "_crowded");
            s.name = names.back().c_str(), s.residency_ok = false;
            v.push_back(s);
        }
    return v;
}

// ---- the sequences ----
// a scripted run of `steps` steps of one propagation and one measurement each, from operation k0 of the script
template <typename Sim>
static void script_run(Sim &sim, const char *what, int steps, bool capture, bool overlap) {
    std::vector<unsigned char> consumes((size_t)2 * steps, 0);
    for (int q = 0; q < steps; q++) consumes[2 * q + 1] = 1;
    emit("call script %s steps=%d capture=%d", what, steps, capture);
    sim.ops(capture ? SRC_CURSOR : SRC_SCRIPT, capture ? 0 : 10, consumes.data(), 2 * steps, /*defer_last_close*/ !capture && overlap);
    sim.state();
}
template <typename Sim>
static void one_op(Sim &sim, int k, bool measurement) {
    const unsigned char consumes = measurement ? 1 : 0;
    emit("call op k=%d consumes=%d", k, consumes);
    sim.ops(SRC_RING, k, &consumes, 1, false);
    sim.state();
}
template <typename Sim>
static void do_settle(Sim &sim) {
    emit("call settle");
    sim.settle();
    sim.state();
}
template <typename Sim>
static void do_close(Sim &sim, bool terminal) {
    emit("call %s", terminal ? "flush" : "close_window");
    sim.close(terminal);
    sim.state();
}

template <typename Sim>
static void run_shape(const Shape &sh) {
    emit("shape %s B=%d maxp=%d overlap=%d inkernel_wait=%d chain_wgs=%d chain_filters=%d solo=%d solo_kernel=%d solo_fuse=%d ngroups=%d persist=%d streams=%d serial=%d profiling=%d "
         "skip_flush=%d drop_marks=%d..%d residency_ok=%d",
         sh.name, sh.B, sh.maxp, sh.overlap, sh.inkernel_wait, sh.chain_wgs, sh.chain_filters, sh.solo, sh.solo_kernel, sh.solo_fuse, sh.ngroups, sh.persist, sh.streams, sh.overlap_serial,
         sh.profiling, sh.dbg_skip_flush, sh.drop_from, sh.drop_to, sh.residency_ok);
    Sim sim(sh);
    const int maxp = sh.maxp;
    sim.n_lm_hi = 300;
    // single operations up to and past a window, a propagation in front of every other measurement
    for (int k = 0; k < maxp + 2; k++) {
        if (k % 2 == 0) one_op(sim, 2 * k, false);
        one_op(sim, 2 * k + 1, true);
    }
    do_settle(sim);
    {  // a propagate-only call of more than EKF_CHAIN_MAX_OPS operations
        std::vector<unsigned char> none(EKF_CHAIN_MAX_OPS + 5, 0);
        emit("call propagate_only nops=%d", (int)none.size());
        sim.ops(SRC_RING, 100, none.data(), (int)none.size(), false);
        sim.state();
        do_settle(sim);
    }
    // scripted runs: exactly one window, one window plus one, strictly between one and two windows (the balanced tail), an exact
    // multiple, more than EKF_PLAN_MAX windows -- from the script, then through the cursor (the capture route)
    const int between = maxp + (maxp > 2 ? maxp / 2 + 1 : 1);
    const int runs[5] = {maxp, maxp + 1, between, 2 * maxp, (EKF_PLAN_MAX + 2) * maxp + 1};
    static const char *const names[5] = {"one_window", "window_plus_one", "between_one_and_two", "two_windows", "more_than_a_plan"};
    for (int capture = 0; capture < 2; capture++)
        for (int r = 0; r < 5; r++) {
            script_run(sim, names[r], runs[r], capture != 0, sh.overlap);
            do_settle(sim);
        }
    // two runs back to back without a settle: the second continues the first one's window and buffers
    script_run(sim, "first_of_two", between, false, sh.overlap);
    script_run(sim, "second_of_two", 2 * maxp, false, sh.overlap);
    do_settle(sim);
    // a call arriving on a window whose close was deferred: an operation, then a run
    script_run(sim, "leaves_a_full_window", maxp, false, sh.overlap);
    one_op(sim, 7, true);
    do_settle(sim);
    script_run(sim, "leaves_a_full_window", maxp, false, sh.overlap);
    script_run(sim, "onto_a_full_window", maxp + 1, false, sh.overlap);
    do_settle(sim);
    // ekf_close_window on an empty window, and on an open one
    do_close(sim, false);
    one_op(sim, 8, true);
    do_close(sim, false);
    do_settle(sim);
    // ekf_flush with a pass in flight (prev_pending > 0 in overlap mode) and without
    script_run(sim, "window_plus_one", maxp + 1, false, sh.overlap);
    do_close(sim, true);
    do_settle(sim);
    one_op(sim, 9, true);
    do_close(sim, true);
    do_close(sim, true);  // (nothing left)
    do_settle(sim);
    // a map without landmarks: no pass in place, a marker event in overlap mode
    sim.n_lm_hi = 0;
    emit("n_lm_hi 0");
    for (int k = 0; k < maxp + 1; k++) one_op(sim, 20 + k, true);
    script_run(sim, "two_windows", 2 * maxp, false, sh.overlap);
    do_close(sim, false);
    do_settle(sim);
    // a small map (fewer than eight tile rows: no tile map)
    sim.n_lm_hi = 100;
    emit("n_lm_hi 100");
    script_run(sim, "window_plus_one", maxp + 1, false, sh.overlap);
    do_settle(sim);
}
