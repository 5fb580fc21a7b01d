// Host-only check of the window scheduler (csrc/ekf_window_plan.h) against tests/golden/window_plans.txt.gz (the test unpacks it), which was recorded from the
// text of close_set, launch_ops, launch_ops_grouped, stream_op and settle before the header existed (the record's first line names the
// commit).  The sequences of window_plan_sequences.h are driven through the planner the way ekf_api.hip drives it; every segment,
// launch, pass order and the state after every call must agree field by field.  Independent of the record, every action is checked
// against the invariants below.   window_plan_check window_plans.txt   (or --dump: print the lines)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "../../2d-ekf-slam_amd/csrc/ekf_window_plan.h"
#include "window_plan_sequences.h"

static int g_broken = 0;
#define INVARIANT(cond)                                                                       \
    do {                                                                                      \
        if (!(cond)) printf("invariant broken at line %zu: %s\n", g_lines.size(), #cond), g_broken++; \
    } while (0)

static const char *ev_name(EvRole r) {
    static const char *const n[] = {"none", "chain", "flush0", "flush1", "prof0", "prof1"};
    return n[r];
}

struct NewSim {
    WindowCfg cfg;
    WindowState st;
    Shape sh;
    int n_lm_hi = 0;
    long long chain_seq = 0;
    bool stream_alive = false;

    explicit NewSim(const Shape &s) : sh(s) {
        cfg.B = s.B, cfg.maxp = s.maxp, cfg.overlap = s.overlap, cfg.inkernel_wait = s.inkernel_wait, cfg.chain_wgs = s.chain_wgs, cfg.chain_filters = s.chain_filters;
        cfg.solo = s.solo, cfg.solo_kernel = s.solo_kernel, cfg.solo_fuse = s.solo_fuse, cfg.ngroups = s.ngroups, cfg.persist = s.persist;
        cfg.overlap_serial = s.overlap_serial, cfg.dbg_skip_flush = s.dbg_skip_flush, cfg.dbg_drop_marks_from = s.drop_from, cfg.dbg_drop_marks_to = s.drop_to;
    }
    void check_state() { INVARIANT(st.pending >= 0 && st.pending <= cfg.maxp); }

    // ---- the sink of plan_ops ----
    int segment(const ChainSeg &sg) {
        int slots = 0;  // (the segment's operations are the call's [k0 - call_k0, ...): counted from the call's consumes)
        for (int q = 0; q < sg.nops; q++) slots += call_consumes[sg.k0 - call_k0 + q] ? 1 : 0;
        INVARIANT(sg.slot0 + slots <= cfg.maxp);
        return 0;
    }
    int launch(ChainPlan &plan, const LaunchOrder &lo) {
        deferred = 0;  // (they go out behind this launch)
        for (ChainLaunch l = chain_launch(cfg, lo, 0); l.nb > 0; l = chain_launch(cfg, lo, l.b0 + l.nb))
            emit_launch("chain", false, true, call_src, plan, l.b0, l.nb, l.start_prof ? "pair" : "none", l.stop_prof ? "pair" : ev_name(l.stop));
        return 0;
    }
    int deferred = 0;  // passes waiting behind the launch that has not been made yet
    int prepare(const PassOrder &) {
        INVARIANT(++deferred <= EKF_DEFER_MAX);
        return 0;
    }
    int pass(const PassOrder &o) {
        if (o.nslots == 0) return 0;
        INVARIANT((o.fin | 1) == 1 && (o.fout | 1) == 1 && (o.set | 1) == 1);
        INVARIANT((o.fout == o.fin) == (!cfg.overlap || o.terminal));
        emit_pass(o.terminal, o.do_pass, o.on == ON_CHAIN ? "chain" : "flush", o.set, o.nslots, o.fin, o.fout, o.nT_hi, o.rev, o.interleave, o.want_tile_map, o.gate_seq, o.gate_idx,
                  o.record_chain, o.wait_chain, ev_name(o.wait_prev), o.prof, o.prof ? "pair" : ev_name(o.stop), o.mark, o.mark_value, o.record_done, o.wait_done_on_chain, ev_name(o.done));
        check_state();
        return 0;
    }

    // ---- the entry points, as ekf_api.hip has them ----
    void close(bool terminal) {
        stream_alive = false;  // (stream_stop)
        pass(plan_close(cfg, st, terminal, n_lm_hi, sh.profiling));
    }
    void settle() {
        close(true);
        land_last_pass(cfg, st);
    }
    void stream_start(long long consumed0, int slot0) {
        ChainPlan plan;
        memset(&plan, 0, sizeof plan);
        plan.s[0] = stream_segment(cfg, st, consumed0, slot0);
        plan.nseg = 1, plan.stream = 1;
        emit_launch("chain", true, true, SRC_RING, plan, 0, 1, "none", "none");
        stream_alive = true;
    }
    void stream_op(int n_slots) {
        const bool closes = stream_closes(cfg, st, n_slots);
        const long long seq = ++chain_seq;
        if (!stream_alive) stream_start(seq - 1, st.pending);
        st.pending += n_slots;
        check_state();
        if (!closes) return;
        stream_alive = false;
        const StreamTurn t = plan_stream_turn(cfg, st, n_lm_hi, sh.profiling);
        if (!t.pass_after_start) pass(t.pass);
        stream_start(seq, st.pending);
        if (t.pass_after_start) pass(t.pass);
    }
    const unsigned char *call_consumes = nullptr;
    int call_k0 = 0, call_src = 0;
    void ops(int source, int k0, const unsigned char *consumes, int nops, bool defer_last_close) {
        if (nops > 0 && st.pending == cfg.maxp) close(false);
        const CallSource src = source == SRC_CURSOR ? FROM_CURSOR : (source == SRC_RING ? FROM_RING : FROM_SCRIPT);
        const CallPlan cp = route_call(cfg, st, sh.streams, src, consumes, nops, defer_last_close, persist_possible(cfg, src, defer_last_close) && sh.residency_ok);
        if (cp.route == ROUTE_STREAM_OPS) {
            for (int q = 0; q < nops; q++) stream_op(consumes[q] ? 1 : 0);
            return;
        }
        if (cp.route == ROUTE_STREAM_SCRIPT) {
            for (int q0 = 0, q1 = 0; q0 < nops; q0 = q1) stream_op(take_ops(consumes, nops, &q1, st.pending, cfg.maxp) - st.pending);
            return;
        }
        stream_alive = false;  // (stream_stop)
        const OpsCall call = {src, k0, nops, consumes, defer_last_close, n_lm_hi, sh.profiling};
        call_consumes = consumes, call_k0 = k0, call_src = source;
        if (cp.route == ROUTE_GROUPED) {
            const int ng = cfg.ngroups, per = (cfg.B + ng - 1) / ng;
            ChainPlan plan;
            memset(&plan, 0, sizeof plan);
            plan.nseg = 1;
            GroupedWindow w;
            for (int i = 0; plan_ops_grouped(cfg, st, call, &i, &chain_seq, &w);) {
                plan.s[0] = w.seg;
                segment(w.seg);
                for (int g = 0; g < ng; g++) {
                    const int b0 = g * per, nb = cfg.B - b0 < per ? cfg.B - b0 : per;
                    if (nb <= 0) break;
                    const std::string grp = g ? "group" + std::to_string(g) : "chain";  // (group 0's stream is the chain's)
                    emit_launch(grp.c_str(), false, false, source, plan, b0, nb, "none", "none");
                    if (w.do_pass) emit_group_pass(grp.c_str(), w.set, w.nslots, w.buf, w.buf, w.nT_hi, w.rev, cfg.batch_interleave, b0, nb, sh.profiling);
                }
                check_state();
            }
            return;
        }
        plan_ops(cfg, st, cp, call, &chain_seq, *this);
    }
    void state() {
        check_state();
        emit_state(st.cur_set, st.pending, st.buf_in, st.prev_pending, st.need_pass, st.pass_seq, st.ev_idx, ev_name(st.pass_done[0]), ev_name(st.pass_done[1]), st.chain_signalled,
                   st.open_set_gate, st.open_gate_idx, st.flush_dir, st.windows_closed, st.last_window_slots, chain_seq, st.seg_count_base);
    }
};

static std::vector<std::string> words(const std::string &line) {
    std::istringstream in(line);
    std::vector<std::string> w;
    for (std::string t; in >> t;) w.push_back(t);
    return w;
}

int main(int argc, char **argv) {
    if (argc < 2) return printf("usage: window_plan_check window_plans.txt | --dump\n"), 2;
    for (const Shape &sh : all_shapes()) run_shape<NewSim>(sh);
    if (g_broken) return printf("window plan check FAILED: %d invariants broken\n", g_broken), 1;
    if (!strcmp(argv[1], "--dump")) {
        for (const std::string &l : g_lines) puts(l.c_str());
        return 0;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) return printf("cannot open %s\n", argv[1]), 2;
    char buf[2048];
    size_t n = 0;
    int bad = 0;
    std::string context;
    while (fgets(buf, sizeof buf, f) && bad < 20) {
        std::string want(buf);
        while (!want.empty() && (want.back() == '\n' || want.back() == '\r')) want.pop_back();
        if (want.empty() || want[0] == '#') continue;
        if (n >= g_lines.size()) {
            printf("the record goes on after the planner's %zu lines: %s\n", n, want.c_str());
            bad++;
            break;
        }
        const std::string &got = g_lines[n++];
        if (got.compare(0, 6, "shape ") == 0 || got.compare(0, 5, "call ") == 0) context = (got[0] == 's' ? got.substr(0, got.find(' ', 6)) : context.substr(0, context.find(" / ")) + " / " + got);
        if (got == want) continue;
        bad++;
        const std::vector<std::string> g = words(got), w = words(want);
        const char *const *names = g.empty() ? nullptr : fields_of(g[0]);
        if (!names || w.empty() || g[0] != w[0] || g.size() != w.size()) {
            printf("line %zu (%s): got `%s`, want `%s`\n", n, context.c_str(), got.c_str(), want.c_str());
            continue;
        }
        for (size_t k = 1; k < g.size(); k++)
            if (g[k] != w[k]) printf("line %zu (%s): %s %s = %s, want %s\n", n, context.c_str(), g[0].c_str(), names[k - 1] ? names[k - 1] : "?", g[k].c_str(), w[k].c_str());
    }
    fclose(f);
    if (!bad && n < g_lines.size()) printf("the record ends after %zu of the planner's %zu lines\n", n, g_lines.size()), bad++;
    if (bad || n < 1000) return printf("window plan check FAILED: %d mismatching lines of %zu\n", bad, n), 1;
    printf("window plans ok: %zu lines\n", n);
    return 0;
}
