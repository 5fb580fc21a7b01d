#!/usr/bin/env python3
"""EKF steps/sec (propagate + full update) on MI355X -- the metric of BASELINE.json.

One step = 1 Propagate + M sequential single-measurement Updates (n_z = 1 each, as slam.cpp:150-171
issues them), all taking the Old branch on a map of N landmarks already in the state.
Default workload: config 3 of BASELINE.json -- one filter, N = 4096 (dense P 8195 x 8195 fp64,
537 MB), M = 4 -- because that is where the north_star quotes its target and the only size whose P
does not fit the 256 MB Infinity Cache.  Inputs (state, the whole step script) are resident in HBM
before the timed region; the timed region is kernel launches only.

Multi-GPU: one process per GPU (torch.distributed, backend nccl = RCCL).  Filters are independent
Monte-Carlo instances, so ranks share nothing on the data path (weak scaling: every rank runs the
same workload with its own seed); the single collective is the all-gather of per-filter NIS/NEES
summaries at the end of the timed region.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the steps and prints the headline (with the dense pass's
roofline from the events inside the timed region); --dump-outputs DIR writes what the last timed step computed.  Everything else --
the decision check, the untimed windows that time the chain kernel alone, the chain record, the CPU baselines, the secondary
configurations and config 5's legs -- runs with --full.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

def compact(o, digits=6):
    """Floats of the JSON line rounded to `digits` significant digits (a 17-digit double is 18 characters; the driver keeps an 8 KB
    tail of the line).  `value` and `ms_per_step` at the top level are printed in full by main()."""
    if isinstance(o, float):
        if o != o or o in (float("inf"), float("-inf")):
            return None
        return float("%.*g" % (digits, o))
    if isinstance(o, dict):
        return {k: compact(v, digits) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [compact(v, digits) for v in o]
    return o


def ekf_environment():
    """Every EKF_* variable this process sees goes into the JSON line; a debug hook (EKF_DEBUG_*: skipped dense passes, dropped
    completion marks -- only the debug variant of the library knows them, but the line must not depend on which library was
    loaded) or a diagnostic library (EKFSLAM_LIB) makes the run invalid: refuse."""
    seen = {k: v for k, v in sorted(os.environ.items()) if k.startswith("EKF")}
    bad = [k for k in seen if k.startswith("EKF_DEBUG_") or k == "EKFSLAM_LIB"]
    if bad:
        raise SystemExit("bench.py refuses to run with %s set (debug hooks / diagnostic library builds are not the measured binary)" % ", ".join(bad))
    return seen


VERBOSE = False  # --verbose: the prose fields (byte model, window note, traffic source) ride on the line; the default line stays under 8 KB
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
FP64_MFMA_PEAK_TFLOPS = 78.6  # MI355X datasheet fp64 matrix; v_mfma_f64_16x16x4_f64 measured 68 TFLOP/s (scripts/micro)

WORKLOADS = {
    # name: (N landmarks, batch per GPU, default steps, default warmup, seed, map half-extent in m, min. target separation)   -- BASELINE.json configs
    "n4096": (4096, 1, 512, 32, 20260003, 50.0, 1.5),   # config 3 (more steps than its 50: a run is only ~30 ms)
    "n1024": (1024, 1, 200, 10, 20260002, 50.0, 1.5),   # config 2
    # not a BASELINE.json config: one size past the 256 MB Infinity Cache in the build's own storage scheme (P_LL triangle
    # 1.08 GB per buffer), at config 3's landmark density -- tells HBM streaming from cache hits in the roofline fraction
    "n8192": (8192, 1, 128, 16, 20260008, 70.7, 1.5),
    # config 4 (config 5 = the same, sharded over --gpus N): 256 landmarks at config 3's landmark density, so that four
    # well-conditioned (range < 9 m, cond(S) < 80) targets exist around the robot at every step; targets at least 1 m from
    # their nearest neighbour: checked on the oracle, all 2048 filters of config 5 take only the intended Old matches
    "batch256": (256, 256, 200, 10, 20260004, 12.5, 1.0),
}

def window_for(workload, asked):
    """measurements per dense pass: --max-pending when given, else the workload's best (the library's own default is 16): 32 for batch256, whose
    one-workgroup filters (k_solo) keep the first half of a long window in accumulation registers -- the chain and the pass are serial there, so
    half as many passes pay -- and, since round 5, 32 for N = 4096 and beyond: the library then shapes the filter as 64 workgroups of one owner
    wave (two windows of 32 fit their LDS), the dense pass runs half as often and stops co-limiting the window (31.2 k -> 36.5 k steps/s over 512
    steps); N = 1024, whose pass is a tenth of its window, is fastest at 16 (42.7 k against 41.9 k at 32)."""
    if asked:
        return asked
    return 16 if workload == "n1024" else 32


def prime_steps_for(window, M, K):
    """Untimed script steps in FRONT of the warm-up (round 6).  The driver's `--warmup 5` is 20 measurements: less than one window of 32, so the
    warm-up never closed a window and the timed region was the first to run a pipeline pass -- second stream, stream gates, k_mark, a
    multi-segment chain launch, both walking directions of the tile map -- with every first-use cost of the runtime (kernel lookup, queue
    creation, signal pools) inside 0.85 ms.  The prime run is at least three windows (two pipeline passes and a terminal one) and at least as
    long as the timed region up to 64 steps, so the timed region repeats a call pattern the process has already executed.  `steps` and
    `warmup` of the JSON line stay the driver's; `prime_steps` is reported beside them."""
    if M <= 0:
        return 0
    return max(min(K, 64), 3 * -(-window // M))


def make_filters(pkg, mc, workload, lo, hi, steps, M, dev_id, max_pending, log_entries, tail_windows=0, prime_for=None):
    """A handle holding global filters [lo, hi) of `workload`, states injected and the step script loaded (all untimed):
    the prime steps (prime_steps_for(window, M, prime_for); f.prime_steps), `steps` steps, and `tail_windows` windows' worth for
    measurements outside the timed region."""
    import numpy as np
    N, _, _, _, seed, extent, min_sep = WORKLOADS[workload]
    f = pkg.FilterBatch(hi - lo, N, device=dev_id, max_pending=max_pending, log_capacity=max(4096, log_entries))
    f.prime_steps = prime_steps_for(f.window, M, prime_for) if prime_for else 0
    total_steps = f.prime_steps + steps + tail_windows * -(-f.window // M)  # (the library may have shortened the window to fit its on-chip buffer)
    scripts = []
    for b, g in enumerate(range(lo, hi)):
        x0, P0 = pkg.scenarios.injected_state(N, seed=mc.filter_seed(seed, g), extent=extent)
        f.set_state(x0, P0, index=b)
        scripts.append(pkg.scenarios.steady_script(x0, steps=total_steps, M=M, seed=mc.filter_seed(seed + 7919, g), min_separation=min_sep))
        del P0
    f.script_load(np.stack([s["ctrl"] for s in scripts], axis=1), np.stack([s["z"] for s in scripts], axis=2),
                  np.stack([s["R"] for s in scripts], axis=2), truth=np.stack([s["truth"] for s in scripts], axis=1))
    return f, scripts


def timed_steps(f, mc, torch, dist, coll_device, W, K, graph):
    """Prime run (untimed, f.prime_steps), W untimed warm-up steps, then exactly K steps bracketed by barrier + synchronize on both
    sides; the timed region ends with P_LL fully folded (ekf_flush) and with the one collective, the all-gather of per-filter NIS / NEES.
    Returns (elapsed s, device ms, gathered rows, phases)."""
    P = getattr(f, "prime_steps", 0)
    if P:
        # every code path of the timed region once, on script steps of its own: multi-segment launch, both pipeline streams, gates,
        # k_mark, the terminal pass, the counters' read-back, the collective
        f.timer_start()
        f.script_run(0, P, use_graph=graph)
        f.flush()
        f.timer_stop()
        mc.gather_device_stats(f, coll_device)
        f.sync()
        f.flush_profile_read()
    # the warm-up goes through every call of the timed region once and ends like it, with P_LL fully folded: the timed region then
    # holds exactly K steps of work
    f.timer_start()
    f.script_run(P, W, use_graph=graph)
    f.flush()
    f.timer_stop()
    mc.gather_device_stats(f, coll_device)
    f.sync()
    f.reset_stats()
    f.flush_profile_read()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f.timer_start()
    f.script_run(P + W, K, use_graph=graph)
    f.flush()                # P_LL fully folded inside the timed region, whatever K*M modulo the window is
    t1 = time.perf_counter()
    dev_ms = f.timer_stop()  # hipEvents on the handle's own stream
    t2 = time.perf_counter()
    gathered = mc.gather_device_stats(f, coll_device)  # the one collective (RCCL all-gather), fed from the device's own summary buffer
    t3 = time.perf_counter()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    # where the host clock's time went: enqueue (launch calls, concurrent with the device), wait (device still busy after the last
    # call returned), stats+gather (the collective), sync (synchronize + barrier); device = hipEvents around the K steps
    phases = {"enqueue": (t1 - t0) * 1e6, "wait": (t2 - t1) * 1e6, "stats_gather": (t3 - t2) * 1e6, "sync_barrier": (t0 + elapsed - t3) * 1e6,
              "device": dev_ms * 1e3, "host_minus_device": elapsed * 1e6 - dev_ms * 1e3}
    if os.environ.get("BENCH_PHASES"):
        print("phases (us): " + "  ".join("%s %.1f" % kv for kv in phases.items()), file=sys.stderr)
    per_rank = [elapsed]
    if dist is not None:
        tl = [torch.zeros(1, dtype=torch.float64, device=coll_device) for _ in range(dist.get_world_size())]
        dist.all_gather(tl, torch.tensor([elapsed], dtype=torch.float64, device=coll_device))
        per_rank = [float(t.item()) for t in tl]
        elapsed = max(per_rank)  # MAX over ranks
    phases["per_rank_ms"] = [t * 1e3 for t in per_rank]
    return elapsed, dev_ms, gathered, phases


CONFIG5_LEG_KEYS = ("filters_total", "filters_per_gpu", "value", "unit", "ms_per_step", "gathered_rows", "ranks_seen", "per_rank_ms",
                    "allgather_us", "roofline")
CONFIG5_ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "bytes_per_launch", "launches", "avg_launch_us")


def config5_leg_record(total, per_gpu, world, K, elapsed, gathered_rows, per_rank_ms, allgather_us, roof):
    """One leg of BASELINE.json config 5 as it goes into the line (the dry run builds the same record with value = None): steps/s of the
    whole job, every rank's own time, the all-gather's time on rank 0, how many ranks' rows arrived, and the dense pass's roofline on rank 0
    -- north_star: "steps/sec and achieved HBM-bandwidth fraction reported at 1/2/4/8 GPUs"."""
    r = dict((k, None) for k in CONFIG5_ROOFLINE_KEYS)
    r.update({"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s"})
    if roof:
        r.update({k: roof.get(k) for k in CONFIG5_ROOFLINE_KEYS})
        for extra in ("fused_pass", "mfma", "measurements_per_launch", "end_to_end_hbm_frac"):
            if extra in roof:
                r[extra] = roof[extra]
    return {"filters_total": total, "filters_per_gpu": per_gpu, "value": (total * K / elapsed) if elapsed else None, "unit": "filter-steps/s",
            "ms_per_step": (elapsed / K * 1e3) if elapsed else None, "gathered_rows": int(gathered_rows),
            "ranks_seen": int(round(gathered_rows * world / float(total))), "per_rank_ms": per_rank_ms, "allgather_us": allgather_us, "roofline": r}


def config5_legs(pkg, mc, torch, dist, coll_device, rank, world, dev_id, M, max_pending, steps=None, legs=("weak", "strong")):
    """BASELINE.json config 5: independent filters at N = 256 sharded over the ranks, RCCL all-gather of NIS / NEES inside
    the timed region.  Weak: 256 filters per GPU.  Strong: 2048 filters in all (more than 256 per GPU go out as several
    chain launches per window).  Every leg carries the dense pass's roofline (rank 0's passes, hipEvents inside the timed region)."""
    N, per_gpu, K, W, _, _, _ = WORKLOADS["batch256"]
    if steps is not None:
        K = steps
    out = {"world_size": world, "N": N, "M": M, "steps": K, "warmup": W}
    for leg, total in (("weak", per_gpu * world), ("strong", 2048)):
        if leg not in legs:
            continue
        lo, hi = mc.shard_range(total, rank, world)
        f, _ = make_filters(pkg, mc, "batch256", lo, hi, W + K, M, dev_id, window_for("batch256", max_pending), (K + W) * M, prime_for=K)
        f.flush_profile(True)
        elapsed, dev_ms, gathered, phases = timed_steps(f, mc, torch, dist, coll_device, W, K, False)
        f.sync()
        launches, flush_ms = f.flush_profile_read()
        st = f.stats()
        assert all(s["n_old"] == K * M for s in st), "a filter left the Old branch"
        roof = roofline_record(pkg, f, "batch256", hi - lo, N, K, M, f.window, launches, flush_ms, 0, 0.0, dev_ms, elapsed)
        f.close()
        out[leg] = config5_leg_record(total, hi - lo, world, K, elapsed, gathered.shape[0], phases["per_rank_ms"], phases["stats_gather"], roof)
    return out


def roofline_record(pkg, f, workload, B, N, K, M, window, launches, flush_ms, alone_launches, alone_ms, dev_ms, elapsed):
    """The dominant kernel = the dense pass k_flush_rb.  Algorithmic bytes per launch: every stored P_LL element (upper-triangle
    64x64 tiles; one triangle authoritative = SURVEY.md 8d's scheme C, 8 n^2 per pass) read once and written once, whatever
    number of measurements the pass folds; duration = hipEvents riding on each dispatch packet inside the timed region."""
    nT = (2 * N + 63) // 64
    tiles = nT * (nT + 1) // 2
    windows = -(-K * M // window)
    groups = max(1, round(launches / windows)) if launches else 1  # (phase groups of a batch launch one pass per group and window)
    filters_per_launch = max(1, B // groups)
    # (a tile is 16 chains of 16 x 16; the six chains below the diagonal of a DIAGONAL tile are dead storage nobody reads, and the pass
    # neither loads, multiplies nor stores them: they are not algorithmic bytes)
    chains = tiles * 16 - nT * 6
    bytes_per_launch = filters_per_launch * chains * 256 * 8 * 2
    slots_per_launch = min(window, K * M)
    if launches:
        # what a launch of THIS run folded on average: a balanced tail (32 | 24 | 24 for the driver's 20 steps) and the terminal pass of a run
        # that is not a whole number of windows fold fewer measurements than the window
        slots_per_launch = min(float(window), K * M * groups / float(launches))
    flops_per_launch = filters_per_launch * chains * (slots_per_launch / 2.0) * 2048  # one v_mfma_f64_16x16x4_f64 per chain and PAIR of measurements
    r = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
         "kernel": "k_flush_rb", "byte_model": "scheme C, DESIGN.md 4.3",
         "bytes_per_launch": bytes_per_launch, "launches": int(launches), "avg_launch_us": None, "measurements_per_launch": slots_per_launch,
         "mfma": {"achieved": None, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": None, "flops_per_launch": flops_per_launch}}
    if VERBOSE:
        r["byte_model"] = "scheme C (one triangle authoritative): every live 16x16 chain of the upper-triangle tiles (2 KiB) read + written per pass -- %d tiles = %d chains, the %d dead chains below the diagonals of the diagonal tiles left out; %.4g measurements folded per pass (window %d)" % (tiles, chains, nT * 6, slots_per_launch, window)
    if VERBOSE and window > 16 and B == 1:
        r["window_note"] = ("window %d: a launch folds up to %d slot pairs into the same bytes that rounds 1-4 folded 8 pairs into (window 16: frac 0.61-0.64, still profiled: "
                            "profiles/r05_n4096_w16_overlap_summary.json) -- half the passes and half the HBM bytes per folded measurement, twice the fp64 MFMA work per byte "
                            "(roofline.mfma): %.1f flop per byte, at the ridge of the fp64 roofline (78.6 TFLOP/s / 8 TB/s = 9.8), so HBM and matrix-pipe fractions are both below their own ceilings; "
                            "DESIGN.md 4.3 has the lab measurements of what that mix reaches" % (window, window // 2, flops_per_launch / float(bytes_per_launch)))
    if launches:
        avg_s = flush_ms / 1e3 / launches
        r["avg_launch_us"] = avg_s * 1e6
        r["achieved"] = bytes_per_launch / avg_s / 1e9
        r["frac"] = r["achieved"] / HBM_PEAK_GBS
        r["mfma"]["achieved"] = flops_per_launch / avg_s / 1e12
        r["mfma"]["frac"] = r["mfma"]["achieved"] / FP64_MFMA_PEAK_TFLOPS
        r["share_of_step_time"] = flush_ms / (dev_ms if dev_ms > 0 else 1.0)
        r["concurrent_with"] = "k_chain" if f.overlap else None  # (overlap mode: the next window's chain kernel runs beside the pass)
        # every pass of the timed region against the whole timed region: what the headline cannot hide (the sequential chain
        # kernels, launch gaps, fill and drain all count as time in which HBM should have been busy)
        r["end_to_end_hbm_frac"] = launches * bytes_per_launch / elapsed / 1e9 / HBM_PEAK_GBS
        if getattr(f, "fused_pass", False):
            # one-workgroup filters with a long window fold their windows inside the chain kernel (k_solo<true>, ChainSeg::self_pass): there is
            # no dense-pass launch to time.  `launches` counts the passes, the duration is that of the k_solo launches that contain them --
            # measurement loops included -- so this fraction is a LOWER bound of the pass's own (the stamps build separates the two:
            # DESIGN.md 4.2); EKF_SOLO_FUSE=0 runs the passes as k_flush_rb launches again.
            r["kernel"] = "k_solo<true> (loop + own pass; avg_launch_us per window)"
            r["fused_pass"] = True
    if alone_launches:
        a_s = alone_ms / 1e3 / alone_launches
        r["alone"] = {"avg_launch_us": a_s * 1e6, "achieved": bytes_per_launch / a_s / 1e9, "frac": bytes_per_launch / a_s / 1e9 / HBM_PEAK_GBS,
                      "launches": int(alone_launches)}  # (the same pass with nothing else on the GPU, outside the timed region)
    # PMC-derived HBM bytes per launch: NOT measured by this run -- replayed from the committed rocprofv3 --pmc passes of this very
    # command (scripts/profile_r0x.sh -> profiles/traffic_*.json); null when no committed pass matches the configuration
    have = kernel_source_digest()
    # (a handle that folds its windows inside the chain kernel has counters of its own: whole k_solo<true> windows, scripts/profile_batch_fused.py)
    names = ("traffic_%s.json" % workload, "traffic_%s_inplace.json" % workload)
    if getattr(f, "fused_pass", False):
        names = ("traffic_%s_fused.json" % workload,) + names
    for tname in names:
        tfile = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tfile):
            tj = json.load(open(tfile))
            if tj.get("max_pending") == window and tj.get("overlap", int(f.overlap)) == int(f.overlap) and tj.get("filters_per_gpu", B) == B:
                if tj.get("kernel_source_sha16") != have:
                    # a counter pass of OTHER kernel sources says nothing about this binary: null, not a stale number
                    r["traffic_source"] = "profiles/%s: stale (sources %s, now %s)" % (tname, tj.get("kernel_source_sha16"), have)
                    continue
                r["traffic"] = tj.get("hbm_bytes_per_launch")
                r["traffic_source"] = "replayed from profiles/%s (rocprofv3 --pmc passes of sources %s)" % (tname, have)
                if tj.get("fused_pass"):
                    # counted on whole windows of k_solo<true>: the measurement loop's own traffic (the B side of the slots, written once per
                    # window, and the matched landmarks' P_LL entries) is included
                    r["traffic_without_slot_emit_ratio"] = tj.get("ratio_without_the_slot_emit")
                elif getattr(f, "fused_pass", False):
                    # the counters were taken on k_flush_rb (EKF_SOLO_FUSE=0), the binary measured here folds inside k_solo: same tiles, but the
                    # in-kernel pass stages a tile row's A operands ONCE per row (LDS-DMA) and walks the exact landmark count, so it re-reads
                    # fewer operand bytes than the pass kernel: the replayed figure is an UPPER bound for this run
                    r["traffic_is_upper_bound"] = True
                break
    return r


def chain_record(workload, window, overlap, alone_us, pipeline_us):
    """The line's `chain` record: what paces the step rate is the measurement chain of Update.cpp:80-194 (sweep -> filter-wide arg-min ->
    winner's record and P_LL column -> fold + gain), a latency chain the HBM roofline of the dense pass says nothing about.
    `us_per_measurement`: measured in this run -- `alone` = hipEvents around chain launches of one window with nothing beside them,
    `in_pipeline` = device time per measurement of the 512-step run (dense passes hidden beside the chain).  The stamp split and the floor
    (scripts/chain_floor.py: instruction-bound parts + 2 x one measured cross-XCC hand-off) are replayed from profiles/chain_<workload>.json,
    collected on the stamps build of the same kernel sources; null when stale."""
    rec = {"reference": "odometry/Update.cpp:80-194", "us_per_measurement": {"alone": alone_us, "in_pipeline": pipeline_us}, "split_us": None,
           "hop_us": None, "floor_us": None, "floor_us_idle": None, "floor_over_measured": None}
    path = os.path.join(ROOT, "profiles", "chain_%s.json" % workload)
    if os.path.exists(path):
        cj = json.load(open(path))
        st = cj.get("stamps", {})
        if cj.get("kernel_source_sha16") != kernel_source_digest():
            rec["source"] = "profiles/chain_%s.json: stale" % workload
        elif st.get("max_pending") == window and st.get("overlap") == overlap:
            w = st["first_worker_us"]
            rec["split_us"] = {"sweep_argmin_publish": w["sweep_argmin_publish"], "exchange_wait": w["wait_pick"], "gate": w["gate_bookkeeping"],
                               "record_trip_wait": w["wait_staged_record"], "pll_wait": w["wait_pll_entries"], "fold": w["fold"],
                               "gain_stores": w["gain_stores_or_robot_block"], "between_and_barriers": w["between_measurements"] + w["end_barrier"] + w["segment_prologue_share"],
                               "stamped_total": st["first_worker_sum_us"]}
            rec.update({"hop_us": cj["hop_us"], "floor_us": cj["floor_us"], "floor_us_idle": cj["floor_us_idle"],
                        "source": "profiles/chain_%s.json" % workload})
            measured = pipeline_us or alone_us
            if measured:
                rec["floor_over_measured"] = cj["floor_us"] / measured
    return rec


def slim_roofline(r):
    """A secondary leg's roofline without the fields the headline's already explains (models, notes): the numbers only."""
    keep = ("achieved", "frac", "traffic", "bytes_per_launch", "launches", "avg_launch_us", "measurements_per_launch",
            "end_to_end_hbm_frac", "fused_pass", "traffic_is_upper_bound", "traffic_without_slot_emit_ratio")  # (bound "hbm", peak and unit as in the headline's record)
    out = {k: r[k] for k in keep if k in r}
    if r.get("mfma"):
        out["mfma_frac"] = r["mfma"].get("frac")
    if r.get("alone"):
        out["alone_frac"] = r["alone"].get("frac")
        out["alone_avg_launch_us"] = r["alone"].get("avg_launch_us")
    return out


def kernel_source_digest():
    """sha256 (first 16 hex digits) over the device sources of the library: profiles/traffic_*.json carry the digest of the sources
    their counter passes ran on (scripts/summarize_profile.py), and a replayed number must come from the same ones."""
    import hashlib
    import re
    h = hashlib.sha256()
    d = os.path.join(ROOT, "2d-ekf-slam_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")) or name == "Makefile":
            text = open(os.path.join(d, name), "r", errors="replace").read()
            if name != "Makefile":
                # the CODE: comments and layout do not change the binary (a reworded comment must not make a counter pass look stale)
                text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
                text = re.sub(r"//[^\n]*", " ", text)
            text = " ".join(text.split())
            h.update(name.encode())
            h.update(text.encode())
    return h.hexdigest()[:16]


def host_cpu_record():
    """CPU model, frequency governor and the pinning the CPU legs ran under."""
    rec = {"host_cpus": os.cpu_count(), "model": None, "governor": None, "affinity_cpus": None, "pinning": None}
    try:
        for l in open("/proc/cpuinfo"):
            if l.startswith("model name"):
                rec["model"] = l.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        rec["governor"] = open("/sys/devices/system/cpu/cpu0/cpufreq/scaling_governor").read().strip()
    except OSError:
        rec["governor"] = "not exposed"
    try:
        aff = sorted(os.sched_getaffinity(0))
        rec["affinity_cpus"] = len(aff)
    except (AttributeError, OSError):
        aff = None
    rec["pinning"] = "1 thread, no taskset; OMP_NUM_THREADS=%s" % os.environ.get("OMP_NUM_THREADS")
    return rec


DUMP_P_ENTRIES = 1 << 21  # P entries sampled across the batch by --dump-outputs: 16 MB of values and 16 MB of indices at most


def dump_outputs(f, out_dir, gathered, K, M):
    """--dump-outputs: what the last timed step hands its caller, one float64 .npy file each -- x (batch, n); P's diagonal and a fixed
    sample of P's entries (the same seeded flat indices in every filter, P_sample_index; all of P when it fits); the poses; the branch,
    matched landmark and Mahalanobis distance of the step's M measurements; the gathered (mean NIS, mean NEES) per filter."""
    import numpy as np
    xs, diag, sample, idx = [], [], [], None
    for b in range(f.batch):
        x, P = f.get_state(b)
        if idx is None:
            per = DUMP_P_ENTRIES // f.batch
            idx = np.arange(P.size) if P.size <= per else np.unique(np.random.default_rng(0).integers(0, P.size, size=per))
        xs.append(x)
        diag.append(np.diag(P).copy())
        sample.append(P.ravel()[idx])
        del P
    out = {"x": np.stack(xs), "P_diag": np.stack(diag), "P_sample": np.stack(sample), "P_sample_index": idx, "poses": f.poses(),
           "nis_nees": gathered}
    if M:
        last = np.array([f.decisions(b, K * M)[-M:] for b in range(f.batch)], dtype=np.float64)  # (batch, M, [decision, matched, mahal])
        out.update({"decision": last[..., 0], "matched": last[..., 1], "mahalanobis": last[..., 2]})
    out = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in out.items()}
    total = sum(v.nbytes for v in out.values())
    assert total <= 64 << 20, "the dump would be %d bytes" % total
    os.makedirs(out_dir, exist_ok=True)
    for k, v in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


def measure(pkg, mc, torch, dist, coll_device, rank, world, dev_id, workload, K, W, M, max_pending, graph, flush_profile, check=True, alone=True, latency=False,
            dump_dir=None):
    """One workload, timed as the contract says (timed_steps); returns its record.  `dump_dir`: dump_outputs() right after the timed steps."""
    import numpy as np
    N, B, _, _, seed, extent, min_sep = WORKLOADS[workload]
    lo, hi = mc.shard_range(B * world, rank, world)
    # (4 windows of untimed tail: dense passes measured one at a time, nothing beside them; latency: one step per call)
    extra = 264 if latency else 0
    max_pending = window_for(workload, max_pending)
    f, scripts = make_filters(pkg, mc, workload, lo, hi, W + K + extra, M, dev_id, max_pending, (K + W + extra + 64) * M, tail_windows=4 if alone else 0, prime_for=K)
    window = f.window  # the library may shorten the window to fit its on-chip buffer
    win_steps = -(-window // M)
    P = f.prime_steps  # script steps run before the warm-up (untimed): every later step index is shifted by it
    f.flush_profile(flush_profile)
    elapsed, dev_ms, gathered, phases = timed_steps(f, mc, torch, dist, coll_device, W, K, graph)
    f.sync()
    launches, flush_ms = f.flush_profile_read()
    if check:
        for b in range(B if B <= 4 else 4):
            dec = f.decisions(b, K * M)
            want = [3 + 2 * int(t) for t in scripts[b]["target"][P + W:P + W + K].ravel()]
            assert len(dec) == K * M and all(d[0] == pkg.ekfslam.OLD for d in dec), "filter %d left the Old branch" % b
            assert [d[1] for d in dec] == want, "filter %d matched an unintended landmark" % b
        st = f.stats()
        assert all(s["n_old"] == K * M and s["n_new"] == 0 and s["n_ignore"] == 0 for s in st)
    if dump_dir:
        dump_outputs(f, dump_dir, gathered, K, M)
    lat = None
    if latency:
        # per-step latency: one scripted step per call, host clock from the call to the moment the pose of
        # that step is readable (kernel launch + completion, no state copy); the window's dense pass falls on every fourth step
        # (the interpreter's cyclic garbage collector is off inside the loop and the samples go into a preallocated array: a one-off
        # pause of 0.65-1.1 ms at a fixed iteration count of this very loop -- whatever the GPU was doing, docs/history section 5 -- was the
        # harness, not the library)
        import gc
        raw = np.empty(extra)
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            for q_, s_ in enumerate(range(P + W + K, P + W + K + extra)):
                t0 = time.perf_counter()
                f.script_run(s_, 1)
                f.poses()
                raw[q_] = (time.perf_counter() - t0) * 1e6
        finally:
            if gc_was_on:
                gc.enable()
        ts = np.sort(raw[8:])
        lat = {"unit": "us per step (one call per step, pose read back)", "samples": int(ts.size),
               "p10": float(np.percentile(ts, 10)), "p50": float(np.percentile(ts, 50)), "p90": float(np.percentile(ts, 90)),
               "p99": float(np.percentile(ts, 99)), "max": float(ts[-1]), "over_1ms": int((ts > 1000.0).sum()),
               "first_calls_us": [float(t) for t in raw[:4]]}  # (the first 8 calls -- host-side first-use costs -- are not ranked; four are listed)
        f.flush()
        f.sync()
        f.flush_profile_read()
    alone_launches, alone_ms, chain_alone_us = 0, 0.0, None
    if flush_profile and alone:
        base = P + W + K + extra
        chain_alone_ms = 0.0
        for r in range(4):
            # a whole window -- the chain kernel with nothing beside it, hipEvents around its launch -- then its pipeline-style pass
            # (buffer to buffer, on the pass's own stream) with the chain kernel already finished and nothing following
            f.timer_start()
            f.script_run(base + r * win_steps, win_steps)
            chain_alone_ms += f.timer_stop()
            f.sync()
            f.close_window()
            f.sync()
        alone_launches, alone_ms = f.flush_profile_read()
        chain_alone_us = chain_alone_ms * 1e3 / (4 * win_steps * M) if M else None
    roof = roofline_record(pkg, f, workload, B, N, K, M, window, launches, flush_ms, alone_launches, alone_ms, dev_ms, elapsed)
    rep = mc.consistency_report(gathered, K * M, K) if check else None
    overlap = int(f.overlap)
    f.close()
    return {"workload": workload, "N": N, "B": B, "K": K, "W": W, "M": M, "window": window, "overlap": overlap, "elapsed": elapsed, "dev_ms": dev_ms,
            "prime_steps": P, "phases_us": phases, "chain_alone_us": chain_alone_us, "value": B * world * K / elapsed, "roofline": roof, "latency": lat, "report": rep, "seed": seed, "extent": extent, "min_sep": min_sep}


def immediate_leg(pkg, dev_id):
    """The reference's own call pattern (slam.cpp:136-170): one synchronising call per operation -- doPropagation, then doUpdate per
    feature, the public mirrors current after each -- from the C++ shim (compat/kalmanfilter.h) through the headless replay driver
    (compat/replay --timing), starting from the injected state of configs 2 and 3.  Host time per 5-call step; never the headline."""
    import subprocess
    import tempfile
    import numpy as np
    replay = os.path.join(ROOT, "compat", "replay")
    if not os.path.exists(replay):
        return {"error": "compat/replay is not built"}
    out = {"unit": "us per 5-call step (doPropagation + 4 doUpdate, C++ shim, host clock)", "call_pattern": "slam.cpp:136-170"}
    for name, N in (("n50", 50), ("n1024", 1024), ("n4096", 4096)):
        # (n50: the reference's own scale, BASELINE.json config 1 -- one workgroup, k_solo; constant landmark density as in tests/test_compat.py)
        _, _, _, _, seed, extent, min_sep = WORKLOADS[name] if name in WORKLOADS else (0, 0, 0, 0, 1, 50.0 * (N / 4096.0) ** 0.5, 1.0)
        x0, P0 = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
        sc = pkg.scenarios.steady_script(x0, steps=120, M=4, seed=seed + 7919, min_separation=min_sep)
        with tempfile.TemporaryDirectory() as td:
            with open(os.path.join(td, "rec.txt"), "w") as f:
                for s_ in range(120):
                    v, w, dt = (float(c) for c in sc["ctrl"][s_])
                    feats = " ".join("%r %r" % (float(1000.0 * z[0]), float(1000.0 * z[1])) for z in sc["z"][s_])
                    f.write("%r %r %r nan %d %s\n" % (dt, v * 1000.0, w * 180.0 / 3.141592654, 4, feats))
            with open(os.path.join(td, "state.bin"), "wb") as f:
                np.array([x0.size], dtype=np.float64).tofile(f)
                np.ascontiguousarray(x0).tofile(f)
                np.ascontiguousarray(P0).tofile(f)
            del P0
            p = subprocess.run([replay, os.path.join(td, "rec.txt"), td, str(N), "--state", os.path.join(td, "state.bin"), "--timing"],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
            if p.returncode != 0 or "timing" not in p.stdout:
                out[name] = {"error": p.stderr[-300:]}
                continue
            t = p.stdout.split("timing")[1].split()
            med = float(t[3])
            out[name] = {"median": med, "p90": float(t[5]), "max": float(t[7]), "iterations": int(t[1]), "steps_per_s": 1e6 / med,
                         "streamed": "streaming 1" in p.stdout}  # (the calls travelled to a resident launch: DESIGN.md 4.4)
    return out


def features_leg(pkg, dev_id, n_scans=4096, calls=3):
    """SURVEY.md 8(f) rank 4, the perception front end that feeds the path (houghtransform.cpp:40-280, featuredetector.cpp:74-289) batched
    over many simulated scans: k_features, one workgroup per scan of 181 readings.  Integer / byte work bound by the reference's
    order-dependent peak selection and LDS atomics (4.3 KB in, < 1 KB out per scan: nowhere near HBM), so the record is scans/s of the
    kernel (the library's own hipEvents) with the share of a workgroup's time spent behind the selection; parity is the tests' business
    (tests/test_features.py: votes, peaks, lines bit for bit against the oracle), the leg only checks that repeated scans repeat.  DESIGN.md 4.6."""
    import numpy as np
    base = [pkg.scenarios.simulated_scan(1000 + s) for s in range(64)]
    scans = base * (n_scans // 64)
    fx = pkg.FeatureExtractor(len(scans), max_points=181, max_corners=16, device=dev_id)
    try:
        best = None
        for _ in range(calls):
            corners, n = fx.extract(scans)
            ms = fx.kernel_ms()
            best = ms if best is None or ms < best else best
        tail = fx.tail_share()
    finally:
        fx.close()
    n = np.asarray(n)
    assert np.array_equal(n[:64], n[64:128]), "the same scans give the same corners"
    out = {"unit": "scans/s of 181 readings", "reference": "houghtransform.cpp:40-280,featuredetector.cpp:74-289", "bound": "latency",
           "scans": len(scans), "kernel_ms": best, "value": len(scans) / best * 1e3, "tail_share": tail, "corners": int(n.sum()),
           "frac_of_hbm_peak": len(scans) * (181 * 3 * 8 + 16 * 2 * 8 + 4) / (best * 1e-3) / 1e9 / HBM_PEAK_GBS}
    return out


def propagate_only_leg(pkg, dev_id, K=2048, W=64):
    """BASELINE.json config 3's "roofline for propagate" (Propagate.cpp:15-75, the row update of :53-60): K scripted steps with NO
    measurement (M = 0) at N = 4096 and N = 1024.  Propagate touches the 3x3 robot block and the three robot rows only --
    72 n - 72 algorithmic bytes per step (590 KB at N = 4096: about 0.07 us of HBM time) -- and the chain kernel keeps
    those rows in registers across the steps of a launch, so the record is a LATENCY figure (dependent fp64 arithmetic of the robot
    block, sincos, one workgroup barrier per step), not a bandwidth one: `bound` says so, the GB/s figure is there to show how far
    from a bandwidth question this is.  The pose after K steps is checked against the motion model of Propagate.cpp:33-38."""
    import math
    import numpy as np
    out = {"unit": "us per step (1 Propagate, no measurement)", "reference": "Propagate.cpp:15-75", "bound": "latency"}  # (72 n - 72 bytes per step)
    for name in ("n4096", "n1024"):
        N, _, _, _, seed, extent, _ = WORKLOADS[name]
        x0, P0 = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
        f = pkg.FilterBatch(1, N, device=dev_id)
        f.set_state(x0, P0)
        del P0
        v, w, dt = 0.3, 0.05, 0.05
        ctrl = np.tile(np.array([v, w, dt]), (W + K, 1, 1))
        f.script_load(ctrl, np.zeros((W + K, 0, 1, 2)), np.zeros((W + K, 0, 1, 4)))
        f.script_run(0, W)
        f.sync()
        t0 = time.perf_counter()
        f.timer_start()
        f.script_run(W, K)
        f.flush()
        dev_ms = f.timer_stop()
        f.sync()
        el = time.perf_counter() - t0
        pose = f.poses()[0]
        want = np.array(x0[:3], dtype=np.float64)
        for _ in range(W + K):  # Propagate.cpp:33-38, no angle wrap
            want = want + dt * np.array([v * math.cos(want[2]), v * math.sin(want[2]), w])
        n = 3 + 2 * N
        nbytes = 72 * n - 72
        us = el / K * 1e6
        out[name] = {"steps": K, "us_per_step": us, "device_us_per_step": dev_ms / K * 1e3, "algorithmic_bytes_per_step": nbytes,
                     "frac_of_hbm_peak": nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, "pose_err_vs_motion_model": float(np.abs(pose - want).max())}
        assert out[name]["pose_err_vs_motion_model"] < 1e-9, out[name]
        f.close()
    return out


def config1_leg(pkg, dev_id):
    """BASELINE.json config 1 as stated: one robot, N = 50 landmarks, 1000 steps of synthetic odometry + range/bearing
    measurements (seed 20260001) from x = 0_3, P = 0 (kalmanfilter.cpp:4-12): the GPU as one scripted run, the faithful-dense
    CPU path (the reference's dense passes, one thread) beside it, decision histogram, final-state digests."""
    import numpy as np
    from oracle import oracle_c as oc
    steps, Mx = 1000, 4
    script = pkg.scenarios.lifecycle_script(seed=20260001, n_landmarks=50, steps=steps)
    ctrl = np.zeros((steps, 1, 3))
    z = np.zeros((steps, Mx, 1, 2))
    R = np.zeros((steps, Mx, 1, 4))
    R[..., 0] = R[..., 3] = 1.0
    valid = np.zeros((steps, Mx, 1), dtype=np.uint8)
    for s_, st in enumerate(script):
        ctrl[s_, 0] = (st["v"], st["w"], st["dt"])
        for m, (fx, fy) in enumerate(st["feats_mm"]):
            zz, RR = pkg.scenarios.measurement_from_feature_mm(fx, fy)
            z[s_, m, 0], R[s_, m, 0], valid[s_, m, 0] = zz, RR.ravel(order="F"), 1
    n_meas = int(valid.sum())
    gpu_s = []
    for rep in range(3):  # (the first run pays for first-touch costs)
        f = pkg.FilterBatch(1, 96, device=dev_id, log_capacity=4096)
        f.script_load(ctrl, z, R, valid=valid)
        f.sync()
        t0 = time.perf_counter()
        f.script_run(0, steps)
        f.flush()
        f.sync()
        gpu_s.append(time.perf_counter() - t0)
        if rep == 2:
            dec = f.decisions(0, n_meas)
            xg, Pg = f.get_state()
        f.close()
    oc.build()
    x, P = np.zeros(3), np.zeros((3, 3))
    hist = {oc.NEW: 0, oc.OLD: 0, oc.IGNORE: 0}
    decs = []
    t0 = time.perf_counter()
    for st in script:
        x, P = oc.propagate(x, P, st["v"], st["w"], oc.make_Q(st["v"]), st["dt"], faithful=True)
        for fx, fy in st["feats_mm"]:
            zz, RR = oc.make_measurement(fx, fy)
            x, P, d, mt, _ = oc.update(x, P, zz.reshape(2, 1), RR, faithful=True)
            hist[d[0]] += 1
            decs.append((d[0], mt[0]))
    cpu_t = time.perf_counter() - t0
    same = [(d[0], d[1]) for d in dec] == decs
    scale = float(np.abs(P).max())
    return {"config": "BASELINE.json config 1: N=50, 1000 steps from x=0, P=0 (seed 20260001)",
            "steps": steps, "measurements": n_meas, "decisions": {"new": hist[oc.NEW], "old": hist[oc.OLD], "ignore": hist[oc.IGNORE]},
            "landmarks_final": int((x.size - 3) // 2), "gpu_steps_per_s": steps / min(gpu_s), "gpu_ms_per_step": min(gpu_s) / steps * 1e3,
            "cpu_baseline": {"value": steps / cpu_t, "unit": "steps/s", "cores": 1, "kind": "port",
                             "sample": "all 1000 steps, faithful-dense oracle, %.2f s" % cpu_t},
            "decisions_identical": bool(same), "max_rel_err_x": float(np.abs(xg - x).max() / max(1.0, np.abs(x).max())),
            "max_err_P_over_maxP": float(np.abs(Pg - P).max() / scale),
            "state_digest": {"oracle": pkg.scenarios.state_digest(x, P)[:16], "gpu": pkg.scenarios.state_digest(xg, Pg)[:16],
                             "of": "sha256[:16] over x, P at 9 significant digits"}}


def secondary_in_a_child(args, dev_id):
    """The secondary records (configs 1, 2, 4, M = 1, 512 steps) are measured by a CHILD process after the headline and the CPU
    baselines are in hand: a GPU fault, a hang or a blown time budget in one of them then costs that record, never the line."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--secondary-only", "--device", str(dev_id), "--M", str(args.M), "--max-pending", str(args.max_pending)]
    if args.verbose:
        cmd.append("--verbose")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.secondary_budget)
    except subprocess.TimeoutExpired:
        return {"error": "the secondary legs exceeded their %.0f s budget and were stopped" % args.secondary_budget}
    for l in reversed(p.stdout.splitlines()):
        if l.startswith('{"secondary"'):
            return json.loads(l)["secondary"]
    return {"error": "the secondary legs ended with rc %d: %s" % (p.returncode, p.stderr[-400:])}


def runs_cpu_baseline(rank, world, no_cpu_baseline=False):
    """The CPU legs (14 s of single-thread faithful-dense work and the OpenMP structured leg) are timed by rank 0 of a ONE-rank run
    only: a multi-rank launch -- the driver's scaling runs -- must not start N single-thread CPU jobs beside its GPU ranks (nor one:
    the scaling records are about the GPUs; the baseline rides on the N = 1 line)."""
    return world == 1 and rank == 0 and not no_cpu_baseline


def dry_run(args, rank, world, ekf_env):
    """--dry-run: what a multi-rank run does AROUND the GPU work -- rendezvous, shard_range of both config-5 legs, the equal-size
    all-gather with NaN padding, the max-over-ranks reduction, one line from rank 0 -- on synthetic rows tagged by global filter
    index.  No device, no library: `value` is null and the line says "dry_run"."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    mc = ge.load_package().montecarlo
    if args.dist_backend == "nccl":
        raise SystemExit("--dry-run is a CPU rehearsal: use --dist-backend gloo")
    if world > 1:
        dist.init_process_group(args.dist_backend)
    per_gpu = WORKLOADS["batch256"][1]
    c5 = {"world_size": world}
    for leg, total in (("weak", per_gpu * world), ("strong", 2048)):
        lo, hi = mc.shard_range(total, rank, world)
        local = np.stack([np.arange(lo, hi, dtype=np.float64), 1e6 + np.arange(lo, hi)], axis=1)
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        out = mc.gather_stats(local, total_filters=total)
        el = time.perf_counter() - t0
        if world > 1:
            te = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            el = float(te.item())
        ok = out.shape == (total, 2) and np.array_equal(out[:, 0], np.arange(total)) and np.array_equal(out[:, 1], 1e6 + np.arange(total))
        if not ok:
            raise SystemExit("rank %d: the gathered rows of the %s leg are not in global filter order" % (rank, leg))
        per_rank = [el * 1e3]
        if world > 1:
            tl = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(tl, torch.tensor([el * 1e3], dtype=torch.float64))
            per_rank = [float(t.item()) for t in tl]
        # the record a real run builds (config5_leg_record), with no GPU work behind it: value and the roofline's numbers are None
        c5[leg] = config5_leg_record(total, hi - lo, world, 1, None, out.shape[0], per_rank, el * 1e6, None)
    # which ranks would time the CPU baselines in a real run of this shape (gathered so that the test sees every rank's answer)
    mine = 1.0 if args.full and runs_cpu_baseline(rank, world, args.no_cpu_baseline) else 0.0
    cpu_ranks = [mine]
    if world > 1:
        tl = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tl, torch.tensor([mine], dtype=torch.float64))
        cpu_ranks = [float(t.item()) for t in tl]
    c5["cpu_baseline_ranks"] = [r for r, v in enumerate(cpu_ranks) if v > 0]
    if rank == 0:
        print(json.dumps({"metric": "EKF steps/sec (propagate+full update) at N landmarks", "value": None, "unit": "steps/s", "n_gpus": world,
                          "steps": 0, "warmup": 0, "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": "f64", "data": "synthetic", "dry_run": True, "config": {"workload": "dry run: no GPU work"},
                          "config5": c5, "ekf_environment": ekf_env}))
    if world > 1:
        dist.destroy_process_group()


def self_launch(n):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks as children through torch.distributed.run (the very
    command the driver uses), let rank 0's single JSON line through on stdout, return non-zero if any rank failed."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: RCCL between processes needs it on this driver)
    env.setdefault("OMP_NUM_THREADS", "16")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    for l in p.stdout.splitlines():
        if l not in lines:
            print(l, file=sys.stderr)
    if p.returncode != 0:
        print("bench.py: the %d-rank launch failed (rc %d)" % (n, p.returncode), file=sys.stderr)
        return p.returncode or 1
    if len(lines) != 1:
        print("bench.py: expected one JSON line from rank 0, got %d" % len(lines), file=sys.stderr)
        return 1
    print(lines[0])
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="n4096", choices=sorted(WORKLOADS))
    ap.add_argument("--M", type=int, default=4, help="measurements per step")
    ap.add_argument("--max-pending", type=int, default=0, help="measurements folded per dense pass over P_LL (1 = a dense pass per measurement, as the reference does); "
                    "0 = the workload's own default: 16, and 32 for the batch of one-workgroup filters (k_solo's long window)")
    ap.add_argument("--graph", type=int, default=0, help="replay steps through HIP graphs (one k_chain launch already covers several steps; plain launches keep the per-launch dense-pass events)")
    ap.add_argument("--full", action="store_true", help="besides the headline: the decision check, the chain kernel timed alone and the chain record, "
                    "the CPU baselines, the secondary records, and config 5's legs for --gpus N > 1 or --workload batch256")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (float64; "
                    "a fixed sample of P): the same arguments give the same inputs, so two builds can be compared output for output")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary records (configs 1, 2, 4 and M = 1)")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, the real thing) or gloo (rehearsal of the multi-rank path on a one-GPU box)")
    ap.add_argument("--device", type=int, default=None, help="force a device id (rehearsal only; default LOCAL_RANK)")
    ap.add_argument("--no-flush-profile", action="store_true", help="do not bracket the dense pass with hipEvents")
    ap.add_argument("--no-config5", action="store_true", help="with --full: skip the config-5 legs (256 filters/GPU weak, 2048 filters strong)")
    ap.add_argument("--config5-steps", type=int, default=None, help="timed steps of the config-5 legs (default: the batch256 workload's 200)")
    ap.add_argument("--secondary-only", action="store_true", help="(internal) run only the secondary records and print them: bench.py starts itself this way as a child, so that a fault or a hang in a secondary leg cannot cost the headline")
    ap.add_argument("--secondary-budget", type=float, default=420.0, help="wall-clock limit in seconds of the child that measures the secondary records")
    ap.add_argument("--cpu-structured-child", action="store_true", help="(internal) one timed run of the structured CPU oracle in a process whose OpenMP runtime starts with the pinning variables set")
    ap.add_argument("--threads", type=int, default=1, help="(internal) OpenMP threads of --cpu-structured-child")
    ap.add_argument("--verbose", action="store_true", help="put the prose fields (byte model, window note, environment notes) on the JSON line; the default line carries numbers and stays under 8 KB (the driver keeps an 8 KB tail)")
    ap.add_argument("--config5", action="store_true", help="run both config-5 legs (weak 256 filters/GPU, strong 2048 in all) whatever the world size; with --full they run for --gpus N > 1, and the weak leg alone rides on a one-GPU --workload batch256 line")
    ap.add_argument("--dry-run", action="store_true", help="launcher / rendezvous / shard / all-gather plumbing only, no GPU work: every rank gathers synthetic per-filter rows of its config-5 shards (CPU rehearsal, gloo)")
    args = ap.parse_args()
    if args.cpu_structured_child:
        return cpu_structured_child(args.workload, args.M, args.threads)
    global VERBOSE
    VERBOSE = bool(args.verbose)
    ekf_env = ekf_environment()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
            # plain `python bench.py --gpus N`: this process becomes the launcher.  Nothing here has touched the GPU yet (no torch.cuda,
            # no HIP library), and the ranks are CHILD processes -- never an exec of a process that holds the device
            raise SystemExit(self_launch(args.gpus))
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))

    if args.dry_run:
        return dry_run(args, rank, world, ekf_env)

    import numpy as np
    import torch  # imported before the HIP library so that one HIP runtime (torch's) serves both

    import __graft_entry__ as ge
    pkg = ge.load_package()
    mc = pkg.montecarlo

    N, B, d_steps, d_warm, seed, extent, min_sep = WORKLOADS[args.workload]
    K = args.steps if args.steps is not None else d_steps
    W = args.warmup if args.warmup is not None else d_warm
    M = args.M

    dev_id = local_rank if args.device is None else args.device
    torch.cuda.set_device(dev_id)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_id))
        else:
            dist.init_process_group(args.dist_backend)
    coll_device = torch.device("cuda", dev_id) if args.dist_backend == "nccl" else torch.device("cpu")

    # ---- the headline: inputs built on the host and moved to HBM (untimed), warm-up (untimed), exactly K timed steps -------
    head = None if args.secondary_only else measure(pkg, mc, torch, dist, coll_device, rank, world, dev_id, args.workload, K, W, M, args.max_pending, bool(args.graph),
                                                    not args.no_flush_profile, check=args.full, alone=args.full, dump_dir=args.dump_outputs if rank == 0 else None)

    config5 = None
    if not args.secondary_only and not args.no_config5 and (args.config5 or (args.full and (world > 1 or args.workload == "batch256"))):
        legs = ("weak", "strong") if (world > 1 or args.config5) else ("weak",)  # (one GPU, --workload batch256: the weak leg is config 4 itself, carrying config 5's keys)
        config5 = config5_legs(pkg, mc, torch, dist, coll_device, rank, world, dev_id, M, args.max_pending, args.config5_steps, legs)

    # ---- secondary records on the same line (one GPU only): the other BASELINE.json configurations a single GPU holds, each with
    # its own roofline, so that the driver's one command puts a number behind every one of them
    secondary = None
    if args.secondary_only:
        secondary = {}
        def leg(name, fn):
            try:
                secondary[name] = fn()
            except Exception as e:  # a secondary record must not cost the headline
                secondary[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        def summarise(r, unit="steps/s"):
            out = {"workload": "%s B%d M%d w%d ov%d K%d W%d P%d" % (r["workload"], r["B"], r["M"], r["window"], r["overlap"], r["K"], r["W"], r["prime_steps"]),  # (batch, measurements per step, window, overlap, timed / warm-up / prime steps)
                   "value": r["value"], "unit": unit, "ms_per_step": r["elapsed"] / r["K"] * 1e3,
                   "device_us_per_measurement": r["dev_ms"] * 1e3 / (r["K"] * r["M"]),
                   "host_minus_device_us": r["phases_us"]["host_minus_device"],
                   "roofline": r["roofline"] if VERBOSE else slim_roofline(r["roofline"])}
            if r["latency"]:
                out["per_step_latency"] = r["latency"]
            return out
        leg("config2_n1024", lambda: summarise(measure(pkg, mc, torch, None, coll_device, 0, 1, dev_id, "n1024", 200, 10, M, args.max_pending, False, True, latency=True)))
        leg("config4_batch256", lambda: summarise(measure(pkg, mc, torch, None, coll_device, 0, 1, dev_id, "batch256", 200, 10, M, args.max_pending, False, True, alone=False), "filter-steps/s"))
        leg("config3_M1", lambda: summarise(measure(pkg, mc, torch, None, coll_device, 0, 1, dev_id, "n4096", 512, 32, 1, args.max_pending, False, True, alone=False)))
        leg("config3_512_steps", lambda: summarise(measure(pkg, mc, torch, None, coll_device, 0, 1, dev_id, "n4096", 512, 32, M, args.max_pending, False, True, alone=False)))
        # the library's DEFAULT window (16; rounds 1-4 measured the headline there) beside the bench's window of 32: round-over-round comparability
        leg("config3_512_steps_w16", lambda: summarise(measure(pkg, mc, torch, None, coll_device, 0, 1, dev_id, "n4096", 512, 32, M, 16, False, True, alone=False)))
        leg("config1_n50", lambda: config1_leg(pkg, dev_id))
        leg("immediate_calls", lambda: immediate_leg(pkg, dev_id))
        leg("propagate_only", lambda: propagate_only_leg(pkg, dev_id))
        leg("features", lambda: features_leg(pkg, dev_id))
        print(json.dumps({"secondary": secondary}))
        return

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    cpu = cpu_strong = None
    if args.full and runs_cpu_baseline(rank, world, args.no_cpu_baseline):
        cpu = cpu_baseline(pkg, N, M, seed, extent, min_sep)
        cpu_strong = cpu_baseline_structured(args.workload, M)
        if cpu and cpu_strong and cpu_strong.get("value"):
            cpu_strong["gpu_over_cpu"] = {"faithful_dense_1_thread": head["value"] / cpu["value"], "structured_all_cores": head["value"] / cpu_strong["value"],
                                          }  # (a ratio says nothing about kernel quality; the roofline does)

    if args.full and world == 1 and not args.no_secondary and args.workload == "n4096":
        secondary = secondary_in_a_child(args, dev_id)

    chain = None
    if args.full and B == 1:
        pipe = None
        if secondary and isinstance(secondary.get("config3_512_steps"), dict) and args.workload == "n4096":
            pipe = secondary["config3_512_steps"].get("device_us_per_measurement")
        chain = chain_record(args.workload, head["window"], head["overlap"], head["chain_alone_us"], pipe)
    rep = head["report"]
    # the steady workload feeds 0.5-sigma measurement noise and a noise-free truth (margins
    # for the gate), so NIS/NEES below their dof are expected here; the chi-square verdict is for config 1 style runs
    mc_stats = None if rep is None else {k: (None if v is None else {"mean": v["mean"], "dof": v["dof"], "filters": v["filters"]}) for k, v in rep.items()}
    elapsed, dev_ms, window = head["elapsed"], head["dev_ms"], head["window"]
    line = {
        "metric": "EKF steps/sec (propagate+full update) at N landmarks",
        "value": head["value"],
        "unit": "steps/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": elapsed / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "%s: %d filter(s)/GPU, N=%d landmarks (n=%d, dense P %.1f MB fp64), M=%d Old updates/step, max_pending=%d, overlap=%d, graph=%d"
                               % (args.workload, B, N, 3 + 2 * N, (3 + 2 * N) ** 2 * 8 / 1e6, M, window, head["overlap"], args.graph),
                   "N": N, "filters_per_gpu": B, "M": M, "max_pending": window, "overlap": head["overlap"]},
        "device_ms_per_step": dev_ms / K,
        "prime_steps": head["prime_steps"],   # untimed script steps in front of the warm-up (prime_steps_for): not part of `warmup`, not timed
        "phases_us": head["phases_us"],       # where the timed region's host-clock time went (timed_steps)
        "max_pending": window,
        "window_is_library_default": window == 16,  # (ekf_default_params: 16; secondary.config3_512_steps_w16 is the default-window figure)
        "roofline": head["roofline"],
        "chain": chain,
        "cpu_baseline": cpu,
        "cpu_baseline_structured": cpu_strong,
        "per_update_us": elapsed / (K * M) * 1e6,
        "mc_stats": mc_stats,
        "config5": config5,
        "secondary": secondary,
        "multi_gpu_note": "no scaling curve measured by the builder (one-GPU boxes)",
        "ekf_environment": ekf_env,
    }
    full = {k: line[k] for k in ("value", "ms_per_step")}
    if not VERBOSE:
        line = compact(line)
        line.update(full)  # the two figures the driver checks against its own clock stay exact
    print(json.dumps(line, separators=(",", ":")))
    if dist is not None:
        dist.destroy_process_group()


def cpu_baseline(pkg, N, M, seed, extent, min_sep):
    """The oracle's faithful-dense path (same dense O(n^2) passes as the reference, 1 thread: the
    reference's Makefile:2 has no OpenMP) timed on this host on a bounded sample of the same workload."""
    import numpy as np

    from oracle import oracle_c as oc

    sample_steps = {4096: 4, 1024: 40, 256: 400}.get(N, 2)  # about 10-20 s of single-thread CPU work
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
    sc = pkg.scenarios.steady_script(x, steps=sample_steps, M=M, seed=seed + 7919, min_separation=min_sep)
    oc.build()
    per_step = []
    for s in range(sample_steps):
        t0 = time.perf_counter()
        v, w, dt = sc["ctrl"][s]
        x, P = oc.propagate(x, P, v, w, oc.make_Q(v), dt, faithful=True)
        for m in range(M):
            x, P, dec, _, _ = oc.update(x, P, sc["z"][s, m].reshape(2, 1), sc["R"][s, m].reshape(2, 2, order="F"), faithful=True)
            assert dec == [oc.OLD]
        per_step.append(time.perf_counter() - t0)
    t = sum(per_step)
    ps = np.array(per_step)
    return {"value": sample_steps / t, "unit": "steps/s", "cores": 1, "kind": "port",
            "sample": "%d step(s) of the same workload (1 Propagate + %d Old Updates) at N=%d, faithful-dense oracle, %.1f s" % (sample_steps, M, N, t),
            "seconds_per_step": {"median": float(np.median(ps)), "p10": float(np.percentile(ps, 10)), "p90": float(np.percentile(ps, 90))},
            "host": host_cpu_record(), "compiler_flags": "gcc -O3 -march=x86-64-v3 -ffp-contract=off"}


def cgroup_cpu_quota():
    """CPUs' worth of time the container may use per period (cgroup v2 cpu.max, v1 cfs_quota_us / cfs_period_us), None = unlimited."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def cpu_structured_child(workload, M, threads):
    """(internal: --cpu-structured-child) one timed structured-oracle run in THIS process, whose OpenMP runtime was started with the
    pinning variables of cpu_baseline_structured in its environment.  Prints one JSON object."""
    import numpy as np
    import __graft_entry__ as ge
    from oracle import oracle_c as oc
    pkg = ge.load_package()
    N, _, _, _, seed, extent, min_sep = WORKLOADS[workload]
    sample_steps = {4096: 40, 1024: 400, 256: 2000}.get(N, 20)
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
    sc = pkg.scenarios.steady_script(x, steps=sample_steps + 2, M=M, seed=seed + 7919, min_separation=min_sep)
    oc.build()
    oc.set_threads(threads)
    ses = oc.Session(x, P, first_touch=True)  # the pages of P are first written inside the parallel region that later updates them
    del P
    t0 = None
    per_step = []
    for s in range(sample_steps + 2):
        ts = time.perf_counter()
        if s == 2:
            t0 = ts   # (two warm-up steps: thread start, caches)
        v, w, dt = sc["ctrl"][s]
        ses.propagate(v, w, oc.make_Q(v), dt)
        for m in range(M):
            dec, _, _ = ses.update(sc["z"][s, m].reshape(2, 1), sc["R"][s, m].reshape(2, 2, order="F"))
            assert dec == [oc.OLD]
        if s >= 2:
            per_step.append(time.perf_counter() - ts)
            if len(per_step) >= 4 and time.perf_counter() - t0 > 15.0:  # (bounded: an oversubscribed host must not hold the bench line for a minute)
                sample_steps = len(per_step)
                break
    t = time.perf_counter() - t0
    ps = np.array(per_step)
    print(json.dumps({"cpu_structured": {"value": sample_steps / t, "unit": "steps/s", "cores": threads, "kind": "port", "seconds": t, "sample_steps": sample_steps, "N": N,
                                         "seconds_per_step": {"median": float(np.median(ps)), "p10": float(np.percentile(ps, 10)), "p90": float(np.percentile(ps, 90))},
                                         "omp": {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OMP_PROC_BIND", "OMP_PLACES")}}}))


def cpu_baseline_structured(workload, M):
    """The strong CPU baseline of SURVEY.md 8(d)(ii): the oracle's structured mode (state advanced in place, only the O(n) rows and
    the one rank-2 pass over P per update, OpenMP over the element-wise loops) on ALL cores this process may use
    (os.sched_getaffinity), threads pinned (OMP_PROC_BIND=spread, OMP_PLACES=threads) and P first touched inside the parallel region
    that updates it -- and, beside it, the 16-thread figure of rounds 2-4 (a one-GPU share of the host).  Each run is a child
    process: the pinning variables are read when the OpenMP runtime starts, which in this process happened long ago (torch).
    Not the reference's algorithmic cost -- what a CPU can do with the same restructuring."""
    import subprocess
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = os.cpu_count() or 1
    # "all cores" = every CPU this process may really use: the affinity mask, capped by the container's CPU quota (a one-GPU share of
    # a 256-thread host shows 256 CPUs in the mask and a cgroup quota of 16: 256 threads on that quota ran at 0.9 steps/s against
    # 18.9 for 16 -- throttled, not parallel)
    quota = cgroup_cpu_quota()
    ncpu = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    runs = {}
    for label, threads in (("all_cores", ncpu), ("threads_16", min(16, ncpu))):
        if label == "threads_16" and threads == ncpu:
            runs[label] = runs["all_cores"]
            continue
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
        env.update({"OMP_NUM_THREADS": str(threads), "OMP_PROC_BIND": "spread", "OMP_PLACES": "threads", "OMP_DYNAMIC": "false"})
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-structured-child", "--workload", workload, "--M", str(M), "--threads", str(threads)]
        try:
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            runs[label] = {"error": "timed out"}
            continue
        rec = None
        for l in reversed(p.stdout.splitlines()):
            if l.startswith('{"cpu_structured"'):
                rec = json.loads(l)["cpu_structured"]
                break
        runs[label] = rec if rec else {"error": "rc %d: %s" % (p.returncode, p.stderr[-300:])}
    ok = {k: v for k, v in runs.items() if v and "error" not in v}
    if not ok:
        return {"value": None, "unit": "steps/s", "cores": ncpu, "kind": "port", "sample": str(runs), "all_cores": runs.get("all_cores"), "threads_16": runs.get("threads_16")}
    # the strong baseline is the FASTER of the two (a host whose cores are shared or throttled without a visible quota can be slower
    # with every thread it shows than with sixteen); both runs are in the record
    best = max(ok.values(), key=lambda v: v["value"])
    def brief(v):
        return v if not v or "error" in v else {k: v[k] for k in ("value", "cores", "seconds", "sample_steps") if k in v}
    same = runs.get("threads_16") is runs.get("all_cores")
    return {"value": best["value"], "unit": "steps/s", "cores": best["cores"], "kind": "port", "all_cores": brief(runs.get("all_cores")),
            "sample": "%d step(s) of the same workload at N=%d, structured oracle, %d OpenMP threads, %.1f s"
                      % (best["sample_steps"], best["N"], best["cores"], best["seconds"]),
            "seconds_per_step": best["seconds_per_step"],
            "pinning": {"OMP_PROC_BIND": "spread", "OMP_PLACES": "threads", "first_touch": "parallel", "affinity_cpus": affinity,
                        "cgroup_cpu_quota": quota, "threads": "min(affinity, quota)"},
            "threads_16": "= all_cores" if same else brief(runs.get("threads_16"))}


if __name__ == "__main__":
    main()
