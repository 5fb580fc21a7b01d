#!/usr/bin/env python3
"""Frame changes (ekf_transform_frame / ekf_anchor_at_robot and their batch forms): one JSON line per case.

Cases: N = 4096 and N = 1024 landmarks in both pipeline modes (EKF_OVERLAP=0/1) and the batch of 256 filters x 256 landmarks, each
with the rigid transform and the anchor.  The parent process never opens the GPU: every case runs in a child of its own under
`timeout -k 10`, and the first failing child ends the run.  Each line carries
  wall_us             the call's wall time on a settled handle (median of --reps; the call synchronises)
  kernel_us, split_us the call's own kernels (k_reframe_vec, k_reframe_tiles, k_reframe_finish) from a second child of the case under
                      `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over the child's calls)
  bytes               algorithmic bytes of the tile kernel (one read and one write of every live chain) and bytes / tile-kernel time
                      as a fraction of 8 TB/s
  dense_pass_us       yardstick 1, same process, same handle: one in-place dense pass folding a one-slot window (ekf_flush under
                      ekf_flush_profile; the same bytes as the tile kernel).  null for handles whose chain kernel folds its own windows
                      (ekf_fused_pass: the batch), where no dense-pass launch exists to time
  host_round_trip_ms  yardstick 2, same process: get_state -> NumPy (tests/reframe_ref.py, blockwise) -> set_state of filter 0
                      (the batch: times 256 is quoted as an estimate)
  tile_vs_dense_pass, wall_vs_host_round_trip   the two ratios the write-up quotes
--pmc COUNTERS adds a third child per case under `rocprofv3 --pmc` alone (counters are never collected together with a trace).
usage: python3 scripts/bench_reframe.py [--reps 5] [--kernel-trace] [--pmc SQ_WAVES,...] [--cases a,b] [--out profiles/reframe.jsonl]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
FRAME = (3.0, -2.0, 0.7)
CASES = ["%s_%s_%s" % (size, mode, call) for size in ("n4096", "n1024", "batch256") for mode in ("inplace", "overlap") for call in ("rigid", "anchor")]
KERNELS = ("k_reframe_vec", "k_reframe_tiles", "k_reframe_finish")
CHILD_TIMEOUT = 420


def parse(case):
    size, mode, call = case.split("_")
    if size == "batch256":
        return dict(B=256, N=256, cap=256, overlap=mode == "overlap", call=call)
    N = int(size[1:])
    return dict(B=1, N=N, cap=N, overlap=mode == "overlap", call=call)


def algorithmic_bytes(c):
    nT = (2 * c["N"] + 63) // 64
    chains = 16 * nT * (nT + 1) // 2 - 6 * nT  # (the six dead chains of every diagonal tile are skipped)
    return c["B"] * chains * 256 * 8 * 2


def child(case, reps, baselines):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    c = parse(case)
    os.environ["EKF_OVERLAP"] = "1" if c["overlap"] else "0"
    f = pkg.FilterBatch(c["B"], c["cap"])
    x0, P0 = pkg.scenarios.injected_state(c["N"], seed=7, extent=12.0 * (c["N"] / 64.0) ** 0.5 + 8.0)
    f.set_state(x0, P0, 0)
    if c["B"] > 1:
        f.broadcast_state()
    line = dict(case=case, N=c["N"], batch=c["B"], overlap=bool(f.overlap), call=c["call"], bytes=algorithmic_bytes(c))
    if baselines:
        # yardstick 1: one dense pass over the same tiles, folding a one-slot window
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:
            sc = pkg.scenarios.steady_script(x0, steps=1, M=1, seed=8, min_separation=1.0)
            passes = []
            z1 = np.tile(sc["z"][0, 0].reshape(1, 1, 2), (c["B"], 1, 1))
            R1 = np.tile(sc["R"][0, 0].reshape(1, 1, 2, 2, order="F"), (c["B"], 1, 1, 1))
            for r in range(3):
                f.set_state(x0, P0, 0)
                if c["B"] > 1:
                    f.broadcast_state()
                f.propagate(*sc["ctrl"][0])
                f.update(z1, R1, want_decisions=False)
                f.sync()
                n0, ms0 = f.flush_profile_read() if r else (0, 0.0)
                f.flush_profile(1)
                f.flush()
                f.sync()
                n1, ms1 = f.flush_profile_read()
                f.flush_profile(0)
                if n1 - n0 == 1:
                    passes.append((ms1 - ms0) * 1e3)
            line["dense_pass_us"] = statistics.median(passes) if passes else None
            f.set_state(x0, P0, 0)
            if c["B"] > 1:
                f.broadcast_state()
    frames = np.tile(np.array(FRAME), (c["B"], 1))
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        if c["call"] == "rigid":
            f.transform_frame(frames) if c["B"] > 1 else f.transform_frame(FRAME, index=0)
        else:
            f.anchor_at_robot() if c["B"] > 1 else f.anchor_at_robot(index=0)
        wall.append((time.perf_counter() - t0) * 1e6)
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        import reframe_ref as rr
        f.set_state(x0, P0, 0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        xn, Pn = rr.rigid(x, P, FRAME) if c["call"] == "rigid" else rr.anchor(x, P)
        f.set_state(xn, Pn, 0)
        line["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
        if c["B"] > 1:
            line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * c["B"]
    f.close()
    print("RESULT " + json.dumps(line), flush=True)


def run_child(case, reps, baselines, prefix=()):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(reps)]
    if not baselines:
        cmd.append("--no-baselines")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("child of case %s failed (%d); nothing more is started:\n%s" % (case, r.returncode, (r.stdout + r.stderr)[-3000:]))
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("child of case %s printed no result:\n%s" % (case, r.stdout[-2000:]))


def kernel_trace(case, reps):
    """The case again in a child under rocprofv3 (the program after --): the kernels' durations per call."""
    with tempfile.TemporaryDirectory() as d:
        run_child(case, reps, False, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rf", "--"])
        rows = []
        for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    for k in KERNELS:
                        if k in row["Kernel_Name"]:
                            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
        stats = [row for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for row in csv.DictReader(open(fn))
                 if any(k in row.get("Name", "") for k in KERNELS)]
    rows.sort()
    calls, cur = [], {}
    for s, e, k in rows:  # every call ends with one k_reframe_finish
        cur[k] = cur.get(k, 0.0) + (e - s) / 1e3
        if k == "k_reframe_finish":
            calls.append(cur)
            cur = {}
    if len(calls) != reps:
        raise SystemExit("%s: expected %d calls in the trace, found %d" % (case, reps, len(calls)))
    return dict(kernel_us=statistics.median(sum(m.values()) for m in calls),
                split_us={k: statistics.median(m.get(k, 0.0) for m in calls) for k in KERNELS}), stats


def pmc_run(case, counters):
    with tempfile.TemporaryDirectory() as d:
        run_child(case, 1, False, prefix=["rocprofv3", "--pmc"] + counters.split(",") + ["--output-format", "csv", "-d", d, "-o", "rf", "--"])
        out = {}
        for fn in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                if "k_reframe_tiles" in row.get("Kernel_Name", ""):
                    out[row["Counter_Name"]] = out.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--kernel-trace", action="store_true", help="also run every case in a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--pmc", default=None, help="comma-separated counters, collected in a run of their own")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, not a.no_baselines)
        return
    lines, all_stats = [], {}
    for case in [c for c in a.cases.split(",") if c]:
        line = run_child(case, a.reps, not a.no_baselines)
        if a.kernel_trace:
            traced, stats = kernel_trace(case, 3)
            line.update(traced)
            all_stats[case] = stats
            t_us = traced["split_us"]["k_reframe_tiles"]
            line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / HBM_PEAK if t_us > 0 else None
            if line.get("dense_pass_us"):
                line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
        if a.pmc:
            line["pmc_tiles"] = pmc_run(case, a.pmc)
        if line.get("host_round_trip_ms"):
            line["wall_vs_host_round_trip"] = line["wall_us"] / (line["host_round_trip_ms"] * 1e3)
        line = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in line.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every case: a later failure keeps what was measured)
            with open(a.out, "w") as fh:
                for ln in lines:
                    fh.write(json.dumps(ln) + "\n")
    if a.out and all_stats:
        with open(os.path.splitext(a.out)[0] + "_kernel_stats.json", "w") as fh:
            json.dump(all_stats, fh, indent=1)


if __name__ == "__main__":
    main()
