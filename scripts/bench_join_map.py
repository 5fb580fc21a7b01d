#!/usr/bin/env python3
"""Map joining (ekf_join_map / ekf_batch_join_map): one JSON line per case.

Cases: Ns = 256 into Ng = 3840 (capacity 4096) and Ns = 64 into Ng = 960 (capacity 1024), each in both pipeline modes of the
destination (EKF_OVERLAP=0/1), and the batch form at 256 filters x (128 + 64, capacity 256).  The source handle has the capacity of
its own map.  The parent process never opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first
failing child ends the run.  Between two timed joins the destination is cut back to Ng landmarks on the device
(ekf_remove_landmarks), so every repetition joins into the same layout.  Each line carries
  wall_us             the call's wall time with both handles settled (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels (k_join_tiles, k_join_vec, k_join_finish) from a second child of the case under
                      `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over the child's calls, all values kept)
  bytes               algorithmic bytes of the tile kernel: the destination tiles that hold a new column, written once, plus the
                      source's stored tiles, read once; and bytes / tile-kernel time as a fraction of 8 TB/s
  dense_pass_us       yardstick 1, same process, the destination handle: one in-place dense pass folding a one-slot window (ekf_flush
                      under ekf_flush_profile), which reads and writes ALL of P.  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass: the batch), where no dense-pass launch exists to time
  host_round_trip_ms  yardstick 2, same process: get_state of both filters -> NumPy (tests/join_ref.py, the block table) ->
                      set_state of filter 0 (the batch: times 256 is quoted as an estimate)
usage: python3 scripts/bench_join_map.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/join_map.jsonl]
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
CASES = ["n4096_inplace", "n4096_overlap", "n1024_inplace", "n1024_overlap", "batch256_inplace"]
KERNELS = ("k_join_tiles", "k_join_vec", "k_join_finish")
CHILD_TIMEOUT = 420


def parse(case):
    size, mode = case.split("_")
    if size == "batch256":
        return dict(B=256, Ng=128, Ns=64, cap=256, cap_s=64, overlap=mode == "overlap")
    cap = int(size[1:])
    Ns = cap // 16
    return dict(B=1, Ng=cap - Ns, Ns=Ns, cap=cap, cap_s=Ns, overlap=mode == "overlap")


def algorithmic_bytes(c):
    J0, J1 = c["Ng"] // 32, (2 * (c["Ng"] + c["Ns"]) + 63) // 64
    Ts = (2 * c["Ns"] + 63) // 64
    return c["B"] * (J1 * (J1 + 1) // 2 - J0 * (J0 + 1) // 2 + Ts * (Ts + 1) // 2) * 4096 * 8


def child(case, reps, baselines):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    c = parse(case)
    B, Ng, Ns = c["B"], c["Ng"], c["Ns"]
    os.environ["EKF_OVERLAP"] = "1" if c["overlap"] else "0"
    f = pkg.FilterBatch(B, c["cap"])
    os.environ["EKF_OVERLAP"] = "0"
    s = pkg.FilterBatch(B, c["cap_s"])
    xg, Pg = pkg.scenarios.injected_state(Ng, seed=7, extent=12.0 * (Ng / 64.0) ** 0.5 + 8.0)
    xs, Ps = pkg.scenarios.injected_state(Ns, seed=9, extent=8.0)
    for h, (x0, P0) in ((f, (xg, Pg)), (s, (xs, Ps))):
        h.set_state(x0, P0, 0)
        if B > 1:
            h.broadcast_state()
    line = dict(case=case, Ng=Ng, Ns=Ns, batch=B, overlap=bool(f.overlap), bytes=algorithmic_bytes(c))
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick 1: one dense pass over all of P, folding a one-slot window
            sc = pkg.scenarios.steady_script(xg, steps=1, M=1, seed=8, min_separation=1.0)
            z1 = np.tile(sc["z"][0, 0].reshape(1, 1, 2), (B, 1, 1))
            R1 = np.tile(sc["R"][0, 0].reshape(1, 1, 2, 2, order="F"), (B, 1, 1, 1))
            passes = []
            for r in range(3):
                f.set_state(xg, Pg, 0)
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
            line["dense_pass_us_all"] = [round(p, 1) for p in passes]
            f.set_state(xg, Pg, 0)
    keep = np.zeros((B, Ng + Ns), dtype=bool)
    keep[:, :Ng] = True
    wall = []
    for r in range(reps):
        f.sync(), s.sync()
        t0 = time.perf_counter()
        if B > 1:
            f.batch_join_map(s)
        else:
            f.join_map(s)
        wall.append((time.perf_counter() - t0) * 1e6)
        assert int(f.num_landmarks()[0]) == Ng + Ns
        f.remove_landmarks(keep if B > 1 else keep[0], index=None if B > 1 else 0)  # back to Ng landmarks, on the device
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        import join_ref as jr
        f.set_state(xg, Pg, 0)
        f.sync()
        t0 = time.perf_counter()
        a, b = f.get_state(0), s.get_state(0)
        xn, Pn = jr.join_blocks(a[0], a[1], b[0], b[1])
        f.set_state(xn, Pn, 0)
        line["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
        if B > 1:
            line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * B
    f.close(), s.close()
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
        run_child(case, reps, False, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "jm", "--"])
        rows = []
        for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    for k in KERNELS:
                        if k in row["Kernel_Name"]:
                            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
    rows.sort()
    calls, cur = [], {}
    for st, en, k in rows:  # every call ends with one k_join_finish
        cur[k] = cur.get(k, 0.0) + (en - st) / 1e3
        if k == "k_join_finish":
            calls.append(cur)
            cur = {}
    if len(calls) != reps:
        raise SystemExit("%s: expected %d calls in the trace, found %d" % (case, reps, len(calls)))
    return dict(kernel_us=statistics.median(sum(m.values()) for m in calls),
                split_us={k: statistics.median(m.get(k, 0.0) for m in calls) for k in KERNELS},
                tiles_us_all=[round(m.get("k_join_tiles", 0.0), 2) for m in calls])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--kernel-trace", action="store_true", help="also run every case in a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, not a.no_baselines)
        return
    lines = []
    for case in [c for c in a.cases.split(",") if c]:
        line = run_child(case, a.reps, not a.no_baselines)
        if a.kernel_trace:
            line.update(kernel_trace(case, a.reps))
            t_us = line["split_us"]["k_join_tiles"]
            line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / HBM_PEAK if t_us > 0 else None
            if line.get("dense_pass_us"):
                line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
                line["kernels_vs_dense_pass"] = line["kernel_us"] / line["dense_pass_us"]
        if line.get("host_round_trip_ms"):
            line["wall_vs_host_round_trip"] = line["wall_us"] / (line["host_round_trip_ms"] * 1e3)
        line = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in line.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every case: a later failure keeps what was measured)
            with open(a.out, "w") as fh:
                for ln in lines:
                    fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
