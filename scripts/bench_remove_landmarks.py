#!/usr/bin/env python3
"""Landmark removal (ekf_remove_landmarks / ekf_batch_remove_landmarks): one JSON line per case.

Cases: N = 1024 and 4096 landmarks, 1 % of them spread out or one contiguous block of 64 removed, both pipeline modes (EKF_OVERLAP=0/1),
and the batch of 256 filters x 256 landmarks (a different 1 % .. 10 % mask per filter).  Each line carries
  wall_us          the call's wall time (median of --reps; the call synchronises)
  kernel_us        the removal's own kernels (k_rm_gather, k_rm_finish, k_rm_vec) per call, from a child run of this script under
                   `rocprofv3 --kernel-trace --stats` (--kernel-trace; median of the child's calls), and their split
  bytes            algorithmic bytes of those kernels (the gather's tile reads and writes, the copy-back or the clearing of the other
                   buffer; x / R / D and the maps are negligible) and bytes / kernel time as a fraction of 8 TB/s
  host_round_trip_ms   get_state -> np.delete -> set_state (one filter; the batch: filter 0 only, times 256 is quoted)
  dense_detour_ms      ekf_reserve(capacity + 32): every filter through k_export -> dense n x n -> k_import on the device, the path a removal
                   through the existing entry points would take on the device
usage: python3 scripts/bench_remove_landmarks.py [--reps 5] [--kernel-trace] [--out FILE]
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

HBM_PEAK = 8.0e12
TILE_BYTES = 4096 * 8
CASES = ["n1024_spread_inplace", "n1024_spread_overlap", "n1024_block64_inplace", "n1024_block64_overlap",
         "n4096_spread_inplace", "n4096_spread_overlap", "n4096_block64_inplace", "n4096_block64_overlap",
         "batch256_inplace", "batch256_overlap"]
RM_KERNELS = ("k_rm_gather", "k_rm_finish", "k_rm_vec")


def parse(case):
    parts = case.split("_")
    mode = parts[-1]
    if parts[0] == "batch256":
        return dict(B=256, N=256, cap=256, pattern="batch", overlap=mode == "overlap")
    N = int(parts[0][1:])
    return dict(B=1, N=N, cap=N, pattern=parts[1], overlap=mode == "overlap")


def masks(c, rng):
    import numpy as np
    keep = np.ones((c["B"], c["N"]), dtype=bool)
    for b in range(c["B"]):
        if c["pattern"] == "spread":
            keep[b, rng.choice(c["N"], size=max(1, c["N"] // 100), replace=False)] = False
        elif c["pattern"] == "block64":
            keep[b, c["N"] // 3:c["N"] // 3 + 64] = False
        else:
            keep[b, rng.choice(c["N"], size=int(rng.integers(c["N"] // 100, c["N"] // 10 + 1)), replace=False)] = False
    return keep


def algorithmic_bytes(c, keep):
    total = 0
    for b in range(c["B"]):
        n_old, n_new = c["N"], int(keep[b].sum())
        to, tn = (2 * n_old + 63) // 64, (2 * n_new + 63) // 64
        t_old, t_new = to * (to + 1) // 2, tn * (tn + 1) // 2
        if c["overlap"]:
            total += (t_new + t_old + t_old) * TILE_BYTES  # gather: sources read, every old-map tile written; the read buffer cleared
        elif n_new != n_old:
            total += (t_new + t_new + t_new + t_old) * TILE_BYTES  # gather into scratch (read, write), copy back (read, write / clear)
    return total


def make(pkg, c, seed=7):
    import numpy as np
    os.environ["EKF_OVERLAP"] = "1" if c["overlap"] else "0"
    f = pkg.FilterBatch(c["B"], c["cap"])
    x0, P0 = pkg.scenarios.injected_state(c["N"], seed=seed, extent=12.0 * (c["N"] / 64.0) ** 0.5 + 8.0)
    f.set_state(x0, P0, 0)
    if c["B"] > 1:
        f.broadcast_state()
    return f, x0, P0


def run_case(pkg, name, reps, baselines):
    import numpy as np
    c = parse(name)
    rng = np.random.default_rng(11)
    keep = masks(c, rng)
    f, x0, P0 = make(pkg, c)
    wall = []
    for r in range(reps):
        if r:
            f.set_state(x0, P0, 0)
            if c["B"] > 1:
                f.broadcast_state()
        f.sync()
        t0 = time.perf_counter()
        f.remove_landmarks(keep) if c["B"] > 1 else f.remove_landmarks(keep[0], index=0)
        wall.append((time.perf_counter() - t0) * 1e6)
    line = dict(case=name, N=c["N"], batch=c["B"], overlap=bool(f.overlap), removed_per_filter_mean=float((~keep).sum(1).mean()),
                wall_us=statistics.median(wall), wall_us_all=[round(w, 1) for w in wall], bytes=algorithmic_bytes(c, keep))
    if baselines:
        f.set_state(x0, P0, 0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        rows = np.flatnonzero(np.concatenate([np.ones(3, dtype=bool), np.repeat(keep[0], 2)]))
        f.set_state(x[rows], P[np.ix_(rows, rows)], 0)
        line["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
        if c["B"] > 1:
            line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * c["B"]
        f.set_state(x0, P0, 0)
        if c["B"] > 1:
            f.broadcast_state()
        f.sync()
        t0 = time.perf_counter()
        f.reserve(c["cap"] + 32)
        line["dense_detour_ms"] = (time.perf_counter() - t0) * 1e3
    f.close()
    return line


def kernel_trace(cases, reps):
    """This script again under rocprofv3 (a child process, the program after --): the removal kernels' durations per call."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rm", "--", sys.executable, os.path.abspath(__file__),
               "--reps", str(reps), "--no-baselines", "--cases", ",".join(cases)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        if r.returncode != 0:
            raise SystemExit("rocprofv3 child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = []
        for fn in files:
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    name = row["Kernel_Name"]
                    for k in RM_KERNELS:
                        if name.startswith(k) or (" " + k) in name or name.find(k + "(") >= 0:
                            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
        rows.sort()
        calls, cur = [], {}
        for s, e, k in rows:  # every call ends with one k_rm_vec
            cur[k] = cur.get(k, 0.0) + (e - s) / 1e3
            if k == "k_rm_vec":
                calls.append(cur)
                cur = {}
        stats_files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        stats = [row for fn in stats_files for row in csv.DictReader(open(fn)) if any(k in row.get("Name", "") for k in RM_KERNELS)]
    if len(calls) != len(cases) * reps:
        raise SystemExit("expected %d removal calls in the trace, found %d" % (len(cases) * reps, len(calls)))
    for i, name in enumerate(cases):
        mine = calls[i * reps:(i + 1) * reps]
        out[name] = dict(kernel_us=statistics.median(sum(m.values()) for m in mine),
                         split_us={k: statistics.median(m.get(k, 0.0) for m in mine) for k in RM_KERNELS})
    return out, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--kernel-trace", action="store_true", help="also run this script under rocprofv3 in a child and add the kernel times")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = [c for c in a.cases.split(",") if c]
    traced, stats = ({}, None)
    if a.kernel_trace:
        traced, stats = kernel_trace(cases, 3)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    lines = []
    for name in cases:
        line = run_case(pkg, name, a.reps, not a.no_baselines)
        if name in traced:
            line.update(traced[name])
            line["hbm_fraction_of_8TBps"] = line["bytes"] / (line["kernel_us"] * 1e-6) / HBM_PEAK if line["kernel_us"] > 0 else None
        line = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in line.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
        if stats:
            with open(os.path.splitext(a.out)[0] + "_kernel_stats.json", "w") as fh:
                json.dump(stats, fh, indent=1)


if __name__ == "__main__":
    main()
