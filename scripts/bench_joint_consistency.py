#!/usr/bin/env python3
"""Whole-state consistency (ekf_joint_consistency / ekf_batch_joint_consistency): one JSON line per case.

Cases: N = 4096 and N = 1024 landmarks (capacity = N), each in both pipeline modes (EKF_OVERLAP=0/1), and the batch form at
256 filters x 256 landmarks.  The parent process never opens the GPU: every case runs in a child of its own under `timeout -k 10`,
and the first failing child ends the run.  Each line carries
  first_call_us       the first call on the handle: the scratch allocation (one more P_LL buffer per filter) and the call
  wall_us             the call's wall time on a settled handle (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels per family (k_chol_stage, k_chol_diag, k_chol_panel, k_chol_trail, k_chol_finish) from a
                      second child of the case under `rocprofv3 --kernel-trace --stats` (--kernel-trace; no counters in that run;
                      median over the child's calls with the range, the first call left out); launches = kernels per call
  dense_pass_us       for scale, same handle: one in-place dense pass folding a one-slot window and one folding a full window of 32
                      slots = 16 pairs (ekf_flush under ekf_flush_profile).  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass: the batch), and when the window did not close as exactly one pass
  host_ms             the host path, same process: get_state -> scipy.linalg.cho_factor / cho_solve on the whole P (the threads the
                      environment allows), split into its two parts (the batch: one filter, times 256 quoted as an estimate)
  worst_rel_err       the device's NEES / log-det fields against that host result
usage: python3 scripts/bench_joint_consistency.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/joint_consistency.jsonl]
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

CASES = ["n4096_inplace", "n4096_overlap", "n1024_inplace", "n1024_overlap", "batch256_inplace"]
KERNELS = ("k_chol_stage", "k_chol_diag", "k_chol_panel", "k_chol_trail", "k_chol_finish")
CHILD_TIMEOUT = 420


def parse(case):
    size, mode = case.split("_")
    if size == "batch256":
        return dict(B=256, N=256, overlap=mode == "overlap")
    return dict(B=1, N=int(size[1:]), overlap=mode == "overlap")


def dense_pass_us(pkg, np, f, x0, P0, slots):
    """One dense pass folding a window of `slots` measurements on the handle (None when it did not come out as exactly one pass)."""
    M = min(slots, 16)
    steps = max(slots // M, 1)
    sc = pkg.scenarios.steady_script(x0, steps=steps, M=M, seed=8, min_separation=1.0)
    passes = []
    for r in range(3):
        f.set_state(x0, P0, 0)
        for s in range(steps):
            f.propagate(*sc["ctrl"][s])
            for m in range(M):
                if s * M + m == slots - 1:  # (the pass of the last slot is the one that is timed)
                    f.sync()
                    n0, ms0 = f.flush_profile_read()
                    f.flush_profile(1)
                f.update(sc["z"][s, m].reshape(1, 1, 2), sc["R"][s, m].reshape(1, 1, 2, 2, order="F"), want_decisions=False)
        f.flush()
        f.sync()
        n1, ms1 = f.flush_profile_read()
        f.flush_profile(0)
        if n1 - n0 == 1:
            passes.append((ms1 - ms0) * 1e3)
    return (statistics.median(passes), [round(p, 1) for p in passes]) if passes else (None, [])


def child(case, reps, baselines):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    c = parse(case)
    B, N = c["B"], c["N"]
    os.environ["EKF_OVERLAP"] = "1" if c["overlap"] else "0"
    f = pkg.FilterBatch(B, N, max_pending=32)
    x0, P0 = pkg.scenarios.injected_state(N, seed=7, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
    f.set_state(x0, P0, 0)
    if B > 1:
        f.broadcast_state()
    xt = x0 + 0.05 * np.random.default_rng(1).standard_normal(len(x0))
    xt_all = np.tile(xt, (B, 1))
    call = (lambda: f.joint_consistency(xt_all)) if B > 1 else (lambda: f.joint_consistency(xt, 0))
    line = dict(case=case, N=N, batch=B, overlap=bool(f.overlap), tile_steps=(2 * N + 63) // 64)
    f.sync()
    bytes0 = f.device_bytes()
    t0 = time.perf_counter()
    rows = call()
    line["first_call_us"] = (time.perf_counter() - t0) * 1e6
    line["scratch_bytes"] = int(f.device_bytes() - bytes0)
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        again = call()
        wall.append((time.perf_counter() - t0) * 1e6)
        assert again.tobytes() == rows.tobytes()
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    assert all(int(v) == 0 for v in rows["info"])
    if baselines:
        import scipy.linalg
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        e = x - xt
        cf = scipy.linalg.cho_factor(P, lower=False)
        nees = float(e @ scipy.linalg.cho_solve(cf, e))
        logdet = 2.0 * float(np.sum(np.log(np.diag(cf[0]))))
        t2 = time.perf_counter()
        line["host_ms"] = dict(get_state=(t1 - t0) * 1e3, factor_and_solve=(t2 - t1) * 1e3, total=(t2 - t0) * 1e3)
        if B > 1:
            line["host_ms_whole_batch_estimate"] = line["host_ms"]["total"] * B
        line["worst_rel_err"] = max(abs(float(rows[0]["nees_joint"]) - nees) / nees, abs(float(rows[0]["logdet_joint"]) - logdet) / abs(logdet))
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:
            one, one_all = dense_pass_us(pkg, np, f, x0, P0, 1)
            full, full_all = dense_pass_us(pkg, np, f, x0, P0, 32)
            line["dense_pass_us"] = dict(one_slot=one, one_slot_all=one_all, pairs16=full, pairs16_all=full_all)
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
    """The case again in a child under rocprofv3 (the program after --): the kernels' durations per call and family."""
    with tempfile.TemporaryDirectory() as d:
        run_child(case, reps, False, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "jc", "--"])
        rows = []
        for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    for k in KERNELS:
                        if k in row["Kernel_Name"]:
                            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
    rows.sort()
    calls, cur, count = [], {}, 0
    for st, en, k in rows:  # every call ends with one k_chol_finish
        cur[k] = cur.get(k, 0.0) + (en - st) / 1e3
        count += 1
        if k == "k_chol_finish":
            cur["launches"] = count
            cur["span"] = (en - cur.pop("t0", st)) / 1e3
            calls.append(cur)
            cur, count = {}, 0
        elif "t0" not in cur:
            cur["t0"] = st
    if len(calls) != reps + 1:
        raise SystemExit("%s: expected %d calls in the trace, found %d" % (case, reps + 1, len(calls)))
    calls = calls[1:]  # (the first call is the one with the allocation)
    total = [sum(m.get(k, 0.0) for k in KERNELS) for m in calls]
    return dict(kernel_us=statistics.median(total), kernel_us_range=[round(min(total), 1), round(max(total), 1)],
                split_us={k: round(statistics.median(m.get(k, 0.0) for m in calls), 1) for k in KERNELS},
                split_us_range={k: [round(min(m.get(k, 0.0) for m in calls), 1), round(max(m.get(k, 0.0) for m in calls), 1)] for k in KERNELS},
                device_span_us=statistics.median(m["span"] for m in calls), launches=calls[0]["launches"])


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
            d = line.get("dense_pass_us") or {}
            if d.get("pairs16"):
                line["kernels_vs_16pair_pass"] = line["kernel_us"] / d["pairs16"]
        if line.get("host_ms"):
            line["host_vs_wall"] = line["host_ms"]["total"] * 1e3 / line["wall_us"]
        line = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in line.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every case: a later failure keeps what was measured)
            with open(a.out, "w") as fh:
                for ln in lines:
                    fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
