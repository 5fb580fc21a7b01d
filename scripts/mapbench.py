"""What the map-operation benchmark scripts share (bench_remove_landmarks.py, bench_reframe.py, bench_join_map.py,
bench_joint_consistency.py, bench_find_duplicates.py): the command line and the per-case loop, the GPU child of a case, the rocprofv3
kernel-trace child with its reader, the injected handle and the dense-pass yardstick.

The shape of a run: the parent process never opens the GPU (importing this module imports neither torch nor the package).  Every case
runs in a child of its own under `timeout -k 10`; the first child that fails or prints no result ends the run with SystemExit and
nothing more is started; --out is rewritten after every case, so a later failure keeps what was measured.  A script keeps what is its
own -- CASES, KERNELS, parse, its byte or tile model, the body of its child, its derived ratios -- and ends in main(...).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):  # (tests/ holds the NumPy references the host yardsticks use)
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12


def package():
    import __graft_entry__ as ge
    return ge.load_package()


def child_command(script, case, reps, baselines, prefix=(), timeout_s=420):
    cmd = ["timeout", "-k", "10", str(timeout_s)] + list(prefix) + [sys.executable, os.path.abspath(script), "--child", case, "--reps", str(reps)]
    return cmd if baselines else cmd + ["--no-baselines"]


def run_child(script, case, reps, baselines, prefix=(), timeout_s=420):
    """One case in a process of its own (under `prefix`, a profiler's command line ending in --): the line it prints behind RESULT."""
    r = subprocess.run(child_command(script, case, reps, baselines, prefix, timeout_s), capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("child of case %s failed (%d); nothing more is started:\n%s" % (case, r.returncode, (r.stdout + r.stderr)[-3000:]))
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("child of case %s printed no result:\n%s" % (case, r.stdout[-2000:]))


def read_trace(d, kernels):
    """(start, end, name) in ns of every launch of the named kernels in the *kernel_trace.csv files under d, sorted by start.  A name
    matches as a substring of the traced one (`void k_reframe_tiles<true>(EkfDev, ...)`): tests/test_mapbench_cpu.py holds the scripts'
    names to what that needs."""
    rows = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            for row in csv.DictReader(fh):
                rows += [(int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k) for k in kernels if k in row["Kernel_Name"]]
    return sorted(rows)


def group_calls(rows, last_kernel, skip_first=False):
    """The rows cut into calls, each ending with one launch of last_kernel: per call the summed us of each kernel, `launches` and
    `span` (first start to last end, us).  skip_first leaves out the first call (the one that allocates the scratch)."""
    calls, cur, t0 = [], {"launches": 0}, None
    for st, en, k in rows:
        t0 = st if t0 is None else t0
        cur[k] = cur.get(k, 0.0) + (en - st) / 1e3
        cur["launches"] += 1
        if k == last_kernel:
            cur["span"] = (en - t0) / 1e3
            calls.append(cur)
            cur, t0 = {"launches": 0}, None
    return calls[1:] if skip_first else calls


def summarize_trace(d, case, n_calls, kernels, last_kernel, skip_first=False, extras=None):
    """The trace under d as the fields of a line: kernel_us and split_us (medians over the calls) and what extras(calls) adds or
    replaces; and the *kernel_stats.csv rows of the kernels."""
    calls = group_calls(read_trace(d, kernels), last_kernel, skip_first)
    if len(calls) != n_calls:
        raise SystemExit("%s: expected %d calls in the trace, found %d" % (case, n_calls, len(calls)))
    out = dict(kernel_us=statistics.median(sum(m.get(k, 0.0) for k in kernels) for m in calls),
               split_us={k: statistics.median(m.get(k, 0.0) for m in calls) for k in kernels})
    out.update(extras(calls) if extras else {})
    stats = []
    for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(fn) as fh:
            stats += [row for row in csv.DictReader(fh) if any(k in row.get("Name", "") for k in kernels)]
    return out, stats


def kernel_trace(script, case, reps, kernels, last_kernel, tag, skip_first=False, extras=None, timeout_s=420):
    """The case again in a child under rocprofv3 (the program after --, no counters in that run): summarize_trace of what it wrote."""
    with tempfile.TemporaryDirectory() as d:
        run_child(script, case, reps, False, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", tag, "--"], timeout_s)
        return summarize_trace(d, case, reps, kernels, last_kernel, skip_first, extras)


def pmc_run(script, case, counters, kernel, tag, timeout_s=420):
    """The case once more in a child under `rocprofv3 --pmc` alone (never together with a trace): the counters summed over `kernel`."""
    with tempfile.TemporaryDirectory() as d:
        run_child(script, case, 1, False, ["rocprofv3", "--pmc"] + counters.split(",") + ["--output-format", "csv", "-d", d, "-o", tag, "--"], timeout_s)
        out = {}
        for fn in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    if kernel in row.get("Kernel_Name", ""):
                        out[row["Counter_Name"]] = out.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return out


def load_state(f, x0, P0):
    """Filter 0's state set, and copied to every other filter of a batch."""
    f.set_state(x0, P0, 0)
    if f.batch > 1:
        f.broadcast_state()


def injected_handle(pkg, B, N, cap, overlap, **kw):
    """A handle of B filters in the given pipeline mode, every filter loaded with the fixed-seed injected state of N landmarks."""
    os.environ["EKF_OVERLAP"] = "1" if overlap else "0"
    f = pkg.FilterBatch(B, cap, **kw)
    x0, P0 = pkg.scenarios.injected_state(N, seed=7, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
    load_state(f, x0, P0)
    return f, x0, P0


def dense_pass_us(pkg, f, x0, P0, slots=1):
    """The yardstick: one dense pass folding a window of `slots` measurements on the handle (ekf_flush under ekf_flush_profile), three
    times: (median, all), or (None, []) when the window never closed as exactly one pass.  It leaves the handle with the last window
    folded; callers whose chain kernel folds its own windows (f.fused_pass) have no such launch and do not come here."""
    import numpy as np
    B, M = f.batch, min(slots, 16)
    steps = max(slots // M, 1)
    sc = pkg.scenarios.steady_script(x0, steps=steps, M=M, seed=8, min_separation=1.0)
    passes = []
    for r in range(3):
        load_state(f, x0, P0)
        for s in range(steps):
            f.propagate(*sc["ctrl"][s])
            for m in range(M):
                if s * M + m == slots - 1:  # (the pass of the last slot is the one that is timed)
                    f.sync()
                    n0, ms0 = f.flush_profile_read()
                    f.flush_profile(1)
                f.update(np.tile(sc["z"][s, m].reshape(1, 1, 2), (B, 1, 1)), np.tile(sc["R"][s, m].reshape(1, 1, 2, 2, order="F"), (B, 1, 1, 1)),
                         want_decisions=False)
        f.flush()
        f.sync()
        n1, ms1 = f.flush_profile_read()
        f.flush_profile(0)
        if n1 - n0 == 1:
            passes.append((ms1 - ms0) * 1e3)
    return (statistics.median(passes), [round(p, 1) for p in passes]) if passes else (None, [])


def main(script, cases, child, trace=None, derive=None, add_args=None, keep_stats=False):
    """The command line and the per-case loop of a script.  child(case, reps, baselines) returns the case's line (it runs in the GPU
    child); trace holds kernel_trace's arguments behind `reps` (its own `reps`, when given, replaces --reps in the traced child);
    derive(line, args) adds the script's ratios in the parent; add_args(parser) its own options; keep_stats writes the traced kernels'
    rocprofv3 statistics to <out>_kernel_stats.json at the end."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(cases))
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--kernel-trace", action="store_true", help="also run every case in a child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=int, default=420, help="seconds a child may take (timeout -k 10)")
    ap.add_argument("--out", default=None)
    if add_args:
        add_args(ap)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.reps, not a.no_baselines)), flush=True)
        return
    lines, all_stats = [], {}
    for case in [c for c in a.cases.split(",") if c]:
        line = run_child(script, case, a.reps, not a.no_baselines, timeout_s=a.child_timeout)
        if a.kernel_trace:
            t = dict(trace)
            traced, all_stats[case] = kernel_trace(script, case, t.pop("reps", a.reps), timeout_s=a.child_timeout, **t)
            line.update(traced)
        if derive:
            derive(line, a)
        line = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in line.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every case: a later failure keeps what was measured)
            with open(a.out, "w") as fh:
                for ln in lines:
                    fh.write(json.dumps(ln) + "\n")
    if a.out and keep_stats and all_stats:
        with open(os.path.splitext(a.out)[0] + "_kernel_stats.json", "w") as fh:
            json.dump(all_stats, fh, indent=1)
