#!/usr/bin/env python3
"""Duplicate search (ekf_find_duplicates / ekf_batch_find_duplicates): one JSON line per case.

Cases: N = 4096 over all pairs, with split = 3840 (the old x new pairs of a 3840 + 256 join), and with max_dist = 2 on a map whose
landmarks are numbered along a path (a line, 0.5 m apart: a group of 32 spans 16 m, so only a tile and its neighbour survive the
bounding-box test); N = 1024 over all pairs; the batch form at 256 filters x N = 256.  States are the injected ones
(scenarios.injected_state) at full capacity, in the in-place pipeline mode.  The parent process never opens the GPU: every case runs
in a child of its own under `timeout -k 10`, and the first failing child ends the run.  Each line carries
  wall_us             the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels (k_dup_boxes, k_dup_tiles) from a second child of the case under
                      `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over the child's calls, all values kept)
  tiles, bytes        tiles the tile kernel loads (those its grid names, less the ones the bounding boxes cull -- recomputed here
                      by the kernel's rule) and the bytes of their live chains (a diagonal tile: 10 of 16); bytes / tile-kernel
                      time as a fraction of 8 TB/s
  dense_pass_us       yardstick 1, same process, the same handle: one in-place dense pass folding a one-slot window (ekf_flush
                      under ekf_flush_profile), which reads and writes ALL of P.  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass: the batch), where no dense-pass launch exists to time
  host_path_ms        yardstick 2, same process: get_state of filter 0 -> NumPy (tests/dup_ref.py), split into its two parts (the
                      batch: times 256 is quoted as an estimate)
usage: python3 scripts/bench_find_duplicates.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/find_duplicates.jsonl]
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
GATE = 9.21
CASES = ["n4096_all", "n4096_split3840", "n4096_path2m", "n1024_all", "batch256_all"]
KERNELS = ("k_dup_boxes", "k_dup_tiles")
CHILD_TIMEOUT = 420


def parse(case):
    size, what = case.split("_")
    B, N = (256, 256) if size == "batch256" else (1, int(size[1:]))
    return dict(B=B, N=N, split=int(what[5:]) if what.startswith("split") else 0, max_dist=float(what[4:-1]) if what.startswith("path") else None,
                path=what.startswith("path"))


def visited_tiles(x, N, split, max_dist):
    """(off-diagonal, diagonal) tiles the tile kernel loads: ekf_device.h's dup_tile_ij list, less the culled ones."""
    import numpy as np
    nT = (N + 31) // 32
    L = x[3:].reshape(-1, 2)
    lo = np.array([L[32 * g:32 * g + 32].min(axis=0) for g in range(nT)])
    hi = np.array([L[32 * g:32 * g + 32].max(axis=0) for g in range(nT)])
    off = diag = 0
    for I in range(nT):
        if split and I > (split - 1) // 32:
            break
        J0 = max(I, split // 32 if split else I)
        gap = np.maximum(np.maximum(lo[I] - hi[J0:], lo[J0:] - hi[I]), 0.0)
        live = np.ones(nT - J0, dtype=bool) if max_dist is None else (gap ** 2).sum(axis=1) <= max_dist * max_dist
        diag += int(live[0]) if J0 == I else 0
        off += int(live.sum()) - (int(live[0]) if J0 == I else 0)
    return off, diag


def child(case, reps, baselines):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    c = parse(case)
    B, N = c["B"], c["N"]
    os.environ["EKF_OVERLAP"] = "0"
    f = pkg.FilterBatch(B, N)
    x0, P0 = pkg.scenarios.injected_state(N, seed=7, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
    xs = x0.copy()  # the searched state: the injected one, or its landmarks laid along a line in the order of their numbers
    if c["path"]:
        rng = np.random.default_rng(11)
        xs[3::2] = 0.5 * np.arange(N)
        xs[4::2] = rng.uniform(-2.0, 2.0, size=N)
    f.set_state(x0, P0, 0)
    off, diag = visited_tiles(xs, N, c["split"], c["max_dist"])
    line = dict(case=case, N=N, batch=B, split=c["split"], max_dist=c["max_dist"], tiles=B * (off + diag), bytes=B * (off * 16 + diag * 10) * 2048)
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick 1: one dense pass over all of P, folding a one-slot window
            sc = pkg.scenarios.steady_script(x0, steps=1, M=1, seed=8, min_separation=1.0)
            passes = []
            for r in range(3):
                f.set_state(x0, P0, 0)
                f.propagate(*sc["ctrl"][0])
                f.update(sc["z"][0, 0].reshape(1, 1, 2), sc["R"][0, 0].reshape(1, 1, 2, 2, order="F"), want_decisions=False)
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
    f.set_state(xs, P0, 0)
    if B > 1:
        f.broadcast_state()
    index = None if B > 1 else 0
    call = lambda: f.find_duplicates(GATE, c["max_dist"], c["split"], index)  # noqa: E731
    first = call()  # (allocates the scratch)
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        got = call()
        wall.append((time.perf_counter() - t0) * 1e6)
    one = got[0] if B > 1 else got
    assert one[0].tobytes() == (first[0] if B > 1 else first)[0].tobytes()
    line["found"], line["degenerate"] = one[1], one[2]
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        import dup_ref as dr
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        ref, _ = dr.find(x, P, GATE, c["max_dist"], c["split"])
        t2 = time.perf_counter()
        line["host_path_ms"] = (t2 - t0) * 1e3
        line["host_get_state_ms"], line["host_numpy_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        line["matches_host"] = bool(ref["i"].tolist() == one[0]["i"].tolist() and ref["j"].tolist() == one[0]["j"].tolist())
        if B > 1:
            line["host_path_ms_whole_batch_estimate"] = line["host_path_ms"] * B
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
        run_child(case, reps, False, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fd", "--"])
        rows = []
        for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    for k in KERNELS:
                        if k in row["Kernel_Name"]:
                            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
    rows.sort()
    calls, cur = [], {}
    for st, en, k in rows:  # every call ends with one k_dup_tiles
        cur[k] = cur.get(k, 0.0) + (en - st) / 1e3
        if k == "k_dup_tiles":
            calls.append(cur)
            cur = {}
    calls = calls[1:]  # (the call that allocates the scratch)
    if len(calls) != reps:
        raise SystemExit("%s: expected %d calls in the trace, found %d" % (case, reps, len(calls)))
    return dict(kernel_us=statistics.median(sum(m.values()) for m in calls),
                split_us={k: statistics.median(m.get(k, 0.0) for m in calls) for k in KERNELS},
                tiles_us_all=[round(m.get("k_dup_tiles", 0.0), 2) for m in calls])


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
            t_us = line["split_us"]["k_dup_tiles"]
            line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / HBM_PEAK if t_us > 0 else None
            if line.get("dense_pass_us"):
                line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
                line["kernels_vs_dense_pass"] = line["kernel_us"] / line["dense_pass_us"]
        if line.get("host_path_ms"):
            line["wall_vs_host_path"] = line["wall_us"] / (line["host_path_ms"] * 1e3)
        line = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in line.items()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every case: a later failure keeps what was measured)
            with open(a.out, "w") as fh:
                for ln in lines:
                    fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
