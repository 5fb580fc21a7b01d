#!/usr/bin/env python3
"""Polar measurements (ekf_update_polar): one JSON line per case.

Cases: 16 and 32 entries of each kind -- RANGE only, BEARING only, BOTH only -- at N = 4096 and at N = 1024 (one and two rounds of
the default window of 16).  States are the injected ones (scenarios.injected_state) at capacity N + 32, in the in-place pipeline
mode; entry k measures landmark k * stride, spread over every tile, z = h(x) + noise drawn from R (the cost does not depend on the
values).  The state is loaded again in front of every timed update.  The parent process never opens the GPU: every case runs in a
child of its own under `timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  range_us, bearing_us, both_us   the call's wall time on the settled handle for a list of that kind (median of --reps, all values
                                  kept in *_us_all; the call synchronises)
  rounds, window                  how many rounds the list took, and the handle's window
  matched_us                      the yardstick, the same handle in the same process: ekf_update_matched with as many measurements
                                  of the same landmarks, the state loaded again in front of each -- timed in turns with the three
                                  kinds, polar first
  *_vs_matched                    each kind's median over the yardstick's
  d2_matches_ref                  the first round's d2 of every kind against tests/polar_ref.py (one round of polar_ref.compat on
                                  the loaded state) within polar_ref.D2_REL
A call is several kernels and a pass, so the per-call grouping of --kernel-trace does not apply: the option is refused.
usage: python3 scripts/bench_update_polar.py [--reps 5] [--cases a,b] [--out profiles/update_polar.jsonl]
"""
import statistics
import sys
import time

import mapbench as mb

CASES = ["n4096_m16", "n4096_m32", "n1024_m16", "n1024_m32"]
KINDS = ("range", "bearing", "both")


def parse(case):
    size, what = case.split("_")
    return dict(N=int(size[1:]), m=int(what[1:]))


def child(case, reps, baselines):
    import numpy as np
    import match_ref as mr
    import polar_ref as pr
    pkg = mb.package()
    c = parse(case)
    N, m = c["N"], c["m"]
    f, x0, P0 = mb.injected_handle(pkg, 1, N, N + 32, False)
    ids = (np.arange(m) * max(N // m, 1)).astype(np.int32)
    assert pr.ranges(x0)[ids].min() > 0.0
    lists = {}
    for name, kd in zip(KINDS, (pr.RANGE, pr.BEARING, pr.BOTH)):
        kind = np.full(m, kd, dtype=np.int32)
        lists[name] = pr.entries_for(x0, ids, kind, 5) + (ids, kind)
    matched = mr.scan_of(pkg, x0, ids, 5) + (ids,)
    line = dict(case=case, N=N, entries=m, window=f.window, rounds=-(-m // f.window))

    def timed(fn):
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e6

    calls = {name: (lambda lst=lst: f.update_polar(*lst)) for name, lst in lists.items()}
    if baselines:
        calls["matched"] = lambda: f.update_matched(*matched)
    first = {name: timed(fn)[0] for name, fn in calls.items()}  # (allocates the scratch)
    wall = {name: [] for name in calls}
    for r in range(reps):
        for name, fn in calls.items():
            got, t = timed(fn)
            wall[name].append(t)
            assert got[1] == m and np.asarray(got[2]).tobytes() == np.asarray(first[name][2]).tobytes()  # the same bits on every call
    for name in calls:
        line[name + "_us"] = statistics.median(wall[name])
        line[name + "_us_all"] = [round(w, 1) for w in wall[name]]
    head = min(m, f.window)
    ok = True
    for name, (z, R, i, k) in lists.items():
        want = pr.compat(x0, P0, z[:head], R[:head], i[:head], k[:head])
        ok = ok and bool(np.all(np.abs(first[name][2][:head] - want) <= pr.D2_REL * want))
    line["d2_matches_ref"] = ok
    f.close()
    return line


def derive(line, a):
    for name in KINDS:
        if line.get("matched_us"):
            line[name + "_vs_matched"] = line[name + "_us"] / line["matched_us"]


if __name__ == "__main__":
    if "--kernel-trace" in sys.argv:
        raise SystemExit("--kernel-trace: a call is several kernels and a pass; the per-call grouping does not apply to this script")
    mb.main(__file__, CASES, child, derive=derive)
