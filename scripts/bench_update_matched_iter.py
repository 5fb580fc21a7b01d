#!/usr/bin/env python3
"""Iterated matched updates (ekf_update_matched_iter) beside ekf_update_matched in the same process: one JSON line per case.

Cases: 16 and 32 matches at N = 4096 and 16 at N = 1024, each ONE round (the handle's window is the number of matches).  States are the
injected ones (scenarios.injected_state) at capacity N + 32 in the in-place pipeline mode; measurement k observes landmark k * stride,
spread over every tile, with half a sigma of noise.  tol = 0, so a call runs exactly max_iter factorisations whatever the values: the
cost of an iteration is what is measured, not how many a scan needs.  The state is loaded again in front of every timed call.  The
parent process never opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first failing child ends the
run (scripts/mapbench.py).  Each line carries
  matched_us            ekf_update_matched's wall time on the settled handle (median of --reps, all values kept; the call synchronises)
  iter_us               {max_iter: wall time of ekf_update_matched_iter}, max_iter = 1, 2, 4, 8, the same way
  us_per_iteration      (iter_us[8] - iter_us[1]) / 7: what one more factorisation costs
  one_iteration_is_matched   max_iter = 1 left the bits of ekf_update_matched (state and d2)
A call is several kernels and a pass, so the per-call grouping of --kernel-trace does not apply: the option is refused.
usage: python3 scripts/bench_update_matched_iter.py [--reps 5] [--cases a,b] [--out profiles/update_matched_iter.jsonl]
"""
import statistics
import sys
import time

import mapbench as mb

CASES = ["n4096_m16", "n4096_m32", "n1024_m16"]
KERNELS = ("k_match_factor_iter",)
MAX_ITERS = (1, 2, 4, 8)


def parse(case):
    size, what = case.split("_")
    return dict(N=int(size[1:]), m=int(what[1:]))


def child(case, reps, baselines):
    import numpy as np
    import match_ref as mr
    pkg = mb.package()
    c = parse(case)
    N, m = c["N"], c["m"]
    f, x0, P0 = mb.injected_handle(pkg, 1, N, N + 32, False, max_pending=m)
    ids = (np.arange(m) * max(N // m, 1)).astype(np.int32)
    z, R = mr.scan_of(pkg, x0, ids, 5)
    line = dict(case=case, N=N, matches=m, window=f.window, rounds=-(-m // f.window), tol=0.0)

    def timed(call):
        mb.load_state(f, x0, P0)
        first = call()  # (allocates the scratch)
        wall = []
        for r in range(reps):
            mb.load_state(f, x0, P0)
            f.sync()
            t0 = time.perf_counter()
            got = call()
            wall.append((time.perf_counter() - t0) * 1e6)
        assert np.asarray(got[2]).tobytes() == np.asarray(first[2]).tobytes() and got[1] == m  # the same bits on every call
        return statistics.median(wall), [round(w, 1) for w in wall], got, f.get_state(0)

    line["matched_us"], line["matched_us_all"], got0, after0 = timed(lambda: f.update_matched(z, R, ids))
    line["iter_us"], line["iter_us_all"] = {}, {}
    for mi in MAX_ITERS:
        us, every, got, after = timed(lambda: f.update_matched_iter(z, R, ids, mi, 0.0))
        line["iter_us"][str(mi)], line["iter_us_all"][str(mi)] = round(us, 2), every
        assert (got[3] == mi).all()
        if mi == 1:
            line["one_iteration_is_matched"] = bool(got[2].tobytes() == got0[2].tobytes() and after[0].tobytes() == after0[0].tobytes() and
                                                    after[1].tobytes() == after0[1].tobytes())
    f.close()
    return line


def derive(line, a):
    it = line["iter_us"]
    line["us_per_iteration"] = (it["8"] - it["1"]) / 7.0
    line["iter1_vs_matched"] = it["1"] / line["matched_us"]


if __name__ == "__main__":
    if "--kernel-trace" in sys.argv:
        raise SystemExit("--kernel-trace: a call is several kernels and a pass; the per-call grouping does not apply to this script")
    mb.main(__file__, CASES, child, derive=derive)
