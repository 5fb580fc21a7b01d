#!/usr/bin/env python3
"""The scan-to-map pose search (ekf_locate_scan): one JSON line per case.

Cases: one filter of N = 256, 1024 and 4096 landmarks (scenarios.injected_state at full capacity, in place), a scan of n_z = 8 and 32
measurements of the landmarks nearest the robot (noise of 1 cm per axis, every fourth measurement replaced by a spurious one inside
the scan's box), max_base = 1 and 4, tol = 0.1, min_sep = 1, max_out = 16.  The parent process never opens the GPU: every case runs in
a child of its own under `timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  wall_us               the call's wall time (median of --reps after one call that allocates the scratch and grows the list where it has
                        to; all values kept; the call synchronises)
  candidates, inliers   the candidates scored and the inliers of the best hypothesis; tests = candidates * n_z * N distance tests
  kernel_us, split_us   the call's own kernels from a second child of the case under `rocprofv3 --kernel-trace --stats`
                        (--kernel-trace; median over the child's calls); tests_per_ns = tests / k_loc_score's time
  host_path_ms          today's route, timed in the same process on the same inputs: ekf_get_x, then the vectorised NumPy search of
                        tests/locate_ref.py, split into its two parts; matches_host: the same hypotheses in the same order with the
                        same ids.  Above HOST_LIMIT distance tests the NumPy search is not run (minutes per case): host_skipped
usage: python3 scripts/bench_locate_scan.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/locate_scan.jsonl]
"""
import statistics
import time

import mapbench as mb

TOL, MIN_SEP, MAX_OUT = 0.1, 1.0, 16
HOST_LIMIT = 3e9
CASES = ["n%d_z%d_b%d" % (N, n_z, mb_) for N in (256, 1024, 4096) for n_z in (8, 32) for mb_ in (1, 4)]
KERNELS = ("k_loc_pairs", "k_loc_score", "k_loc_pick", "k_loc_fit")


def parse(case):
    n, z, b = case.split("_")
    return dict(N=int(n[1:]), n_z=int(z[1:]), max_base=int(b[1:]))


def scan(x0, n_z):
    import numpy as np
    import locate_ref as lr
    L = x0[3:].reshape(-1, 2)
    lms = np.argsort(np.hypot(L[:, 0] - x0[0], L[:, 1] - x0[1]), kind="stable")[:n_z]
    z = lr.scan_of_landmarks(x0, lms, 4321)
    rng = np.random.default_rng(4322)
    lo, hi = z.min(axis=0), z.max(axis=0)
    for k in range(3, n_z, 4):
        z[k] = rng.uniform(lo, hi)
    return z


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    N, n_z, max_base = c["N"], c["n_z"], c["max_base"]
    f, x0, _ = mb.injected_handle(pkg, 1, N, N, False, max_pending=16)
    z = scan(x0, n_z)
    call = lambda: f.locate_scan(z, TOL, MIN_SEP, max_base, MAX_OUT)  # noqa: E731
    line = dict(case=case, N=N, n_z=n_z, max_base=max_base, tol=TOL)
    first = call()  # (allocates the scratch, grows the list where it has to)
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        got = call()
        wall.append((time.perf_counter() - t0) * 1e6)
    assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
    line["wall_us"], line["wall_us_all"] = statistics.median(wall), [round(w, 1) for w in wall]
    line["candidates"], line["inliers"] = got[2], int(got[0]["inliers"][0]) if len(got[0]) else 0
    line["tests"] = got[2] * n_z * N
    if baselines and line["tests"] > HOST_LIMIT:
        line["host_skipped"] = "more than %g distance tests" % HOST_LIMIT
    elif baselines:
        import locate_ref as lr
        f.sync()
        t0 = time.perf_counter()
        x = f.get_x(0)
        t1 = time.perf_counter()
        ref = lr.locate(x, z, TOL, MIN_SEP, max_base, MAX_OUT)
        t2 = time.perf_counter()
        line["host_path_ms"], line["host_get_x_ms"], line["host_numpy_ms"] = (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3
        ints = ("inliers", "meas_a", "meas_b", "lm_i", "lm_j")
        line["matches_host"] = bool(ref.n_cand == got[2] and all(ref.hyps[k].tolist() == got[0][k].tolist() for k in ints) and np.array_equal(ref.ids, got[1]))
    f.close()
    return line


def derive(line, a):
    if line.get("host_path_ms"):
        line["wall_vs_host_path"] = line["wall_us"] / (line["host_path_ms"] * 1e3)
    score = (line.get("split_us") or {}).get("k_loc_score")
    if score:
        line["tests_per_ns"] = line["tests"] / (score * 1e3)
        line["score_share_of_kernels"] = score / line["kernel_us"]


if __name__ == "__main__":  # (every call ends with one k_loc_fit; the first call is the one that allocates the scratch)
    mb.main(__file__, CASES, child, derive=derive, trace=dict(kernels=KERNELS, last_kernel="k_loc_fit", tag="ls", skip_first=True))
