#!/usr/bin/env python3
"""Landmark fusion (ekf_fuse_landmarks / ekf_batch_fuse_landmarks): one JSON line per case.

Cases: 32 pairs (one round of the default window) and 256 pairs (eight rounds) at N = 4096, 32 pairs at N = 1024, and the batch form at
256 filters x (128 + 64) landmarks with 16 pairs each.  States are the injected ones (scenarios.injected_state) at full capacity, in
the in-place pipeline mode; pair k is (k * stride, N / 2 + k * stride), spread over every tile, fused with slack = 1e-4 (the cost does
not depend on the values).  The state is loaded again in front of every timed call (a call removes landmarks).  The parent process
never opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first failing child ends the run
(scripts/mapbench.py).  Each line carries
  wall_us             the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises): rounds x
                      (gather, factor, apply, finish, dense pass), the progress record back, the removal
  rounds, window      how many rounds the list took, and the handle's window
  dense_pass_us       yardstick 1, same process, the same handle: one in-place dense pass folding a one-slot window (ekf_flush under
                      ekf_flush_profile).  null for handles whose chain kernel folds its own windows (ekf_fused_pass: the batch)
  host_path_ms        yardstick 2, same process: get_state of filter 0 -> NumPy (LAPACK Cholesky, BLAS products, np.delete) ->
                      set_state, split into its three parts (the batch: times 256 is quoted as an estimate)
  matches_host        the device result against that NumPy result within the tests' parity bound
A call is several rounds of four kernels and a pass, so the per-call grouping of --kernel-trace does not apply: the option is refused.
usage: python3 scripts/bench_fuse_landmarks.py [--reps 5] [--cases a,b] [--out profiles/fuse_landmarks.jsonl]
"""
import statistics
import sys
import time

import mapbench as mb

SLACK = 1e-4
CASES = ["n4096_p32", "n4096_p256", "n1024_p32", "batch256_p16"]
KERNELS = ("k_fuse_gather", "k_fuse_factor", "k_fuse_apply", "k_fuse_finish")


def parse(case):
    size, what = case.split("_")
    B, N = (256, 192) if size == "batch256" else (1, int(size[1:]))
    return dict(B=B, N=N, pairs=int(what[1:]))


def pair_list(N, m):
    """m pairs (i, j) with i in the first half of the map, j in the second, every landmark at most once, spread over the tiles."""
    import numpy as np
    stride = max((N // 2) // m, 1)
    out = np.zeros(m, dtype=[("i", "i4"), ("j", "i4"), ("d2", "f8")])
    out["i"] = np.arange(m) * stride
    out["j"] = N // 2 + np.arange(m) * stride
    return out


def host_fuse(x, P, pairs, window):
    """The host's way: the same rounds with LAPACK and BLAS, then the rows and columns of every j deleted."""
    import numpy as np
    x, P = x.copy(), P.copy()
    for r0 in range(0, len(pairs), window):
        blk = pairs[r0:r0 + window]
        ci = np.stack([3 + 2 * blk["i"], 4 + 2 * blk["i"]], axis=1).reshape(-1)
        cj = np.stack([3 + 2 * blk["j"], 4 + 2 * blk["j"]], axis=1).reshape(-1)
        W = P[:, ci] - P[:, cj]
        S = W[ci] - W[cj] + SLACK * np.eye(len(ci))
        Lc = np.linalg.cholesky(0.5 * (S + S.T))
        V = np.linalg.solve(Lc, W.T).T
        x -= V @ np.linalg.solve(Lc, x[ci] - x[cj])
        P -= V @ V.T
    rows = np.concatenate([3 + 2 * pairs["j"], 4 + 2 * pairs["j"]]).astype(np.int64)
    return np.delete(x, rows), np.delete(np.delete(P, rows, axis=0), rows, axis=1)


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    B, N, m = c["B"], c["N"], c["pairs"]
    f, x0, P0 = mb.injected_handle(pkg, B, N, N, False)
    pairs = pair_list(N, m)
    line = dict(case=case, N=N, batch=B, pairs=m, window=f.window, rounds=-(-m // f.window), slack=SLACK)
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick 1: one dense pass over all of P
            line["dense_pass_us"], line["dense_pass_us_all"] = mb.dense_pass_us(pkg, f, x0, P0)
    index = None if B > 1 else 0
    arg = [pairs] * B if B > 1 else pairs
    call = lambda: f.fuse_landmarks(arg, SLACK, index)  # noqa: E731
    mb.load_state(f, x0, P0)
    first = call()  # (allocates the scratch)
    first_state = f.get_state(0)
    wall = []
    for r in range(reps):
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        got = call()
        wall.append((time.perf_counter() - t0) * 1e6)
    n_after = int(got[0][0]) if B > 1 else got[0]
    fused = int(got[1][0]) if B > 1 else got[1]
    assert (n_after, fused) == (N - m, m) and np.array_equal(np.asarray(got[0]), np.asarray(first[0]))
    after = f.get_state(0)
    assert np.array_equal(after[0], first_state[0]) and np.array_equal(after[1], first_state[1])  # the same bits on every call
    line["fused"], line["landmarks_after"] = fused, n_after
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        xr, Pr = host_fuse(x, P, pairs, f.window)
        t2 = time.perf_counter()
        f.set_state(xr, Pr, 0)
        f.sync()
        t3 = time.perf_counter()
        line["host_path_ms"] = (t3 - t0) * 1e3
        line["host_get_state_ms"], line["host_numpy_ms"], line["host_set_state_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
        scale = np.abs(Pr).max()
        line["matches_host"] = bool(np.all(np.abs(after[0] - xr) <= 1e-6 * np.abs(xr) + 1e-9) and np.all(np.abs(after[1] - Pr) <= 1e-6 * np.abs(Pr) + 1e-12 * scale))
        line["max_dP_over_max_P"] = float(np.abs(after[1] - Pr).max() / scale)
        if B > 1:
            line["host_path_ms_whole_batch_estimate"] = line["host_path_ms"] * B
    f.close()
    return line


def derive(line, a):
    if line.get("dense_pass_us"):
        line["wall_per_round_vs_dense_pass"] = line["wall_us"] / line["rounds"] / line["dense_pass_us"]
    if line.get("host_path_ms"):
        line["wall_vs_host_path"] = line["wall_us"] / (line["host_path_ms"] * 1e3)


if __name__ == "__main__":
    if "--kernel-trace" in sys.argv:
        raise SystemExit("--kernel-trace: a call is several rounds of four kernels and a pass; the per-call grouping does not apply to this script")
    mb.main(__file__, CASES, child, derive=derive)
