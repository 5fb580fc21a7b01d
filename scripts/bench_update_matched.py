#!/usr/bin/env python3
"""Matched updates (ekf_update_matched / ekf_batch_update_matched) and the score of a hypothesis (ekf_joint_compat): one JSON line per
case.

Cases: 16 matches at N = 4096 and at N = 1024 (one round of the default window), the batch form at 256 filters x 256 landmarks with 8
matches each, and ekf_joint_compat of 8 and of 32 pairings at N = 4096.  States are the injected ones (scenarios.injected_state) at
capacity N + 32 (the batch: N), in the in-place pipeline mode; measurement k observes landmark k * stride, spread over every tile, with half a sigma of
noise (the cost does not depend on the values).  The state is loaded again in front of every timed update.  The parent process never
opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first failing child ends the run
(scripts/mapbench.py).  Each line carries
  wall_us             the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises)
  rounds, window      how many rounds the list took, and the handle's window
  host_path_ms        yardstick (a), same process: get_state of filter 0 -> NumPy (the same rounds with LAPACK and BLAS) -> set_state,
                      split into its three parts (the batch: times 256 is quoted as an estimate)
  update_path_us      yardstick (b), the same handle: the same measurements through ekf_update (one call each, then ekf_flush and
                      ekf_sync: the chain and one dense pass).  Its arithmetic differs (one measurement at a time, the filter's own
                      association): time only.  Not for the batch and not for ekf_joint_compat
  dense_pass_us       yardstick (c), the same handle: one in-place dense pass folding a window of as many slots as the case has
                      matches (ekf_flush under ekf_flush_profile).  null for handles whose chain kernel folds its own windows
  matches_host        the device result (state, or d2) against that NumPy result within the tests' parity bound
A call is several kernels and a pass, so the per-call grouping of --kernel-trace does not apply: the option is refused.
usage: python3 scripts/bench_update_matched.py [--reps 5] [--cases a,b] [--out profiles/update_matched.jsonl]
"""
import statistics
import sys
import time

import mapbench as mb

CASES = ["n4096_m16", "n1024_m16", "batch256_m8", "n4096_jc8", "n4096_jc32"]
KERNELS = ("k_match_factor", "k_match_gather", "k_fuse_apply", "k_fuse_finish")


def parse(case):
    size, what = case.split("_")
    B, N = (256, 256) if size == "batch256" else (1, int(size[1:]))
    score = what.startswith("jc")
    return dict(B=B, N=N, m=int(what[2:] if score else what[1:]), score=score)


def scan(x0, N, m):
    """m measurements (z, R, ids): landmark k * stride seen from the pose of x0 with half a sigma of noise."""
    import numpy as np
    import match_ref as mr
    ids = (np.arange(m) * max(N // m, 1)).astype(np.int32)
    z, R = mr.scan_of(mb.package(), x0, ids, 5)
    return z, R, ids


def host_update(x, P, z, R, ids, window):
    """The host's way: the same rounds with LAPACK and BLAS."""
    import numpy as np
    import match_ref as mr
    x, P = x.copy(), P.copy()
    for r0 in range(0, len(ids), window):
        W, S, d = mr.linearise(x, P, z[r0:r0 + window], R[r0:r0 + window], ids[r0:r0 + window])
        Lc = np.linalg.cholesky(0.5 * (S + S.T))
        V = np.linalg.solve(Lc, W.T).T
        x -= V @ np.linalg.solve(Lc, d)
        P -= V @ V.T
    return x, P


def child(case, reps, baselines):
    import numpy as np
    import match_ref as mr
    pkg = mb.package()
    c = parse(case)
    B, N, m = c["B"], c["N"], c["m"]
    f, x0, P0 = mb.injected_handle(pkg, B, N, N if B > 1 else N + 32, False)  # (room: yardstick (b) may decide New)
    z, R, ids = scan(x0, N, m)
    line = dict(case=case, N=N, batch=B, matches=m, window=f.window, rounds=1 if c["score"] else -(-m // f.window))
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick (c): one dense pass over all of P with as many slots
            line["dense_pass_us"], line["dense_pass_us_all"] = mb.dense_pass_us(pkg, f, x0, P0, slots=min(m, f.window))
    index = None if B > 1 else 0
    args = (np.tile(z, (B, 1, 1)), np.tile(R, (B, 1, 1, 1)), np.tile(ids, (B, 1))) if B > 1 else (z, R, ids)
    call = (lambda: f.joint_compat(*args, index)) if c["score"] else (lambda: f.update_matched(*args, index))
    mb.load_state(f, x0, P0)
    first = call()  # (allocates the scratch)
    wall = []
    for r in range(reps):
        if not c["score"]:
            mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        got = call()
        wall.append((time.perf_counter() - t0) * 1e6)
    d2 = got if c["score"] else got[-1]
    assert np.asarray(d2).tobytes() == np.asarray(first if c["score"] else first[-1]).tobytes()  # the same bits on every call
    if not c["score"]:
        assert int(np.asarray(got[-2]).reshape(-1)[0]) == m
    after = f.get_state(0)
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        if c["score"]:
            want = mr.joint_compat(x, P, z, R, ids)
        else:
            xr, Pr = host_update(x, P, z, R, ids, f.window)
        t2 = time.perf_counter()
        if not c["score"]:
            f.set_state(xr, Pr, 0)
            f.sync()
        t3 = time.perf_counter()
        line["host_path_ms"] = (t3 - t0) * 1e3
        line["host_get_state_ms"], line["host_numpy_ms"], line["host_set_state_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
        if c["score"]:
            line["matches_host"] = bool(np.all(np.abs(np.asarray(d2) - want) <= mr.D2_REL * want))
        else:
            scale = np.abs(Pr).max()
            line["matches_host"] = bool(np.all(np.abs(after[0] - xr) <= 1e-6 * np.abs(xr) + 1e-9) and np.all(np.abs(after[1] - Pr) <= 1e-6 * np.abs(Pr) + 1e-12 * scale))
            line["max_dP_over_max_P"] = "%.3e" % (np.abs(after[1] - Pr).max() / scale)  # (text: the harness rounds floats to 5 places)
        if B > 1:
            line["host_path_ms_whole_batch_estimate"] = line["host_path_ms"] * B
        if B == 1 and not c["score"]:  # yardstick (b): the same measurements through ekf_update, the window folded at the end
            ups = []
            for r in range(reps):
                mb.load_state(f, x0, P0)
                f.sync()
                t0 = time.perf_counter()
                for k in range(m):
                    f.update(z[k].reshape(1, 1, 2), R[k].reshape(1, 1, 2, 2), want_decisions=False)
                f.flush()
                f.sync()
                ups.append((time.perf_counter() - t0) * 1e6)
            line["update_path_us"] = statistics.median(ups)
            line["update_path_us_all"] = [round(u, 1) for u in ups]
    f.close()
    return line


def derive(line, a):
    if line.get("dense_pass_us"):
        line["wall_per_round_vs_dense_pass"] = line["wall_us"] / line["rounds"] / line["dense_pass_us"]
    if line.get("host_path_ms"):
        line["wall_vs_host_path"] = line["wall_us"] / (line["host_path_ms"] * 1e3)
    if line.get("update_path_us"):
        line["wall_vs_update_path"] = line["wall_us"] / line["update_path_us"]


if __name__ == "__main__":
    if "--kernel-trace" in sys.argv:
        raise SystemExit("--kernel-trace: a call is several kernels and a pass; the per-call grouping does not apply to this script")
    mb.main(__file__, CASES, child, derive=derive)
