#!/usr/bin/env python3
"""Absolute fixes (ekf_update_fixes / ekf_batch_update_fixes) and the score of a list (ekf_fix_compat): one JSON line per case.

Cases: 16 entries -- 1 position + 1 heading + 14 landmark fixes -- at N = 4096 and at N = 1024 (one round of the default window), the
batch form at 256 filters x 256 landmarks with 8 entries each (1 + 1 + 6), and ekf_fix_compat of 32 entries (1 + 1 + 30) at N = 4096.
States are the injected ones (scenarios.injected_state) at capacity N + 32 (the batch: N), in the in-place pipeline mode; landmark
entry k fixes landmark k * stride, spread over every tile, every z within a sigma of P + R of the state (the cost does not depend on
the values).  The state is loaded again in front of every timed update.  The parent process never opens the GPU: every case runs in a
child of its own under `timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  wall_us             the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises)
  rounds, window      how many rounds the list took, and the handle's window
  matched_us          yardstick (a), the same handle in the same process: ekf_update_matched (ekf_joint_compat for the score) with as
                      many measurements, of the landmarks k * stride, the state loaded again in front of each -- timed in turns with
                      the fixes, fix first
  host_path_ms        yardstick (b), same process: get_state of filter 0 -> NumPy (the same rounds with LAPACK and BLAS) -> set_state,
                      split into its three parts (the batch: times 256 is quoted as an estimate)
  matches_host        the device result (state, or d2) against that NumPy result within the tests' parity bound
A call is several kernels and a pass, so the per-call grouping of --kernel-trace does not apply: the option is refused.
usage: python3 scripts/bench_update_fixes.py [--reps 5] [--cases a,b] [--out profiles/update_fixes.jsonl]
"""
import statistics
import sys
import time

import mapbench as mb

CASES = ["n4096_m16", "n1024_m16", "batch256_m8", "n4096_fc32"]
KERNELS = ("k_fix_factor", "k_fix_gather", "k_fuse_apply", "k_fuse_finish")


def parse(case):
    size, what = case.split("_")
    B, N = (256, 256) if size == "batch256" else (1, int(size[1:]))
    score = what.startswith("fc")
    return dict(B=B, N=N, m=int(what[2:] if score else what[1:]), score=score)


def lists(x0, P0, N, m):
    """(z, R, what) of m fixes -- position, heading, m - 2 landmarks k * stride -- and (z, R, ids) of m matched measurements of the
    landmarks k * stride."""
    import numpy as np
    import fix_ref as fx
    import match_ref as mr
    ids = (np.arange(m) * max(N // m, 1)).astype(np.int32)
    what = np.concatenate([[fx.POSITION, fx.HEADING], ids[:m - 2]]).astype(np.int32)
    z, R = fx.entries_for(x0, P0, what, 5)
    z[1, 1], R[1].flat[1:] = 0.0, 0.0  # (the heading entry's unread values: finite for the host's arithmetic)
    return (z, R, what), mr.scan_of(mb.package(), x0, ids, 5) + (ids,)


def host_update(x, P, z, R, what, window):
    """The host's way: the same rounds with LAPACK and BLAS."""
    import numpy as np
    import fix_ref as fx
    x, P = x.copy(), P.copy()
    for r0 in range(0, len(what), window):
        W, S, d = fx.assemble(x, P, z[r0:r0 + window], R[r0:r0 + window], what[r0:r0 + window])
        Lc = np.linalg.cholesky(np.triu(S) + np.triu(S, 1).T)
        V = np.linalg.solve(Lc, W.T).T
        x -= V @ np.linalg.solve(Lc, d)
        P -= V @ V.T
    return x, P


def child(case, reps, baselines):
    import numpy as np
    import fix_ref as fx
    pkg = mb.package()
    c = parse(case)
    B, N, m = c["B"], c["N"], c["m"]
    f, x0, P0 = mb.injected_handle(pkg, B, N, N if B > 1 else N + 32, False)
    (z, R, what), matched = lists(x0, P0, N, m)
    line = dict(case=case, N=N, batch=B, entries=m, window=f.window, rounds=1 if c["score"] else -(-m // f.window))
    index = None if B > 1 else 0

    def tiled(a3):
        return tuple(np.tile(v, (B,) + (1,) * v.ndim) for v in a3) if B > 1 else a3

    fix_args, match_args = tiled((z, R, what)), tiled(matched)
    call = (lambda: f.fix_compat(*fix_args, index)) if c["score"] else (lambda: f.update_fixes(*fix_args, index))
    yard = (lambda: f.joint_compat(*match_args, index)) if c["score"] else (lambda: f.update_matched(*match_args, index))

    def timed(fn):
        if not c["score"]:
            mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e6

    mb.load_state(f, x0, P0)
    first = call()  # (allocates the scratch)
    if baselines:
        mb.load_state(f, x0, P0)
        yard()
    wall, ywall = [], []
    for r in range(reps):
        got, t = timed(call)
        wall.append(t)
        if baselines:
            ywall.append(timed(yard)[1])
    if not c["score"]:  # (once more, for the state it leaves)
        got = timed(call)[0]
        after = f.get_state(0)
    d2 = got if c["score"] else got[-1]
    assert np.asarray(d2).tobytes() == np.asarray(first if c["score"] else first[-1]).tobytes()  # the same bits on every call
    if not c["score"]:
        assert int(np.asarray(got[-2]).reshape(-1)[0]) == m
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        line["matched_us"] = statistics.median(ywall)
        line["matched_us_all"] = [round(w, 1) for w in ywall]
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        if c["score"]:
            want = fx.compat(x, P, z, R, what)
        else:
            xr, Pr = host_update(x, P, z, R, what, f.window)
        t2 = time.perf_counter()
        if not c["score"]:
            f.set_state(xr, Pr, 0)
            f.sync()
        t3 = time.perf_counter()
        line["host_path_ms"] = (t3 - t0) * 1e3
        line["host_get_state_ms"], line["host_numpy_ms"], line["host_set_state_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
        if c["score"]:
            line["matches_host"] = bool(np.all(np.abs(np.asarray(d2).reshape(-1)[:m] - want) <= fx.D2_REL * want))
        else:
            scale = np.abs(Pr).max()
            line["matches_host"] = bool(np.all(np.abs(after[0] - xr) <= 1e-6 * np.abs(xr) + 1e-9) and np.all(np.abs(after[1] - Pr) <= 1e-6 * np.abs(Pr) + 1e-12 * scale))
            line["max_dP_over_max_P"] = "%.3e" % (np.abs(after[1] - Pr).max() / scale)  # (text: the harness rounds floats to 5 places)
        if B > 1:
            line["host_path_ms_whole_batch_estimate"] = line["host_path_ms"] * B
    f.close()
    return line


def derive(line, a):
    if line.get("matched_us"):
        line["wall_vs_matched"] = line["wall_us"] / line["matched_us"]
    if line.get("host_path_ms"):
        line["wall_vs_host_path"] = line["wall_us"] / (line["host_path_ms"] * 1e3)


if __name__ == "__main__":
    if "--kernel-trace" in sys.argv:
        raise SystemExit("--kernel-trace: a call is several kernels and a pass; the per-call grouping does not apply to this script")
    mb.main(__file__, CASES, child, derive=derive)
