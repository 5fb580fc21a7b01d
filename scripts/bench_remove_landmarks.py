#!/usr/bin/env python3
"""Landmark removal (ekf_remove_landmarks / ekf_batch_remove_landmarks): one JSON line per case.

Cases: N = 1024 and 4096 landmarks, 1 % of them spread out or one contiguous block of 64 removed, both pipeline modes (EKF_OVERLAP=0/1),
and the batch of 256 filters x 256 landmarks (a different 1 % .. 10 % mask per filter).  The parent process never opens the GPU: every
case runs in a child of its own under `timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  wall_us          the call's wall time (median of --reps; the call synchronises)
  kernel_us        the removal's own kernels (k_rm_gather, k_rm_finish, k_rm_vec) per call, from a second child of the case under
                   `rocprofv3 --kernel-trace --stats` (--kernel-trace; median of that child's three calls), and their split
  bytes            algorithmic bytes of those kernels (the gather's tile reads and writes, the copy-back or the clearing of the other
                   buffer; x / R / D and the maps are negligible) and bytes / kernel time as a fraction of 8 TB/s
  host_round_trip_ms   get_state -> np.delete -> set_state (one filter; the batch: filter 0 only, times 256 is quoted)
  dense_detour_ms      ekf_reserve(capacity + 32): every filter through k_export -> dense n x n -> k_import on the device, the path a removal
                   through the existing entry points would take on the device
usage: python3 scripts/bench_remove_landmarks.py [--reps 5] [--kernel-trace] [--cases a,b] [--out FILE]
"""
import statistics
import time

import mapbench as mb

TILE_BYTES = 4096 * 8
CASES = ["n1024_spread_inplace", "n1024_spread_overlap", "n1024_block64_inplace", "n1024_block64_overlap",
         "n4096_spread_inplace", "n4096_spread_overlap", "n4096_block64_inplace", "n4096_block64_overlap",
         "batch256_inplace", "batch256_overlap"]
KERNELS = ("k_rm_gather", "k_rm_finish", "k_rm_vec")


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


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    keep = masks(c, np.random.default_rng(11))
    f, x0, P0 = mb.injected_handle(pkg, c["B"], c["N"], c["cap"], c["overlap"])
    wall = []
    for r in range(reps):
        if r:
            mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        f.remove_landmarks(keep) if c["B"] > 1 else f.remove_landmarks(keep[0], index=0)
        wall.append((time.perf_counter() - t0) * 1e6)
    line = dict(case=case, N=c["N"], batch=c["B"], overlap=bool(f.overlap), removed_per_filter_mean=float((~keep).sum(1).mean()),
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
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        f.reserve(c["cap"] + 32)
        line["dense_detour_ms"] = (time.perf_counter() - t0) * 1e3
    f.close()
    return line


def derive(line, a):
    if "kernel_us" in line:
        line["hbm_fraction_of_8TBps"] = line["bytes"] / (line["kernel_us"] * 1e-6) / mb.HBM_PEAK if line["kernel_us"] > 0 else None


if __name__ == "__main__":  # (every call ends with one k_rm_vec; the traced child makes three calls whatever --reps says)
    mb.main(__file__, CASES, child, trace=dict(kernels=KERNELS, last_kernel="k_rm_vec", tag="rm", reps=3), derive=derive, keep_stats=True)
