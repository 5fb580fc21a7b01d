#!/usr/bin/env python3
"""Submap extraction (ekf_extract_map / ekf_batch_extract_map / ekf_get_submap): one JSON line per case.

Cases: the 256 landmarks nearest to the robot out of 4096 into a handle of capacity 256, in both pipeline modes of the SOURCE
(EKF_OVERLAP=0/1); the whole map 4096 -> 4096 (ids = None: a copy); 64 of 1024 into capacity 64; the batch form at 256 filters x
(64 of 256); and get_submap of 256 of 4096.  The parent process never opens the GPU: every case runs in a child of its own under
`timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  wall_us             the call's wall time with both handles settled (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels (k_ext_tiles, k_ext_vec) from a second child of the case under `rocprofv3 --kernel-trace
                      --stats` (--kernel-trace; the extraction cases only: name them with --cases, the read-out's one kernel is
                      k_ext_dense and ends no such call)
  bytes               algorithmic bytes of the tile kernel: the destination's stored tiles written once and as many bytes read; a
                      scattered selection moves twice the bytes it reads for (half of every 32-byte piece is used); the read-out: the
                      dense matrix written once and read once by the copy
  dense_pass_us       yardstick 1, same process, the source handle: one in-place dense pass folding a one-slot window (ekf_flush
                      under ekf_flush_profile), which reads and writes ALL of P.  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass), where no dense-pass launch exists to time
  host_round_trip_ms  yardstick 2, same process, what the call replaces: get_state of the source -> NumPy index -> set_state of the
                      destination (the read-out: get_state -> index; the batch: one filter, times 256 quoted as an estimate)
--dry prints every case's plan (sizes, ids, bytes) without starting a child: nothing touches the GPU.
usage: python3 scripts/bench_extract_map.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/extract_map.jsonl] [--dry]
"""
import json
import os
import statistics
import sys
import time

import mapbench as mb

CASES = ["near256_of_4096_inplace", "near256_of_4096_overlap", "copy_4096", "n64_of_1024", "batch256_n64_of_256", "submap256_of_4096"]
KERNELS = ("k_ext_tiles", "k_ext_vec", "k_ext_dense")
TABLE = {
    #                          B    N     source cap  count (None: every landmark)  destination cap  source overlap  kind
    "near256_of_4096_inplace": (1, 4096, 4096, 256, 256, False, "extract"),
    "near256_of_4096_overlap": (1, 4096, 4096, 256, 256, True, "extract"),
    "copy_4096": (1, 4096, 4096, None, 4096, False, "extract"),
    "n64_of_1024": (1, 1024, 1024, 64, 64, False, "extract"),
    "batch256_n64_of_256": (256, 256, 256, 64, 64, False, "extract"),
    "submap256_of_4096": (1, 4096, 4096, 256, 0, False, "submap"),
}


def parse(case):
    B, N, cap, count, cap_d, overlap, kind = TABLE[case]
    return dict(B=B, N=N, cap=cap, count=count, cap_d=cap_d, overlap=overlap, kind=kind)


def lm_tiles(n):
    return (2 * n + 63) // 64


def algorithmic_bytes(c):
    n = c["N"] if c["count"] is None else c["count"]
    if c["kind"] == "submap":
        return 2 * (3 + 2 * n) ** 2 * 8
    t = lm_tiles(n)
    return c["B"] * 2 * (t * (t + 1) // 2) * 4096 * 8


def nearest_ids(x0, count):
    """The `count` landmarks nearest to the robot, nearest first: a scattered selection in no particular order of ids."""
    import numpy as np
    L = x0[3:].reshape(-1, 2)
    return np.argsort(np.hypot(*(L - x0[0:2]).T), kind="stable")[:count].astype(np.int32)


def plan(case):
    c = parse(case)
    n = c["N"] if c["count"] is None else c["count"]
    return dict(case=case, kind=c["kind"], batch=c["B"], N=c["N"], count=n, ids="all" if c["count"] is None else "robot-nearest",
                source_capacity=c["cap"], destination_capacity=c["cap_d"] or None, source_overlap=c["overlap"], bytes=algorithmic_bytes(c))


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    B, N = c["B"], c["N"]
    f, x0, P0 = mb.injected_handle(pkg, B, N, c["cap"], c["overlap"])
    line = plan(case)
    line["overlap"] = bool(f.overlap)
    ids = None if c["count"] is None else nearest_ids(x0, c["count"])
    n = N if ids is None else ids.size
    d = None
    if c["kind"] == "extract":
        os.environ["EKF_OVERLAP"] = "0"
        d = pkg.FilterBatch(B, c["cap_d"])
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick 1: one dense pass over all of the source's P
            line["dense_pass_us"], line["dense_pass_us_all"] = mb.dense_pass_us(pkg, f, x0, P0)
            mb.load_state(f, x0, P0)
    wall = []
    for r in range(reps):
        f.sync()
        if d is not None:
            d.sync()
        t0 = time.perf_counter()
        if c["kind"] == "submap":
            got = f.get_submap(ids)
        elif B > 1:
            d.batch_extract_map(f, None if ids is None else np.tile(ids, (B, 1)))
        else:
            d.extract_map(f, ids)
        wall.append((time.perf_counter() - t0) * 1e6)
        if d is not None:
            assert int(d.num_landmarks()[0]) == n
        else:
            assert got[0].size == 3 + 2 * n
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:  # yardstick 2: the host round trip the call replaces
        sel = np.arange(3 + 2 * N) if ids is None else np.concatenate([np.arange(3), np.stack([3 + 2 * ids, 4 + 2 * ids], axis=1).reshape(-1)])
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        xs, Ps = x[sel], P[np.ix_(sel, sel)]
        if d is not None:
            d.set_state(xs, Ps, 0)
        line["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
        if B > 1:
            line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * B
    f.close()
    if d is not None:
        d.close()
    return line


def derive(line, a):
    if "split_us" in line:
        t_us = line["split_us"]["k_ext_tiles"]
        line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / mb.HBM_PEAK if t_us > 0 else None
        if line.get("dense_pass_us"):
            line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
            line["kernels_vs_dense_pass"] = line["kernel_us"] / line["dense_pass_us"]
    if line.get("dense_pass_us"):
        line["wall_vs_dense_pass"] = line["wall_us"] / line["dense_pass_us"]
    if line.get("host_round_trip_ms"):
        line["wall_vs_host_round_trip"] = line["wall_us"] / (line["host_round_trip_ms"] * 1e3)


if __name__ == "__main__":  # (every extraction ends with one k_ext_vec)
    if "--dry" in sys.argv[1:]:
        for case in CASES:
            print(json.dumps(plan(case)))
        sys.exit(0)
    mb.main(__file__, CASES, child, derive=derive, trace=dict(kernels=KERNELS, last_kernel="k_ext_vec", tag="xm", extras=lambda calls: dict(
        tiles_us_all=[round(m.get("k_ext_tiles", 0.0), 2) for m in calls])))
