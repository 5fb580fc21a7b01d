#!/usr/bin/env python3
"""Map joining (ekf_join_map / ekf_batch_join_map): one JSON line per case.

Cases: Ns = 256 into Ng = 3840 (capacity 4096) and Ns = 64 into Ng = 960 (capacity 1024), each in both pipeline modes of the
destination (EKF_OVERLAP=0/1), and the batch form at 256 filters x (128 + 64, capacity 256).  The source handle has the capacity of
its own map.  The parent process never opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first
failing child ends the run (scripts/mapbench.py).  Between two timed joins the destination is cut back to Ng landmarks on the device
(ekf_remove_landmarks), so every repetition joins into the same layout.  Each line carries
  wall_us             the call's wall time with both handles settled (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels (k_join_tiles, k_join_vec, k_join_finish) from a second child of the case under
                      `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over the child's calls, all values kept)
  bytes               algorithmic bytes of the tile kernel: the destination tiles that hold a new column, written once, plus the
                      source's stored tiles, read once; and bytes / tile-kernel time as a fraction of 8 TB/s
  dense_pass_us       yardstick 1, same process, the destination handle: one in-place dense pass folding a one-slot window (ekf_flush
                      under ekf_flush_profile), which reads and writes ALL of P.  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass: the batch), where no dense-pass launch exists to time
  host_round_trip_ms  yardstick 2, same process: get_state of both filters -> NumPy (tests/join_ref.py, the block table) ->
                      set_state of filter 0 (the batch: times 256 is quoted as an estimate)
usage: python3 scripts/bench_join_map.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/join_map.jsonl]
"""
import os
import statistics
import time

import mapbench as mb

CASES = ["n4096_inplace", "n4096_overlap", "n1024_inplace", "n1024_overlap", "batch256_inplace"]
KERNELS = ("k_join_tiles", "k_join_vec", "k_join_finish")


def parse(case):
    size, mode = case.split("_")
    if size == "batch256":
        return dict(B=256, Ng=128, Ns=64, cap=256, cap_s=64, overlap=mode == "overlap")
    cap = int(size[1:])
    Ns = cap // 16
    return dict(B=1, Ng=cap - Ns, Ns=Ns, cap=cap, cap_s=Ns, overlap=mode == "overlap")


def algorithmic_bytes(c):
    J0, J1 = c["Ng"] // 32, (2 * (c["Ng"] + c["Ns"]) + 63) // 64
    Ts = (2 * c["Ns"] + 63) // 64
    return c["B"] * (J1 * (J1 + 1) // 2 - J0 * (J0 + 1) // 2 + Ts * (Ts + 1) // 2) * 4096 * 8


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    B, Ng, Ns = c["B"], c["Ng"], c["Ns"]
    f, xg, Pg = mb.injected_handle(pkg, B, Ng, c["cap"], c["overlap"])
    os.environ["EKF_OVERLAP"] = "0"
    s = pkg.FilterBatch(B, c["cap_s"])
    mb.load_state(s, *pkg.scenarios.injected_state(Ns, seed=9, extent=8.0))
    line = dict(case=case, Ng=Ng, Ns=Ns, batch=B, overlap=bool(f.overlap), bytes=algorithmic_bytes(c))
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick 1: one dense pass over all of P
            line["dense_pass_us"], line["dense_pass_us_all"] = mb.dense_pass_us(pkg, f, xg, Pg)
            mb.load_state(f, xg, Pg)
    keep = np.zeros((B, Ng + Ns), dtype=bool)
    keep[:, :Ng] = True
    wall = []
    for r in range(reps):
        f.sync(), s.sync()
        t0 = time.perf_counter()
        if B > 1:
            f.batch_join_map(s)
        else:
            f.join_map(s)
        wall.append((time.perf_counter() - t0) * 1e6)
        assert int(f.num_landmarks()[0]) == Ng + Ns
        f.remove_landmarks(keep if B > 1 else keep[0], index=None if B > 1 else 0)  # back to Ng landmarks, on the device
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        import join_ref as jr
        f.set_state(xg, Pg, 0)
        f.sync()
        t0 = time.perf_counter()
        a, b = f.get_state(0), s.get_state(0)
        xn, Pn = jr.join_blocks(a[0], a[1], b[0], b[1])
        f.set_state(xn, Pn, 0)
        line["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
        if B > 1:
            line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * B
    f.close(), s.close()
    return line


def derive(line, a):
    if "split_us" in line:
        t_us = line["split_us"]["k_join_tiles"]
        line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / mb.HBM_PEAK if t_us > 0 else None
        if line.get("dense_pass_us"):
            line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
            line["kernels_vs_dense_pass"] = line["kernel_us"] / line["dense_pass_us"]
    if line.get("host_round_trip_ms"):
        line["wall_vs_host_round_trip"] = line["wall_us"] / (line["host_round_trip_ms"] * 1e3)


if __name__ == "__main__":  # (every call ends with one k_join_finish)
    mb.main(__file__, CASES, child, derive=derive, trace=dict(kernels=KERNELS, last_kernel="k_join_finish", tag="jm", extras=lambda calls: dict(
        tiles_us_all=[round(m.get("k_join_tiles", 0.0), 2) for m in calls])))
