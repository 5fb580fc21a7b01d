#!/usr/bin/env python3
"""Frame changes (ekf_transform_frame / ekf_anchor_at_robot and their batch forms): one JSON line per case.

Cases: N = 4096 and N = 1024 landmarks in both pipeline modes (EKF_OVERLAP=0/1) and the batch of 256 filters x 256 landmarks, each
with the rigid transform and the anchor.  The parent process never opens the GPU: every case runs in a child of its own under
`timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  wall_us             the call's wall time on a settled handle (median of --reps; the call synchronises)
  kernel_us, split_us the call's own kernels (k_reframe_vec, k_reframe_tiles, k_reframe_finish) from a second child of the case under
                      `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over that child's three calls)
  bytes               algorithmic bytes of the tile kernel (one read and one write of every live chain) and bytes / tile-kernel time
                      as a fraction of 8 TB/s
  dense_pass_us       yardstick 1, same process, same handle: one in-place dense pass folding a one-slot window (ekf_flush under
                      ekf_flush_profile; the same bytes as the tile kernel).  null for handles whose chain kernel folds its own windows
                      (ekf_fused_pass: the batch), where no dense-pass launch exists to time
  host_round_trip_ms  yardstick 2, same process: get_state -> NumPy (tests/reframe_ref.py, blockwise) -> set_state of filter 0
                      (the batch: times 256 is quoted as an estimate)
  tile_vs_dense_pass, wall_vs_host_round_trip   the two ratios the write-up quotes
--pmc COUNTERS adds a third child per case under `rocprofv3 --pmc` alone (counters are never collected together with a trace).
usage: python3 scripts/bench_reframe.py [--reps 5] [--kernel-trace] [--pmc SQ_WAVES,...] [--cases a,b] [--out profiles/reframe.jsonl]
"""
import statistics
import time

import mapbench as mb

FRAME = (3.0, -2.0, 0.7)
CASES = ["%s_%s_%s" % (size, mode, call) for size in ("n4096", "n1024", "batch256") for mode in ("inplace", "overlap") for call in ("rigid", "anchor")]
KERNELS = ("k_reframe_vec", "k_reframe_tiles", "k_reframe_finish")


def parse(case):
    size, mode, call = case.split("_")
    if size == "batch256":
        return dict(B=256, N=256, cap=256, overlap=mode == "overlap", call=call)
    N = int(size[1:])
    return dict(B=1, N=N, cap=N, overlap=mode == "overlap", call=call)


def algorithmic_bytes(c):
    nT = (2 * c["N"] + 63) // 64
    chains = 16 * nT * (nT + 1) // 2 - 6 * nT  # (the six dead chains of every diagonal tile are skipped)
    return c["B"] * chains * 256 * 8 * 2


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    f, x0, P0 = mb.injected_handle(pkg, c["B"], c["N"], c["cap"], c["overlap"])
    line = dict(case=case, N=c["N"], batch=c["B"], overlap=bool(f.overlap), call=c["call"], bytes=algorithmic_bytes(c))
    if baselines:  # yardstick 1: one dense pass over the same tiles
        line["dense_pass_us"] = None if f.fused_pass else mb.dense_pass_us(pkg, f, x0, P0)[0]
        mb.load_state(f, x0, P0)
    frames = np.tile(np.array(FRAME), (c["B"], 1))
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        if c["call"] == "rigid":
            f.transform_frame(frames) if c["B"] > 1 else f.transform_frame(FRAME, index=0)
        else:
            f.anchor_at_robot() if c["B"] > 1 else f.anchor_at_robot(index=0)
        wall.append((time.perf_counter() - t0) * 1e6)
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        import reframe_ref as rr
        f.set_state(x0, P0, 0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        xn, Pn = rr.rigid(x, P, FRAME) if c["call"] == "rigid" else rr.anchor(x, P)
        f.set_state(xn, Pn, 0)
        line["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
        if c["B"] > 1:
            line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * c["B"]
    f.close()
    return line


def derive(line, a):
    if "split_us" in line:
        t_us = line["split_us"]["k_reframe_tiles"]
        line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / mb.HBM_PEAK if t_us > 0 else None
        if line.get("dense_pass_us"):
            line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
    if a.pmc:
        line["pmc_tiles"] = mb.pmc_run(__file__, line["case"], a.pmc, "k_reframe_tiles", "rf", a.child_timeout)
    if line.get("host_round_trip_ms"):
        line["wall_vs_host_round_trip"] = line["wall_us"] / (line["host_round_trip_ms"] * 1e3)


if __name__ == "__main__":  # (every call ends with one k_reframe_finish; the traced child makes three calls whatever --reps says)
    mb.main(__file__, CASES, child, trace=dict(kernels=KERNELS, last_kernel="k_reframe_finish", tag="rf", reps=3), derive=derive, keep_stats=True,
            add_args=lambda ap: ap.add_argument("--pmc", default=None, help="comma-separated counters, collected in a run of their own"))
