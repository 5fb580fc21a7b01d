#!/usr/bin/env python3
"""Landmark initialisation (ekf_add_landmarks / ekf_batch_add_landmarks) and the scan step (ekf_update_joint): one JSON line per case.

Cases: m = 8 into N = 4088 and m = 64 into N = 3840 (capacity 4096), m = 8 into N = 56 (capacity 64), the batch form at 256 filters
x (N = 128, m = 8, capacity 256), and one ekf_update_joint call of the ambiguous 12-measurement scan at N = 200 of
bench_associate_joint.py: as it is (joint_n200: nothing is New, the third part is a no-op), and with two far features in FRONT of it
(joint_n200_new2: the third part adds two landmarks; behind the scan the two would loosen the search's bound cnt + (m - i) for every
node and cost two orders of magnitude more nodes).  The parent process never
opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first failing child ends the run
(scripts/mapbench.py).  Between two timed adds the filter is cut back to N landmarks on the device (ekf_remove_landmarks), so every
repetition adds into the same layout; the scans are tests/add_ref.py's grid (features the filter's own gate calls New as well).
Each add line carries
  wall_us               the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us   the call's own kernels (k_add_vec, k_add_tiles, k_add_finish) from a second child of the case under
                        `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over the child's calls)
  bytes                 algorithmic bytes of the tile kernel: the tiles that hold a new column, written once; and bytes / tile-kernel
                        time as a fraction of 8 TB/s
  host_round_trip_ms    baseline 1: get_state -> NumPy (tests/add_ref.py) -> set_state of filter 0 (the batch: times 256 quoted as
                        an estimate)
  join_route_us         baseline 2: a scratch handle loaded with the block-diagonal source x = (0, 0, 0, z..), P = blockdiag(0_3, R..)
                        by ekf_set_state, then ekf_join_map (the batch: set_state, ekf_broadcast_state, ekf_batch_join_map); the
                        scratch handle exists before the clock starts
                        Both baselines run in a child of their own and call nothing but entry points that exist without this
                        one (ekf_get_state, ekf_set_state, ekf_broadcast_state, ekf_join_map)
The ekf_update_joint line carries wall_us and the wall times of ekf_associate_joint, ekf_update_matched and ekf_add_landmarks made
in sequence from the same entry state, their sum, and the kinds of the scan.
--kernel-trace expects one k_add_finish per call: run joint_n200, which launches none, without it.
usage: python3 scripts/bench_add_landmarks.py [--reps 7] [--kernel-trace] [--cases a,b] [--out profiles/add_landmarks.jsonl]
"""
import os
import statistics
import time

import mapbench as mb
from bench_gate_candidates import timed

CASES = ["m8_n4088", "m64_n3840", "m8_n56", "batch256", "joint_n200", "joint_n200_new2"]
KERNELS = ("k_add_vec", "k_add_tiles", "k_add_finish")
SHAPES = {"m8_n4088": (1, 4088, 8, 4096), "m64_n3840": (1, 3840, 64, 4096), "m8_n56": (1, 56, 8, 64), "batch256": (256, 128, 8, 256)}


def algorithmic_bytes(B, N, m):
    J0, J1 = N // 32, (2 * (N + m) + 63) // 64
    return B * (J1 * (J1 + 1) // 2 - J0 * (J0 + 1) // 2) * 4096 * 8


def reset(f, B, N, m):
    import numpy as np
    keep = np.zeros((B, N + m), dtype=bool)
    keep[:, :N] = True
    f.remove_landmarks(keep if B > 1 else keep[0], index=None if B > 1 else 0)  # back to N landmarks, on the device


def add_child(case, reps, baselines):
    import numpy as np
    import add_ref as ad
    pkg = mb.package()
    B, N, m, cap = SHAPES[case]
    f, x0, P0 = mb.injected_handle(pkg, B, N, cap, False)
    z, R = ad.grid_scan(pkg, m)
    zb, Rb = (np.tile(z, (B, 1, 1)), np.tile(R, (B, 1, 1, 1))) if B > 1 else (z, R)
    index = None if B > 1 else 0
    line = dict(case=case, N=N, m=m, batch=B, overlap=int(f.overlap), bytes=algorithmic_bytes(B, N, m))
    f.add_landmarks(zb, Rb, None, index)  # (allocates the scratch)
    wall = []
    for r in range(reps):
        reset(f, B, N, m)
        f.sync()
        t0 = time.perf_counter()
        n, _ = f.add_landmarks(zb, Rb, None, index)
        wall.append((time.perf_counter() - t0) * 1e6)
        assert int(np.max(n)) == N + m
    line["wall_us"], line["wall_us_all"] = statistics.median(wall), [round(w, 1) for w in wall]
    f.close()
    return line


def base_child(case, reps):
    """The two baselines: nothing here calls a new entry point."""
    import numpy as np
    import add_ref as ad
    pkg = mb.package()
    B, N, m, cap = SHAPES[case]
    f, x0, P0 = mb.injected_handle(pkg, B, N, cap, False)
    z, R = ad.grid_scan(pkg, m)
    line = {}
    host = []
    for r in range(3):
        mb.load_state(f, x0, P0)
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        f.set_state(*ad.add(x, P, z, R), 0)
        host.append((time.perf_counter() - t0) * 1e3)
    line["host_round_trip_ms"], line["host_round_trip_ms_all"] = statistics.median(host), [round(h, 3) for h in host]
    if B > 1:
        line["host_round_trip_ms_whole_batch_estimate"] = line["host_round_trip_ms"] * B
    mb.load_state(f, x0, P0)
    os.environ["EKF_OVERLAP"] = "0"
    s = pkg.FilterBatch(B, max(m, 8))
    xs, Ps = ad.as_join_source(z, R)
    route = []
    for r in range(reps):
        f.sync(), s.sync()
        t0 = time.perf_counter()
        s.set_state(xs, Ps, 0)
        if B > 1:
            s.broadcast_state()
            f.batch_join_map(s)
        else:
            f.join_map(s)
        route.append((time.perf_counter() - t0) * 1e6)
        assert int(f.num_landmarks()[0]) == N + m
        reset(f, B, N, m)
    line["join_route_us"], line["join_route_us_all"] = statistics.median(route), [round(w, 1) for w in route]
    f.close(), s.close()
    return line


def joint_child(case, reps, baselines):
    import numpy as np
    import assoc_ref as ar
    pkg = mb.package()
    E = pkg.ekfslam
    N, cap, extent, count, seed = ar.AMBIGUOUS[1]
    x0, P0, z, R, _ = ar.ambiguous_scan(pkg, N, extent, count, seed)
    far = [pkg.scenarios.measurement_from_feature_mm(60000.0, 35000.0), pkg.scenarios.measurement_from_feature_mm(-45000.0, 52000.0)]
    if case.endswith("_new2"):
        z = np.concatenate([fz[0].reshape(1, 2) for fz in far] + [z])
        R = np.concatenate([fz[1].reshape(1, 2, 2) for fz in far] + [R])
    os.environ["EKF_OVERLAP"] = "0"
    f = pkg.FilterBatch(1, cap, max_pending=16)
    load = lambda: f.set_state(x0, P0)  # noqa: E731
    load()
    first = f.update_joint(z, R)  # (allocates the scratch)
    line = dict(case=case, N=N, n_z=len(z), overlap=int(f.overlap), kinds=first[2].tolist(), nodes=int(first[4]["nodes"]))
    line["wall_us"], line["wall_us_all"], got = timed(f, lambda: f.update_joint(z, R), reps, before=load)
    assert got[1].tolist() == first[1].tolist()
    if baselines:
        ids, _, _, near, _ = f.associate_joint(z, R)
        is_new = (ids < 0) & (near["decision"] == E.NEW)
        matched = lambda: (load(), f.update_matched(z, R, ids))  # noqa: E731
        line["associate_us"], line["associate_us_all"], _ = timed(f, lambda: f.associate_joint(z, R), reps, before=load)
        line["update_matched_us"], line["update_matched_us_all"], _ = timed(f, lambda: f.update_matched(z, R, ids), reps, before=load)
        line["add_landmarks_us"], line["add_landmarks_us_all"], _ = timed(f, lambda: f.add_landmarks(z, R, is_new), reps, before=matched)
        line["three_calls_us"] = line["associate_us"] + line["update_matched_us"] + line["add_landmarks_us"]
    f.close()
    return line


def child(case, reps, baselines):
    if case.startswith("base:"):
        return base_child(case[5:], reps)
    return joint_child(case, reps, baselines) if case.startswith("joint") else add_child(case, reps, baselines)


def derive(line, a):
    if "split_us" in line and line.get("bytes"):
        t_us = line["split_us"]["k_add_tiles"]
        line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / mb.HBM_PEAK if t_us > 0 else None
    if line["case"] in SHAPES and not a.no_baselines:  # the baselines: a child of their own
        line.update(mb.run_child(__file__, "base:" + line["case"], a.reps, True, timeout_s=a.child_timeout))
        line["wall_vs_join_route"] = line["wall_us"] / line["join_route_us"]
        line["wall_vs_host_round_trip"] = line["wall_us"] / (line.get("host_round_trip_ms_whole_batch_estimate", line["host_round_trip_ms"]) * 1e3)
    if line.get("three_calls_us"):
        line["wall_vs_three_calls"] = line["wall_us"] / line["three_calls_us"]


if __name__ == "__main__":  # (every call ends with one k_add_finish; the first call is the one that allocates the scratch)
    mb.main(__file__, CASES, child, derive=derive, add_args=lambda ap: ap.set_defaults(reps=7),
            trace=dict(kernels=KERNELS, last_kernel="k_add_finish", tag="al", skip_first=True))
