#!/usr/bin/env python3
"""Whole-state consistency (ekf_joint_consistency / ekf_batch_joint_consistency): one JSON line per case.

Cases: N = 4096 and N = 1024 landmarks (capacity = N), each in both pipeline modes (EKF_OVERLAP=0/1), and the batch form at
256 filters x 256 landmarks.  The parent process never opens the GPU: every case runs in a child of its own under `timeout -k 10`,
and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  first_call_us       the first call on the handle: the scratch allocation (one more P_LL buffer per filter) and the call
  wall_us             the call's wall time on a settled handle (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels per family (k_chol_stage, k_chol_diag, k_chol_panel, k_chol_trail, k_chol_finish) from a
                      second child of the case under `rocprofv3 --kernel-trace --stats` (--kernel-trace; no counters in that run;
                      median over the child's calls with the range, the first call left out); launches = kernels per call
  dense_pass_us       for scale, same handle: one in-place dense pass folding a one-slot window and one folding a full window of 32
                      slots = 16 pairs (ekf_flush under ekf_flush_profile).  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass: the batch), and when the window did not close as exactly one pass
  host_ms             the host path, same process: get_state -> scipy.linalg.cho_factor / cho_solve on the whole P (the threads the
                      environment allows), split into its two parts (the batch: one filter, times 256 quoted as an estimate)
  worst_rel_err       the device's NEES / log-det fields against that host result
usage: python3 scripts/bench_joint_consistency.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/joint_consistency.jsonl]
"""
import statistics
import time

import mapbench as mb

CASES = ["n4096_inplace", "n4096_overlap", "n1024_inplace", "n1024_overlap", "batch256_inplace"]
KERNELS = ("k_chol_stage", "k_chol_diag", "k_chol_panel", "k_chol_trail", "k_chol_finish")


def parse(case):
    size, mode = case.split("_")
    if size == "batch256":
        return dict(B=256, N=256, overlap=mode == "overlap")
    return dict(B=1, N=int(size[1:]), overlap=mode == "overlap")


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    B, N = c["B"], c["N"]
    f, x0, P0 = mb.injected_handle(pkg, B, N, N, c["overlap"], max_pending=32)
    xt = x0 + 0.05 * np.random.default_rng(1).standard_normal(len(x0))
    xt_all = np.tile(xt, (B, 1))
    call = (lambda: f.joint_consistency(xt_all)) if B > 1 else (lambda: f.joint_consistency(xt, 0))
    line = dict(case=case, N=N, batch=B, overlap=bool(f.overlap), tile_steps=(2 * N + 63) // 64)
    f.sync()
    bytes0 = f.device_bytes()
    t0 = time.perf_counter()
    rows = call()
    line["first_call_us"] = (time.perf_counter() - t0) * 1e6
    line["scratch_bytes"] = int(f.device_bytes() - bytes0)
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        again = call()
        wall.append((time.perf_counter() - t0) * 1e6)
        assert again.tobytes() == rows.tobytes()
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    assert all(int(v) == 0 for v in rows["info"])
    if baselines:
        import scipy.linalg
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        e = x - xt
        cf = scipy.linalg.cho_factor(P, lower=False)
        nees = float(e @ scipy.linalg.cho_solve(cf, e))
        logdet = 2.0 * float(np.sum(np.log(np.diag(cf[0]))))
        t2 = time.perf_counter()
        line["host_ms"] = dict(get_state=(t1 - t0) * 1e3, factor_and_solve=(t2 - t1) * 1e3, total=(t2 - t0) * 1e3)
        if B > 1:
            line["host_ms_whole_batch_estimate"] = line["host_ms"]["total"] * B
        line["worst_rel_err"] = max(abs(float(rows[0]["nees_joint"]) - nees) / nees, abs(float(rows[0]["logdet_joint"]) - logdet) / abs(logdet))
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:
            one, one_all = mb.dense_pass_us(pkg, f, x0, P0, 1)
            full, full_all = mb.dense_pass_us(pkg, f, x0, P0, 32)
            line["dense_pass_us"] = dict(one_slot=one, one_slot_all=one_all, pairs16=full, pairs16_all=full_all)
    f.close()
    return line


def trace_extras(calls):
    """The ranges beside the medians (split_us to one digit), the device time from a call's first start to its last end, the launches."""
    total = [sum(m.get(k, 0.0) for k in KERNELS) for m in calls]
    per = {k: [m.get(k, 0.0) for m in calls] for k in KERNELS}
    return dict(kernel_us_range=[round(min(total), 1), round(max(total), 1)],
                split_us={k: round(statistics.median(v), 1) for k, v in per.items()},
                split_us_range={k: [round(min(v), 1), round(max(v), 1)] for k, v in per.items()},
                device_span_us=statistics.median(m["span"] for m in calls), launches=calls[0]["launches"])


def derive(line, a):
    if "kernel_us" in line and (line.get("dense_pass_us") or {}).get("pairs16"):
        line["kernels_vs_16pair_pass"] = line["kernel_us"] / line["dense_pass_us"]["pairs16"]
    if line.get("host_ms"):
        line["host_vs_wall"] = line["host_ms"]["total"] * 1e3 / line["wall_us"]


if __name__ == "__main__":  # (every call ends with one k_chol_finish; the first call is the one with the allocation)
    mb.main(__file__, CASES, child, derive=derive,
            trace=dict(kernels=KERNELS, last_kernel="k_chol_finish", tag="jc", skip_first=True, extras=trace_extras))
