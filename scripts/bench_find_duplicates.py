#!/usr/bin/env python3
"""Duplicate search (ekf_find_duplicates / ekf_batch_find_duplicates): one JSON line per case.

Cases: N = 4096 over all pairs, with split = 3840 (the old x new pairs of a 3840 + 256 join), and with max_dist = 2 on a map whose
landmarks are numbered along a path (a line, 0.5 m apart: a group of 32 spans 16 m, so only a tile and its neighbour survive the
bounding-box test); N = 1024 over all pairs; the batch form at 256 filters x N = 256.  States are the injected ones
(scenarios.injected_state) at full capacity, in the in-place pipeline mode.  The parent process never opens the GPU: every case runs
in a child of its own under `timeout -k 10`, and the first failing child ends the run (scripts/mapbench.py).  Each line carries
  wall_us             the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises)
  kernel_us, split_us the call's own kernels (k_dup_boxes, k_dup_tiles) from a second child of the case under
                      `rocprofv3 --kernel-trace --stats` (--kernel-trace; median over the child's calls, all values kept)
  tiles, bytes        tiles the tile kernel loads (those its grid names, less the ones the bounding boxes cull -- recomputed here
                      by the kernel's rule) and the bytes of their live chains (a diagonal tile: 10 of 16); bytes / tile-kernel
                      time as a fraction of 8 TB/s
  dense_pass_us       yardstick 1, same process, the same handle: one in-place dense pass folding a one-slot window (ekf_flush
                      under ekf_flush_profile), which reads and writes ALL of P.  null for handles whose chain kernel folds its own
                      windows (ekf_fused_pass: the batch), where no dense-pass launch exists to time
  host_path_ms        yardstick 2, same process: get_state of filter 0 -> NumPy (tests/dup_ref.py), split into its two parts (the
                      batch: times 256 is quoted as an estimate)
usage: python3 scripts/bench_find_duplicates.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/find_duplicates.jsonl]
"""
import statistics
import time

import mapbench as mb

GATE = 9.21
CASES = ["n4096_all", "n4096_split3840", "n4096_path2m", "n1024_all", "batch256_all"]
KERNELS = ("k_dup_boxes", "k_dup_tiles")


def parse(case):
    size, what = case.split("_")
    B, N = (256, 256) if size == "batch256" else (1, int(size[1:]))
    return dict(B=B, N=N, split=int(what[5:]) if what.startswith("split") else 0, max_dist=float(what[4:-1]) if what.startswith("path") else None,
                path=what.startswith("path"))


def visited_tiles(x, N, split, max_dist):
    """(off-diagonal, diagonal) tiles the tile kernel loads: ekf_device.h's dup_tile_ij list, less the culled ones."""
    import numpy as np
    nT = (N + 31) // 32
    L = x[3:].reshape(-1, 2)
    lo = np.array([L[32 * g:32 * g + 32].min(axis=0) for g in range(nT)])
    hi = np.array([L[32 * g:32 * g + 32].max(axis=0) for g in range(nT)])
    off = diag = 0
    for I in range(nT):
        if split and I > (split - 1) // 32:
            break
        J0 = max(I, split // 32 if split else I)
        gap = np.maximum(np.maximum(lo[I] - hi[J0:], lo[J0:] - hi[I]), 0.0)
        live = np.ones(nT - J0, dtype=bool) if max_dist is None else (gap ** 2).sum(axis=1) <= max_dist * max_dist
        diag += int(live[0]) if J0 == I else 0
        off += int(live.sum()) - (int(live[0]) if J0 == I else 0)
    return off, diag


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    c = parse(case)
    B, N = c["B"], c["N"]
    f, x0, P0 = mb.injected_handle(pkg, B, N, N, False)
    xs = x0.copy()  # the searched state: the injected one, or its landmarks laid along a line in the order of their numbers
    if c["path"]:
        rng = np.random.default_rng(11)
        xs[3::2] = 0.5 * np.arange(N)
        xs[4::2] = rng.uniform(-2.0, 2.0, size=N)
    off, diag = visited_tiles(xs, N, c["split"], c["max_dist"])
    line = dict(case=case, N=N, batch=B, split=c["split"], max_dist=c["max_dist"], tiles=B * (off + diag), bytes=B * (off * 16 + diag * 10) * 2048)
    if baselines:
        if f.fused_pass:
            line["dense_pass_us"] = None
        else:  # yardstick 1: one dense pass over all of P
            line["dense_pass_us"], line["dense_pass_us_all"] = mb.dense_pass_us(pkg, f, x0, P0)
    mb.load_state(f, xs, P0)
    index = None if B > 1 else 0
    call = lambda: f.find_duplicates(GATE, c["max_dist"], c["split"], index)  # noqa: E731
    first = call()  # (allocates the scratch)
    wall = []
    for r in range(reps):
        f.sync()
        t0 = time.perf_counter()
        got = call()
        wall.append((time.perf_counter() - t0) * 1e6)
    one = got[0] if B > 1 else got
    assert one[0].tobytes() == (first[0] if B > 1 else first)[0].tobytes()
    line["found"], line["degenerate"] = one[1], one[2]
    line["wall_us"] = statistics.median(wall)
    line["wall_us_all"] = [round(w, 1) for w in wall]
    if baselines:
        import dup_ref as dr
        f.sync()
        t0 = time.perf_counter()
        x, P = f.get_state(0)
        t1 = time.perf_counter()
        ref, _ = dr.find(x, P, GATE, c["max_dist"], c["split"])
        t2 = time.perf_counter()
        line["host_path_ms"] = (t2 - t0) * 1e3
        line["host_get_state_ms"], line["host_numpy_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        line["matches_host"] = bool(ref["i"].tolist() == one[0]["i"].tolist() and ref["j"].tolist() == one[0]["j"].tolist())
        if B > 1:
            line["host_path_ms_whole_batch_estimate"] = line["host_path_ms"] * B
    f.close()
    return line


def derive(line, a):
    if "split_us" in line:
        t_us = line["split_us"]["k_dup_tiles"]
        line["hbm_fraction_of_8TBps"] = line["bytes"] / (t_us * 1e-6) / mb.HBM_PEAK if t_us > 0 else None
        if line.get("dense_pass_us"):
            line["tile_vs_dense_pass"] = t_us / line["dense_pass_us"]
            line["kernels_vs_dense_pass"] = line["kernel_us"] / line["dense_pass_us"]
    if line.get("host_path_ms"):
        line["wall_vs_host_path"] = line["wall_us"] / (line["host_path_ms"] * 1e3)


if __name__ == "__main__":  # (every call ends with one k_dup_tiles; the first call is the one that allocates the scratch)
    mb.main(__file__, CASES, child, derive=derive, trace=dict(kernels=KERNELS, last_kernel="k_dup_tiles", tag="fd", skip_first=True, extras=lambda calls: dict(
        tiles_us_all=[round(m.get("k_dup_tiles", 0.0), 2) for m in calls])))
