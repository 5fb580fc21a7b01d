#!/usr/bin/env python3
"""The joint-compatibility search (ekf_associate_joint / ekf_batch_associate_joint): one JSON line per case.

Cases: the ambiguous scan of 12 measurements at N = 200 in capacity 320 (tests/assoc_ref.py: greedy matching gets 6 of them wrong),
one filter of N = 4096 with a scan of the 32 landmarks nearest the robot, and the batch form at 256 filters x N = 256 with that scan
length.  The parent process never opens the GPU: every case runs in a child of its own under `timeout -k 10`, and the first failing
child ends the run (scripts/mapbench.py).  Each line carries
  wall_us               the call's wall time on the settled handle (median of --reps, all values kept; the call synchronises): the
                        sweep of ekf_gate_candidates, the host's table, the search, k_match_factor on the winner, the copies back
  nodes, n_paired       of the search (filter 0 of the batch), complete
  wall_one_node_us      the same call with max_nodes = 1: everything but the search beyond its root
  per_node_us           (wall_us - wall_one_node_us) / (nodes - 1)
  gate_candidates_us    yardstick 1, same handle: ekf_gate_candidates alone on the scan
  host_loop_ms          yardstick 2, same handle: the identical traversal driven from Python, one gate_candidates call and one
                        joint_compat call per tried extension (host_extensions of them; both calls exist without this one); the
                        batch: filter 0 alone, times 256 quoted as an estimate
  matches_host          the same ids, n_paired and nodes from both
  kernel_us, split_us   k_assoc_search and the kernels around it from a second child under `rocprofv3 --kernel-trace --stats`
                        (--kernel-trace; median over the child's calls)
usage: python3 scripts/bench_associate_joint.py [--reps 5] [--kernel-trace] [--cases a,b] [--out profiles/associate_joint.jsonl]
"""
import time

import mapbench as mb
from bench_gate_candidates import scan, timed

GATE = 9.21
MAX_BRANCH, MAX_NODES = 8, 65536
CASES = ["ambiguous200_inplace", "n4096_inplace", "batch256_inplace"]
KERNELS = ("k_gate_nearest", "k_gate(", "k_assoc_search", "k_match_factor")


def host_search(f, z, R, jg, index, max_branch, max_nodes):
    """The recursion of include/ekfslam_c.h over gate_candidates and one joint_compat call per tried extension:
    (ids, n_paired, nodes, complete, extensions)."""
    import numpy as np
    n_z = len(z)
    cands = f.gate_candidates(z, R, GATE, index)[0]
    lists = [[int(c["landmark"]) for c in cands if c["meas"] == k][:max_branch] for k in range(n_z)]
    best = dict(cnt=0, d2=0.0, ids=np.full(n_z, -1, dtype=np.int32))
    st = dict(nodes=0, complete=1, ext=0)
    if len(cands) == 0:
        return best["ids"], 0, 0, 1, 0

    class Stop(Exception):
        pass

    def rec(ids, i, cnt, D2):
        rest = cnt + (n_z - i)
        if rest < best["cnt"] or (rest == best["cnt"] and D2 >= best["d2"]):
            return
        if i == n_z:
            best.update(cnt=cnt, d2=D2, ids=ids.copy())
            return
        if st["nodes"] == max_nodes:
            st["complete"] = 0
            raise Stop
        st["nodes"] += 1
        for l in lists[i]:
            if l in ids:
                continue
            ids[i] = l
            st["ext"] += 1
            d = f.joint_compat(z, R, ids, index)[i]
            if d <= jg[cnt]:
                rec(ids, i + 1, cnt + 1, d)
            ids[i] = -1
        rec(ids, i + 1, cnt, D2)

    try:
        rec(best["ids"].copy(), 0, 0, 0.0)
    except Stop:
        pass
    return best["ids"], best["cnt"], st["nodes"], st["complete"], st["ext"]


def child(case, reps, baselines):
    import numpy as np
    pkg = mb.package()
    size = case.split("_")[0]
    if size.startswith("ambiguous"):
        import os
        import assoc_ref as ar
        N, cap, extent, count, seed = ar.AMBIGUOUS[1]
        B = 1
        x0, P0, z, R, _ = ar.ambiguous_scan(pkg, N, extent, count, seed)
        os.environ["EKF_OVERLAP"] = "0"
        f = pkg.FilterBatch(1, cap, max_pending=16)
        f.set_state(x0, P0)
    else:
        B, N = (256, int(size[5:])) if size.startswith("batch") else (1, int(size[1:]))
        f, x0, P0 = mb.injected_handle(pkg, B, N, N, False, max_pending=16)
        z, R = scan(pkg, x0, 32)
    zb, Rb = (np.tile(z, (B, 1, 1)), np.tile(R, (B, 1, 1, 1))) if B > 1 else (z, R)
    index = None if B > 1 else 0
    jg = pkg.joint_gates(0.99)
    call = lambda nodes=MAX_NODES: f.associate_joint(zb, Rb, GATE, None, MAX_BRANCH, nodes, index)  # noqa: E731
    line = dict(case=case, N=N, batch=B, n_z=len(z), overlap=int(f.overlap), max_branch=MAX_BRANCH)
    first = call()  # (allocates the scratch)
    line["wall_us"], line["wall_us_all"], got = timed(f, call, reps)
    one, one_first = (got[0], first[0]) if B > 1 else (got, first)
    assert one[0].tobytes() == one_first[0].tobytes() and one[2].tobytes() == one_first[2].tobytes()
    info = one[2]
    line.update(nodes=int(info["nodes"]), n_paired=int(info["n_paired"]), complete=int(info["complete"]), n_candidates=int(info["n_candidates"]))
    if baselines:
        line["wall_one_node_us"], line["wall_one_node_us_all"], _ = timed(f, lambda: call(1), reps)
        line["gate_candidates_us"], line["gate_candidates_us_all"], _ = timed(f, lambda: f.gate_candidates(zb, Rb, GATE, index), reps)
        f.joint_compat(z, R, one[0], 0)
        f.sync()
        t0 = time.perf_counter()
        ids, paired, nodes, complete, ext = host_search(f, z, R, jg, 0, MAX_BRANCH, MAX_NODES)
        line["host_loop_ms"], line["host_extensions"] = (time.perf_counter() - t0) * 1e3, ext
        line["matches_host"] = bool(ids.tolist() == one[0].tolist() and (paired, nodes, complete) == (line["n_paired"], line["nodes"], line["complete"]))
        if B > 1:
            line["host_loop_ms_whole_batch_estimate"] = line["host_loop_ms"] * B
    f.close()
    return line


def derive(line, a):
    if line.get("wall_one_node_us") and line["nodes"] > 1:
        line["per_node_us"] = (line["wall_us"] - line["wall_one_node_us"]) / (line["nodes"] - 1)
    if line.get("host_loop_ms"):
        line["wall_vs_host_loop"] = line["wall_us"] / (line.get("host_loop_ms_whole_batch_estimate", line["host_loop_ms"]) * 1e3)


if __name__ == "__main__":  # (every call ends with one k_match_factor; the first call is the one that allocates the scratch)
    mb.main(__file__, CASES, child, derive=derive, trace=dict(kernels=KERNELS, last_kernel="k_match_factor", tag="aj", skip_first=True))
