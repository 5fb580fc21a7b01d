"""NumPy statement of ekf_associate_joint (include/ekfslam_c.h) on a dense export: the candidates from gate_ref.table / gate_ref.find,
every joint distance by match_ref.joint_compat (a full refactorisation of the hypothesis), the recursion exactly as the header
states it.  search(...) -> Result(ids, n_paired, complete, nodes, n_candidates, n_dropped, d2, evaluated): `evaluated` lists every
(D2', gate it was compared with) and every (D2, Best.D2) pair whose order decided a pruning or a new Best, for margins().
dtype=np.longdouble scores the hypotheses in extended precision (the candidate lists stay the double reference's).
The inputs of tests/test_gpu_associate_joint.py are named here and checked on the CPU in tests/test_associate_joint_cpu.py.

Measured with this file (tests/test_associate_joint_cpu.py asserts the first four columns and prints the margins): gate 9.21,
joint_gates(0.99), max_branch 8, true pose k = 2 sigma of P_RR from the estimate
    N    extent  count  seed | greedy gets wrong | joint search  | nodes | with max_nodes = 20             | smallest margin
    100  5.0     10     34   | 4 of 10           | recovers all  | 62    | 10 paired, other ids, D2 8.42  | 2.0e-4
    200  7.0     12     33   | 6 of 12           | recovers all  | 113   | 12 paired, other ids, D2 21.9  | 2.7e-4
    planted N=100 / N=200 (match_ref.SIZES): greedy right, 24 nodes each, margins 2.6e-2 / 0.15
margins() here counts EVERY comparison the recursion makes -- each D2' with its joint gate, and each D2 with Best.D2 where the two
hypotheses can still end with the same count (the pruning test and the test at a leaf are the same comparison) --, which is why
the figures are smaller than the distance of the final Best from its runner-up; all lie far above gate_ref.EDGE = 1e-6."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_ref as gr  # noqa: E402
import match_ref as mr  # noqa: E402

Result = collections.namedtuple("Result", "ids n_paired complete nodes n_candidates n_dropped d2 evaluated")
GATE = 9.21
AMBIGUOUS = [(100, 200, 5.0, 10, 34), (200, 320, 7.0, 12, 33)]   # (N, capacity, extent, count, seed): k_solo and k_chain
BUDGET = 20


def chi2_even_cdf(x, q):
    """CDF of chi-square with 2 q degrees of freedom (closed form)."""
    term, total = 1.0, 0.0
    for i in range(q):
        total += term
        term = term * (0.5 * x) / (i + 1)
    return 1.0 - np.exp(-0.5 * x) * total


class _Stop(Exception):
    pass


def search(x, P, z, R, joint_gate, valid=None, gate=GATE, max_branch=8, max_nodes=65536, cond_limit=gr.COND_LIMIT, dtype=np.float64):
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    n_z = len(z)
    valid = np.ones(n_z, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    N = (len(x) - 3) // 2
    meas = [int(k) for k in np.flatnonzero(valid)]
    m = len(meas)
    cands = gr.find(gr.table_of(x, P, z, R, valid, cond_limit), gate, cond_limit, valid=valid)[0] if N and m else np.zeros(0, dtype=gr.CAND_DTYPE)
    lists = {k: [int(c["landmark"]) for c in cands if c["meas"] == k] for k in meas}
    dropped = sum(max(0, len(v) - max_branch) for v in lists.values())
    lists = {k: v[:max_branch] for k, v in lists.items()}
    ids0 = np.full(n_z, -1, dtype=np.int32)
    if len(cands) == 0:
        return Result(ids0, 0, 1, 0, 0, 0, 0.0, [])
    best = {"cnt": 0, "d2": 0.0, "ids": ids0.copy()}
    state = {"nodes": 0, "complete": 1}
    evaluated = []

    def rec(ids, i, cnt, D2):
        rest = cnt + (m - i)
        if rest < best["cnt"]:
            return
        if rest == best["cnt"]:
            if best["cnt"]:
                evaluated.append((float(D2), float(best["d2"])))
            if D2 >= best["d2"]:
                return
        if i == m:
            best.update(cnt=cnt, d2=D2, ids=ids.copy())
            return
        if state["nodes"] == max_nodes:
            state["complete"] = 0
            raise _Stop
        state["nodes"] += 1
        k = meas[i]
        for l in lists[k]:
            if l in ids:
                continue
            ids[k] = l
            d = mr.joint_compat(x, P, z, R, ids, dtype=dtype)[k]
            if not np.isnan(d):
                evaluated.append((float(d), float(joint_gate[cnt])))
            if d <= joint_gate[cnt]:
                rec(ids, i + 1, cnt + 1, d)
            ids[k] = -1
        rec(ids, i + 1, cnt, D2)

    try:
        rec(ids0.copy(), 0, 0, 0.0)
    except _Stop:
        pass
    return Result(best["ids"], best["cnt"], state["complete"], state["nodes"], len(cands), dropped, float(best["d2"]), evaluated)


def margins(result):
    """The smallest relative distance of two compared quantities of a search (inf: nothing was compared)."""
    return min([abs(a - b) / max(abs(a), abs(b)) for a, b in result.evaluated if max(abs(a), abs(b)) > 0.0], default=np.inf)


def ambiguous_scan(pkg, N, extent, count, seed, k=2.0):
    """(x, P, z, R, ids): scenarios.injected_state and a scan of the `count` landmarks nearest the ESTIMATE, taken from a true pose
    k sigma of P_RR away from it (direction from default_rng(seed + 3000))."""
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
    rng = np.random.default_rng(seed + 3000)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    xt = np.array(x)
    xt[0:3] = x[0:3] + k * np.linalg.cholesky(P[0:3, 0:3]) @ u
    L = x[3:].reshape(-1, 2)
    near = np.argsort(np.hypot(L[:, 0] - x[0], L[:, 1] - x[1]), kind="stable")[:count]
    ids = rng.permutation(near).astype(np.int32)
    z, R = np.empty((count, 2)), np.empty((count, 2, 2))
    for q, i in enumerate(ids):
        z[q], R[q] = mr.measurement_of(pkg, xt, int(i), rng.normal(size=2))
    return x, P, z, R, ids


def inputs(pkg):
    """(name, capacity, x, P, z, R, valid or None, planted ids or None, kwargs of search) of every call the GPU tests compare."""
    out = []
    for N, cap, extent, count, seed in AMBIGUOUS:
        x, P, z, R, ids = ambiguous_scan(pkg, N, extent, count, seed)
        out.append(("ambiguous N=%d" % N, cap, x, P, z, R, None, ids, {}))
        out.append(("ambiguous N=%d, budget %d" % (N, BUDGET), cap, x, P, z, R, None, None, {"max_nodes": BUDGET}))
    N, cap, extent, count, seed = AMBIGUOUS[0]
    x, P, z, R, ids = ambiguous_scan(pkg, N, extent, count, seed)
    out.append(("ambiguous N=%d, max_branch 1" % N, cap, x, P, z, R, None, None, {"max_branch": 1}))
    z2 = z.copy()
    z2[3] += 40.0   # (no landmark within the gate of this one)
    out.append(("ambiguous N=%d, one measurement without a candidate" % N, cap, x, P, z2, R, None, None, {}))
    for N, cap in mr.SIZES:
        x, P, z, R, ids = mr.planted_scan(pkg, N, mr.SCAN_SEED[N])
        out.append(("planted N=%d" % N, cap, x, P, z, R, None, ids, {}))
    x, P, z, R, _ = gr.edge_scan(pkg, 1)
    out.append(("N=1", 8, x, P, z, R, None, None, {}))
    x, P = pkg.scenarios.injected_state(257, seed=1400, extent=mr.map_extent(257))
    ids = [0, 31, 32, 255, 256]
    out.append(("257 in 320", 320, x, P) + mr.scan_of(pkg, x, ids, 1460) + (None, np.array(ids), {}))
    x, P = mr.planted_scan(pkg, 100, mr.SCAN_SEED[100])[:2]
    L = x[3:].reshape(-1, 2)
    ids = np.argsort(np.hypot(L[:, 0] - x[0], L[:, 1] - x[1]), kind="stable")[:32].astype(np.int32)
    out.append(("32 measurements", 200, x, P) + mr.scan_of(pkg, x, ids, 1470) + (None, ids, {}))
    for b, (x, P, z, R, valid) in enumerate(gr.wide_scans(pkg)):   # the batch of match_ref.WIDE_COUNTS, masked entries NaN
        out.append(("wide batch, filter %d" % b, 320, x, P, z, R, valid, None, {}))
    return out
