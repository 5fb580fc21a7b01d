"""NumPy statement of ekf_add_landmarks and ekf_update_joint (include/ekfslam_c.h) on a dense export.

add(x, P, z, R, mask): the selected measurements become landmarks N, N + 1, .. in list order, all linearised at the entry state.
With C = Rot(phi), J = [[0,-1],[1,0]], h_k = C J z_k, G_k = [I_2 | h_k]:

    L_k = p + C z_k      P[k, robot] = G_k P_RR      P[k, old m] = G_k P_R,m      P[k, l] = G_k P_RR G_l^T + [k == l] C R_k C^T

written block by block from these formulas (only the symmetric part of R_k enters); everything old is copied, so old rows are bitwise
the input's and the result is bitwise symmetric by construction.  cos / sin are math.cos / math.sin (the device takes its own, which
may differ by an ulp: the comparisons carry helpers.assert_state_close).  tests/test_add_landmarks_cpu.py holds it to the join of a
block-diagonal source (join_ref), to the oracle's sequential New, and to central differences of the map.

update_joint_ref(...) composes assoc_ref.search, match_ref.update and add() as the header orders them; loop_script(pkg) is the
20-step scenario of tests/test_gpu_update_joint.py, chosen and checked for wide margins on the CPU."""
import collections
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import gate_ref as gr  # noqa: E402
import match_ref as mr  # noqa: E402

NEW, OLD, IGNORE = gr.NEW, gr.OLD, gr.IGNORE
JM = np.array([[0.0, -1.0], [1.0, 0.0]])


def _lists(z, R, mask):
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    mask = np.ones(len(z), dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    assert mask.shape == (len(z),)
    return z[mask], R[mask], mask


def add_g(x, z, mask=None):
    """The map (x, z) -> x' itself."""
    x = np.asarray(x, dtype=np.float64)
    zs, _, _ = _lists(z, np.zeros((len(np.asarray(z).reshape(-1, 2)), 2, 2)), mask)
    c, s = math.cos(x[2]), math.sin(x[2])
    C = np.array([[c, -s], [s, c]])
    return np.concatenate([x, (x[0:2] + zs @ C.T).reshape(-1)])


def add(x, P, z, R, mask=None):
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    zs, Rs, _ = _lists(z, R, mask)
    n, m = x.size, len(zs)
    c, s = math.cos(x[2]), math.sin(x[2])
    C = np.array([[c, -s], [s, c]])
    G = np.zeros((2 * m, 3))  # the G_k stacked
    G[0::2, 0] = 1.0
    G[1::2, 1] = 1.0
    G[:, 2] = (zs @ (C @ JM).T).reshape(-1)
    out = np.empty((n + 2 * m, n + 2 * m))
    out[:n, :n] = P
    out[n:, :n] = G @ P[0:3, :]            # robot columns and every old landmark's
    out[:n, n:] = out[n:, :n].T
    NN = G @ P[0:3, 0:3] @ G.T
    for k in range(m):
        Rk = 0.5 * (Rs[k] + Rs[k].T)
        NN[2 * k:2 * k + 2, 2 * k:2 * k + 2] += C @ Rk @ C.T
    out[n:, n:] = 0.5 * (NN + NN.T)
    return add_g(x, zs), out


def as_join_source(z, R, mask=None):
    """The block-diagonal source whose join is the add: xs = (0, 0, 0, z_0, ..), Ps = blockdiag(0_3, R_0, ..)."""
    zs, Rs, _ = _lists(z, R, mask)
    m = len(zs)
    xs = np.concatenate([np.zeros(3), zs.reshape(-1)])
    Ps = np.zeros((3 + 2 * m, 3 + 2 * m))
    for k in range(m):
        Ps[3 + 2 * k:5 + 2 * k, 3 + 2 * k:5 + 2 * k] = 0.5 * (Rs[k] + Rs[k].T)
    return xs, Ps


def new_ids(N, mask, n_z):
    """ids_out of ekf_add_landmarks."""
    mask = np.ones(n_z, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    ids = np.full(n_z, -1, dtype=np.int32)
    ids[mask] = N + np.arange(int(mask.sum()))
    return ids


def grid_scan(pkg, m, first=0):
    """(z [m][2], R [m][2][2]): features first .. first + m - 1 of a grid 36 m and more ahead of the robot, 2.5 m apart -- outside
    the injected maps of helpers.make_filter (at most 30 m from the origin) and each other's gates: the filter's own gate says New
    for every one of them, also one after the other (tests/test_add_landmarks_cpu.py asserts it on the oracle)."""
    z, R = np.empty((m, 2)), np.empty((m, 2, 2))
    for q in range(m):
        k = first + q
        zz, RR = pkg.scenarios.measurement_from_feature_mm(36000.0 + 2500.0 * (k % 8), -6000.0 + 2500.0 * (k // 8))
        z[q], R[q] = zz.reshape(2), RR.reshape(2, 2)
    return z, R


Joint = collections.namedtuple("Joint", "x P ids kinds d2 search nearest")


def update_joint_ref(x, P, z, R, joint_gate, valid=None, gate=ar.GATE, max_branch=8, max_nodes=65536, window=None):
    """ekf_update_joint: search at the entry state, kinds, matched update in rounds of `window`, additions at the state it left."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    n_z, N = len(z), (x.size - 3) // 2
    valid = np.ones(n_z, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    res = ar.search(x, P, z, R, joint_gate, valid=valid, gate=gate, max_branch=max_branch, max_nodes=max_nodes)
    if N and valid.any():
        nearest = gr.find(gr.table_of(x, P, z, R, valid, gr.COND_LIMIT), gate, valid=valid)[1]
    else:  # a filter without landmarks: every valid measurement New (matched 0, mahal = the reference's INF)
        nearest = np.zeros(n_z, dtype=[("decision", "i4"), ("matched", "i4"), ("mahal", "f8")])
        nearest["decision"][valid], nearest["mahal"][valid] = NEW, 999999999999.0
    ids = np.array(res.ids, dtype=np.int32)
    kinds = np.where(~valid, 0, np.where(ids >= 0, OLD, np.where(nearest["decision"] == NEW, NEW, IGNORE))).astype(np.int32)
    x1, P1, applied, d2 = mr.update(x, P, z, R, ids, round_size=window)
    for q in np.flatnonzero(ids >= 0)[applied:]:
        ids[q], kinds[q] = -1, IGNORE
    is_new = kinds == NEW
    x2, P2 = add(x1, P1, z, R, is_new) if is_new.any() else (x1, P1)
    ids[is_new] = N + np.arange(int(is_new.sum()))
    return Joint(x2, P2, ids, kinds, d2, res, nearest)


def decision_margin(j, gate=ar.GATE):
    """The smallest relative distance of a quantity update_joint_ref compared from the threshold that decided it: the search's own
    comparisons (assoc_ref.margins) and every nearest distance against gamma_max / gamma_min and the individual gate."""
    m = ar.margins(j.search)
    for k in np.flatnonzero(j.nearest["matched"] != 0):
        d = float(j.nearest["mahal"][k])
        m = min([m] + [abs(d / g - 1.0) for g in (gr.GAMMA_MAX, gr.GAMMA_MIN, gate)])
    return m


# ---- the small scenario: pairs, two fresh far features, one measurement between two close landmarks -----------------------------
def between_scenario(pkg, N=60, extent=6.0, count=6, seed=33):
    """(x, P, z, R, expected kinds): the ambiguous scan shape of assoc_ref on an injected map of N landmarks (a true pose two sigma
    of P_RR from the estimate), then two far features (New) and one measurement half way between the two landmarks of the map that
    lie closest together among those isolated from the rest -- inside gamma_max of them, outside every joint gate (Ignore)."""
    x, P, z, R, _ = ar.ambiguous_scan(pkg, N, extent, count, seed)
    far = [pkg.scenarios.measurement_from_feature_mm(60000.0, 35000.0), pkg.scenarios.measurement_from_feature_mm(-45000.0, 52000.0)]
    L = x[3:].reshape(-1, 2)
    d = np.hypot(*(L[:, None, :] - L[None, :, :]).transpose(2, 0, 1))
    d[np.diag_indices(N)] = np.inf
    c, s = mr.libm_trig(float(x[2]))
    C = np.array([[c, -s], [s, c]])
    return x, P, z, R, far, L, d, C


def scan_with_kinds(pkg, N=60, extent=6.0, count=6, seed=33):
    """The scan of tests/test_gpu_update_joint.py: `count` ambiguous pairings, two far features, one in-between measurement; and
    the kinds the CPU reference gives it (asserted in tests/test_add_landmarks_cpu.py: all paired Old, far New, in-between Ignore).
    The in-between measurement is the midpoint of the closest pair of landmarks, neither of them in the scan, whose midpoint lies
    at an individual distance in [16, 36] from its nearest landmark -- one of the two: above the gate 9.21, so it has no candidate
    and no joint hypothesis holds it, and below gamma_max = 50, so the filter's own gate does not call it New."""
    x, P, z, R, far, L, d, C = between_scenario(pkg, N, extent, count, seed)
    zq = (L - x[0:2]) @ C
    used = {int(np.argmin(np.hypot(*(zq - zz).T))) for zz in z}
    pairs = sorted((d[i, j], i, j) for i in range(N) for j in range(i + 1, N) if i not in used and j not in used and d[i, j] <= 3.0)
    found = None
    for _, i, j in pairs:
        zb = C.T @ (0.5 * (L[i] + L[j]) - x[0:2])
        Rb = pkg.scenarios.measurement_from_feature_mm(1000.0 * zb[0], 1000.0 * zb[1])[1].reshape(2, 2)
        opt, dist = gr.table(x, P, [zb], [Rb]).best[0]
        if opt in (3 + 2 * i, 3 + 2 * j) and 16.0 <= dist <= 36.0:
            found = (i, j, zb, Rb)
            break
    assert found is not None, "no pair of landmarks with a midpoint between the gate and gamma_max: another seed"
    i, j, zb, Rb = found
    zs = np.concatenate([z, [far[0][0].reshape(2)], [zb], [far[1][0].reshape(2)]])
    Rs = np.concatenate([R, [far[0][1].reshape(2, 2)], [Rb], [far[1][1].reshape(2, 2)]])
    kinds = np.array([OLD] * len(z) + [NEW, IGNORE, NEW], dtype=np.int32)
    return x, P, zs, Rs, kinds, (i, j)


# ---- the 20-step loop -----------------------------------------------------------------------------------------------------------
LOOP_STEPS, LOOP_M, LOOP_SEED = 20, 6, 5


def loop_world(seed=LOOP_SEED, n=40):
    """n landmarks on a jittered ring-and-grid around the path, at least 1.2 m apart (far outside each other's gates)."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        p = rng.uniform(-7.0, 7.0, size=2)
        if all(np.hypot(*(p - q)) >= 1.2 for q in pts):
            pts.append(p)
    return np.array(pts)


def loop_script(pkg, seed=LOOP_SEED):
    """[(v, w, dt, z [M][2], R [M][2][2])] for LOOP_STEPS steps: the truth drives a slow arc; every step measures LOOP_M landmarks
    of the world in a fixed rotation (step s sees 6 s .. 6 s + 5 modulo 40: every landmark three times), with small seeded noise."""
    world = loop_world(seed)
    rng = np.random.default_rng(seed + 1)
    pose = np.zeros(3)
    out = []
    for s in range(LOOP_STEPS):
        v, w, dt = 0.3, 0.05, 0.5
        pose = pose + np.array([v * dt * math.cos(pose[2]), v * dt * math.sin(pose[2]), w * dt])
        c, sn = math.cos(pose[2]), math.sin(pose[2])
        Ct = np.array([[c, sn], [-sn, c]])
        z, R = np.empty((LOOP_M, 2)), np.empty((LOOP_M, 2, 2))
        for q in range(LOOP_M):
            zt = Ct @ (world[(LOOP_M * s + q) % len(world)] - pose[0:2])
            _, R[q] = pkg.scenarios.measurement_from_feature_mm(1000.0 * zt[0], 1000.0 * zt[1])
            z[q] = zt + 0.2 * np.linalg.cholesky(R[q]) @ rng.normal(size=2)
        out.append((v, w, dt, z, R))
    return world, out
