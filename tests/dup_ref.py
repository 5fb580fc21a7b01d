"""NumPy statement of ekf_find_duplicates (include/ekfslam_c.h) on a dense export, and the builder of states with planted duplicates.

find(x, P, gate, max_dist, split) -> (pairs, n_degenerate): for landmarks i < j (with a split: i < split <= j), d = L_i - L_j,
    a = P_ii.xx + P_jj.xx - 2 P_ij[0][0],  b = P_ii.xy + P_jj.xy - P_ij[0][1] - P_ij[1][0],  c = P_ii.yy + P_jj.yy - 2 P_ij[1][1],
    degenerate: !(a > 0 and a c - b^2 > 0);  else d2 = (c dx^2 - 2 b dx dy + a dy^2) / (a c - b^2);
considered with max_dist > 0 only when dx^2 + dy^2 <= max_dist^2; listed, in (i, j) order, when not degenerate and d2 <= gate.
find(..., dtype=np.longdouble) is the same statement in extended precision (the check of the double one)."""
import numpy as np

DUP_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("d2", "f8")])
GATE = 9.21
TARGETS = (0.0, 1e-6, 0.5, 3.0, 9.0, 9.4, 12.0, 30.0)


def terms(x, P, dtype=np.float64):
    """Every pair's (dx, dy, a, b, c, det) as (N, N) arrays, row i, column j."""
    x, P = np.asarray(x, dtype=dtype), np.asarray(P, dtype=dtype)
    L = x[3:].reshape(-1, 2)
    PL = P[3:, 3:]
    xx, xy, yy = np.diag(PL)[0::2], np.diag(PL, 1)[0::2], np.diag(PL)[1::2]
    dx, dy = L[:, None, 0] - L[None, :, 0], L[:, None, 1] - L[None, :, 1]
    a = (xx[:, None] + xx[None, :]) - 2.0 * PL[0::2, 0::2]
    b = ((xy[:, None] + xy[None, :]) - PL[0::2, 1::2]) - PL[1::2, 0::2]
    c = (yy[:, None] + yy[None, :]) - 2.0 * PL[1::2, 1::2]
    return dx, dy, a, b, c, a * c - b * b


def find(x, P, gate=GATE, max_dist=None, split=0, dtype=np.float64, with_terms=False):
    N = (len(x) - 3) // 2
    if N < 2:
        none = np.zeros(0, dtype=bool)
        terms_of_nothing = dict(i=np.zeros(0, dtype=int), j=np.zeros(0, dtype=int), d2=np.zeros(0), r2=np.zeros(0), considered=none, ok=none)
        return (np.zeros(0, dtype=DUP_DTYPE), 0) + ((terms_of_nothing,) if with_terms else ())
    dx, dy, a, b, c, det = terms(x, P, dtype)
    i, j = np.triu_indices(N, 1)
    if split > 0:
        m = (i < split) & (j >= split)
        i, j = i[m], j[m]
    dx, dy, a, b, c, det = (v[i, j] for v in (dx, dy, a, b, c, det))
    r2 = dx * dx + dy * dy
    considered = np.ones(i.size, dtype=bool)
    if max_dist is not None and max_dist > 0:
        considered = r2 <= dtype(max_dist) * dtype(max_dist)
    ok = (a > 0) & (det > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = ((c * dx * dx - 2.0 * b * dx * dy) + a * dy * dy) / det
    listed = considered & ok & (d2 <= gate)
    out = np.zeros(int(listed.sum()), dtype=DUP_DTYPE)
    out["i"], out["j"], out["d2"] = i[listed], j[listed], d2[listed].astype(np.float64)  # (triu_indices: already in (i, j) order)
    if with_terms:
        return out, int((considered & ~ok).sum()), dict(i=i, j=j, d2=d2, r2=r2, considered=considered, ok=ok)
    return out, int((considered & ~ok).sum())


def margins(x, P, gate=GATE, max_dist=None, split=0):
    """How close a non-degenerate pair's d2 comes to the gate, and how close the distance of a pair that the unbounded search lists
    or counts as degenerate comes to max_dist (a pair that fails the gate anyway may lie anywhere), both relative: the
    precondition of a comparison of LISTS (a pair on the edge may fall either way in another evaluation order)."""
    _, _, t = find(x, P, gate, None, split, with_terms=True)
    m_gate = np.abs(t["d2"][t["ok"]] / gate - 1.0).min() if t["ok"].any() and gate > 0 else np.inf
    m_dist = np.inf
    counts = ~t["ok"] | (t["d2"] <= gate)
    if max_dist is not None and max_dist > 0 and counts.any():
        m_dist = np.abs(np.sqrt(t["r2"][counts]) / max_dist - 1.0).min()
    return float(m_gate), float(m_dist)


def with_duplicates(x, P, targets=TARGETS, seed=0, exact=0, permute=True):
    """Append, for len(targets) chosen landmarks k, a landmark L_k + e with covariance P_kk + R_k and every cross covariance copied
    from landmark k (so P_new,k = P_kk and S of the pair (k, new) is exactly R_k): R_k a random SPD matrix of size 1e-3,
    e = chol(R_k) u sqrt(target) with |u| = 1, hence d^T S^-1 d = target.  `exact`: that many further landmarks copied with R = 0, e = 0
    (S = 0: a degenerate pair).  Then the landmarks are renumbered by a fixed-seed permutation.  Returns (x, P, planted) with planted =
    [(i, j, target or None)] in the new numbering, i < j."""
    rng = np.random.default_rng(seed)
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    N = (len(x) - 3) // 2
    K = len(targets) + int(exact)
    chosen = list(rng.choice(N, size=K, replace=False))
    n0 = 3 + 2 * N
    src = np.concatenate([np.arange(n0)] + [[3 + 2 * int(k), 4 + 2 * int(k)] for k in chosen]).astype(int)
    x1 = x[src].copy()
    P1 = P[np.ix_(src, src)].copy()
    for t, k in enumerate(chosen):
        if t >= len(targets):
            continue
        A = rng.normal(size=(2, 2))
        R = 1e-3 * (A @ A.T + 0.5 * np.eye(2))
        R = 0.5 * (R + R.T)
        th = rng.uniform(0.0, 2.0 * np.pi)
        e = np.linalg.cholesky(R) @ np.array([np.cos(th), np.sin(th)]) * np.sqrt(targets[t])
        at = n0 + 2 * t
        x1[at:at + 2] += e
        P1[at:at + 2, at:at + 2] += R
    assert np.array_equal(P1, P1.T)
    perm = rng.permutation(N + K) if permute else np.arange(N + K)  # new landmark q is old landmark perm[q]
    rows = np.concatenate([np.arange(3), np.stack([3 + 2 * perm, 4 + 2 * perm], axis=1).reshape(-1)])
    x2, P2 = x1[rows].copy(), P1[np.ix_(rows, rows)].copy()
    where = np.empty(N + K, dtype=int)
    where[perm] = np.arange(N + K)
    planted = []
    for t, k in enumerate(chosen):
        a, b = int(where[int(k)]), int(where[N + t])
        planted.append((min(a, b), max(a, b), targets[t] if t < len(targets) else None))
    return x2, P2, planted


def without_cross_blocks(P):
    """P with every landmark-to-landmark cross block zeroed: what a gate that ignores P_ij sees."""
    Q = np.array(P, dtype=np.float64)
    N = (Q.shape[0] - 3) // 2
    keep = np.kron(np.eye(N), np.ones((2, 2))).astype(bool)
    Q[3:, 3:] = np.where(keep, Q[3:, 3:], 0.0)
    return Q
