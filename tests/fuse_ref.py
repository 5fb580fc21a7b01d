"""NumPy statement of ekf_fuse_landmarks (include/ekfslam_c.h) on a dense export, and the builders of joined maps with duplicates and
of maps whose chosen landmarks are noisy copies of others (with_noisy_copies: any pair list, S well conditioned).

fuse(x, P, pairs, slack, round_size) -> (x, P, n_fused): for the pairs (i_k, j_k) of a round,
    W = P[:, i] - P[:, j] (column pairs),  d = x_i - x_j,  S = W[i] - W[j] + slack I = U^T U,  V = W U^-1,  y = U^-T d,
    x <- x - V y,  P <- P - V V^T;
rounds of round_size pairs in list order (None: all at once); a round whose S is not positive definite stops the call, that round
and the later ones not applied; then the j of the fused pairs go (map_model.reduce_state).  The triangular solve and V V^T are
written with element-wise operations and einsum, not BLAS: two equal rows of W give two equal rows of V and of P, whatever their
position, so an exact copy stays one (and its S exactly singular) across a round.
fuse_extended is the same arithmetic in np.longdouble with a hand-written Cholesky (the check of the double one)."""
import numpy as np

import join_ref as jr
import map_model as mm

DUP_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("d2", "f8")])


def as_ij(pairs):
    a = np.asarray(pairs)
    if a.dtype.names:
        return np.stack([a["i"], a["j"]], axis=1).astype(np.int64).reshape(-1, 2)
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def as_pairs(ij):
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(ij), dtype=DUP_DTYPE)
    out["i"], out["j"] = ij[:, 0], ij[:, 1]
    return out


def _cholesky_upper(S):
    """U with U^T U = S from the upper triangle, right-looking; None at the first pivot that is not positive."""
    A = np.array(S)
    M = A.shape[0]
    for k in range(M):
        if not A[k, k] > 0:
            return None
        A[k, k:] = A[k, k:] / np.sqrt(A[k, k])
        for a in range(k + 1, M):
            A[a, a:] = A[a, a:] - A[k, a] * A[k, a:]
    return np.triu(A)


def update(x, P, ij, slack=0.0, dtype=np.float64):
    """One joint update with the constraints of the pairs ij; None when S is not positive definite."""
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    ci = np.stack([3 + 2 * ij[:, 0], 4 + 2 * ij[:, 0]], axis=1).reshape(-1)
    cj = np.stack([3 + 2 * ij[:, 1], 4 + 2 * ij[:, 1]], axis=1).reshape(-1)
    W = P[:, ci] - P[:, cj]
    d = x[ci] - x[cj]
    M = len(ci)
    S = W[ci] - W[cj] + dtype(slack) * np.eye(M, dtype=dtype)
    if dtype == np.float64:
        try:
            U = np.linalg.cholesky(S).T
        except np.linalg.LinAlgError:
            return None
    else:
        U = _cholesky_upper(S)
        if U is None:
            return None
    V = np.empty_like(W)
    y = np.empty(M, dtype=dtype)
    for c in range(M):
        acc, accy = W[:, c].copy(), d[c]
        for k in range(c):
            acc -= V[:, k] * U[k, c]
            accy = accy - y[k] * U[k, c]
        V[:, c] = acc / U[c, c]
        y[c] = accy / U[c, c]
    x1 = x - np.einsum("ik,k->i", V, y)
    P1 = P - np.einsum("ik,jk->ij", V, V)
    return x1, P1


def fuse(x, P, pairs, slack=0.0, round_size=None, dtype=np.float64, reduce=True):
    x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
    ij = as_ij(pairs)
    rs = int(round_size) if round_size else max(len(ij), 1)
    fused = 0
    for r0 in range(0, len(ij), rs):
        out = update(x, P, ij[r0:r0 + rs], slack, dtype)
        if out is None:
            break
        x, P = out
        fused += len(ij[r0:r0 + rs])
    if reduce:
        keep = np.ones((len(x) - 3) // 2, dtype=bool)
        keep[ij[:fused, 1]] = False
        x, P = mm.reduce_state(x, P, keep)
    return x, P, fused


def fuse_extended(x, P, pairs, slack=0.0, round_size=None, reduce=True):
    return fuse(x, P, pairs, slack, round_size, dtype=np.longdouble, reduce=reduce)


def check_pairs(pairs, N):
    """What the library requires of a list: 0 <= i < j < N, every landmark at most once."""
    ij = as_ij(pairs)
    assert np.all((0 <= ij[:, 0]) & (ij[:, 0] < ij[:, 1]) & (ij[:, 1] < N)), ij
    assert len(np.unique(ij)) == ij.size, "a landmark appears twice"
    return ij


ROBOT_SCALE = 0.3  # the injected robot block (sigma 0.1 m / 0.12 rad) scaled to 0.03 m / 0.04 rad: a few cm at a few metres


def source_map(pkg, xg, N, Ns, n_dup, seed, extent):
    """The local map a second pass would build: its frame origin is the destination's pose, its own pose a short move on; its first
    n_dup landmarks are noisy re-observations of destination landmarks (the ones nearest the robot: lever arms of a few metres), the
    others fresh; its covariance is independent of the destination's.  Returns (xs, Ps, seen) with seen[k] the destination landmark
    source landmark k re-observes."""
    rng = np.random.default_rng(seed + 1000)
    xs, Ps = pkg.scenarios.injected_state(Ns, seed=seed + 1, extent=extent)
    Ps = Ps * 0.05  # a fresh local map: sigma 2-3 cm
    xs[0:3] = (0.6, -0.2, 0.1)
    L = xg[3:].reshape(-1, 2)
    C = jr._rot(float(xg[2]))
    order = np.argsort(np.hypot(L[:, 0] - xg[0], L[:, 1] - xg[1]), kind="stable")
    seen = rng.permutation(order[:n_dup])
    for k, m in enumerate(seen):
        xs[3 + 2 * k:5 + 2 * k] = C.T @ (L[m] - xg[0:2]) + rng.normal(0.0, 0.02, size=2)
    return xs, Ps, seen


def joined_with_duplicates(pkg, N, Ns, n_dup, seed, extent=7.0):
    """(xg, Pg, xs, Ps, x, P, truth): destination (scenarios.injected_state(N), the robot block scaled by ROBOT_SCALE), source map,
    their join (join_ref.join) and the true pairs [(m, N + k)] sorted by (i, j)."""
    xg, Pg = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
    D = np.ones(len(xg))
    D[:3] = ROBOT_SCALE
    Pg = Pg * D[:, None] * D[None, :]
    Pg = 0.5 * (Pg + Pg.T)
    xs, Ps, seen = source_map(pkg, xg, N, Ns, n_dup, seed, extent)
    x, P = jr.join(xg, Pg, xs, Ps)
    truth = as_pairs(sorted((int(m), N + k) for k, m in enumerate(seen)))
    return xg, Pg, xs, Ps, x, P, truth


def with_exact_copy(x, P, i):
    """The state with one more landmark, an exact copy of landmark i (rows of P equal): S of the pair is exactly zero."""
    n = len(x)
    src = np.concatenate([np.arange(n), [3 + 2 * i, 4 + 2 * i]]).astype(int)
    return x[src].copy(), P[np.ix_(src, src)].copy()


def with_noisy_copies(x, P, pairs, seed, target=2.0):
    """The state with landmark j of every pair (i, j) made a noisy copy of landmark i, as dup_ref.with_duplicates plants one: every
    cross covariance of j copied from i, P_jj = P_ii + R and L_j = L_i + e with R a random SPD matrix of size 1e-3 and
    e^T R^-1 e = target.  S of the pair list is then exactly blockdiag(R): well conditioned whatever the list."""
    rng = np.random.default_rng(seed)
    ij = as_ij(pairs)
    src = np.arange(len(x))
    for i, j in ij:
        src[3 + 2 * j:5 + 2 * j] = (3 + 2 * i, 4 + 2 * i)
    x1, P1 = np.array(x, dtype=np.float64)[src], np.array(P, dtype=np.float64)[np.ix_(src, src)]
    for i, j in ij:
        A = rng.normal(size=(2, 2))
        R = 1e-3 * (A @ A.T + 0.5 * np.eye(2))
        R = 0.5 * (R + R.T)
        th = rng.uniform(0.0, 2.0 * np.pi)
        x1[3 + 2 * j:5 + 2 * j] += np.linalg.cholesky(R) @ np.array([np.cos(th), np.sin(th)]) * np.sqrt(target)
        P1[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] += R
    assert np.array_equal(P1, P1.T)
    return x1, P1
