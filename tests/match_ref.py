"""NumPy statement of ekf_update_matched and ekf_joint_compat (include/ekfslam_c.h) on a dense export, and the builder of scans with
planted correspondences.

update(x, P, z, R, ids, round_size) -> (x, P, n_applied, d2): the measurements with ids[k] >= 0, in rounds of round_size in list
order (None: all at once); a round with measurements k of landmarks i_k, all linearised at the round's entry state:
    C = Rot(phi),  dp_k = L_ik - p,  H_R,k = [-C^T | -C^T J dp_k],  H_L = C^T,  d_k = C^T dp_k - z_k,
    column pair k of W = P[:, 0:3] H_R,k^T + P[:, L_ik] C,  S = H W + blockdiag(R_k) = U^T U,  V = W U^-1,  y = U^-T d,
    x <- x - V y,  P <- P - V V^T,  d2[k] = sum of y^2 over the round's columns 0 .. 2 k_round + 1.
A round whose S has a pivot that is not above PIVOT_TOL of its own diagonal entry stops the call, that round and the later ones not
applied (their d2 NaN, as for skipped entries).  Written like fuse_ref.update: element-wise triangular solve, einsum for V V^T, the
right-looking Cholesky by hand (its row k is final after step k, which is what makes the prefix sums of y^2 the distances of the
prefix hypotheses).  dtype=np.longdouble is the extended-precision restatement.
`trig` says where cos phi and sin phi come from: the device takes them from its own cos() / sin(), which may differ from libm's by an
ulp; trig=None is libm (math.cos, math.sin; np.cos / np.sin in extended precision), tests/test_update_matched_cpu.py shows that an
ulp either way stays far inside the bounds.
joint_compat(x, P, z, R, ids) -> d2 is one round over everything, nothing applied, NaN from the refused pivot on."""
import math

import numpy as np

PIVOT_TOL = 2.0 ** -44
_J = np.array([[0.0, -1.0], [1.0, 0.0]])


def libm_trig(phi):
    return math.cos(phi), math.sin(phi)


def extended_trig(phi):
    return np.cos(np.longdouble(phi)), np.sin(np.longdouble(phi))


def ulp_trig(dc, ds):
    """libm's values moved by dc / ds units in the last place."""
    def f(phi):
        c, s = libm_trig(float(phi))
        for _ in range(abs(dc)):
            c = np.nextafter(c, np.inf if dc > 0 else -np.inf)
        for _ in range(abs(ds)):
            s = np.nextafter(s, np.inf if ds > 0 else -np.inf)
        return float(c), float(s)
    return f


def cholesky_upper(S, rhs):
    """Right-looking U^T U = S from the upper triangle, the columns of rhs carried along (they end as U^-T rhs).  Returns
    (U, U^-T rhs, bad): bad = None, or the index of the first refused pivot -- the rows in front of it are final."""
    M = S.shape[0]
    A = np.concatenate([np.array(S), np.array(rhs).reshape(M, -1)], axis=1)
    floor = PIVOT_TOL * np.diag(S)
    bad = None
    for k in range(M):
        if not A[k, k] > floor[k]:
            bad = k
            break
        A[k, k:] = A[k, k:] / np.sqrt(A[k, k])
        for a in range(k + 1, M):
            A[a, a:] = A[a, a:] - A[k, a] * A[k, a:]
    return np.triu(A[:, :M]), A[:, M:], bad


def linearise(x, P, z, R, ids, dtype=np.float64, trig=None):
    """(W, S, d) of one round."""
    trig = trig or (libm_trig if dtype == np.float64 else extended_trig)
    c, s = trig(x[2])
    C = np.array([[c, -s], [s, c]], dtype=dtype)
    J = _J.astype(dtype)
    m, n = len(ids), len(x)
    W = np.empty((n, 2 * m), dtype=dtype)
    H = np.zeros((2 * m, n), dtype=dtype)
    d = np.empty(2 * m, dtype=dtype)
    for k, i in enumerate(ids):
        Li = 3 + 2 * int(i)
        dp = x[Li:Li + 2] - x[0:2]
        H_R = np.empty((2, 3), dtype=dtype)
        H_R[:, 0:2] = -C.T
        H_R[:, 2] = -C.T @ J @ dp
        H[2 * k:2 * k + 2, 0:3] += H_R
        H[2 * k:2 * k + 2, Li:Li + 2] += C.T
        W[:, 2 * k:2 * k + 2] = P[:, 0:3] @ H_R.T + P[:, Li:Li + 2] @ C
        d[2 * k:2 * k + 2] = C.T @ dp - np.asarray(z[k], dtype=dtype)
    S = H @ W
    for k in range(m):
        S[2 * k:2 * k + 2, 2 * k:2 * k + 2] += np.asarray(R[k], dtype=dtype)
    return W, S, d


def prefix_d2(y, bad):
    m = len(y) // 2
    d2 = np.cumsum(np.asarray(y) ** 2)[1::2].astype(np.float64)
    if bad is not None:
        d2[[k for k in range(m) if 2 * k + 1 >= bad]] = np.nan
    return d2


def round_update(x, P, z, R, ids, dtype=np.float64, trig=None):
    """One joint update: (x1, P1, d2), or (None, None, d2) when S is refused."""
    W, S, d = linearise(x, P, z, R, ids, dtype, trig)
    U, y, bad = cholesky_upper(S, d)
    y = y[:, 0]
    d2 = prefix_d2(y, bad)
    if bad is not None:
        return None, None, d2
    M = len(d)
    V = np.empty_like(W)
    for c in range(M):
        acc = W[:, c].copy()
        for k in range(c):
            acc -= V[:, k] * U[k, c]
        V[:, c] = acc / U[c, c]
    x1 = x - np.einsum("ik,k->i", V, y)
    P1 = P - np.einsum("ik,jk->ij", V, V)
    return x1, P1, d2


def update(x, P, z, R, ids, round_size=None, dtype=np.float64, trig=None):
    x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    kept = np.flatnonzero(ids >= 0)
    rs = int(round_size) if round_size else max(len(kept), 1)
    d2 = np.full(len(ids), np.nan)
    applied = 0
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        x1, P1, dr = round_update(x, P, z[sel], R[sel], ids[sel], dtype, trig)
        if x1 is None:
            break
        x, P = x1, P1
        d2[sel] = dr
        applied += len(sel)
    return x, P, applied, d2


def update_extended(x, P, z, R, ids, round_size=None):
    return update(x, P, z, R, ids, round_size, dtype=np.longdouble)


def joint_compat(x, P, z, R, ids, dtype=np.float64, trig=None):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    kept = np.flatnonzero(ids >= 0)
    d2 = np.full(len(ids), np.nan)
    if len(kept):
        x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
        _, S, d = linearise(x, P, z[kept], R[kept], ids[kept], dtype, trig)
        _, y, bad = cholesky_upper(S, d)
        d2[kept] = prefix_d2(y[:, 0], bad)
    return d2


def measurement_of(pkg, x, i, noise=None):
    """(z, R) of landmark i seen from the pose of x: z = C^T (L - p) + 0.5 chol(R) noise, R of slam.cpp for that feature."""
    c, s = libm_trig(float(x[2]))
    C = np.array([[c, -s], [s, c]])
    zt = C.T @ (x[3 + 2 * i:5 + 2 * i] - x[0:2])
    _, R = pkg.scenarios.measurement_from_feature_mm(1000.0 * zt[0], 1000.0 * zt[1])
    if noise is not None:
        zt = zt + 0.5 * np.linalg.cholesky(R) @ noise
    return zt, R


def planted_scan(pkg, N, seed, extent=7.0, count=24):
    """(x, P, z [count][2], R [count][2][2], ids [count]): scenarios.injected_state(N, seed, extent) and one noisy measurement of each
    of the `count` landmarks nearest the robot, in a seeded random order."""
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=extent)
    rng = np.random.default_rng(seed + 2000)
    L = x[3:].reshape(-1, 2)
    near = np.argsort(np.hypot(L[:, 0] - x[0], L[:, 1] - x[1]), kind="stable")[:count]
    ids = rng.permutation(near).astype(np.int32)
    z, R = np.empty((count, 2)), np.empty((count, 2, 2))
    for k, i in enumerate(ids):
        z[k], R[k] = measurement_of(pkg, x, int(i), rng.normal(size=2))
    return x, P, z, R, ids


def as_oracle_chunk(z, R):
    """The (2, n_z) and (2, 2 n_z) arrays oracle/ekf_numpy.update takes."""
    z, R = np.asarray(z).reshape(-1, 2), np.asarray(R).reshape(-1, 2, 2)
    return z.T.copy(), np.concatenate(list(R), axis=1) if len(R) else np.zeros((2, 0))


# ---- the inputs of tests/test_update_matched.py (checked on the CPU in tests/test_update_matched_cpu.py) ----------------------------
SIZES = [(200, 320), (100, 200)]          # (N, capacity): k_chain and k_solo, as tests/test_fuse_landmarks.py
SCAN_SEED = {100: 7, 200: 9}
EDGE_IDS = [31, 32, 63, 64, 0, 99]        # either side of the tile edges, the first and the last landmark of N = 100
BATCH_COUNTS = (100, 45, 64, 33)
BATCH_IDS = [[0, 99, -1, 31, 32, -1, 63, 64, 5], [-1] * 9, [1, 63, -1, -1, 1, -1, -1, -1, -1], [32, -1, 0, 7, -1, 7, 31, -1, 16]]
# Relative agreement asked of d2 on the device: 20 times what test_update_matched_cpu.py measures between the double reference
# and its extended-precision restatement over every input below (2.48e-13 at worst, batch filter 3, whose smallest d2 is 1.5e-3;
# 3.6e-13 with cos phi and sin phi an ulp off).
D2_REL = 5e-12


def scan_of(pkg, x, ids, seed):
    """(z, R) for the list ids on the state x: a noisy measurement per entry (measurement_of), NaN where ids[k] == -1."""
    rng = np.random.default_rng(seed)
    z, R = np.full((len(ids), 2), np.nan), np.full((len(ids), 2, 2), np.nan)
    for k, i in enumerate(ids):
        noise = rng.normal(size=2)
        if i >= 0:
            z[k], R[k] = measurement_of(pkg, x, int(i), noise)
    return z, R


def edge_lists():
    """(name, ids) of the tile-edge and repeat cases on N = 100."""
    return [("tile edges", EDGE_IDS),
            ("one landmark three times", [40, 7, 40, 64, 40]),
            ("skips interleaved", [-1, 31, -1, -1, 32, 99, -1, 0, -1])]


def wrong_pairing(ids):
    """The planted hypothesis with its first two landmarks exchanged."""
    w = np.array(ids).copy()
    w[0], w[1] = ids[1], ids[0]
    return w


def hypothesis_of_32(pkg, x, z, R, ids):
    """The 24 planted measurements and 8 more of the first 8 landmarks: 32 pairings, landmarks repeated."""
    z2, R2 = scan_of(pkg, x, list(ids[:8]), 4242)
    return np.concatenate([z, z2]), np.concatenate([R, R2]), np.concatenate([ids, ids[:8]])


def gpu_inputs(pkg):
    """(name, x, P, z, R, ids, round_size) of every matched update the GPU tests ask for (the states with an open window differ from
    their stand-in here by a few propagations and Old updates)."""
    out = []
    for N, _ in SIZES:
        x, P, z, R, ids = planted_scan(pkg, N, SCAN_SEED[N])
        out.append(("planted N=%d, rounds of 16" % N, x, P, z, R, ids, 16))
        out.append(("planted N=%d, rounds of 1" % N, x, P, z, R, ids, 1))
        out.append(("planted N=%d, rounds of 8" % N, x, P, z, R, ids, 8))
        out.append(("planted N=%d, rounds of 8 reversed" % N, x, P, z[::-1], R[::-1], ids[::-1], 8))
        out.append(("planted N=%d, one round of 24" % N, x, P, z, R, ids, 24))
        z32, R32, ids32 = hypothesis_of_32(pkg, x, z, R, ids)
        out.append(("planted N=%d, hypothesis of 32" % N, x, P, z32, R32, ids32, 32))
    x, P = pkg.scenarios.injected_state(100, seed=13, extent=12.0 * (100 / 64.0) ** 0.5 + 8.0)
    ids = [3, 40, 31, 32, 63, 64, 5, 99]
    out.append(("open window pair", x, P) + scan_of(pkg, x, ids, 313) + (ids, 16))
    x, P = pkg.scenarios.injected_state(100, seed=51, extent=15.0)
    for k, (name, ids) in enumerate(edge_lists()):
        out.append((name, x, P) + scan_of(pkg, x, ids, 510 + k) + (ids, 16))
    for b, n in enumerate(BATCH_COUNTS):
        x, P = pkg.scenarios.injected_state(n, seed=80 + b, extent=10.0 + b)
        out.append(("batch filter %d" % b, x, P) + scan_of(pkg, x, BATCH_IDS[b], 800 + b) + (BATCH_IDS[b], 4))
    return out
