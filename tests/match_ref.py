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


def assert_d2_close(got, want, what, bound=None):
    """NaN where the reference has NaN, relative agreement within `bound` (D2_REL) elsewhere; returns the worst relative difference."""
    bound = D2_REL if bound is None else bound
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    rel = float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max())
    print("%s: d2 relative %.3e" % (what, rel))
    assert rel <= bound, (what, rel)
    return rel


# ---- the matched updates of tests/test_map_edges.py: the grid, tile, chunk and capacity edges ------------------------------------------
def map_extent(N):
    """helpers.make_filter's."""
    return 12.0 * (N / 64.0) ** 0.5 + 8.0


def chunk_ids(N):
    """Eleven entries on a map of 511 / 512 / 513 landmarks (columns of 1025 / 1027 / 1029 elements): the first and the last landmark,
    either side of a tile edge and of k_match_gather's second block, the last again; a round of 8 and one of 3."""
    return [0, N - 1, 479, 480, 256, N - 1, 255, 31, 32, 1, N - 2]


def chunk_hypothesis(N):
    """32 pairings for ekf_joint_compat on the same maps, the last landmark among them."""
    return [N - 1, 0, 479, 480, 256, 255] + list(range(100, 126))


def nearest_with_repeats(x, count, distinct, seed):
    """`count` ids: the `distinct` landmarks nearest the robot in a seeded order, then count - distinct of them again."""
    rng = np.random.default_rng(seed)
    L = x[3:].reshape(-1, 2)
    near = np.argsort(np.hypot(L[:, 0] - x[0], L[:, 1] - x[1]), kind="stable")[:distinct]
    return np.concatenate([rng.permutation(near), rng.choice(near, size=count - distinct)]).astype(np.int32)


# name -> (N, capacity, window, ids or the number of measurements of the 24 nearest landmarks, seed of the state; the scan's is
# seed + SCAN_OFFSET).  The shapes are the smallest at which each piece of code first runs: k_match_gather's grid is
# cdiv(N, 256) blocks of 256 landmarks, a dense vector is walked in chunks of 1024 elements, a round holds `window` measurements.
SCAN_OFFSET = 50
MAP_EDGES = {
    "257: gather's second block holds one landmark": (257, 320, 8, [0, 255, 256, 31, 32, 256, 128], 1400),
    "256: gather ends on a block": (256, 320, 8, [255, 0, 224, 223], 1401),
    "511: columns of 1025": (511, 520, 8, chunk_ids(511), 1402),
    "512: columns of 1027": (512, 520, 8, chunk_ids(512), 1403),
    "513: columns of 1029": (513, 520, 8, chunk_ids(513), 1404),
    "300 in 320: 33 measurements, window 32": (300, 320, 32, 33, 1405),
    "100 in 200: 33 measurements, window 32": (100, 200, 32, 33, 1406),
    "100 in 200: 25 measurements, window 24": (100, 200, 24, 25, 1407),
    "1 in 8: the only landmark three times": (1, 8, 8, [0, 0, 0], 1408),
    "32 in 32: the map fills its capacity": (32, 32, 8, [0, 31], 1509),   # (seed 1409's first d2 is 3.9e-5)
    "64 in 64: the map fills its capacity": (64, 64, 8, [0, 31, 32, 63], 1410),
    "33: alone in the last tile": (33, 64, 8, [32, 0, 32], 1411),
}
CHUNK_CASES = [k for k in MAP_EDGES if MAP_EDGES[k][0] >= 511]
FULL_ROUND_CASES = [k for k in MAP_EDGES if MAP_EDGES[k][2] > 8]
GROWN_IDS = [32, 5]   # behind the window in which landmark 32 was created (tests/test_map_edges.py: grown), and an old one
GROWN_SCAN_SEED = 1350
GROWN_NAME = "behind 32 -> 33"
# Relative agreement asked of d2 in tests/test_map_edges.py: 20 times what test_update_matched_cpu.py measures between the double
# reference and its extended-precision restatement over map_edge_inputs (1.39e-12 at worst: behind 32 -> 33, where landmark 32 is
# the far New landmark, 70 m from the robot, and no d2 is small -- 0.051 and 0.071; 2.87e-13 on the maps of 511 landmarks, whose
# extent is 42 m; 1.78e-12 and 1.29e-12 with cos phi and sin phi an ulp off).  Choosing scans without a tiny d2 does not help
# there: it is the distance of the measured landmark that sets the error of the residual.  D2_REL stays what it was for the inputs
# it was measured on, and holds for the batch inputs of divergent_batch_inputs too (1.82e-13 at worst).
D2_REL_EDGES = 2.8e-11


def map_edge_ids(case, x):
    ids, seed = MAP_EDGES[case][3:5]
    return nearest_with_repeats(x, ids, 24, seed + 1) if isinstance(ids, int) else ids


# ---- the batch calls of tests/test_update_matched.py where the filters diverge -------------------------------------------------------
# one refused filter among four: BATCH_COUNTS in capacity 128, window 4; filter 2 (anchored at its robot) has the same exact
# measurement of landmark 17 twice at the head of its second round, its siblings carry three rounds
REFUSED_IDS = [[0, 99, 31, 32, 63, 64, 5, 99, 7, 31, 50, 0],
               [1, -1, 44, 31, 32, -1, 0, 7, 44, -1, 12, 1],
               [3, 40, 31, 32, 17, 17, 5, 1, 2, -1, -1, -1],
               [32, 0, -1, 31, 7, 16, 32, -1, 1, 2, 30, 16]]
FOLLOW_IDS = [[5, -1, 64, 31, 98], [44, 0, -1, -1, 31], [17, 32, 31, -1, 63], [-1, 32, 0, 31, -1]]
# lists of 70 entries (more than the 64 the measurement table starts with), then 9: three filters in capacity 128, window 16
LONG_COUNTS = (100, 45, 64)
LONG_NINE = [[0, 99, -1, 31, 32, -1, 63, 64, 5], [1, 44, -1, 31, 32, -1, 0, -1, 7], [1, 63, -1, -1, 1, -1, -1, -1, -1]]
NINE_SCAN_SEED = 980  # (no first distance below 0.19; the scans of seeds 880 + b start with 0.014 and 0.022)
# 0 landmarks beside 257: capacity 320, window 8; filter 1's list is all -1, filter 0 measures landmark 256
WIDE_COUNTS = (257, 0, 33, 64)
WIDE_IDS = [[256, 0, -1, 255, 31, 32, 256, -1, 128], [-1] * 9, [32, 0, -1, 31, -1, 32, -1, -1, 5], [63, -1, 0, 32, 31, -1, 63, 7, -1]]


def long_lists():
    """[3][70] ids: 70, 41 and 65 measurements (the others -1, interleaved), landmarks repeated."""
    rng = np.random.default_rng(70)
    out = np.empty((3, 70), dtype=np.int32)
    for b, (n, kept) in enumerate(zip(LONG_COUNTS, (70, 41, 65))):
        out[b] = rng.integers(0, n, size=70)
        out[b, rng.permutation(70)[:70 - kept]] = -1
    out[0, :4], out[2, -2:] = (0, 99, 31, 32), (63, 0)
    return out


def batch_states(pkg, counts, seed):
    """The states of tests/test_update_matched.py's batch handles: injected_state(n, seed + b, extent 10 + b); a fresh filter for n = 0."""
    return [pkg.scenarios.injected_state(n, seed=seed + b, extent=10.0 + b) if n else (np.zeros(3), np.zeros((3, 3))) for b, n in enumerate(counts)]


def refused_scan(pkg, states):
    """(z [4][12][2], R [4][12][2][2]) for REFUSED_IDS on the four states (filter 2's anchored): entries 4 and 5 of filter 2 are the
    same measurement with R = 0, so S of its second round is exactly singular."""
    zs, Rs = zip(*[scan_of(pkg, states[b][0], REFUSED_IDS[b], 820 + b) for b in range(4)])
    z, R = np.stack(zs), np.stack(Rs)
    R[2, 4:6] = 0.0
    z[2, 5] = z[2, 4]
    return z, R


def gpu_inputs(pkg):
    """(name, x, P, z, R, ids, round_size) of every matched update the GPU tests ask for (the states with an open window differ from
    their stand-in here by a few propagations and Old updates; a state behind an earlier call of the same test is the reference's)."""
    by_bound = ((D2_REL, _update_inputs(pkg)), (D2_REL_EDGES, map_edge_inputs(pkg)), (D2_REL, divergent_batch_inputs(pkg)))
    out = [t for _, group in by_bound for t in group]
    assert len(set(t[0] for t in out)) == len(out), "two inputs of one name"
    _BOUNDS.clear()
    _BOUNDS.update({t[0]: bound for bound, group in by_bound for t in group})
    return out


_BOUNDS = {}  # name -> bound, by the list an input came from (filled by gpu_inputs)


def d2_bound(name):
    """The relative agreement asked of d2 for the input `name` of gpu_inputs: D2_REL_EDGES for what map_edge_inputs gives, D2_REL
    for everything else."""
    return _BOUNDS[name]


def map_edge_inputs(pkg):
    """tests/test_map_edges.py: the updates, the full-round cases' 8 / 16 / 24 / 32 prefixes as one round each, the hypotheses of 32."""
    from helpers import far_feature
    from oracle import oracle_c
    oracle_c.build()
    out = []
    for case, (N, _, window, _, seed) in MAP_EDGES.items():
        x, P = pkg.scenarios.injected_state(N, seed=seed, extent=map_extent(N))
        ids = map_edge_ids(case, x)
        z, R = scan_of(pkg, x, ids, seed + SCAN_OFFSET)
        out.append((case, x, P, z, R, ids, window))
        if case in FULL_ROUND_CASES:
            out += [("%s, prefix of %d" % (case, p), x, P, z[:p], R[:p], ids[:p], p) for p in (8, 16, 24, 32) if p <= window]
        if case in CHUNK_CASES:
            ids = chunk_hypothesis(N)
            out.append((case + ", hypothesis of 32", x, P) + scan_of(pkg, x, ids, seed + SCAN_OFFSET + 1) + (ids, 32))
    x, P = pkg.scenarios.injected_state(32, seed=1300, extent=12.0 * 0.5 ** 0.5 + 8.0)
    zf, Rf = far_feature(pkg, 0)
    x, P, dec, _, _ = oracle_c.update(x, P, zf.reshape(2, 1), Rf)
    assert dec == [oracle_c.NEW] and x.size == 3 + 2 * 33
    out.append((GROWN_NAME, x, P) + scan_of(pkg, x, GROWN_IDS, GROWN_SCAN_SEED) + (GROWN_IDS, 8))
    return out


def divergent_batch_inputs(pkg):
    """tests/test_update_matched.py: the refused filter's siblings, its own first round and the call behind; the lists of 70 and of 9;
    0 landmarks beside 257."""
    import reframe_ref as rr  # (beside this file)
    out = []
    states = batch_states(pkg, BATCH_COUNTS, 80)
    states[2] = rr.anchor(*states[2])
    z, R = refused_scan(pkg, states)
    after = []
    for b in range(4):
        ids = REFUSED_IDS[b][:4] if b == 2 else REFUSED_IDS[b]
        n = len(ids)
        out.append(("refused among four, filter %d" % b, *states[b], z[b, :n], R[b, :n], ids, 4))
        after.append(update(*states[b], z[b, :n], R[b, :n], ids, 4)[:2])
    for b in range(4):
        out.append(("behind the refusal, filter %d" % b, *after[b]) + scan_of(pkg, after[b][0], FOLLOW_IDS[b], 840 + b) + (FOLLOW_IDS[b], 4))
    ids70 = long_lists()
    for b, (x, P) in enumerate(batch_states(pkg, LONG_COUNTS, 80)):
        z, R = scan_of(pkg, x, ids70[b], 870 + b)
        out.append(("list of 70, filter %d" % b, x, P, z, R, ids70[b], 16))
        x, P = update(x, P, z, R, ids70[b], 16)[:2]
        out.append(("list of 9 behind it, filter %d" % b, x, P) + scan_of(pkg, x, LONG_NINE[b], NINE_SCAN_SEED + b) + (LONG_NINE[b], 16))
    for b, (x, P) in enumerate(batch_states(pkg, WIDE_COUNTS, 90)):
        if WIDE_COUNTS[b] == 0:
            continue  # (no landmark, so no measurement: nothing to restate)
        out.append(("0 beside 257, filter %d" % b, x, P) + scan_of(pkg, x, WIDE_IDS[b], 890 + b) + (WIDE_IDS[b], 8))
    return out


def _update_inputs(pkg):
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
