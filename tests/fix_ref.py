"""NumPy statement of ekf_update_fixes and ekf_fix_compat (include/ekfslam_c.h) on a dense export, and the builders of the lists the
tests use.

update(x, P, z, R, what, round_size) -> (x, P, n_applied, d2): the entries with what[k] != SKIP, in rounds of round_size in list order
(None: all at once); a round is one joint update, every entry two columns (n = 3 + 2N, e_r the unit vectors):
    POSITION:    rows e_0, e_1 of H;         columns P[:, 0], P[:, 1] of W;          d = (x_R - z_0, y_R - z_1)
    HEADING:     row e_2 and an inert row;   columns P[:, 2], 0;                     d = (wrap(phi - z_0), 0)
    landmark i:  rows e_3+2i, e_4+2i;        columns P[:, 3+2i], P[:, 4+2i];         d = L_i - z
    S = H W + blockdiag(R_k) = U^T U,  V = W U^-1,  y = U^-T d,  x <- x - V y,  P <- P - V V^T,
    d2[k] = sum of y^2 over the round's columns 0 .. 2 k_round + 1.
The inert row of a heading entry (a zero row and column of S, diagonal exactly 1, d = 0) is kept here too, so that the prefixes of
y^2 line up with the device's; z[k][1] and R[k] beyond R[k][0][0] of a heading entry are not read.
wrap(e) = e - 2 pi floor((e + pi) / (2 pi)) with the constants of ekf_filter_math.h (nees_sample).
A round whose S has a pivot that is not above PIVOT_TOL of its own diagonal entry stops the call, that round and the later ones not
applied (their d2 NaN, as for skipped entries).  Written like match_ref: its hand-written right-looking cholesky_upper, the
element-wise triangular solve, einsum for V V^T.  dtype=np.longdouble is the extended-precision restatement.
compat(x, P, z, R, what) -> d2 is one round over everything, nothing applied, NaN from the refused pivot on.
textbook(...) is the same update in the form K = P H^T S^-1, x + K res, P - K S K^T with np.linalg.solve and unpadded heading rows."""
import numpy as np

import match_ref as mr
from match_ref import PIVOT_TOL, cholesky_upper, prefix_d2  # noqa: F401

SKIP, POSITION, HEADING = -1, -2, -3
TWO_PI, PI = 6.283185307179586, 3.141592653589793


def wrap(e):
    return e - TWO_PI * np.floor((e + PI) / TWO_PI)


def state_rows(what):
    """The state rows (None: the inert row) of the two columns of an entry."""
    what = int(what)
    if what == POSITION:
        return (0, 1)
    if what == HEADING:
        return (2, None)
    assert what >= 0, what
    return (3 + 2 * what, 4 + 2 * what)


def assemble(x, P, z, R, what, dtype=np.float64):
    """(W, S, d) of one round; z [m][2], R [m][2][2], what [m] without skipped entries."""
    m, n = len(what), len(x)
    rows = [r for w in what for r in state_rows(w)]
    W = np.zeros((n, 2 * m), dtype=dtype)
    S = np.zeros((2 * m, 2 * m), dtype=dtype)
    d = np.zeros(2 * m, dtype=dtype)
    for a, ra in enumerate(rows):
        if ra is None:
            S[a, a] = 1.0
            continue
        W[:, a] = P[:, ra]
        for c, rc in enumerate(rows):
            if rc is not None:
                S[a, c] = P[ra, rc]
    for k, w in enumerate(what):
        if int(w) == HEADING:
            S[2 * k, 2 * k] += dtype(R[k][0][0])
            d[2 * k] = wrap(x[2] - dtype(z[k][0]))
        else:
            S[2 * k:2 * k + 2, 2 * k:2 * k + 2] += np.asarray(R[k], dtype=dtype)
            r0 = state_rows(w)[0]
            d[2 * k:2 * k + 2] = x[r0:r0 + 2] - np.asarray(z[k], dtype=dtype)
    return W, S, d


def round_update(x, P, z, R, what, dtype=np.float64):
    """One joint update: (x1, P1, d2), or (None, None, d2) when S is refused."""
    W, S, d = assemble(x, P, z, R, what, dtype)
    U, y, bad = cholesky_upper(S, d)
    y = y[:, 0]
    d2 = prefix_d2(y, bad)
    if bad is not None:
        return None, None, d2
    V = np.empty_like(W)
    for c in range(len(d)):
        acc = W[:, c].copy()
        for k in range(c):
            acc -= V[:, k] * U[k, c]
        V[:, c] = acc / U[c, c]
    return x - np.einsum("ik,k->i", V, y), P - np.einsum("ik,jk->ij", V, V), d2


def _lists(z, R, what):
    what = np.asarray(what, dtype=np.int64).reshape(-1)
    return np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2), what


def update(x, P, z, R, what, round_size=None, dtype=np.float64):
    x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
    z, R, what = _lists(z, R, what)
    kept = np.flatnonzero(what != SKIP)
    rs = int(round_size) if round_size else max(len(kept), 1)
    d2 = np.full(len(what), np.nan)
    applied = 0
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        x1, P1, dr = round_update(x, P, z[sel], R[sel], what[sel], dtype)
        if x1 is None:
            break
        x, P = x1, P1
        d2[sel] = dr
        applied += len(sel)
    return x, P, applied, d2


def update_extended(x, P, z, R, what, round_size=None):
    return update(x, P, z, R, what, round_size, dtype=np.longdouble)


def compat(x, P, z, R, what, dtype=np.float64):
    z, R, what = _lists(z, R, what)
    kept = np.flatnonzero(what != SKIP)
    d2 = np.full(len(what), np.nan)
    if len(kept):
        x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
        _, S, d = assemble(x, P, z[kept], R[kept], what[kept], dtype)
        _, y, bad = cholesky_upper(S, d)
        d2[kept] = prefix_d2(y[:, 0], bad)
    return d2


def textbook(x, P, z, R, what, round_size=None):
    """The same rounds as K = P H^T S^-1 (np.linalg.solve), x + K res, P - K S K^T: a heading entry is ONE row of H.  Returns
    (x, P, d2) with d2[k] the distance res^T S^-1 res of k's round cut after entry k."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    z, R, what = _lists(z, R, what)
    kept = np.flatnonzero(what != SKIP)
    rs = int(round_size) if round_size else max(len(kept), 1)
    d2 = np.full(len(what), np.nan)
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        rows, res, blocks, ends = [], [], [], []
        for k in sel:
            if what[k] == HEADING:
                rows.append(2), res.append(-wrap(x[2] - z[k, 0])), blocks.append(R[k, :1, :1])
            else:
                r = state_rows(what[k])
                rows += list(r)
                res += list(z[k] - x[list(r)])
                blocks.append(np.array([[R[k, 0, 0], R[k, 0, 1]], [R[k, 0, 1], R[k, 1, 1]]]))  # (the upper triangle, as the factorisation reads it)
            ends.append(len(rows))
        H = np.zeros((len(rows), len(x)))
        H[np.arange(len(rows)), rows] = 1.0
        S = H @ P @ H.T
        at = 0
        for blk in blocks:
            S[at:at + len(blk), at:at + len(blk)] += blk
            at += len(blk)
        res = np.array(res)
        for k, e in zip(sel, ends):
            d2[k] = float(res[:e] @ np.linalg.solve(S[:e, :e], res[:e]))
        K = np.linalg.solve(S, H @ P).T
        x = x + K @ res
        P = P - K @ S @ K.T
    return x, P, d2


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
R_POSITION = np.array([[4.0e-3, 1.0e-3], [1.0e-3, 2.5e-3]])
R_LANDMARK = np.array([[2.5e-3, -5.0e-4], [-5.0e-4, 1.0e-3]])
VAR_HEADING = 4.0e-4


def entries_for(x, P, what, seed, R_scale=1.0):
    """(z [n][2], R [n][2][2]) for the kinds `what` on the state (x, P): R the constants above times R_scale, every z the observed
    part of the state plus u chol(P_block + R) with |u| <= 1 in a seeded direction -- at most one sigma of P + R away, so that no
    distance is tiny and none is large.  NaN where what[k] == SKIP, and in what a heading entry does not read."""
    rng = np.random.default_rng(seed)
    n = len(what)
    z, R = np.full((n, 2), np.nan), np.full((n, 2, 2), np.nan)
    for k, w in enumerate(what):
        u = rng.normal(size=2)
        u *= rng.uniform(0.3, 1.0) / np.linalg.norm(u)
        w = int(w)
        if w == SKIP:
            continue
        if w == HEADING:
            R[k, 0, 0] = VAR_HEADING * R_scale
            z[k, 0] = x[2] + np.sqrt(P[2, 2] + R[k, 0, 0]) * np.sign(u[0]) * np.linalg.norm(u)
            continue
        r = list(state_rows(w))
        R[k] = (R_POSITION if w == POSITION else R_LANDMARK) * R_scale
        C = P[np.ix_(r, r)] + R[k]
        z[k] = x[r] + (np.linalg.cholesky(C) @ u if C.any() else 0.0)
    return z, R


def nearest(x, count):
    L = x[3:].reshape(-1, 2)
    return np.argsort(np.hypot(L[:, 0] - x[0], L[:, 1] - x[1]), kind="stable")[:count].astype(np.int64)


def mixed_list(pkg, x, P, seed):
    """(z, R, what) of 24 entries: position, heading, the 20 landmarks nearest the robot (in a seeded order), position again, heading
    with its z shifted by 2 pi."""
    rng = np.random.default_rng(seed + 3000)
    what = np.array([POSITION, HEADING] + list(rng.permutation(nearest(x, 20))) + [POSITION, HEADING], dtype=np.int32)
    z, R = entries_for(x, P, what, seed)
    z[-1, 0] += TWO_PI
    return z, R, what


# ---- the inputs of tests/test_update_fixes.py (checked on the CPU in tests/test_update_fixes_cpu.py) ----------------------------------
SIZES = mr.SIZES
STATE_SEED = {100: 17, 200: 19}
# Relative agreement asked of d2 on the device: 20 times what test_update_fixes_cpu.py measures between the double reference and its
# extended-precision restatement over every input of gpu_inputs, as an update in its rounds and as one round of ekf_fix_compat
# (7.59e-14 at worst: "mixed N=200, rounds of 1").  The margin covers the device's other summation order and FMA contraction, as for
# match_ref.D2_REL.
D2_REL = 1.52e-12
EDGE_WHAT_257 = [0, 31, POSITION, 32, 63, 64, HEADING, 255, 256]
EDGE_WHAT_256 = [255, 0, HEADING, 31, 32, POSITION, 63, 64]
WIDE_COUNTS = (257, 0, 33, 64)   # capacity 320, window 4
WIDE_WHAT = [[256, POSITION, SKIP, 255, HEADING, 31, 32, SKIP, 0, 128],
             [SKIP, HEADING, SKIP, SKIP, POSITION, SKIP, SKIP, SKIP, SKIP, SKIP],
             [32, SKIP, 0, HEADING, SKIP, 31, SKIP, SKIP, 32, SKIP],
             [POSITION, 63, SKIP, 0, 32, 31, HEADING, 63, POSITION, 7]]
# one refused filter among four: counts as match_ref.BATCH_COUNTS in capacity 128, window 4; filter 2 fixes landmark 17 twice with
# R = 0 at the head of its second round, its siblings carry three rounds
REFUSED_COUNTS = mr.BATCH_COUNTS
REFUSED_WHAT = [[0, 99, POSITION, 32, 63, HEADING, 5, 99, 7, 31, POSITION, 0],
                [1, HEADING, 44, 31, 32, SKIP, 0, 7, 44, POSITION, 12, 1],
                [3, POSITION, 31, HEADING, 17, 17, 5, 1, 2, SKIP, SKIP, SKIP],
                [32, 0, SKIP, HEADING, 7, 16, 32, SKIP, POSITION, 2, 30, 16]]
SINGULAR_WHAT = [3, HEADING, 40, 31, POSITION, POSITION, 17, 5, 32, 2]   # window 4: the position twice with R = 0 in round two of three
OPEN_WINDOW_WHAT = [POSITION, 3, 40, HEADING, 31, 32, 63, 64, 5, 99]


def batch_states(pkg, counts, seed):
    """match_ref.batch_states; the filter without landmarks is a fresh filter after one propagate(0.3, 0.05, 0.05)."""
    from oracle import oracle_c
    oracle_c.build()
    out = mr.batch_states(pkg, counts, seed)
    for b, n in enumerate(counts):
        if n == 0:
            out[b] = fresh_propagated()
    return out


def fresh_propagated():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c.propagate(np.zeros(3), np.zeros((3, 3)), 0.3, 0.05, oracle_c.make_Q(0.3), 0.05)


def wide_lists(pkg, states):
    zs, Rs = zip(*[entries_for(*states[b], WIDE_WHAT[b], 900 + b) for b in range(4)])
    return np.stack(zs), np.stack(Rs), np.array(WIDE_WHAT, dtype=np.int32)


def refused_lists(pkg, states):
    """(z [4][12][2], R [4][12][2][2], what): entries 4 and 5 of filter 2 are the same hard fix of landmark 17, so S of its second
    round is exactly singular."""
    zs, Rs = zip(*[entries_for(*states[b], REFUSED_WHAT[b], 920 + b) for b in range(4)])
    z, R = np.stack(zs), np.stack(Rs)
    R[2, 4:6] = 0.0
    z[2, 5] = z[2, 4]
    return z, R, np.array(REFUSED_WHAT, dtype=np.int32)


def singular_list(pkg, x, P):
    z, R = entries_for(x, P, SINGULAR_WHAT, 931)
    R[4:6] = 0.0
    z[5] = z[4]
    return z, R, np.array(SINGULAR_WHAT, dtype=np.int32)


def long_list(pkg, x, P, count, seed):
    """`count` entries on a map of 100: position and heading at the head and again at the end, landmarks (the nearest 24, repeated)
    between."""
    rng = np.random.default_rng(seed)
    near = nearest(x, 24)
    what = np.array([POSITION, HEADING] + list(rng.choice(near, size=count - 4)) + [HEADING, POSITION], dtype=np.int32)
    return entries_for(x, P, what, seed + 1) + (what,)


def gpu_inputs(pkg):
    """(name, x, P, z, R, what, round_size) of every update the GPU tests ask for (the states with an open window differ from their
    stand-in here by a few propagations and Old updates; a state behind an earlier call of the same test is the reference's)."""
    out = []
    for N, _ in SIZES:
        x, P = pkg.scenarios.injected_state(N, seed=STATE_SEED[N], extent=mr.map_extent(N))
        z, R, what = mixed_list(pkg, x, P, STATE_SEED[N])
        for rs in (16, 1, 5, 24):
            out.append(("mixed N=%d, rounds of %d" % (N, rs), x, P, z, R, what, rs))
        out.append(("mixed N=%d, rounds of 5 reversed" % N, x, P, z[::-1], R[::-1], what[::-1], 5))
        out.append(("mixed N=%d, list of 9 in a window of 16" % N, x, P, z[:9], R[:9], what[:9], 16))
    x, P = pkg.scenarios.injected_state(100, seed=STATE_SEED[100], extent=mr.map_extent(100))
    for count in (17, 32):
        out.append(("list of %d, window 32" % count, x, P) + long_list(pkg, x, P, count, 40 + count) + (32,))
    for N, what in ((257, EDGE_WHAT_257), (256, EDGE_WHAT_256)):
        x, P = pkg.scenarios.injected_state(N, seed=1500 + N, extent=mr.map_extent(N))
        out.append(("tile edges N=%d" % N, x, P) + entries_for(x, P, what, 1600 + N) + (what, 8))
    x, P = fresh_propagated()
    what = [POSITION, HEADING]
    out.append(("no landmarks", x, P) + entries_for(x, P, what, 61, R_scale=1e-2) + (what, 16))
    x, P = pkg.scenarios.injected_state(100, seed=13, extent=mr.map_extent(100))
    out.append(("open window pair", x, P) + entries_for(x, P, OPEN_WINDOW_WHAT, 313) + (OPEN_WINDOW_WHAT, 16))
    states = batch_states(pkg, WIDE_COUNTS, 90)
    z, R, what = wide_lists(pkg, states)
    for b in range(4):
        out.append(("wide batch, filter %d" % b, *states[b], z[b], R[b], what[b], 4))
    states = mr.batch_states(pkg, REFUSED_COUNTS, 80)
    z, R, what = refused_lists(pkg, states)
    for b in range(4):
        keep = 4 if b == 2 else 12
        out.append(("refused among four, filter %d" % b, *states[b], z[b, :keep], R[b, :keep], what[b, :keep], 4))
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    z, R, what = singular_list(pkg, x, P)
    out.append(("singular second round: round one", x, P, z[:4], R[:4], what[:4], 4))
    out += sequence_inputs(pkg)
    assert len(set(t[0] for t in out)) == len(out), "two inputs of one name"
    return out


# ---- the short mixed sequence: update_fixes -> update_matched -> add_landmarks -> remove_landmarks -> update_fixes ---------------------
SEQ_FIX_1 = [POSITION, 3, HEADING, 40, 31, 32, 99]
SEQ_MATCH = [5, 31, 64, 0]
SEQ_REMOVE = [31, 99, 100]      # (100: the landmark the addition made)
SEQ_FIX_2 = [HEADING, 97, 31, POSITION]  # (97: the last landmark behind the removal)


def sequence_start(pkg):
    return pkg.scenarios.injected_state(100, seed=23, extent=mr.map_extent(100))


def sequence_add_measurement(pkg):
    from helpers import far_feature
    return far_feature(pkg, 0)


def sequence_inputs(pkg):
    """The two update_fixes steps of the sequence on the references' states (match_ref, the oracle's New, NumPy removal between)."""
    from oracle import oracle_c
    oracle_c.build()
    x, P = sequence_start(pkg)
    z1, R1 = entries_for(x, P, SEQ_FIX_1, 71)
    out = [("sequence, step 1", x, P, z1, R1, SEQ_FIX_1, 16)]
    x, P = update(x, P, z1, R1, SEQ_FIX_1, 16)[:2]
    zm, Rm = mr.scan_of(pkg, x, SEQ_MATCH, 72)
    x, P = mr.update(x, P, zm, Rm, SEQ_MATCH, 16)[:2]
    zf, Rf = sequence_add_measurement(pkg)
    x, P, dec, _, _ = oracle_c.update(x, P, zf.reshape(2, 1), Rf)
    assert dec == [oracle_c.NEW] and x.size == 3 + 2 * 101
    x, P = remove(x, P, SEQ_REMOVE)
    z2, R2 = entries_for(x, P, SEQ_FIX_2, 73)
    out.append(("sequence, step 5", x, P, z2, R2, SEQ_FIX_2, 16))
    return out


def remove(x, P, ids):
    """The state without the landmarks `ids`."""
    N = (len(x) - 3) // 2
    keep = [l for l in range(N) if l not in set(int(i) for i in ids)]
    s = np.concatenate([np.arange(3), np.stack([3 + 2 * np.array(keep), 4 + 2 * np.array(keep)], axis=1).reshape(-1)]).astype(np.int64)
    return x[s].copy(), P[np.ix_(s, s)].copy()
