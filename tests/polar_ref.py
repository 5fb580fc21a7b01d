"""NumPy statement of ekf_update_polar and ekf_polar_compat (include/ekfslam_c.h) on a dense export, and the builders of the lists the
tests use.

update(x, P, z, R, ids, kind, round_size) -> (x, P, n_applied, d2): the entries with ids[k] >= 0, in rounds of round_size in list
order (None: all at once); a round is one joint update, every entry linearised at the round's entry state, two columns each.  With
dx = L_i.x - x_R, dy = L_i.y - y_R, q = dx^2 + dy^2, r = sqrt(q):
    range row:    h = r,                     H_R = [-dx / r, -dy / r,  0],   d = r - z[k][0]
    bearing row:  h = atan2(dy, dx) - phi,   H_R = [ dy / q, -dx / q, -1],   d = wrap(h - z[k][1])
    H_L = -H_R[0:2];   column c of W = ((P[:, 0] h0 + P[:, 1] h1) + P[:, 2] h2) - P[:, L_i.x] h0 - P[:, L_i.y] h1   (this order),
    S[a, c] = ((h0 W[0, c] + h1 W[1, c]) + h2 W[2, c]) - h0 W[L_i.x, c] - h1 W[L_i.y, c]   (row a's h, this order)  + blockdiag(R_k),
    S = U^T U,  V = W U^-1,  y = U^-T d,  x <- x - V y,  P <- P - V V^T,  d2[k] = sum of y^2 over the round's columns 0 .. 2 k_round + 1.
BOTH: row 0 of the slot is the range row, row 1 the bearing row, R[k] the 2x2 over (range, bearing) (its upper triangle is read).  A
RANGE or BEARING entry has its one live row in row 0 and the inert row of fix_ref's heading entry in row 1 (a zero row and column of
S, diagonal exactly 1, d = 0, a zero column of W), so that the prefixes of y^2 line up with the device's; it reads z[k][0] and
R[k][0][0] (RANGE) or z[k][1] and R[k][1][1] (BEARING) alone.  wrap is fix_ref.wrap.
A round whose S has a pivot that is not above PIVOT_TOL of its own diagonal entry -- or NaN: a landmark exactly at the robot's
position, q == 0 -- stops the call, that round and the later ones not applied (their d2 NaN, as for skipped entries).  Written like
fix_ref: match_ref's right-looking cholesky_upper and prefix_d2, the element-wise triangular solve, einsum for V V^T.
dtype=np.longdouble is the extended-precision restatement (sqrt and atan2 in extended precision too).
compat(x, P, z, R, ids, kind) -> d2 is one round over everything, nothing applied, NaN from the refused pivot on.
textbook(...) is the same update as K = P H^T S^-1, x + K res, P - K S K^T with np.linalg.solve and one-row entries unpadded."""
import numpy as np

import fix_ref as fx
import match_ref as mr
from fix_ref import TWO_PI, wrap  # noqa: F401
from match_ref import PIVOT_TOL, cholesky_upper, prefix_d2  # noqa: F401

SKIP = -1
RANGE, BEARING, BOTH = 1, 2, 3


def slot_rows(x, i, kind, z, dtype=np.float64):
    """The two rows of an entry's slot: [(H_R [3], d), (H_R, d) or None for the inert row]; z = (range, bearing) as the caller gave it."""
    Li = 3 + 2 * int(i)
    dx, dy = x[Li] - x[0], x[Li + 1] - x[1]
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        hr = np.array([-dx / r, -dy / r, dtype(0.0)], dtype=dtype)
        hb = np.array([dy / q, -dx / q, dtype(-1.0)], dtype=dtype)
    rng = (hr, r - dtype(z[0]))
    kind = int(kind)
    if kind == RANGE:
        return [rng, None]
    brg = (hb, wrap((np.arctan2(dy, dx) - x[2]) - dtype(z[1])))
    if kind == BEARING:
        return [brg, None]
    assert kind == BOTH, kind
    return [rng, brg]


def noise_of(R, kind):
    """The slot's 2x2 block of blockdiag(R_k), before the inert row's 1: what of R[k] the kind reads, its upper triangle."""
    kind = int(kind)
    if kind == RANGE:
        return np.array([[R[0][0], 0.0], [0.0, 0.0]])
    if kind == BEARING:
        return np.array([[R[1][1], 0.0], [0.0, 0.0]])
    return np.array([[R[0][0], R[0][1]], [R[0][1], R[1][1]]])


def assemble(x, P, z, R, ids, kind, dtype=np.float64):
    """(W, S, d) of one round; z [m][2], R [m][2][2], ids and kind [m] without skipped entries."""
    m, n = len(ids), len(x)
    W = np.zeros((n, 2 * m), dtype=dtype)
    S = np.zeros((2 * m, 2 * m), dtype=dtype)
    d = np.zeros(2 * m, dtype=dtype)
    rows = []
    for k in range(m):
        rows += [(3 + 2 * int(ids[k]), row) for row in slot_rows(x, ids[k], kind[k], z[k], dtype)]
    with np.errstate(invalid="ignore"):
        for c, (Li, row) in enumerate(rows):
            if row is not None:
                h = row[0]
                W[:, c] = ((P[:, 0] * h[0] + P[:, 1] * h[1]) + P[:, 2] * h[2]) - P[:, Li] * h[0] - P[:, Li + 1] * h[1]
                d[c] = row[1]
        live = np.array([row is not None for _, row in rows])
        for a, (Li, row) in enumerate(rows):
            if row is None:
                S[a, a] = 1.0
                continue
            h = row[0]
            S[a, :] = np.where(live, ((h[0] * W[0, :] + h[1] * W[1, :]) + h[2] * W[2, :]) - h[0] * W[Li, :] - h[1] * W[Li + 1, :], 0.0)
    for k in range(m):
        S[2 * k:2 * k + 2, 2 * k:2 * k + 2] += noise_of(R[k], kind[k]).astype(dtype)
    return W, S, d


def round_update(x, P, z, R, ids, kind, dtype=np.float64):
    """One joint update: (x1, P1, d2), or (None, None, d2) when S is refused."""
    W, S, d = assemble(x, P, z, R, ids, kind, dtype)
    with np.errstate(invalid="ignore"):
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


def _lists(z, R, ids, kind):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    return np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2), ids, np.asarray(kind, dtype=np.int64).reshape(-1)


def update(x, P, z, R, ids, kind, round_size=None, dtype=np.float64):
    x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
    z, R, ids, kind = _lists(z, R, ids, kind)
    kept = np.flatnonzero(ids >= 0)
    rs = int(round_size) if round_size else max(len(kept), 1)
    d2 = np.full(len(ids), np.nan)
    applied = 0
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        x1, P1, dr = round_update(x, P, z[sel], R[sel], ids[sel], kind[sel], dtype)
        if x1 is None:
            break
        x, P = x1, P1
        d2[sel] = dr
        applied += len(sel)
    return x, P, applied, d2


def update_extended(x, P, z, R, ids, kind, round_size=None):
    return update(x, P, z, R, ids, kind, round_size, dtype=np.longdouble)


def compat(x, P, z, R, ids, kind, dtype=np.float64):
    z, R, ids, kind = _lists(z, R, ids, kind)
    kept = np.flatnonzero(ids >= 0)
    d2 = np.full(len(ids), np.nan)
    if len(kept):
        x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
        _, S, d = assemble(x, P, z[kept], R[kept], ids[kept], kind[kept], dtype)
        with np.errstate(invalid="ignore"):
            _, y, bad = cholesky_upper(S, d)
        d2[kept] = prefix_d2(y[:, 0], bad)
    return d2


def jacobian(x, i, kind):
    """H of one entry over the whole state, unpadded: [1 or 2][n]."""
    rows = [row for row in slot_rows(x, i, kind, (0.0, 0.0)) if row is not None]
    H = np.zeros((len(rows), len(x)))
    Li = 3 + 2 * int(i)
    for a, (h, _) in enumerate(rows):
        H[a, 0:3] = h
        H[a, Li:Li + 2] = -h[0:2]
    return H


def predict(x, i, kind):
    """h(x) of one entry, unpadded: (range), (bearing, not wrapped) or both."""
    Li = 3 + 2 * int(i)
    dx, dy = x[Li] - x[0], x[Li + 1] - x[1]
    both = [np.sqrt(dx * dx + dy * dy), np.arctan2(dy, dx) - x[2]]
    return np.array({RANGE: both[:1], BEARING: both[1:], BOTH: both}[int(kind)])


def textbook(x, P, z, R, ids, kind, round_size=None):
    """The same rounds as K = P H^T S^-1 (np.linalg.solve), x + K res, P - K S K^T: a one-component entry is ONE row of H.  Returns
    (x, P, d2) with d2[k] the distance res^T S^-1 res of k's round cut after entry k."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    z, R, ids, kind = _lists(z, R, ids, kind)
    kept = np.flatnonzero(ids >= 0)
    rs = int(round_size) if round_size else max(len(kept), 1)
    d2 = np.full(len(ids), np.nan)
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        Hs, res, blocks, ends = [], [], [], []
        for k in sel:
            Hs.append(jacobian(x, ids[k], kind[k]))
            hx = predict(x, ids[k], kind[k])
            if kind[k] == RANGE:
                res.append(z[k, 0] - hx[0]), blocks.append(R[k, :1, :1])
            elif kind[k] == BEARING:
                res.append(-wrap(hx[0] - z[k, 1])), blocks.append(R[k, 1:, 1:])
            else:
                res += [z[k, 0] - hx[0], -wrap(hx[1] - z[k, 1])]
                blocks.append(noise_of(R[k], BOTH))
            ends.append(len(res))
        H = np.concatenate(Hs)
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
VAR_RANGE, VAR_BEARING = 2.5e-3, 4.0e-4                      # 5 cm, 20 mrad
R_BOTH = np.array([[2.5e-3, 1.0e-4], [1.0e-4, 4.0e-4]])
KIND_CYCLE = (BOTH, RANGE, BEARING)
SIZES = mr.SIZES
STATE_SEED = fx.STATE_SEED


def cycle(n):
    return np.array([KIND_CYCLE[k % 3] for k in range(n)], dtype=np.int32)


def entries_for(x, ids, kind, seed, turns=0):
    """(z [n][2], R [n][2][2]) for the entries (ids, kind) on the state x: R from the constants above, z = h(x) + noise drawn from R,
    a bearing wrapped into [-pi, pi) as a sensor reports it (+ `turns` whole turns).  NaN where ids[k] == -1 and in what a kind does
    not read."""
    rng = np.random.default_rng(seed)
    n = len(ids)
    z, R = np.full((n, 2), np.nan), np.full((n, 2, 2), np.nan)
    for k in range(n):
        u = rng.normal(size=2)
        if ids[k] < 0:
            continue
        kd = int(kind[k])
        hx = predict(x, ids[k], BOTH)
        if kd == BOTH:
            R[k] = R_BOTH
            v = np.linalg.cholesky(R_BOTH) @ u
        else:
            R[k, 0, 0] = VAR_RANGE
            R[k, 1, 1] = VAR_BEARING
            v = np.sqrt([VAR_RANGE, VAR_BEARING]) * u
        zz = np.array([hx[0] + v[0], wrap(hx[1] + v[1]) + TWO_PI * turns])
        if kd == RANGE:
            zz[1], R[k, 1, 1] = np.nan, np.nan
        if kd == BEARING:
            zz[0], R[k, 0, 0] = np.nan, np.nan
        z[k] = zz
    return z, R


def ranges(x):
    L = x[3:].reshape(-1, 2)
    return np.hypot(L[:, 0] - x[0], L[:, 1] - x[1])


def nearest(x, count, floor=1.0, without=()):
    """The `count` landmarks nearest the robot that are at least `floor` metres away and not in `without`."""
    r = ranges(x)
    order = [int(i) for i in np.argsort(r, kind="stable") if r[i] >= floor and int(i) not in without]
    return np.array(order[:count], dtype=np.int64)


def behind(x):
    """The landmark at least 1 m away whose world-frame direction atan2(dy, dx) is nearest +-pi: due west of the robot."""
    L = x[3:].reshape(-1, 2)
    a = np.abs(np.arctan2(L[:, 1] - x[1], L[:, 0] - x[0]))
    a[ranges(x) < 1.0] = 0.0
    return int(np.argmax(a))


def mixed_list(pkg, x, P, seed):
    """(z, R, ids, kind) of 24 entries, kinds cycling BOTH / RANGE / BEARING: landmarks 0, 15, 16 and N - 1 (tile edges), the nearest
    landmark as a RANGE and as a BEARING entry next to each other (one round for every window above 2), the landmark due west of the
    robot (atan2 near +-pi) as BOTH and as BEARING, entries 7 and 18 skipped, the rest the nearest landmarks in a seeded order; the
    last entry's bearing is reported a whole turn up.  Every range is at least 1 m."""
    N = (len(x) - 3) // 2
    west = behind(x)
    fixed = [0, 15, 16, N - 1, west]
    near = nearest(x, 1 + 24, without=fixed)
    twice, rest = int(near[0]), list(np.random.default_rng(seed + 3000).permutation(near[1:]))
    ids = [0, twice, twice, 15, 16, N - 1, west, SKIP, west]
    ids += [int(rest.pop()) for _ in range(18 - len(ids))] + [SKIP] + [int(rest.pop()) for _ in range(5)]
    ids, kind = np.array(ids, dtype=np.int32), cycle(24)
    assert len(ids) == 24 and kind[1] == RANGE and kind[2] == BEARING and kind[8] == BEARING and kind[23] == BEARING
    assert ranges(x)[ids[ids >= 0]].min() >= 1.0
    z, R = entries_for(x, ids, kind, seed)
    z[23, 1] += TWO_PI
    return z, R, ids, kind


def list_of_nine(z, R, ids, kind):
    """The head of a list up to its ninth non-skipped entry."""
    end = int(np.flatnonzero(np.cumsum(np.asarray(ids) >= 0) == 9)[0]) + 1
    return z[:end], R[:end], ids[:end], kind[:end]


def uniform_list(x, kind, count, seed):
    """`count` entries of one kind: the 24 nearest landmarks (at least 1 m away) in a seeded order, then some of them again."""
    near = nearest(x, 24)
    rng = np.random.default_rng(seed)
    ids = np.concatenate([rng.permutation(near), rng.choice(near, size=max(count - 24, 0))])[:count].astype(np.int32)
    kinds = np.full(count, kind, dtype=np.int32)
    return entries_for(x, ids, kinds, seed + 1) + (ids, kinds)


# the batch form: three filters in capacity 128, window 4, ragged lists padded with -1
BATCH_COUNTS = (100, 45, 64)
BATCH_IDS = [[0, 99, -1, 31, 32, -1, 63, 64, 5, 31], [1, 44, -1, -1, 1, -1, -1, -1, -1, -1], [32, -1, 0, 7, -1, 7, 31, 63, 16, 15]]
OPEN_WINDOW_IDS = [3, 40, 31, 32, 63, 64, 5, 99]
# window 4 on a map of 60: the same landmark's range twice with R = 0 at the head of round two of three
SINGULAR_IDS = [3, 40, 31, 32, 17, 17, 5, 2, 33, 8]
SINGULAR_KINDS = [BOTH, RANGE, BEARING, BOTH, RANGE, RANGE, BEARING, BOTH, RANGE, BEARING]
ON_POSE = 21  # the landmark the q == 0 state has exactly at the robot's position; entry 1 of the list measures it, in round one:
              # behind a completed round the pose and the landmark have moved apart, by the round's own correction


def batch_lists(pkg, states):
    ids = np.array(BATCH_IDS, dtype=np.int32)
    kind = np.stack([np.roll(cycle(ids.shape[1]), b) for b in range(len(states))])
    zs, Rs = zip(*[entries_for(states[b][0], ids[b], kind[b], 940 + b) for b in range(len(states))])
    return np.stack(zs), np.stack(Rs), ids, kind


def singular_list(pkg, x, P):
    ids, kind = np.array(SINGULAR_IDS, dtype=np.int32), np.array(SINGULAR_KINDS, dtype=np.int32)
    z, R = entries_for(x, ids, kind, 951)
    R[4:6, 0, 0] = 0.0
    z[5] = z[4]
    return z, R, ids, kind


def on_pose_state(pkg):
    """The map of 60 with landmark ON_POSE moved exactly onto the robot's position."""
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    x = x.copy()
    x[3 + 2 * ON_POSE:5 + 2 * ON_POSE] = x[0:2]
    return x, P


def on_pose_list(pkg, x, P, kind_of_it):
    """SINGULAR_IDS' list with entry 1 a measurement of the landmark on the pose, of the given kind (z: one metre, straight ahead)."""
    ids, kind = np.array(SINGULAR_IDS, dtype=np.int32), np.array(SINGULAR_KINDS, dtype=np.int32)
    ids[1], kind[1] = ON_POSE, kind_of_it
    probe = ids.copy()
    probe[1] = SKIP
    z, R = entries_for(x, probe, kind, 961)
    z[1], R[1] = (1.0, 0.0), R_BOTH
    return z, R, ids, kind


def gpu_inputs(pkg):
    """(name, x, P, z, R, ids, kind, round_size) of every update the GPU tests of tests/test_update_polar.py ask for (the state with
    an open window differs from its stand-in here by a few propagations and Old updates)."""
    out = []
    for N, _ in SIZES:
        x, P = pkg.scenarios.injected_state(N, seed=STATE_SEED[N], extent=mr.map_extent(N))
        lst = mixed_list(pkg, x, P, STATE_SEED[N])
        for rs in (1, 5, 16, 32):
            out.append(("mixed N=%d, rounds of %d" % (N, rs), x, P) + lst + (rs,))
        out.append(("mixed N=%d, list of 9 in a window of 16" % N, x, P) + list_of_nine(*lst) + (16,))
        out.append(("32 BOTH N=%d, window 32" % N, x, P) + uniform_list(x, BOTH, 32, 400 + N) + (32,))
        out.append(("RANGE only N=%d" % N, x, P) + uniform_list(x, RANGE, 12, 500 + N) + (16,))
        out.append(("BEARING only N=%d" % N, x, P) + uniform_list(x, BEARING, 12, 600 + N) + (16,))
    states = mr.batch_states(pkg, BATCH_COUNTS, 80)
    z, R, ids, kind = batch_lists(pkg, states)
    for b in range(len(states)):
        out.append(("batch filter %d" % b, *states[b], z[b], R[b], ids[b], kind[b], 4))
    x, P = pkg.scenarios.injected_state(100, seed=13, extent=mr.map_extent(100))
    kind = cycle(len(OPEN_WINDOW_IDS))
    out.append(("open window pair", x, P) + entries_for(x, OPEN_WINDOW_IDS, kind, 313) + (np.array(OPEN_WINDOW_IDS), kind, 16))
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    z, R, ids, kind = singular_list(pkg, x, P)
    out.append(("singular second round: round one", x, P, z[:4], R[:4], ids[:4], kind[:4], 4))
    assert len(set(t[0] for t in out)) == len(out), "two inputs of one name"
    return out


# Relative agreement asked of d2 on the device: 20 times what test_update_polar_cpu.py measures between the double reference and its
# extended-precision restatement over every input of gpu_inputs, as an update in its rounds and as one round of ekf_polar_compat
# (3.444e-13 at worst: "mixed N=100, rounds of 1").  The margin covers the device's sqrt / atan2, which may differ from NumPy's by
# an ulp, its FMA contraction and the other order of the elimination's sums, as for fix_ref.D2_REL and match_ref.D2_REL.
D2_REL = 6.89e-12
