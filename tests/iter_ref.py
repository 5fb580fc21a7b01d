"""NumPy statement of ekf_update_matched_iter (include/ekfslam_c.h) on a dense export, built from match_ref.linearise and
match_ref.cholesky_upper, and the inputs of tests/test_update_matched_iter.py.

update(x, P, z, R, ids, max_iter, tol, round_size) -> (x, P, n_applied, d2, iters, step): the measurements with ids[k] >= 0 in rounds
of round_size in list order, as match_ref.update; a round with entry state (xh, P) and linearisation points xi_0 = xh, xi_1, ...:
    (W_i, S_i, h(xi_i) - z) = match_ref.linearise(xi_i, P, ...),   H_i = jacobian(xi_i, ...),
    d_0 = h(xh) - z;   i > 0:  d_i = (h(xi_i) - z) + H_i (xh - xi_i),
    S_i = U_i^T U_i (match_ref.cholesky_upper: its pivot rule in every iteration),   y_i = U_i^-T d_i,   q_i = U_i^-1 y_i = S_i^-1 d_i,
    xi_i+1 = xh - W_i q_i on the touched components (the pose and the round's landmarks; the others never enter H or d),
    step_i = max |xi_i+1 - xi_i| over them;   the round stops behind iteration i when step_i <= tol or i + 1 == max_iter:
    x <- xh - V_i y_i,   P <- P - V_i V_i^T,   V_i = W_i U_i^-1     (match_ref.round_update's own lines, so max_iter = 1 is its bits).
A pivot refused in any iteration stops the call, that round and the later ones not applied.  d2 is match_ref.prefix_d2 of y_0;
iters[k] the factorisations of k's round (0: skipped or not applied), step[k] its last step (NaN: skipped or not applied).
dtype=np.longdouble is the extended-precision restatement, `trig` match_ref's hook for cos phi and sin phi.  `trace`, a list, gets
every step of every round appended.

map_cost and map_gradient state what the iteration minimises, (x - xh)^T P^-1 (x - xh) + sum (h_k(x) - z_k)^T R_k^-1 (h_k(x) - z_k),
for one round over the whole list."""
import numpy as np

import match_ref as mr

ITER_MAX = 16


def jacobian(xi, ids, dtype=np.float64, trig=None):
    """H [2 m][n] at xi, rows as match_ref.linearise builds them."""
    trig = trig or (mr.libm_trig if dtype == np.float64 else mr.extended_trig)
    c, s = trig(xi[2])
    C = np.array([[c, -s], [s, c]], dtype=dtype)
    J = mr._J.astype(dtype)
    H = np.zeros((2 * len(ids), len(xi)), dtype=dtype)
    for k, i in enumerate(ids):
        Li = 3 + 2 * int(i)
        dp = xi[Li:Li + 2] - xi[0:2]
        H[2 * k:2 * k + 2, 0:2] += -C.T
        H[2 * k:2 * k + 2, 2] += -C.T @ J @ dp
        H[2 * k:2 * k + 2, Li:Li + 2] += C.T
    return H


def back_substitute(U, y):
    """q with U q = y, U upper triangular."""
    M = len(y)
    q = np.array(y)
    for k in range(M - 1, -1, -1):
        q[k] = q[k] / U[k, k]
        q[:k] = q[:k] - U[:k, k] * q[k]
    return q


def touched_of(ids):
    out = [0, 1, 2]
    for i in ids:
        out += [3 + 2 * int(i), 4 + 2 * int(i)]
    return np.array(sorted(set(out)), dtype=np.int64)


def round_update(xh, P, z, R, ids, max_iter, tol, dtype=np.float64, trig=None, trace=None):
    """One iterated round: (x1, P1, d2, iters, step); x1 = P1 = None when a pivot was refused."""
    sel = touched_of(ids)
    xi = np.array(xh)
    d2 = None
    for it in range(max_iter):
        W, S, d = mr.linearise(xi, P, z, R, ids, dtype, trig)
        if it > 0:
            d = d + jacobian(xi, ids, dtype, trig) @ (xh - xi)
        U, y, bad = mr.cholesky_upper(S, d)
        y = y[:, 0]
        if it == 0:
            d2 = mr.prefix_d2(y, bad)
        if bad is not None:
            return None, None, d2, it + 1, np.nan
        nxt = np.array(xh)
        nxt[sel] = xh[sel] - W[sel] @ back_substitute(U, y)
        step = float(np.abs(nxt[sel] - xi[sel]).max())
        if trace is not None:
            trace.append(step)
        if step <= tol or it + 1 == max_iter:
            break
        xi = nxt
    M = len(d)
    V = np.empty_like(W)
    for c in range(M):
        acc = W[:, c].copy()
        for k in range(c):
            acc -= V[:, k] * U[k, c]
        V[:, c] = acc / U[c, c]
    x1 = xh - np.einsum("ik,k->i", V, y)
    P1 = P - np.einsum("ik,jk->ij", V, V)
    return x1, P1, d2, it + 1, step


def update(x, P, z, R, ids, max_iter, tol, round_size=None, dtype=np.float64, trig=None, trace=None):
    assert 1 <= max_iter <= ITER_MAX and np.isfinite(tol) and tol >= 0.0
    x, P = np.array(x, dtype=dtype), np.array(P, dtype=dtype)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    kept = np.flatnonzero(ids >= 0)
    rs = int(round_size) if round_size else max(len(kept), 1)
    d2, step = np.full(len(ids), np.nan), np.full(len(ids), np.nan)
    iters = np.zeros(len(ids), dtype=np.int32)
    applied = 0
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        x1, P1, dr, n_it, st = round_update(x, P, z[sel], R[sel], ids[sel], max_iter, tol, dtype, trig, trace)
        if x1 is None:
            break
        x, P = x1, P1
        d2[sel], iters[sel], step[sel] = dr, n_it, st
        applied += len(sel)
    return x, P, applied, d2, iters, step


def update_extended(x, P, z, R, ids, max_iter, tol, round_size=None, trace=None):
    return update(x, P, z, R, ids, max_iter, tol, round_size, dtype=np.longdouble, trace=trace)


# ---- what the iteration minimises -----------------------------------------------------------------------------------------------------
def _residual(x, z, ids, dtype):
    c, s = (mr.libm_trig if dtype == np.float64 else mr.extended_trig)(x[2])
    C = np.array([[c, -s], [s, c]], dtype=dtype)
    return np.concatenate([C.T @ (x[3 + 2 * int(i):5 + 2 * int(i)] - x[0:2]) - np.asarray(z[k], dtype=dtype) for k, i in enumerate(ids)])


def _solve_spd(P, b):
    """P^-1 b by the Cholesky factor of P, in P's precision."""
    n = len(b)
    A = np.array(P)
    for k in range(n):
        A[k, k:] = A[k, k:] / np.sqrt(A[k, k])
        A[k + 1:, k + 1:] -= np.outer(A[k, k + 1:], A[k, k + 1:])
    U = np.triu(A)
    t = np.array(b)
    for k in range(n):  # U^T t = b
        t[k] = t[k] / U[k, k]
        t[k + 1:] = t[k + 1:] - U[k, k + 1:] * t[k]
    return back_substitute(U, t)


def _weighted(r, R, dtype, magnitudes=False):
    """blockdiag(R_k)^-1 r; magnitudes: |R_k^-1| |r|, what the products of the sum amount to before they cancel."""
    out = np.empty_like(r)
    for k in range(len(r) // 2):
        Rk = np.asarray(R[k], dtype=dtype)
        det = Rk[0, 0] * Rk[1, 1] - Rk[0, 1] * Rk[1, 0]
        inv = np.array([[Rk[1, 1], -Rk[0, 1]], [-Rk[1, 0], Rk[0, 0]]], dtype=dtype) / det
        out[2 * k:2 * k + 2] = np.abs(inv) @ np.abs(r[2 * k:2 * k + 2]) if magnitudes else inv @ r[2 * k:2 * k + 2]
    return out


def map_cost(x, xh, P, z, R, ids, dtype=np.longdouble):
    x, xh, P = np.asarray(x, dtype=dtype), np.asarray(xh, dtype=dtype), np.asarray(P, dtype=dtype)
    r = _residual(x, z, ids, dtype)
    return float((x - xh) @ _solve_spd(P, x - xh) + r @ _weighted(r, R, dtype))


def map_gradient(x, xh, P, z, R, ids, dtype=np.longdouble):
    """Half the cost's gradient, multiplied by P (which is regular: zero together with the gradient, and no inverse of P is taken):
    (prior, meas, scale) with prior = x - xh and meas = P H(x)^T R^-1 (h(x) - z), the two terms that cancel at the minimum, and
    scale = |P| |H^T| |R^-1| (|h(x)| + |z|), the size of the products meas is summed from -- h(x) - z itself is a difference of
    ranges of metres that leaves centimetres, and R^-1 multiplies its rounding like everything else."""
    x, xh, P = np.asarray(x, dtype=dtype), np.asarray(xh, dtype=dtype), np.asarray(P, dtype=dtype)
    r = _residual(x, z, ids, dtype)
    H = jacobian(x, ids, dtype)
    zz = np.concatenate([np.asarray(z[k], dtype=dtype) for k in range(len(ids))])
    scale = np.abs(P) @ (np.abs(H).T @ _weighted(np.abs(r + zz) + np.abs(zz), R, dtype, magnitudes=True))
    return x - xh, P @ (H.T @ _weighted(r, R, dtype)), scale


# ---- the inputs of tests/test_update_matched_iter.py (checked on the CPU in tests/test_update_matched_iter_cpu.py) --------------------
HEADINGS = (0.02, 0.1, 0.3)   # the three regimes of the pose's displacement, rad
MAX_ITER = 12
# name -> tol: the steps shrink about 100 times per iteration, and every step of every round of an input lies a factor of 5.5 and
# more from its tol, in the double and in the extended run (test_update_matched_iter_cpu.py asks for 4) -- so the device, whose steps
# differ from the reference's by rounding, stops at the same iteration and `iters` can be asked for exactly.  A batch call has one
# tol: the filters of WIDE_COUNTS share theirs.
TOL_OF = {"planted N=200, heading off by 0.02": 5e-7, "planted N=200, heading off by 0.1": 1e-10, "planted N=200, heading off by 0.3": 2e-10,
          "planted N=100, heading off by 0.02": 2e-7, "planted N=100, heading off by 0.1": 1e-8, "planted N=100, heading off by 0.3": 2e-8,
          "one measurement": 5e-10, "one landmark three times in a round": 5e-10, "a full round of 32": 5e-9, "9 entries in rounds of 4": 2e-7,
          "tol = 0": 0.0, "tile edges": 1e-9, "open window pair": 3e-10, "refused second round": 5e-9,
          "0 beside 257, filter 0": 5e-7, "0 beside 257, filter 2": 5e-7, "0 beside 257, filter 3": 5e-7}
WIDE_TOL = 5e-7


def tol_of(name):
    return TOL_OF[name]


def tol_between(x, P, z, R, ids, round_size, near=1e-8):
    """A tol for a state that only the test's run knows (a handle's own export): the geometric mean of the two successive steps of
    the reference's run to a standstill that lie either side of `near`, and their ratio -- at least 16 puts both a factor of 4 away.
    One round only."""
    trace = []
    update(x, P, z, R, ids, ITER_MAX, 0.0, round_size, trace=trace)
    k = next(k for k in range(1, len(trace)) if trace[k] <= near < trace[k - 1])
    return float(np.sqrt(trace[k - 1] * trace[k])), trace[k - 1] / trace[k]


def displaced(x, P, e):
    """The state as a coarse pose reset leaves it: the pose moved by (e, -e / 2) m and e rad, the robot uncorrelated with the map,
    a standard deviation of e m and e rad."""
    x, P = np.array(x), np.array(P)
    x[0:3] += (e, -0.5 * e, e)
    P[0:3, :] = 0.0
    P[:, 0:3] = 0.0
    P[0:3, 0:3] = np.diag([e * e] * 3)
    return x, P


def seen_from(pkg, x, ids, seed, e):
    """mr.scan_of for a robot that stands (e, -e / 2) m and e rad away from where x has it: the measurements of a pose that is off."""
    t = np.array(x)
    t[0:3] += (e, -0.5 * e, e)
    return mr.scan_of(pkg, t, ids, seed)


REFUSED_IDS = [3, 40, 31, 32, 17, 17, 5]   # window 4: the second round starts with the same exact measurement twice
WIDE_E = (0.1, 0.0, 0.05, 0.3)


def refused_input(pkg):
    x, P = displaced(*pkg.scenarios.injected_state(60, seed=91, extent=12.0), 0.1)
    z, R = seen_from(pkg, x, REFUSED_IDS, 91, -0.1)
    R[4:6] = 0.0
    z[5] = z[4]
    return x, P, z, R, REFUSED_IDS


def wide_inputs(pkg):
    """[(x, P, z, R, ids)] of match_ref.WIDE_COUNTS' four filters (capacity 320, window 8); filter 1 has no landmark."""
    out = []
    for b, (x, P) in enumerate(mr.batch_states(pkg, mr.WIDE_COUNTS, 90)):
        if mr.WIDE_COUNTS[b]:
            x, P = displaced(x, P, WIDE_E[b])
        out.append((x, P) + seen_from(pkg, x, mr.WIDE_IDS[b], 890 + b, -WIDE_E[b]) + (mr.WIDE_IDS[b],))
    return out


def gpu_inputs(pkg):
    """(name, x, P, z, R, ids, round_size, max_iter) of every iterated update the GPU tests compare with the reference; tol is
    tol_of(name).  The truth is the planted state, the filter's pose is displaced (or, where the state is the handle's own, the
    measurements are those of a displaced robot)."""
    out = []
    for N, _ in mr.SIZES:
        xt, Pt, z, R, ids = mr.planted_scan(pkg, N, mr.SCAN_SEED[N])
        for e in HEADINGS:
            x, P = displaced(xt, Pt, e)
            out.append(("planted N=%d, heading off by %g" % (N, e), x, P, z, R, ids, 32, MAX_ITER))
        x, P = displaced(xt, Pt, 0.1)
        if N == 100:
            out.append(("one measurement", x, P, z[:1], R[:1], ids[:1], 16, MAX_ITER))
            twice = [0, 1, 0, 2, 0]
            out.append(("one landmark three times in a round", x, P, z[twice], R[twice], ids[twice], 16, MAX_ITER))
            z32, R32, ids32 = mr.hypothesis_of_32(pkg, xt, z, R, ids)
            out.append(("a full round of 32", x, P, z32, R32, ids32, 32, MAX_ITER))
            out.append(("9 entries in rounds of 4", x, P, z[:9], R[:9], ids[:9], 4, MAX_ITER))
            out.append(("tol = 0", x, P, z[:8], R[:8], ids[:8], 16, 3))
    xt, Pt = pkg.scenarios.injected_state(100, seed=51, extent=15.0)
    x, P = displaced(xt, Pt, 0.1)
    out.append(("tile edges", x, P) + mr.scan_of(pkg, xt, mr.EDGE_IDS, 510) + (mr.EDGE_IDS, 16, MAX_ITER))
    x, P = pkg.scenarios.injected_state(100, seed=13, extent=12.0 * (100 / 64.0) ** 0.5 + 8.0)
    ids = [3, 40, 31, 32, 63, 64, 5, 99]
    out.append(("open window pair", x, P) + seen_from(pkg, x, ids, 313, 0.02) + (ids, 16, MAX_ITER))
    out.append(("refused second round",) + refused_input(pkg) + (4, MAX_ITER))
    for b, t in enumerate(wide_inputs(pkg)):
        if mr.WIDE_COUNTS[b]:
            out.append((("0 beside 257, filter %d" % b,) + t + (8, MAX_ITER)))
    return out


# What test_update_matched_iter_cpu.py measures between the double reference and its extended-precision restatement over gpu_inputs
# (the worst input of each), and 20 times that: what the GPU tests ask of the device.
MEASURED_X = 5.42e-15     # max |dx|, m and rad: "0 beside 257, filter 3", the heading off by 0.3 (2.0e-15 with libm's cos and sin alone)
MEASURED_P = 3.38e-14     # max |dP| / max |P|: the same input
MEASURED_D2 = 1.37e-13    # relative: "open window pair", whose smallest d2 is the smallest of all inputs
MEASURED_STEP = 5.84e-15  # absolute: "0 beside 257, filter 3"; a step is the difference of coordinates of up to 40 m
BOUND_X, BOUND_P, BOUND_D2, BOUND_STEP = 20 * MEASURED_X, 20 * MEASURED_P, 20 * MEASURED_D2, 20 * MEASURED_STEP
