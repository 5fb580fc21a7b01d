"""NumPy references of ekf_joint_consistency (include/ekfslam_c.h): joint / map NEES, log det P, pivots and the pose covariance
conditioned on the map, from a dense (x, P).

  lapack(x, P, x_true)   scipy.linalg.cho_factor on the WHOLE P (robot first, as the state is stored) for the joint quantities and on
                         P_LL for the map quantities; `info` from LAPACK's potrf itself
  tiled(x, P, x_true)    a restatement of the device algorithm: P_LL padded to whole 64-row tiles with a unit diagonal, right-looking
                         tile steps (diagonal tile, panel, trailing update), four right-hand sides carried along, the robot last
  longdouble(...)        an unblocked np.longdouble Cholesky of the whole P: what both are measured against

All return a dict with the fields of ekf_joint plus U (the upper factor of P_LL, when there is one)."""
import math

import numpy as np
import scipy.linalg

FIELDS = ("nees_map", "nees_joint", "logdet_map", "logdet_joint", "min_pivot", "max_pivot")
NAN = float("nan")


def wrap_error(x, x_true):
    """e = x - x_true with the heading wrapped as the library's NEES sample wraps it (ekf_filter_math.h: nees_sample)."""
    e = np.asarray(x, dtype=np.float64) - np.asarray(x_true, dtype=np.float64)
    e[2] -= 6.283185307179586 * math.floor((e[2] + 3.141592653589793) / 6.283185307179586)
    return e


def _blank(N):
    r = dict((f, NAN) for f in FIELDS)
    r.update(n_landmarks=N, info=0, cov_robot_given_map=np.full((3, 3), NAN), U=None)
    return r


def _robot_last(r, P, e, U, y, W):
    """The fields that follow from U^T [y | W] = [e_L | P_LR] (y None: no truth)."""
    N = r["n_landmarks"]
    d = np.diag(U) ** 2 if N else np.zeros(0)
    r["logdet_map"] = float(np.sum(np.log(d))) if N else 0.0
    r["min_pivot"], r["max_pivot"] = (float(d.min()), float(d.max())) if N else (0.0, 0.0)
    r["U"] = U
    yy = float(y @ y) if y is not None else NAN
    r["nees_map"] = yy
    S = P[:3, :3] - W.T @ W
    S = 0.5 * (S + S.T)
    r["cov_robot_given_map"] = S
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        r["info"] = -1
        return r
    if not np.all(np.isfinite(L)) or np.any(np.diag(L) <= 0):
        r["info"] = -1
        return r
    r["logdet_joint"] = r["logdet_map"] + 2.0 * float(np.sum(np.log(np.diag(L))))
    if y is not None:
        z = scipy.linalg.solve_triangular(L, e[:3] - W.T @ y, lower=True)
        r["nees_joint"] = yy + float(z @ z)
    return r


def potrf_info(A):
    """LAPACK's own verdict on a symmetric matrix: 0, or the order of the first leading minor that is not positive."""
    if A.shape[0] == 0:
        return 0
    _, info = scipy.linalg.lapack.dpotrf(np.asfortranarray(A), lower=0)
    return int(info)


def lapack(x, P, x_true=None):
    n = len(x)
    N = (n - 3) // 2
    r = _blank(N)
    PLL = P[3:, 3:]
    info = potrf_info(PLL)
    if info > 0:
        r["info"] = info
        return r
    e = wrap_error(x, x_true) if x_true is not None else None
    if N:
        c = scipy.linalg.cho_factor(PLL, lower=False)
        U = np.triu(c[0])
        W = scipy.linalg.solve_triangular(U, P[3:, :3], trans="T", lower=False)
        y = scipy.linalg.solve_triangular(U, e[3:], trans="T", lower=False) if e is not None else None
    else:
        U, W, y = np.zeros((0, 0)), np.zeros((0, 3)), (np.zeros(0) if e is not None else None)
    r = _robot_last(r, P, e, U, y, W)
    if r["info"] == 0:  # the joint fields from the whole P, robot first: independent of the ordering above
        cw = scipy.linalg.cho_factor(P, lower=False)
        r["logdet_joint"] = 2.0 * float(np.sum(np.log(np.diag(cw[0]))))
        if e is not None:
            r["nees_joint"] = float(e @ scipy.linalg.cho_solve(cw, e))
    return r


def tiled(x, P, x_true=None, tile=64):
    n = len(x)
    N = (n - 3) // 2
    r = _blank(N)
    m = 2 * N
    T = (m + tile - 1) // tile
    A = np.eye(T * tile)
    A[:m, :m] = P[3:, 3:]
    e = wrap_error(x, x_true) if x_true is not None else None
    B = np.zeros((T * tile, 4))
    if e is not None:
        B[:m, 0] = e[3:]
    B[:m, 1:] = P[3:, :3]
    for k in range(T):
        a, b = k * tile, (k + 1) * tile
        # diagonal tile, unblocked right-looking, right-hand sides as extra columns
        for i in range(a, b):
            d = A[i, i]
            if i < m and not d > 0.0:
                r["info"] = i + 1
                r["min_pivot"] = float(d)
                return r
            s = math.sqrt(d)
            A[i, i:b] /= s
            A[i, i] = s
            B[i] /= s
            A[i + 1:b, i + 1:b] -= np.outer(A[i, i + 1:b], A[i, i + 1:b])
            B[i + 1:b] -= np.outer(A[i, i + 1:b], B[i])
        if b < T * tile:
            A[a:b, b:] = scipy.linalg.solve_triangular(np.triu(A[a:b, a:b]), A[a:b, b:], trans="T", lower=False)
            B[b:] -= A[a:b, b:].T @ B[a:b]
            A[b:, b:] -= A[a:b, b:].T @ A[a:b, b:]
    U = np.triu(A)[:m, :m]
    return _robot_last(r, P, e, U, B[:m, 0] if e is not None else None, B[:m, 1:])


def longdouble(x, P, x_true=None):
    """Unblocked Cholesky of the whole P in np.longdouble, landmarks first and the robot last (the ordering does not change the
    values): the yardstick of the CPU tests.  Expects a positive definite P."""
    ld = np.longdouble
    n = len(x)
    N = (n - 3) // 2
    perm = np.r_[3:n, 0:3]
    A = np.asarray(P, dtype=ld)[np.ix_(perm, perm)].copy()
    e = wrap_error(x, x_true)[perm].astype(ld) if x_true is not None else np.zeros(n, dtype=ld)
    U = np.zeros((n, n), dtype=ld)
    for i in range(n):
        d = A[i, i] - U[:i, i] @ U[:i, i]
        U[i, i] = np.sqrt(d)
        U[i, i + 1:] = (A[i, i + 1:] - U[:i, i] @ U[:i, i + 1:]) / U[i, i]
    y = np.zeros(n, dtype=ld)
    for i in range(n):
        y[i] = (e[i] - U[:i, i] @ y[:i]) / U[i, i]
    d = np.diag(U) ** 2
    r = _blank(N)
    r["logdet_map"] = float(np.sum(np.log(d[:2 * N])))
    r["logdet_joint"] = float(np.sum(np.log(d)))
    r["nees_map"] = float(y[:2 * N] @ y[:2 * N]) if x_true is not None else NAN
    r["nees_joint"] = float(y @ y) if x_true is not None else NAN
    r["min_pivot"], r["max_pivot"] = (float(d[:2 * N].min()), float(d[:2 * N].max())) if N else (0.0, 0.0)
    L3 = U[2 * N:, 2 * N:]
    r["cov_robot_given_map"] = np.asarray(L3.T @ L3, dtype=np.float64)
    r["U"] = np.asarray(U[:2 * N, :2 * N], dtype=np.float64)
    return r


def draw_truth(x, P, seed):
    """x_true = x + L xi for a fixed seed, P = L L^T (a truth the estimate is consistent with)."""
    rng = np.random.default_rng(seed)
    L = np.linalg.cholesky(P)
    return x + L @ rng.standard_normal(len(x))


def rel_err(a, b):
    return abs(a - b) / max(abs(b), 1e-300)
