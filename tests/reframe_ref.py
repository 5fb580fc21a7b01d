"""NumPy reference of the two frame changes (ekf_transform_frame, ekf_anchor_at_robot): x' = g(x), P' = J P J^T.

Two forms of each: the dense one (`*_g`, `*_J`, `apply_dense`: J built as a matrix, checked against central differences of g in
tests/test_reframe_cpu.py) and the blockwise one (`rigid`, `anchor`: J is block diagonal over the landmarks plus three robot
columns, so P' costs O(n^2); this is what the GPU tests compare with, N = 4096 included).  The blockwise results are symmetrised
(0.5 (P + P^T), exact for a symmetric P); with theta = 0 `rigid` returns P bit for bit and x as the single subtraction.
cos / sin are math.cos / math.sin, the two numbers the library takes on the host."""
import math

import numpy as np

S = np.array([[0.0, -1.0], [1.0, 0.0]])


def rot(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s], [s, c]])


def _q(a, dtype=np.float64):
    """Rot(-a) written with cos(a), sin(a): [[c, s], [-s, c]] (the float64 values of math.cos / math.sin in every dtype)."""
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, s], [-s, c]], dtype=dtype)


def inverse_frame(frame):
    """The pose of the OLD frame's origin in the new frame: rigid(rigid(x, F), inverse_frame(F)) = x."""
    tx, ty, th = frame
    t = _q(th) @ np.array([tx, ty])
    return np.array([-t[0], -t[1], -th])


# ---- dense forms ---------------------------------------------------------------------------------
# (dtype=np.longdouble: the same expressions carried in extended precision -- the yardstick of the float64 results; cos / sin stay
# the float64 values the library takes)
def rigid_g(x, frame, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    Q, t = _q(frame[2], dtype), np.array([frame[0], frame[1]], dtype=dtype)
    out = np.empty_like(x)
    out[0:2] = Q @ (x[0:2] - t)
    out[2] = x[2] - dtype(frame[2])
    out[3:] = ((x[3:].reshape(-1, 2) - t) @ Q.T).reshape(-1)
    return out


def rigid_J(x, frame, dtype=np.float64):
    n = len(x)
    Q = _q(frame[2], dtype)
    J = np.zeros((n, n), dtype=dtype)
    J[0:2, 0:2] = Q
    J[2, 2] = 1.0
    for a in range(3, n, 2):
        J[a:a + 2, a:a + 2] = Q
    return J


def anchor_g(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    Q = _q(float(x[2]), dtype)
    out = np.zeros_like(x)
    out[3:] = ((x[3:].reshape(-1, 2) - x[0:2]) @ Q.T).reshape(-1)
    return out


def anchor_J(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    n = len(x)
    Q = _q(float(x[2]), dtype)
    J = np.zeros((n, n), dtype=dtype)
    for a in range(3, n, 2):
        d = x[a:a + 2] - x[0:2]
        J[a:a + 2, 0:2] = -Q
        J[a:a + 2, 2] = -Q @ (S.astype(dtype) @ d)
        J[a:a + 2, a:a + 2] = Q
    return J


def apply_dense(x, P, g, J, dtype=None):
    """g(x), J(x) P J(x)^T; with a dtype, g and J are called with it and P is carried in it."""
    if dtype is None:
        return g(x), J(x) @ P @ J(x).T
    Jx = J(x, dtype=dtype)
    return g(x, dtype=dtype), Jx @ np.asarray(P, dtype=dtype) @ Jx.T


def central_difference(g, x, h=1e-6):
    n = len(x)
    J = np.empty((n, n))
    for k in range(n):
        e = np.zeros(n)
        e[k] = h
        J[:, k] = (g(x + e) - g(x - e)) / (2.0 * h)
    return J


# ---- blockwise forms -----------------------------------------------------------------------------
def _rotate_blocks(PLL, Q):
    """Q P_lm Q^T for every 2x2 block of PLL [N, 2, N, 2]."""
    r1 = np.empty_like(PLL)
    r1[:, 0] = Q[0, 0] * PLL[:, 0] + Q[0, 1] * PLL[:, 1]
    r1[:, 1] = Q[1, 0] * PLL[:, 0] + Q[1, 1] * PLL[:, 1]
    r2 = np.empty_like(PLL)
    r2[..., 0] = r1[..., 0] * Q[0, 0] + r1[..., 1] * Q[0, 1]
    r2[..., 1] = r1[..., 0] * Q[1, 0] + r1[..., 1] * Q[1, 1]
    return r2


def rigid(x, P, frame):
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    n = x.size
    N = (n - 3) // 2
    Q, t = _q(frame[2]), np.array([frame[0], frame[1]])
    JR = np.eye(3)
    JR[0:2, 0:2] = Q
    xo = np.empty(n)
    d = x[0:2] - t
    xo[0:2] = (Q[0, 0] * d[0] + Q[0, 1] * d[1], Q[1, 0] * d[0] + Q[1, 1] * d[1])
    xo[2] = x[2] - frame[2]
    L = x[3:].reshape(N, 2) - t
    xo[3::2] = Q[0, 0] * L[:, 0] + Q[0, 1] * L[:, 1]
    xo[4::2] = Q[1, 0] * L[:, 0] + Q[1, 1] * L[:, 1]
    Po = np.empty((n, n))
    Po[:3, :3] = JR @ P[:3, :3] @ JR.T
    PLR = P[3:, :3].reshape(N, 2, 3)
    r1 = np.empty_like(PLR)
    r1[:, 0] = Q[0, 0] * PLR[:, 0] + Q[0, 1] * PLR[:, 1]
    r1[:, 1] = Q[1, 0] * PLR[:, 0] + Q[1, 1] * PLR[:, 1]
    Po[3:, :3] = (r1 @ JR.T).reshape(2 * N, 3)
    Po[:3, 3:] = Po[3:, :3].T
    Po[3:, 3:] = _rotate_blocks(P[3:, 3:].reshape(N, 2, N, 2), Q).reshape(2 * N, 2 * N)
    return xo, 0.5 * (Po + Po.T)


def anchor(x, P):
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    n = x.size
    N = (n - 3) // 2
    Q = _q(x[2])
    d = x[3:].reshape(N, 2) - x[0:2]
    Lp = d @ Q.T
    xo = np.zeros(n)
    xo[3:] = Lp.reshape(-1)
    A = np.empty((N, 2, 3))
    A[:, :, 0:2] = -Q
    A[:, :, 2] = -(d @ S.T) @ Q.T  # -Q S d
    PLR = P[3:, :3].reshape(N, 2, 3)
    W = np.einsum("ab,lbk->lak", Q, PLR) + 0.5 * np.einsum("laj,jk->lak", A, P[:3, :3])
    A2, W2 = A.reshape(2 * N, 3), W.reshape(2 * N, 3)
    Po = np.zeros((n, n))
    Po[3:, 3:] = _rotate_blocks(P[3:, 3:].reshape(N, 2, N, 2), Q).reshape(2 * N, 2 * N) + A2 @ W2.T + W2 @ A2.T
    return xo, 0.5 * (Po + Po.T)
