"""NumPy reference of map joining (ekf_join_map): a local map `s`, whose frame origin is the destination's estimated robot pose, is
appended to the destination `g`; the two estimates are independent.

    dst: pose p = (t, phi), landmarks L_m, covariance Pg        src: pose q = (u, psi), landmarks M_k, covariance Ps
    L_m' = L_m        M_k' = t + C M_k  (landmark Ng + k)        t' = t + C u,  phi' = phi + psi        C = Rot(phi)

`join` builds the dense Jacobian of that map on the stacked state [xg; xs], forms J blockdiag(Pg, Ps) J^T and drops nothing but
the old pose (the map has no output for it).  `join_blocks` writes the same result block by block, as include/ekfslam_c.h states
it and the kernels compute it; tests/test_join_map_cpu.py checks the one against the other and the Jacobian against central
differences.  cos / sin are math.cos / math.sin, the two numbers the library takes on the host.  Output order: [robot (3), old
landmarks, new landmarks]."""
import math

import numpy as np

JM = np.array([[0.0, -1.0], [1.0, 0.0]])


def _rot(phi, dtype=np.float64):
    c, s = math.cos(phi), math.sin(phi)  # (float64 in every dtype)
    return np.array([[c, -s], [s, c]], dtype=dtype)


# (dtype=np.longdouble: the same expressions carried in extended precision -- the yardstick of the float64 results)
def join_g(xg, xs, dtype=np.float64):
    """The map itself on the two state vectors."""
    xg, xs = np.asarray(xg, dtype=dtype), np.asarray(xs, dtype=dtype)
    C, t = _rot(float(xg[2]), dtype), xg[0:2]
    Ng, Ns = (xg.size - 3) // 2, (xs.size - 3) // 2
    out = np.empty(3 + 2 * (Ng + Ns), dtype=dtype)
    out[0:2] = t + C @ xs[0:2]
    out[2] = xg[2] + xs[2]
    out[3:3 + 2 * Ng] = xg[3:]
    out[3 + 2 * Ng:] = (t + xs[3:].reshape(Ns, 2) @ C.T).reshape(-1)
    return out


def join_J(xg, xs, dtype=np.float64):
    """d join_g / d [xg; xs]: (3 + 2 (Ng + Ns)) x (len(xg) + len(xs))."""
    xg, xs = np.asarray(xg, dtype=dtype), np.asarray(xs, dtype=dtype)
    ng, ns = xg.size, xs.size
    Ng, Ns = (ng - 3) // 2, (ns - 3) // 2
    C = _rot(float(xg[2]), dtype)
    Jm = JM.astype(dtype)
    J = np.zeros((3 + 2 * (Ng + Ns), ng + ns), dtype=dtype)
    # robot: t + C u, phi + psi
    J[0:2, 0:2] = np.eye(2)
    J[0:2, 2] = C @ Jm @ xs[0:2]
    J[0:2, ng:ng + 2] = C
    J[2, 2] = 1.0
    J[2, ng + 2] = 1.0
    # old landmarks
    J[3:3 + 2 * Ng, 3:ng] = np.eye(2 * Ng)
    # new landmarks: t + C M_k
    for k in range(Ns):
        r = 3 + 2 * (Ng + k)
        J[r:r + 2, 0:2] = np.eye(2)
        J[r:r + 2, 2] = C @ Jm @ xs[3 + 2 * k:5 + 2 * k]
        J[r:r + 2, ng + 3 + 2 * k:ng + 5 + 2 * k] = C
    return J


def join(xg, Pg, xs, Ps, dtype=np.float64):
    """(x', P') through the dense Jacobian."""
    xg, xs = np.asarray(xg, dtype=dtype), np.asarray(xs, dtype=dtype)
    Pg, Ps = np.asarray(Pg, dtype=dtype), np.asarray(Ps, dtype=dtype)
    ng, ns = xg.size, xs.size
    big = np.zeros((ng + ns, ng + ns), dtype=dtype)
    big[:ng, :ng] = Pg
    big[ng:, ng:] = Ps
    J = join_J(xg, xs, dtype)
    P = J @ big @ J.T
    return join_g(xg, xs, dtype), 0.5 * (P + P.T)


def join_blocks(xg, Pg, xs, Ps):
    """The block table: old x old untouched, every new column a rank-3 product of the destination's robot rows plus the rotated
    source block.  Joining into x = 0_3, P = 0 returns the source bit for bit, joining x = 0_3, P = 0 the destination."""
    xg, xs = np.asarray(xg, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    Pg, Ps = np.asarray(Pg, dtype=np.float64), np.asarray(Ps, dtype=np.float64)
    Ng, Ns = (xg.size - 3) // 2, (xs.size - 3) // 2
    C = _rot(xg[2])
    C3 = np.eye(3)
    C3[0:2, 0:2] = C
    GR = np.eye(3)
    GR[0:2, 2] = C @ JM @ xs[0:2]
    G = np.zeros((2 * Ns, 3))  # the G_k stacked
    G[0::2, 0] = 1.0
    G[1::2, 1] = 1.0
    G[:, 2] = (xs[3:].reshape(Ns, 2) @ (C @ JM).T).reshape(-1)
    Cs = np.kron(np.eye(Ns), C)  # blockdiag(C, ..., C)
    PRR, PLR = Pg[:3, :3], Pg[3:, :3]
    n = 3 + 2 * (Ng + Ns)
    a = 3 + 2 * Ng
    P = np.empty((n, n))
    P[3:a, 3:a] = Pg[3:, 3:]
    P[3:a, a:] = PLR @ G.T
    P[a:, 3:a] = P[3:a, a:].T
    P[a:, a:] = G @ PRR @ G.T + Cs @ Ps[3:, 3:] @ Cs.T
    P[3:a, :3] = PLR @ GR.T
    P[a:, :3] = G @ PRR @ GR.T + Cs @ Ps[3:, :3] @ C3.T
    P[:3, 3:] = P[3:, :3].T
    P[:3, :3] = GR @ PRR @ GR.T + C3 @ Ps[:3, :3] @ C3.T
    P = 0.5 * (P + P.T)
    P[3:a, 3:a] = Pg[3:, 3:]  # (exactly, whatever the symmetry of the input)
    return join_g(xg, xs), P


def central_difference(g, x, h=1e-6):
    n = len(x)
    cols = []
    for k in range(n):
        e = np.zeros(n)
        e[k] = h
        cols.append((g(x + e) - g(x - e)) / (2.0 * h))
    return np.stack(cols, axis=1)
