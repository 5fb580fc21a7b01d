"""Shared test helpers: the parity tolerance of BASELINE.json's north_star, made well-defined, and the scaffolding of the GPU tests of
the map operations (removal, frame change, joining, duplicate search, fusion, extraction): injected filters, immediate-call scripts,
window and stream probes, the reference of the submap extraction (NumPy indexing) and the contract of a duplicate list."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np

REL_TOL = 1e-6       # north_star: "within 1e-6 relative on x and P"
ABS_P = 1e-12        # element-wise floor relative to max|P|
ABS_X = 1e-9
FRO_TOL = 1e-9       # norm-wise bound, expected agreement is ~1e-12


def assert_state_close(xg, Pg, xo, Po, what=""):
    assert xg.shape == xo.shape and Pg.shape == Po.shape, (what, xg.shape, xo.shape)
    scale = max(np.abs(Po).max(), 1e-300)
    dx = np.abs(xg - xo)
    assert np.all(dx <= REL_TOL * np.abs(xo) + ABS_X), "%s x: max err %.3e" % (what, dx.max())
    dP = np.abs(Pg - Po)
    assert np.all(dP <= REL_TOL * np.abs(Po) + ABS_P * scale), "%s P: max err %.3e (scale %.3e)" % (what, dP.max(), scale)
    fro = np.linalg.norm(Pg - Po) / max(np.linalg.norm(Po), 1e-300)
    assert fro <= FRO_TOL, "%s P: relative Frobenius error %.3e" % (what, fro)
    return dx.max(), dP.max() / scale


def assert_bitwise_symmetric(P):
    assert np.array_equal(P, P.T)


def correlated_state(pkg, oc, copies=16, rho=0.8, seed=20260011, n_landmarks=64, steps=700):
    """A large, strongly correlated state of the kind SLAM really produces.  A config-1 style lifecycle
    (x = 0_3, P = 0, noisy odometry, New/Old/Ignore as they come) is run on the oracle until its map of
    N_s <= n_landmarks landmarks is correlated throughout via the robot; that filter is then tiled:
    copy c holds the same landmarks shifted by a 40 m grid offset, with

        P_RR = P_RR_s,   P_R,Lc = sqrt(rho) P_RL_s,   P_Lc,Ld = (rho + (1 - rho) [c == d]) P_LL_s.

    This is positive semidefinite for 0 <= rho <= 1 (Schur complement: (1-rho) I (x) P_LL_s +
    rho 11^T (x) (P_LL_s - P_LR_s P_RR_s^-1 P_RL_s)), every off-diagonal block is of the size of the
    diagonal blocks, and the robot sits among copy 0's landmarks, so measurements of those move every
    other copy through the cross-covariances.  Returns (x, P) with N_s * copies landmarks."""
    script = pkg.scenarios.lifecycle_script(seed=seed, n_landmarks=n_landmarks, steps=steps)
    S = oc.Session(np.zeros(3), np.zeros((3, 3)), capacity_landmarks=n_landmarks + 8)
    for st in script:
        S.propagate(st["v"], st["w"], oc.make_Q(st["v"]), st["dt"])
        for fx, fy in st["feats_mm"]:
            z, R = oc.make_measurement(fx, fy)
            S.update(z.reshape(2, 1), R)
    xs, Ps = S.state()
    Ns = (xs.size - 3) // 2
    n = 3 + 2 * Ns * copies
    x = np.empty(n)
    x[:3] = xs[:3]
    P = np.empty((n, n))
    P[:3, :3] = Ps[:3, :3]
    side = int(np.ceil(np.sqrt(copies)))
    for c in range(copies):
        off = np.tile([40.0 * (c % side), 40.0 * (c // side)], Ns)
        a = 3 + 2 * Ns * c
        x[a:a + 2 * Ns] = xs[3:] + off
        P[:3, a:a + 2 * Ns] = np.sqrt(rho) * Ps[:3, 3:]
        P[a:a + 2 * Ns, :3] = np.sqrt(rho) * Ps[3:, :3]
        for d in range(copies):
            b = 3 + 2 * Ns * d
            P[a:a + 2 * Ns, b:b + 2 * Ns] = (1.0 if c == d else rho) * Ps[3:, 3:]
    P = 0.5 * (P + P.T)
    return x, P


def assert_bitwise(a, b, what=""):
    """Two exported states (x, P), equal bit for bit."""
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, (what, a[0].shape, b[0].shape)
    assert np.array_equal(a[0], b[0]), "%s: x differs" % what
    dP = a[1] != b[1]
    assert not dP.any(), "%s: P differs at %d elements, first %s" % (what, int(dP.sum()), np.argwhere(dP)[:3].tolist())


def check_joint(r, ref, P, what):
    """Every field of a device record against a factor_ref result; returns the worst relative error seen."""
    import factor_ref as fr  # (beside this file; SciPy is needed by the tests that get here only)
    N = ref["n_landmarks"]
    assert int(r["n_landmarks"]) == N and int(r["info"]) == ref["info"], (what, int(r["n_landmarks"]), int(r["info"]), ref["info"])
    worst = 0.0
    for k in fr.FIELDS:
        got, want = float(r[k]), ref[k]
        if math.isnan(want):
            assert math.isnan(got), (what, k, got)
            continue
        if k.startswith("logdet"):
            err = abs(got - want)
            print("%s %s: |err| %.3e" % (what, k, err))
            assert err <= 1e-6 * (3 + 2 * N), (what, k, got, want)
            worst = max(worst, err / max(abs(want), 1.0))
        else:
            err = fr.rel_err(got, want) if want != 0.0 else abs(got)
            print("%s %s: rel %.3e" % (what, k, err))
            assert err <= REL_TOL, (what, k, got, want)
            worst = max(worst, err)
    S, Sr = r["cov_robot_given_map"], ref["cov_robot_given_map"]
    if np.isnan(Sr).all():
        assert np.isnan(S).all(), what
    else:
        dS = np.abs(S - Sr)
        print("%s cov_robot_given_map: max |err| %.3e" % (what, dS.max()))
        assert np.all(dS <= REL_TOL * np.abs(Sr) + ABS_P * np.abs(P).max()), (what, dS.max())
    return worst


def windows_closed(f):
    f.L.ekf_debug_windows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)]
    a, b = ctypes.c_longlong(), ctypes.c_int()
    assert f.L.ekf_debug_windows(f.h, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value


def stream_starts(f):
    f.L.ekf_debug_stream.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    a, b = ctypes.c_longlong(), ctypes.c_longlong()
    on = f.L.ekf_debug_stream(f.h, ctypes.byref(a), ctypes.byref(b))
    return on, a.value


def far_feature(pkg, k):
    """A feature well away from every landmark of the injected maps and from the other far features: a New landmark."""
    return pkg.scenarios.measurement_from_feature_mm(70000.0 + 9000.0 * (k % 7), -40000.0 + 11000.0 * (k // 7))


def run_steps(pkg, f, sc, s0, steps, M, new_every=0, k_new=0, oracle=None, oc=None):
    """Immediate calls on a one-filter handle: propagate, M Old-type measurements of the script, every `new_every`-th step a far
    feature (New).  Returns the decisions with their distances (and advances `oracle`, an oc.Session, the same way, asserting
    identical decisions)."""
    decs = []
    for s in range(s0, s0 + steps):
        v, w, dt = sc["ctrl"][s]
        f.propagate(v, w, dt)
        if oracle is not None:
            oracle.propagate(v, w, oc.make_Q(v), dt)
        meas = [(sc["z"][s, m], sc["R"][s, m].reshape(2, 2, order="F")) for m in range(M)]
        if new_every and s % new_every == 0:
            meas.append(far_feature(pkg, k_new))
            k_new += 1
        for z, R in meas:
            d = f.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2))[0][0]
            decs.append(d)
            if oracle is not None:
                od, om, _ = oracle.update(z.reshape(2, 1), R)
                assert (d[0], d[1]) == (od[0], om[0]), (s, d, od, om)
    return decs, k_new


def make_filter(pkg, N, cap, seed, extent=None, max_pending=16):
    """A one-filter handle loaded with the fixed-seed injected state of N landmarks."""
    x0, P0 = pkg.scenarios.injected_state(N, seed=seed, extent=extent or 12.0 * (N / 64.0) ** 0.5 + 8.0)
    f = pkg.FilterBatch(1, cap, max_pending=max_pending, log_capacity=4096)
    f.set_state(x0, P0)
    return f, x0, P0


def open_window_pair(pkg, N, cap, seed, steps, extent=None, M=2, max_pending=16):
    """Handles A and B after the same immediate calls (window open, streaming launch live on both) and their script; B is the witness
    whose export, counters and decisions say what A held in front of the call under test."""
    a, x0, _ = make_filter(pkg, N, cap, seed, extent, max_pending)
    b, _, _ = make_filter(pkg, N, cap, seed, extent, max_pending)
    sc = pkg.scenarios.steady_script(x0, steps=steps, M=M, seed=seed + 1, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc, 0, steps, M)
    db, _ = run_steps(pkg, b, sc, 0, steps, M)
    assert da == db
    return a, b, sc


def batch_script(pkg, B, steps, M):
    """A script for B filters: measurement 0 near the robot (Old or New as it falls), the others far features (New)."""
    ctrl = np.tile(np.array([0.3, 0.05, 0.05]), (steps, B, 1))
    z = np.empty((steps, M, B, 2))
    R = np.empty((steps, M, B, 4))
    for s in range(steps):
        for m in range(M):
            for b in range(B):
                if m == 0:
                    zz, RR = pkg.scenarios.measurement_from_feature_mm(3000.0 + 37.0 * ((b + s) % 11), 800.0 - 53.0 * ((b * 3 + s) % 7))
                else:
                    zz, RR = far_feature(pkg, s + 3 * b % 5)
                z[s, m, b], R[s, m, b] = zz, RR.ravel(order="F")
    return ctrl, z, R


def run_cpp_check(tmp_path, name):
    """tests/cpp/<name>.cpp compiled for the host into tmp_path and run: the finished process, for the caller to assert on."""
    exe = str(tmp_path / name)
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", name + ".cpp")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-o", exe, src])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@functools.lru_cache(maxsize=None)
def gpu_present():
    """torch.cuda.is_available(), asked in a child process.  torch's HIP runtime is requested as libamdhip64.so, the library's as
    libamdhip64.so.7: once the library is loaded, torch initialised in the same process is a second runtime, and the library's then
    finds no device for every later test of the session."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(int(torch.cuda.is_available()))"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split()[-1] == "1"


# ---- submap extraction: the reference is indexing --------------------------------------------------------
def sel_of(ids):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    return np.concatenate([np.arange(3), np.stack([3 + 2 * ids, 4 + 2 * ids], axis=1).reshape(-1)]).astype(np.int64)


def index_state(state, ids):
    """The reference of ekf_extract_map / ekf_get_submap: rows and columns of an exported state (ids None: every landmark)."""
    x, P = state
    s = np.arange(x.size) if ids is None else sel_of(ids)
    return x[s].copy(), P[np.ix_(s, s)].copy()


def shuffled_ids(N, count, seed):
    """`count` distinct landmarks of N in shuffled order, the tile edges 0, 31, 32, 63, 64 and the last landmark among them."""
    rng = np.random.default_rng(seed)
    must = sorted({l for l in (0, 31, 32, 63, 64, N - 1) if 0 <= l < N})[:count]
    rest = [l for l in rng.permutation(N) if l not in must][:count - len(must)]
    ids = np.array(must + rest, dtype=np.int32)
    rng.shuffle(ids)
    assert ids.size == count and np.unique(ids).size == count
    return ids


# ---- duplicate search: the contract of a list against tests/dup_ref.py -------------------------------------
MARGIN = 1e-3  # no pair of a compared list within this (relative) of the gate or of max_dist


def ij(pairs):
    return list(zip(pairs["i"].tolist(), pairs["j"].tolist()))


def check_duplicates(got, x, P, gate=9.21, max_dist=None, split=0, what=""):
    """A device result (pairs, n_found, n_degenerate) against the reference on the export (x, P); returns the worst d2 error."""
    import dup_ref as dr  # (beside this file)
    pairs, found, degen = got
    m_gate, m_dist = dr.margins(x, P, gate, max_dist, split)
    assert m_gate > MARGIN and m_dist > MARGIN, (what, "the reference has a pair on the edge: another seed", m_gate, m_dist)
    ref, ref_degen = dr.find(x, P, gate, max_dist, split)
    assert found == len(ref) and degen == ref_degen, (what, found, len(ref), degen, ref_degen)
    assert ij(pairs) == ij(ref)[:len(pairs)], (what, ij(pairs), ij(ref))
    if len(pairs) == 0:
        return 0.0
    err = np.abs(pairs["d2"] - ref["d2"][:len(pairs)])
    assert np.all(err <= REL_TOL * np.abs(ref["d2"][:len(pairs)]) + 1e-9), (what, err.max())
    return float((err / np.maximum(np.abs(ref["d2"][:len(pairs)]), 1e-9)).max())
