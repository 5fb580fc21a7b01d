"""Whole-state consistency on the device: ekf_joint_consistency / ekf_batch_joint_consistency (joint and map NEES, log det P, the
pivots of the factorisation of P_LL, the pose covariance conditioned on the map) and ekf_debug_joint_factor.  The reference is
tests/factor_ref.py (LAPACK on the dense export; checked on the CPU in tests/test_joint_consistency_cpu.py).  Tolerances are the
project's own: REL_TOL on the NEES values, the pivots and the conditioned pose covariance (with the floor ABS_P max|P|),
1e-6 (3 + 2N) absolute on the log-determinants (sums of 2N logs of values held to REL_TOL), REL_TOL |U_ref| + ABS_P max|U| on the
factor.  The observed errors are printed; they are expected around 1e-15 .. 1e-12.  The call only reads the filter: a witness handle
that exported at the same point stays bit for bit the same, before and after more steps."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ref as fr  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import (ABS_P, REL_TOL, assert_bitwise, batch_script, check_joint as check, correlated_state, far_feature,  # noqa: E402
                     make_filter, open_window_pair, run_steps, stream_starts)

pytestmark = pytest.mark.gpu

# partial tile, exactly one tile, two tiles with one landmark in the second; T = 4: the first size with an off-diagonal trailing
# tile; the several-workgroup and the one-workgroup chain kernel
CASES = [(31, 64), (32, 64), (33, 64), (100, 128), (280, 320), (180, 200)]
NAN_OK = ("nees_map", "nees_joint", "logdet_map", "logdet_joint")


def truth_for(x, P, seed):
    """x_true = x + L xi, its heading a full turn away (the error's heading component is wrapped)."""
    xt = fr.draw_truth(x, P, seed)
    xt[2] += 2.0 * math.pi
    return xt


# ---- 1. parity with a window open -------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", CASES)
def test_parity_with_a_window_open(pkg, pipeline_mode, N, cap):
    a, b, _ = open_window_pair(pkg, N, cap, seed=11, steps=5)
    x, P = b.get_state()
    xt = truth_for(x, P, seed=100 + N)
    r = a.joint_consistency(xt, 0)[0]
    ref = fr.lapack(x, P, xt)
    assert ref["info"] == 0
    worst = check(r, ref, P, "N=%d" % N)
    print("N=%d: worst relative error %.3e" % (N, worst))
    assert a.joint_consistency(xt, 0).tobytes() == r.tobytes()  # an unchanged state: the same bits
    a.close(), b.close()


# ---- 2. the factor ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", CASES)
def test_the_factor(pkg, pipeline_mode, N, cap):
    a, b, _ = open_window_pair(pkg, N, cap, seed=21, steps=5)
    x, P = b.get_state()
    assert int(a.joint_consistency(None, 0)[0]["info"]) == 0
    U = a.joint_factor(0)
    Ur = scipy.linalg.cholesky(P[3:, 3:], lower=False)
    assert U.shape == Ur.shape == (2 * N, 2 * N)
    dU = np.abs(U - Ur)
    res = np.abs(U.T @ U - P[3:, 3:]).max()
    print("N=%d: max |U - U_ref| %.3e, max |U^T U - P_LL| %.3e (max |P_LL| %.3e)" % (N, dU.max(), res, np.abs(P[3:, 3:]).max()))
    assert np.all(dU <= REL_TOL * np.abs(Ur) + ABS_P * np.abs(Ur).max())
    assert res <= REL_TOL * np.abs(P[3:, 3:]).max()
    assert not np.tril(U, -1).any()  # exactly zero below the diagonal
    a.close(), b.close()


# ---- 3. read-only, and the twin -----------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", [(33, 64), (100, 128), (280, 320), (180, 200)])
def test_the_filter_is_only_read(pkg, pipeline_mode, N, cap):
    a, b, _ = open_window_pair(pkg, N, cap, seed=31, steps=5)
    on, starts0 = stream_starts(a)
    x, P = b.get_state()  # B exports at the point where A is assessed
    xt = truth_for(x, P, seed=3)
    r = a.joint_consistency(xt, 0)[0]
    assert int(r["info"]) == 0
    assert a.stats() == b.stats() and a.decisions() == b.decisions() and np.array_equal(a.poses(), b.poses())
    assert np.array_equal(a.robot_cov(), b.robot_cov()) and np.array_equal(a.num_landmarks(), b.num_landmarks())
    assert_bitwise(a.get_state(), (x, P), "after the call")
    sc2 = pkg.scenarios.steady_script(x, steps=12, M=2, seed=34, min_separation=1.0)
    da, ka = run_steps(pkg, a, sc2, 0, 12, 2, new_every=2)
    db, kb = run_steps(pkg, b, sc2, 0, 12, 2, new_every=2)
    assert da == db and ka == kb == 6 and int(a.num_landmarks()[0]) >= N + 6
    if on:
        assert stream_starts(a)[1] > starts0  # immediate-mode calls stream again
    with pytest.raises(pkg.EkfError) as ei:  # the state has changed since the factor was made
        a.joint_factor(0)
    assert ei.value.code == pkg.ekfslam.ERR_STATE
    xb, Pb = b.get_state()
    r2 = a.joint_consistency(truth_for(xb, Pb, seed=4), 0)[0]
    check(r2, fr.lapack(xb, Pb, truth_for(xb, Pb, seed=4)), Pb, "N=%d after 12 more steps" % N)
    assert a.joint_factor(0).shape == (len(xb) - 3, len(xb) - 3)
    assert_bitwise(a.get_state(), (xb, Pb), "after 12 more steps")
    assert a.stats() == b.stats() and a.decisions() == b.decisions()
    a.close(), b.close()


# ---- 4. a correlated state ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def correlated(pkg, oc):
    x, P = correlated_state(pkg, oc, copies=4, n_landmarks=24, steps=400)
    xt = truth_for(x, P, seed=41)
    return x, P, xt, fr.lapack(x, P, xt)


def test_correlated_state(pkg, pipeline_mode, correlated):
    x, P, xt, ref = correlated
    N = (len(x) - 3) // 2
    f = pkg.FilterBatch(1, 288)
    f.set_state(x, P)
    r = f.joint_consistency(xt, 0)[0]
    print("correlated state: N = %d, cond %.2e" % (N, np.linalg.cond(P)))
    assert ref["info"] == 0 and N > 32
    print("worst relative error %.3e" % check(r, ref, P, "correlated N=%d" % N))
    kf = pkg.KalmanFilter(capacity_landmarks=288)
    kf.set_state(x, P)
    assert kf.joint_consistency(xt).tobytes() == r.tobytes()  # the mirror class: one record, the same bits
    f.close(), kf._f.close()


# ---- 5. edge cases of info ----------------------------------------------------------------------------
def test_a_fresh_filter(pkg, pipeline_mode):
    f = pkg.FilterBatch(1, 64)
    r = f.joint_consistency(np.array([0.1, -0.2, 0.3]), 0)[0]
    assert int(r["n_landmarks"]) == 0 and int(r["info"]) == -1
    assert r["nees_map"] == 0.0 and r["logdet_map"] == 0.0 and r["min_pivot"] == 0.0 and r["max_pivot"] == 0.0
    assert math.isnan(r["nees_joint"]) and math.isnan(r["logdet_joint"])
    assert not r["cov_robot_given_map"].any()
    x = np.array([1.0, -2.0, 0.4])  # a pose covariance, no map: the joint fields come from P_RR alone
    P = np.array([[0.04, 0.01, -0.002], [0.01, 0.03, 0.004], [-0.002, 0.004, 0.01]])
    f.set_state(x, P)
    xt = x + np.array([0.1, -0.2, 0.05])
    r = f.joint_consistency(xt, 0)[0]
    check(r, fr.lapack(x, P, xt), P, "N=0 with a pose covariance")
    assert int(r["info"]) == 0 and np.array_equal(r["cov_robot_given_map"], P)
    f.close()


def test_an_anchored_filter(pkg, pipeline_mode):
    f, _, _ = make_filter(pkg, 100, 128, seed=51)
    f.anchor_at_robot(index=0)
    x, P = f.get_state()
    xt = x.copy()
    xt[3:] = fr.draw_truth(x[3:], P[3:, 3:], seed=52)
    r = f.joint_consistency(xt, 0)[0]
    ref = fr.lapack(x, P, xt)
    assert ref["info"] == -1 and math.isfinite(ref["nees_map"]) and math.isfinite(ref["logdet_map"])
    check(r, ref, P, "anchored")
    f.close()


def test_a_zeroed_landmark_is_reported_not_raised(pkg, pipeline_mode):
    x, P = pkg.scenarios.injected_state(100, seed=53, extent=23.0)
    a = 3 + 2 * 40
    P[a:a + 2, :] = 0.0
    P[:, a:a + 2] = 0.0
    f = pkg.FilterBatch(1, 128)
    f.set_state(x, P)
    r = f.joint_consistency(x, 0)[0]  # (EKF_OK: no exception)
    ref = fr.tiled(x, P, x)
    assert int(r["info"]) == 81 == ref["info"] == fr.potrf_info(P[3:, 3:])
    for k in NAN_OK:
        assert math.isnan(r[k]), k
    assert r["min_pivot"] == ref["min_pivot"] == 0.0
    assert np.isnan(r["cov_robot_given_map"]).all()
    assert_bitwise(f.get_state(), (x, P), "after the call")
    f.propagate(0.3, 0.05, 0.05)
    z, R = far_feature(pkg, 0)
    d = f.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2))[0][0]
    assert d[0] in (pkg.ekfslam.NEW, pkg.ekfslam.OLD, pkg.ekfslam.IGNORE) and int(f.num_landmarks()[0]) >= 100  # the filter works on
    f.close()


def test_without_truth(pkg, pipeline_mode):
    f, x, P = make_filter(pkg, 33, 64, seed=54)
    r = f.joint_consistency(None, 0)[0]
    ref = fr.lapack(x, P, None)
    assert math.isnan(r["nees_map"]) and math.isnan(r["nees_joint"])
    check(r, ref, P, "no truth")
    rb = f.joint_consistency()[0]  # the batch form of a batch of one
    assert rb.tobytes() == r.tobytes()
    f.close()


def test_bad_arguments_leave_the_handle_untouched(pkg, pipeline_mode):
    E = pkg.ekfslam
    f, x, P = make_filter(pkg, 33, 64, seed=55)
    out = (E.EkfJoint * 1)()
    xt = np.ascontiguousarray(x)
    assert f.L.ekf_joint_consistency(f.h, 1, xt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out) == E.ERR_BAD_ARG
    assert f.L.ekf_joint_consistency(f.h, -1, None, out) == E.ERR_BAD_ARG
    assert f.L.ekf_joint_consistency(f.h, 0, None, None) == E.ERR_BAD_ARG
    assert f.L.ekf_batch_joint_consistency(f.h, None, 0, None) == E.ERR_BAD_ARG
    assert f.L.ekf_batch_joint_consistency(f.h, xt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(x) - 1, out) == E.ERR_BAD_ARG
    assert f.L.ekf_debug_joint_factor(f.h, 0, None, 0) == E.ERR_STATE  # no factor yet
    assert f.L.ekf_debug_joint_factor(f.h, 3, None, 0) == E.ERR_BAD_ARG
    assert_bitwise(f.get_state(), (x, P), "after the refused calls")
    check(f.joint_consistency(x, 0)[0], fr.lapack(x, P, x), P, "after the refused calls")
    U = np.zeros((66, 66))
    assert f.L.ekf_debug_joint_factor(f.h, 0, U.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 65) == E.ERR_BAD_ARG  # ld < 2N
    f.close()


# ---- 6. batches ------------------------------------------------------------------------------------------
def test_batch_equals_the_single_calls(pkg, pipeline_mode):
    f = pkg.FilterBatch(3, 128)
    states = [(np.zeros(3), np.zeros((3, 3)))]
    for b, N in ((1, 5), (2, 70)):
        x, P = pkg.scenarios.injected_state(N, seed=60 + b, extent=15.0)
        f.set_state(x, P, index=b)
        states.append((x, P))
    ld = 3 + 2 * 70
    xt = np.zeros((3, ld))
    xt[0, :3] = (0.1, 0.2, 0.3)
    for b in (1, 2):
        xt[b, :len(states[b][0])] = truth_for(*states[b], seed=63 + b)
    rows = f.joint_consistency(xt).copy()
    for b in range(3):
        one = f.joint_consistency(xt[b, :len(states[b][0])], b)[0]
        assert one.tobytes() == rows[b].tobytes(), b
        check(rows[b], fr.lapack(states[b][0], states[b][1], xt[b, :len(states[b][0])]), states[b][1], "filter %d" % b)
    assert [int(v) for v in rows["info"]] == [-1, 0, 0] and [int(v) for v in rows["n_landmarks"]] == [0, 5, 70]
    assert f.joint_factor(2).shape == (140, 140)  # (the last call covered filter 2 alone)
    with pytest.raises(pkg.EkfError):
        f.joint_factor(1)
    rep = pkg.montecarlo.joint_consistency_report(rows)
    assert rep["skipped"] == 1 and rep["joint"]["dof"] == 13 + 143 and rep["map"]["dof"] == 10 + 140
    f.close()


def test_batch_after_a_scripted_run_with_a_window_open(pkg, pipeline_mode):
    B, cap = 4, 64
    f, g = pkg.FilterBatch(B, cap), pkg.FilterBatch(B, cap)
    ctrl, z, R = batch_script(pkg, B, 6, 2)
    for h in (f, g):
        h.script_load(ctrl, z, R)
        h.script_run(0, 3)
    states = [g.get_state(b) for b in range(B)]
    ld = max(len(s[0]) for s in states)
    xt = np.zeros((B, ld))
    for b in range(B):
        xt[b, :len(states[b][0])] = truth_for(*states[b], seed=70 + b)
    rows = f.joint_consistency(xt)
    for b in range(B):
        assert int(rows[b]["n_landmarks"]) >= 1
        check(rows[b], fr.lapack(states[b][0], states[b][1], xt[b, :len(states[b][0])]), states[b][1], "scripted filter %d" % b)
    for h in (f, g):
        h.script_run(3, 3)
    for b in range(B):
        assert_bitwise(f.get_state(b), g.get_state(b), "filter %d after the rest of the script" % b)
    assert f.stats() == g.stats()
    f.close(), g.close()


# ---- 7. after the other map operations -----------------------------------------------------------------
def test_after_removal_frame_change_and_join(pkg, pipeline_mode):
    f, x0, P0 = make_filter(pkg, 100, 128, seed=71)
    xt0 = truth_for(x0, P0, seed=72)
    r0 = f.joint_consistency(xt0, 0)[0]
    check(r0, fr.lapack(x0, P0, xt0), P0, "before")
    frame = (3.0, -2.0, 0.7)
    f.transform_frame(frame, index=0)
    xt1 = rr.rigid(xt0, P0, frame)[0]
    r1 = f.joint_consistency(xt1, 0)[0]
    x1, P1 = f.get_state()
    check(r1, fr.lapack(x1, P1, xt1), P1, "after a rigid transform")
    # a rigid transform is volume-preserving and moves estimate and truth alike: log det P and the joint NEES do not change
    print("rigid transform: logdet_joint %.3e, nees_joint rel %.3e" % (abs(r1["logdet_joint"] - r0["logdet_joint"]), fr.rel_err(r1["nees_joint"], r0["nees_joint"])))
    assert abs(r1["logdet_joint"] - r0["logdet_joint"]) <= 1e-6 * 203 and abs(r1["logdet_map"] - r0["logdet_map"]) <= 1e-6 * 203
    assert fr.rel_err(r1["nees_joint"], r0["nees_joint"]) <= REL_TOL and fr.rel_err(r1["nees_map"], r0["nees_map"]) <= REL_TOL
    keep = np.ones(100, dtype=bool)
    keep[[0, 17, 31, 32, 63, 64, 99]] = False
    assert f.remove_landmarks(keep, index=0) == 93
    x2, P2 = f.get_state()
    xt2 = truth_for(x2, P2, seed=73)
    check(f.joint_consistency(xt2, 0)[0], fr.lapack(x2, P2, xt2), P2, "after a removal")
    src, _, _ = make_filter(pkg, 20, 64, seed=74)
    assert f.join_map(src, index=0, src_index=0) == 113
    x3, P3 = f.get_state()
    xt3 = truth_for(x3, P3, seed=75)
    check(f.joint_consistency(xt3, 0)[0], fr.lapack(x3, P3, xt3), P3, "after a join")
    f.close(), src.close()


# ---- 8. after a growth of the capacity ------------------------------------------------------------------
def test_after_reserve(pkg, pipeline_mode):
    f, x, P = make_filter(pkg, 100, 128, seed=81)
    xt = truth_for(x, P, seed=82)
    bytes0 = f.device_bytes()
    ref = fr.lapack(x, P, xt)
    check(f.joint_consistency(xt, 0)[0], ref, P, "capacity 128")
    bytes1 = f.device_bytes()
    assert bytes1 > bytes0  # the scratch is counted
    f.reserve(300)
    assert f.device_bytes() > bytes1  # ... and has followed the capacity
    with pytest.raises(pkg.EkfError) as ei:
        f.joint_factor(0)  # (the old factor went with the old buffers)
    assert ei.value.code == pkg.ekfslam.ERR_STATE
    bytes2 = f.device_bytes()
    check(f.joint_consistency(xt, 0)[0], ref, P, "capacity 300")
    assert f.device_bytes() == bytes2  # no second allocation
    Ur = scipy.linalg.cholesky(P[3:, 3:], lower=False)
    assert np.all(np.abs(f.joint_factor(0) - Ur) <= REL_TOL * np.abs(Ur) + ABS_P * np.abs(Ur).max())
    assert_bitwise(f.get_state(), (x, P), "after the growth and the call")
    f.close()
