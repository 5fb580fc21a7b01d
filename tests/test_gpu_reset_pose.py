"""ekf_reset_pose and its batch form on the device: the pose replaced, P_RR the symmetrised input, every robot-landmark block exactly
+0.0, P_LL and the landmarks of x bit for bit; the host mirror; behind an open window; on a filter without landmarks; and the claim
that every device buffer ends as ekf_set_state of the result would leave it -- a following propagate + update step equals the same
step on a handle loaded by ekf_set_state with the reset state, bit for bit.  The reference is locate_ref.reset_pose (NumPy: set the
pose block, zero the cross blocks).  The map sizes lie either side of the kernel's workgroup of 256 columns (3 + 2 N of them).
No test keeps more than two handles open at a time, and the module's name sorts behind tests/test_gpu_configs.py: the docstring of
tests/test_gpu_gate_candidates.py says why."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_ref as lr  # noqa: E402
from helpers import assert_bitwise, make_filter, open_window_pair, run_steps, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

POSE = np.array([1.25, -0.5, 0.7])
P_RR = np.array([[0.04, 0.002, -0.001], [0.004, 0.05, 0.0005], [0.001, 0.0015, 0.01]])   # not symmetric: the call averages


def assert_reset(after, before, pose, P_RR, what):
    x, P = after
    want = lr.reset_pose(before[0], before[1], pose, P_RR)
    assert_bitwise(after, want, what)
    assert not np.signbit(P[:3, 3:]).any() and not np.signbit(P[3:, :3]).any(), what   # +0.0, not -0.0
    assert np.array_equal(P[:3, :3], P[:3, :3].T) and P[0, 1] == 0.5 * (P_RR[0][1] + P_RR[1][0]), what
    assert np.array_equal(x[3:], before[0][3:]) and np.array_equal(P[3:, 3:], before[1][3:, 3:]), what


# the columns of the robot rows: 3 + 2 N = 255, 257 either side of one workgroup; 511, 513, 515 of two; a tile edge; one landmark
@pytest.mark.parametrize("N,cap", [(126, 128), (127, 128), (254, 256), (255, 256), (256, 256), (64, 64), (1, 8)])
def test_reset_against_the_reference(pkg, pipeline_mode, N, cap):
    f, x0, P0 = make_filter(pkg, N, cap, seed=2100 + N)
    st, dec = f.stats(), f.decisions()
    before = f.get_state()
    assert np.abs(before[1][:3, 3:]).max() > 0.0   # there is a correlation to cut
    f.reset_pose(POSE, P_RR)
    assert_reset(f.get_state(), before, POSE, P_RR, "N=%d" % N)
    assert f.stats() == st and f.decisions() == dec
    assert np.array_equal(f.poses()[0], POSE)   # the host mirror
    assert np.array_equal(f.robot_cov(), lr.reset_pose(*before, POSE, P_RR)[1][:3, :3])
    f.reset_pose(POSE + 1.0, np.zeros((3, 3)))   # a known pose
    x, P = f.get_state()
    assert np.array_equal(x[:3], POSE + 1.0) and not P[:3, :].any() and not P[:, :3].any()
    f.close()


def test_reset_on_a_filter_without_landmarks(pkg, pipeline_mode):
    f = pkg.FilterBatch(1, 8, max_pending=8, log_capacity=64)
    f.reset_pose(POSE, P_RR)
    x, P = f.get_state()
    assert x.tolist() == POSE.tolist() and np.array_equal(P, lr.reset_pose(np.zeros(3), np.zeros((3, 3)), POSE, P_RR)[1])
    f.propagate(0.3, 0.05, 0.1)
    assert f.num_landmarks()[0] == 0 and np.isfinite(f.get_state()[1]).all()
    f.close()


def test_reset_behind_an_open_window(pkg, pipeline_mode):
    a, b, sc = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    w0 = windows_closed(a)
    before = b.get_state()   # (the witness folds its own window for the export)
    st, dec = a.stats(), a.decisions()
    a.reset_pose(POSE, P_RR)
    assert 0 <= windows_closed(a) - w0 <= 1   # the deferred slots were folded first, as ekf_transform_frame folds them
    assert_reset(a.get_state(), before, POSE, P_RR, "behind an open window")
    assert a.stats() == st and a.decisions() == dec
    a.close(), b.close()


@pytest.mark.parametrize("N,cap", [(100, 200), (200, 320)])
def test_every_buffer_ends_as_set_state_would_leave_it(pkg, pipeline_mode, N, cap):
    """k_solo and k_chain: the immediate calls that follow read x, the robot rows, D and the tiles; a stale copy would show."""
    a, x0, _ = make_filter(pkg, N, cap, seed=2300 + N)
    sc = pkg.scenarios.steady_script(x0, steps=4, M=2, seed=2301 + N, min_separation=1.0)
    run_steps(pkg, a, sc, 0, 2, 2)   # a window open, slots in use
    pose = a.get_x()[:3] + np.array([0.02, -0.01, 0.005])   # near enough for the script's measurements to stay Old
    a.reset_pose(pose, P_RR)
    b = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    b.set_state(*a.get_state())
    da, _ = run_steps(pkg, a, sc, 2, 2, 2)
    db, _ = run_steps(pkg, b, sc, 2, 2, 2)
    assert da == db and any(d[0] == pkg.ekfslam.OLD for d in da)
    assert_bitwise(a.get_state(), b.get_state(), "the steps behind the reset against the steps behind set_state")
    a.close(), b.close()


def test_batch_form_against_the_one_filter_calls(pkg, pipeline_mode):
    counts = (257, 0, 33, 64)
    f = pkg.FilterBatch(4, 320, max_pending=8, log_capacity=256)
    g = pkg.FilterBatch(1, 320, max_pending=8, log_capacity=256)
    states = [pkg.scenarios.injected_state(n, seed=2400 + b, extent=10.0 + b) if n else (np.zeros(3), np.zeros((3, 3))) for b, n in enumerate(counts)]
    for b, (x, P) in enumerate(states):
        if counts[b]:
            f.set_state(x, P, index=b)
    poses = np.stack([POSE + b for b in range(4)])
    covs = np.stack([P_RR * (1.0 + b) for b in range(4)])
    f.reset_pose(poses, covs, index=None)
    assert np.array_equal(f.poses(), poses) and list(f.num_landmarks()) == list(counts)
    for b, (x, P) in enumerate(states):
        assert_reset(f.get_state(b), (x, P), poses[b], covs[b], "filter %d" % b)
        g.set_state(x, P)
        g.reset_pose(poses[b], covs[b])
        assert_bitwise(f.get_state(b), g.get_state(), "filter %d against the one-filter call" % b)
    f.reset_pose(POSE, P_RR, index=2)   # one filter of a batch: the others stay
    assert np.array_equal(f.poses()[[0, 1, 3]], poses[[0, 1, 3]]) and np.array_equal(f.poses()[2], POSE)
    f.close(), g.close()


def test_bad_arguments_and_sticky_statuses(pkg, pipeline_mode):
    f, x0, _ = make_filter(pkg, 8, 8, seed=73)
    L, E = f.L, pkg.ekfslam
    dp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    before = f.get_state()
    bad_pose, bad_cov, neg = POSE.copy(), P_RR.copy(), P_RR.copy()
    bad_pose[1], bad_cov[2, 0], neg[1, 1] = np.nan, np.inf, -1e-12
    for index, p, c in ((0, bad_pose, P_RR), (0, POSE, bad_cov), (0, POSE, neg), (1, POSE, P_RR), (-1, POSE, P_RR)):
        assert L.ekf_reset_pose(f.h, index, dp(p), dp(c)) == E.ERR_BAD_ARG
    assert L.ekf_reset_pose(f.h, 0, None, dp(P_RR)) == E.ERR_BAD_ARG and L.ekf_reset_pose(f.h, 0, dp(POSE), None) == E.ERR_BAD_ARG
    assert L.ekf_reset_pose(None, 0, dp(POSE), dp(P_RR)) == E.ERR_BAD_ARG and L.ekf_batch_reset_pose(f.h, None, dp(P_RR)) == E.ERR_BAD_ARG
    assert L.ekf_batch_reset_pose(f.h, dp(bad_pose), dp(P_RR)) == E.ERR_BAD_ARG
    for kw in (dict(pose=bad_pose, P_RR=P_RR), dict(pose=POSE, P_RR=neg), dict(pose=POSE[:2], P_RR=P_RR), dict(pose=POSE, P_RR=P_RR[:2])):
        with pytest.raises(ValueError):
            f.reset_pose(**kw)
    assert_bitwise(f.get_state(), before, "behind the refused calls")
    zf, Rf = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    f.update(zf.reshape(1, 1, 2), Rf.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room: a sticky EKF_ERR_CAPACITY
    assert L.ekf_reset_pose(f.h, 0, dp(POSE), dp(P_RR)) == E.ERR_CAPACITY
    f.set_state(*before)   # the way out
    f.reset_pose(POSE, P_RR)
    assert_reset(f.get_state(), before, POSE, P_RR, "behind set_state")
    f.close()
