"""Frame changes on the device: ekf_transform_frame (a known rigid transform of the whole estimate) and ekf_anchor_at_robot (the map
re-expressed relative to the estimated pose, the pose uncertainty moved into the landmarks), single and batch forms.  The reference
is tests/reframe_ref.py (NumPy, x' = g(x), P' = J P J^T; checked on the CPU in tests/test_reframe_cpu.py); tolerances are the
project's own (helpers.assert_state_close), every comparison covers the whole exported state.  Every device buffer must be left as
ekf_set_state of the transformed state leaves it: a twin loaded with set_state goes on bit for bit the same."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reframe_ref as rr  # noqa: E402
from helpers import (ABS_X, REL_TOL, assert_bitwise, assert_bitwise_symmetric, assert_state_close, batch_script,  # noqa: E402
                     make_filter, open_window_pair, run_steps, stream_starts, windows_closed)

pytestmark = pytest.mark.gpu

FRAME = (3.0, -2.0, 0.7)
SIZES = [(280, 320), (180, 200)]  # (capacity > 256: the several-workgroup chain kernel; <= 256: the one-workgroup kernel)


def apply_call(f, call, frame=FRAME, index=0):
    if call == "rigid":
        f.transform_frame(frame, index=index)
    else:
        f.anchor_at_robot(index=index)


def reference(call, x, P, frame=FRAME):
    return rr.rigid(x, P, frame) if call == "rigid" else rr.anchor(x, P)


# ---- 1. parity with a window open ------------------------------------------------------------------
@pytest.mark.parametrize("call", ["rigid", "anchor"])
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_with_a_window_open(pkg, pipeline_mode, N, cap, call):
    a, b, _ = open_window_pair(pkg, N, cap, seed=11, steps=5)
    before = b.get_state()
    st_b, dec_b = b.stats(), b.decisions()
    apply_call(a, call)
    after = a.get_state()
    err = assert_state_close(after[0], after[1], *reference(call, *before), what=call)
    print("%s N=%d: max |dx| %.3e, max |dP| / max |P| %.3e" % (call, N, err[0], err[1]))
    assert_bitwise_symmetric(after[1])
    assert a.stats() == st_b and a.decisions() == dec_b and int(a.num_landmarks()[0]) == N
    assert np.array_equal(a.poses()[0], after[0][:3]) and np.array_equal(a.robot_cov(), after[1][:3, :3])
    # the same call on B, whose window was folded by the export: the same bits
    apply_call(b, call)
    assert_bitwise(b.get_state(), after, "the call on a settled state")
    a.close(), b.close()


# ---- 2. pure translation is exact ---------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_pure_translation_is_exact(pkg, pipeline_mode, N, cap):
    a, b, _ = open_window_pair(pkg, N, cap, seed=21, steps=5)
    x, P = b.get_state()
    a.transform_frame((3.0, -2.0, 0.0), index=0)
    xa, Pa = a.get_state()
    assert np.array_equal(Pa, P)
    want = x.copy()
    want[0], want[1] = x[0] - 3.0, x[1] - (-2.0)
    want[3::2], want[4::2] = x[3::2] - 3.0, x[4::2] - (-2.0)
    assert np.array_equal(xa, want)
    a.close(), b.close()


# ---- 3. anchor exactness ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_anchor_is_exact_at_the_robot(pkg, pipeline_mode, N, cap):
    a, b, _ = open_window_pair(pkg, N, cap, seed=31, steps=5)
    a.anchor_at_robot(index=0)
    assert np.array_equal(a.poses()[0], np.zeros(3))
    assert np.array_equal(a.robot_cov(), np.zeros((3, 3)))
    xa, Pa = a.get_state()
    assert np.array_equal(xa[:3], np.zeros(3))
    assert not Pa[:3, :].any() and not Pa[:, :3].any()
    b.transform_frame(b.poses()[0], index=0)  # the twin: a rigid transform by the pose estimate moves the map the same way
    xb = b.get_x()
    assert np.all(np.abs(xa - xb) <= REL_TOL * np.abs(xb) + ABS_X), np.abs(xa - xb).max()
    a.close(), b.close()


# ---- 4. continuation twin -----------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["rigid", "anchor"])
@pytest.mark.parametrize("N,cap", SIZES)
def test_continuation_twin_and_oracle(pkg, oc, pipeline_mode, N, cap, call):
    a, ref, _ = open_window_pair(pkg, N, cap, seed=41, steps=3, max_pending=8)
    before = ref.get_state()
    ref.close()
    apply_call(a, call)
    b = pkg.FilterBatch(1, cap, max_pending=8, log_capacity=4096)
    b.set_state(*a.get_state())
    xr, Pr = reference(call, *before)
    S = oc.Session(xr, Pr, capacity_landmarks=cap)
    sc2 = pkg.scenarios.steady_script(xr, steps=12, M=2, seed=44, min_separation=1.0)
    da, ka = run_steps(pkg, a, sc2, 0, 12, 2, new_every=2, oracle=S, oc=oc)
    db, kb = run_steps(pkg, b, sc2, 0, 12, 2, new_every=2)
    assert da == db and ka == kb == 6
    assert sum(1 for d in da if d[0] == pkg.ekfslam.NEW) >= 6 and int(a.num_landmarks()[0]) >= N + 6
    sa, sb = a.get_state(), b.get_state()
    assert_bitwise(sa, sb, "A vs set_state twin")
    assert_state_close(sa[0], sa[1], *S.state(), what="A vs oracle")
    a.close(), b.close()


# ---- 5. the filter does not care about the frame --------------------------------------------------------
@pytest.mark.parametrize("N,cap", [(60, 64), (180, 200)])
def test_filter_is_equivariant_under_a_rigid_transform(pkg, pipeline_mode, N, cap):
    """Relative Cartesian measurements: K steps then transform equals transform then the same controls and measurements."""
    a, x0, P0 = make_filter(pkg, N, cap, seed=11)
    b, _, _ = make_filter(pkg, N, cap, seed=11)
    sc = pkg.scenarios.steady_script(x0, steps=6, M=3, seed=12, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc, 0, 6, 3)
    a.transform_frame(FRAME, index=0)
    b.transform_frame(FRAME, index=0)
    db, _ = run_steps(pkg, b, sc, 0, 6, 3)
    assert [(d[0], d[1]) for d in da] == [(d[0], d[1]) for d in db]
    assert all(d[0] == pkg.ekfslam.OLD for d in da)
    sa, sb = a.get_state(), b.get_state()
    err = assert_state_close(sa[0], sa[1], sb[0], sb[1], what="run-then-transform vs transform-then-run")
    print("equivariance N=%d: max |dx| %.3e, max |dP| / max |P| %.3e" % (N, err[0], err[1]))
    a.close(), b.close()


# ---- 6. anchored blocks are innovation covariances ------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_anchored_blocks_are_innovation_covariances(pkg, pipeline_mode, N, cap):
    a, b, sc = open_window_pair(pkg, N, cap, seed=61, steps=5)
    b.close()
    a.anchor_at_robot(index=0)
    for s in range(3):  # (each update moves the state: read it again, still without a propagation in between)
        x, covs = a.get_x(), a.landmark_covs()
        l = int(sc["target"][s, 0])
        R = sc["R"][s, 0].reshape(2, 2, order="F")
        z = x[3 + 2 * l:5 + 2 * l] + np.array([0.01, -0.02])
        r = z - x[3 + 2 * l:5 + 2 * l]
        Sm = np.array([[covs[l, 0], covs[l, 1]], [covs[l, 1], covs[l, 2]]]) + R
        want = float(r @ np.linalg.solve(Sm, r))
        d = a.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2))[0][0]
        print("landmark %d: mahal %.17g, host %.17g" % (l, d[2], want))
        assert (d[0], d[1]) == (pkg.ekfslam.OLD, 2 * l + 3), d
        assert abs(d[2] - want) <= 1e-9 * abs(want), (d[2], want)
    a.close()


# ---- 7. sizes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["rigid", "anchor"])
def test_full_size(pkg, pipeline_mode, call):
    """N = 4096 (capacity 4096), the whole 8195 x 8195 export against the blockwise reference."""
    N = 4096
    a, b, _ = open_window_pair(pkg, N, N, seed=71, steps=2, M=2)
    before = b.get_state()
    b.close()
    apply_call(a, call)
    after = a.get_state()
    err = assert_state_close(after[0], after[1], *reference(call, *before), what=call)
    print("%s N=4096: max |dx| %.3e, max |dP| / max |P| %.3e" % (call, err[0], err[1]))
    assert_bitwise_symmetric(after[1])
    a.close()


def test_batch_every_filter_its_own_frame(pkg, pipeline_mode):
    """256 filters x 256 landmarks: a different frame per filter in one call, each filter against its own reference; then the batch
    anchor the same way; then a scripted continuation against a twin batch loaded with set_state: bitwise."""
    B, cap, N = 256, 256, 240
    states = [pkg.scenarios.injected_state(N, seed=400 + k, extent=30.0) for k in range(4)]
    f = pkg.FilterBatch(B, cap)
    for b in range(B):
        f.set_state(*states[b % 4], index=b)
    ctrl, z, R = batch_script(pkg, B, 6, 2)
    f.script_load(ctrl[:3], z[:3], R[:3])
    f.script_run(0, 3)
    before = [f.get_state(b) for b in range(B)]
    counts = f.num_landmarks().copy()
    rng = np.random.default_rng(81)
    frames = np.stack([rng.uniform(-20, 20, B), rng.uniform(-20, 20, B), rng.uniform(-3.0, 3.0, B)], axis=1)
    frames[0] = 0.0
    f.transform_frame(frames)
    mid = [f.get_state(b) for b in range(B)]
    for b in range(B):
        assert_state_close(mid[b][0], mid[b][1], *rr.rigid(*before[b], frames[b]), what="rigid, filter %d" % b)
        assert_bitwise_symmetric(mid[b][1])
    assert_bitwise(mid[0], before[0], "the zero frame")
    assert np.array_equal(f.poses(), np.stack([m[0][:3] for m in mid]))
    f.anchor_at_robot()
    end = [f.get_state(b) for b in range(B)]
    for b in range(B):
        assert_state_close(end[b][0], end[b][1], *rr.anchor(*mid[b]), what="anchor, filter %d" % b)
        assert_bitwise_symmetric(end[b][1])
        assert not end[b][1][:3, :].any() and not end[b][0][:3].any()
    assert np.array_equal(f.num_landmarks(), counts)
    f.script_load(ctrl[3:], z[3:], R[3:])
    f.script_run(0, 3)
    ours = [(f.get_state(b), f.decisions(b, 6)) for b in range(B)]
    f.close()  # (the twin after it: a batch of 256 may hold every CU of the GPU)
    twin = pkg.FilterBatch(B, cap)
    for b in range(B):
        twin.set_state(*end[b], index=b)
    twin.script_load(ctrl[3:], z[3:], R[3:])
    twin.script_run(0, 3)
    for b in range(B):
        assert_bitwise(ours[b][0], twin.get_state(b), "continuation, filter %d" % b)
        assert ours[b][1] == twin.decisions(b, 6)
    twin.close()


# ---- 8. edges -----------------------------------------------------------------------------------------
def test_bad_arguments_and_sticky_status_change_nothing(pkg, pipeline_mode):
    f, x0, P0 = make_filter(pkg, 60, 64, seed=91)
    sc = pkg.scenarios.steady_script(x0, steps=4, M=2, seed=92, min_separation=1.0)
    run_steps(pkg, f, sc, 0, 4, 2)
    st = f.get_state()
    L, BAD = f.L, pkg.ekfslam.ERR_BAD_ARG
    dp = ctypes.POINTER(ctypes.c_double)
    good = np.array(FRAME)
    assert L.ekf_transform_frame(f.h, 1, good.ctypes.data_as(dp)) == BAD
    assert L.ekf_transform_frame(f.h, -1, good.ctypes.data_as(dp)) == BAD
    assert L.ekf_transform_frame(f.h, 0, None) == BAD
    for bad in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, np.nan), (0.0, 0.0, -np.inf)):
        fr = np.array(bad)
        assert L.ekf_transform_frame(f.h, 0, fr.ctypes.data_as(dp)) == BAD
        assert L.ekf_batch_transform_frame(f.h, fr.ctypes.data_as(dp)) == BAD
    assert L.ekf_batch_transform_frame(f.h, None) == BAD
    assert L.ekf_anchor_at_robot(f.h, 1) == BAD and L.ekf_anchor_at_robot(f.h, -1) == BAD
    assert L.ekf_transform_frame(None, 0, good.ctypes.data_as(dp)) == BAD and L.ekf_batch_anchor_at_robot(None) == BAD
    assert_bitwise(f.get_state(), st, "after bad arguments")
    f.close()
    # a sticky capacity error is returned unchanged and nothing changes
    g, gx, gP = make_filter(pkg, 8, 8, seed=93)
    z, R = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    held = g.get_state()
    for call in ("rigid", "anchor"):
        with pytest.raises(pkg.EkfError) as ei:
            apply_call(g, call)
        assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
        assert_bitwise(g.get_state(), held, "sticky capacity, %s" % call)
    with pytest.raises(pkg.EkfError) as ei:
        g.sync()
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    g.close()


@pytest.mark.parametrize("call", ["rigid", "anchor"])
@pytest.mark.parametrize("N,cap", SIZES)
def test_no_dense_pass_of_its_own_and_streaming_resumes(pkg, pipeline_mode, N, cap, call):
    """With a window open the call folds it (at most one window closes); on a settled handle no window closes.  A one-filter handle
    streams again afterwards, and goes on exactly as a twin loaded with set_state."""
    a, x0, P0 = make_filter(pkg, N, cap, seed=101)
    sc = pkg.scenarios.steady_script(x0, steps=12, M=2, seed=102, min_separation=1.0)
    run_steps(pkg, a, sc, 0, 3, 2)  # 6 slots of a 16-slot window: open
    w0 = windows_closed(a)
    apply_call(a, call)
    w1 = windows_closed(a)
    assert 0 <= w1 - w0 <= 1
    apply_call(a, call)  # settled now
    assert windows_closed(a) == w1
    a.get_state()
    apply_call(a, call)
    assert windows_closed(a) == w1
    on, starts0 = stream_starts(a)
    st = a.get_state()
    b = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    b.set_state(*st)
    sc2 = pkg.scenarios.steady_script(st[0], steps=6, M=2, seed=104, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc2, 0, 6, 2)
    db, _ = run_steps(pkg, b, sc2, 0, 6, 2)
    on1, starts1 = stream_starts(a)
    if on:
        assert starts1 > starts0
    assert da == db
    assert_bitwise(a.get_state(), b.get_state(), "streamed continuation")
    a.close(), b.close()


@pytest.mark.parametrize("call", ["rigid", "anchor"])
def test_reserve_before_and_after_and_a_loaded_script(pkg, pipeline_mode, call):
    N, cap = 60, 64
    f, x0, P0 = make_filter(pkg, N, cap, seed=111)
    sc = pkg.scenarios.steady_script(x0, steps=6, M=2, seed=112, min_separation=1.0)
    ctrl, z, R = sc["ctrl"].reshape(6, 1, 3), sc["z"].reshape(6, 2, 1, 2), sc["R"].reshape(6, 2, 1, 4)
    f.script_load(ctrl, z, R)
    f.script_run(0, 2)
    f.reserve(2 * cap)
    before = f.get_state()
    f.script_run(2, 1)
    f.sync()
    twin = pkg.FilterBatch(1, 2 * cap, max_pending=16, log_capacity=4096)
    twin.set_state(*before)
    twin.script_load(ctrl, z, R)
    twin.script_run(2, 1)
    mid = twin.get_state()
    apply_call(f, call)  # a window open, a script loaded, after a reserve
    after = f.get_state()
    assert_state_close(after[0], after[1], *reference(call, *mid), what="after reserve")
    f.reserve(4 * cap)
    assert_bitwise(f.get_state(), after, "reserve after the call")
    twin.close()
    twin = pkg.FilterBatch(1, 4 * cap, max_pending=16, log_capacity=4096)
    twin.set_state(*after)
    twin.script_load(ctrl, z, R)
    f.script_run(3, 3)  # the script loaded before the call still runs
    twin.script_run(3, 3)
    assert_bitwise(f.get_state(), twin.get_state(), "scripted continuation")
    assert f.decisions(0, 6) == twin.decisions(0, 6)
    f.close(), twin.close()


def test_kalmanfilter_mirrors(pkg, pipeline_mode):
    x0, P0 = pkg.scenarios.injected_state(10, seed=121, extent=10.0)
    kf = pkg.KalmanFilter(capacity_landmarks=16)
    kf.set_state(x0, P0)
    kf.transform_frame(FRAME)
    xr, Pr = rr.rigid(x0, P0, FRAME)
    assert np.allclose([kf.X, kf.Y, kf.Phi], xr[:3], rtol=REL_TOL, atol=ABS_X)
    assert_state_close(*kf.state(), xr, Pr, what="KalmanFilter rigid")
    kf.anchor_at_robot()
    assert (kf.X, kf.Y, kf.Phi) == (0.0, 0.0, 0.0) and kf.Num_Landmarks == 10
    assert_state_close(*kf.state(), *rr.anchor(xr, Pr), what="KalmanFilter anchor")
    kf._f.close()
