"""Landmark removal on the device (ekf_remove_landmarks / ekf_batch_remove_landmarks) and the per-landmark covariance readout
(ekf_get_landmark_covs).  Marginalising a landmark out of a Gaussian deletes its two rows and columns: the reduced state must be
np.delete of the state before, bit for bit, and every device buffer must be left as ekf_set_state of that reduced state leaves it --
a twin handle loaded with set_state goes on bit for bit the same, New landmarks reusing the freed rows included."""
import ctypes

import numpy as np
import pytest

from helpers import (assert_bitwise, assert_bitwise_symmetric, assert_state_close, batch_script, make_filter, run_steps, stream_starts,
                     windows_closed)

pytestmark = pytest.mark.gpu


def reduce_state(x, P, keep):
    keep = np.asarray(keep, dtype=bool)
    kept = np.flatnonzero(keep)
    rows = np.sort(np.concatenate([np.arange(3), 3 + 2 * kept, 4 + 2 * kept]))
    return x[rows].copy(), P[np.ix_(rows, rows)].copy()


def kinds(decs):
    """(decision, matched index) of run_steps' decisions: what the removal tests compare."""
    return [(d[0], d[1]) for d in decs]


# (capacity > 256: the several-workgroup chain kernel; <= 256: the one-workgroup kernel)
@pytest.mark.parametrize("N,cap", [(280, 320), (180, 200)])
def test_removal_is_np_delete_bit_for_bit_with_a_window_open(pkg, pipeline_mode, N, cap):
    """Two identical handles run the same calls; the window is left open (and a streaming launch live) on both.  B's state is
    exported (which folds the window) and A removes a random mask straight away: A's export equals np.delete of B's bit for bit,
    and pose, robot block, counters, stats and the count are those of before."""
    a, x0, P0 = make_filter(pkg, N, cap, seed=11)
    b, _, _ = make_filter(pkg, N, cap, seed=11)
    sc = pkg.scenarios.steady_script(x0, steps=5, M=2, seed=12, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc, 0, 5, 2)
    db, _ = run_steps(pkg, b, sc, 0, 5, 2)
    assert kinds(da) == kinds(db)
    before = b.get_state()
    pose_b, rcov_b, st_b = b.poses()[0].copy(), b.robot_cov(), b.stats()
    keep = np.random.default_rng(13).random(N) > 0.3
    keep[0] = False
    n_new = a.remove_landmarks(keep, index=0)
    assert n_new == int(keep.sum()) == int(a.num_landmarks()[0])
    after = a.get_state()
    assert_bitwise(after, reduce_state(*before, keep), "after removal")
    assert_bitwise_symmetric(after[1])
    assert np.array_equal(a.poses()[0], pose_b) and np.array_equal(a.robot_cov(), rcov_b)
    assert a.stats() == st_b
    # the same removal on B, whose window was folded by the export
    assert b.remove_landmarks(keep, index=0) == n_new
    assert_bitwise(b.get_state(), after, "removal of a settled state")
    a.close(), b.close()


@pytest.mark.parametrize("N,cap,n_remove", [(280, 320, 28), (180, 200, 20)])
def test_continuation_twin_reuses_the_freed_rows(pkg, oc, pipeline_mode, N, cap, n_remove):
    """A removes landmarks with a window open; B is loaded with set_state(np.delete(...)).  Both run the same windows of
    propagations, Old updates and New landmarks -- more New than were removed, so the map grows past its old size through the freed
    rows.  Decisions and final states are bitwise equal, and A is within tolerance of the C oracle driven from the reduced state."""
    a, x0, P0 = make_filter(pkg, N, cap, seed=21, max_pending=8)
    ref, _, _ = make_filter(pkg, N, cap, seed=21, max_pending=8)
    sc = pkg.scenarios.steady_script(x0, steps=40, M=2, seed=22, min_separation=1.0)
    run_steps(pkg, a, sc, 0, 3, 2)
    run_steps(pkg, ref, sc, 0, 3, 2)
    xs, Ps = ref.get_state()
    ref.close()
    rng = np.random.default_rng(23)
    keep = np.ones(N, dtype=bool)
    keep[rng.choice(N, size=n_remove, replace=False)] = False
    a.remove_landmarks(keep, index=0)
    xr, Pr = reduce_state(xs, Ps, keep)
    b = pkg.FilterBatch(1, cap, max_pending=8, log_capacity=4096)
    b.set_state(xr, Pr)
    S = oc.Session(xr, Pr, capacity_landmarks=cap)
    sc2 = pkg.scenarios.steady_script(xr, steps=40, M=2, seed=24, min_separation=1.0)
    n_new_needed = n_remove + 6
    steps = n_new_needed  # one New per step
    da, ka = run_steps(pkg, a, sc2, 0, steps, 2, new_every=1, oracle=S, oc=oc)
    db, kb = run_steps(pkg, b, sc2, 0, steps, 2, new_every=1)
    assert kinds(da) == kinds(db) and ka == kb == n_new_needed
    assert sum(1 for d in da if d[0] == pkg.ekfslam.NEW) >= n_new_needed
    assert int(a.num_landmarks()[0]) > N  # grown past the old size: freed rows reused
    sa, sb = a.get_state(), b.get_state()
    assert_bitwise(sa, sb, "A vs B")
    assert_state_close(sa[0], sa[1], *S.state(), what="A vs oracle")
    a.close(), b.close()


def test_full_size_removals(pkg, pipeline_mode):
    """N = 4096: the first landmark, the last, a contiguous block of 64 and 1 % spread out, one after the other, each bitwise
    against np.delete of the export in front of it."""
    N = 4096
    f, x0, P0 = make_filter(pkg, N, N + 8, seed=31)
    sc = pkg.scenarios.steady_script(x0, steps=3, M=3, seed=32, min_separation=1.0)
    run_steps(pkg, f, sc, 0, 3, 3)
    rng = np.random.default_rng(33)
    st = f.get_state()
    for case in ("first", "last", "block64", "spread1pct"):
        n = (st[0].size - 3) // 2
        keep = np.ones(n, dtype=bool)
        if case == "first":
            keep[0] = False
        elif case == "last":
            keep[-1] = False
        elif case == "block64":
            keep[1500:1564] = False
        else:
            keep[rng.choice(n, size=n // 100, replace=False)] = False
        assert f.remove_landmarks(keep, index=0) == int(keep.sum())
        after = f.get_state()
        assert_bitwise(after, reduce_state(*st, keep), case)
        st = after
    assert_bitwise_symmetric(st[1])
    f.close()


def test_batch_removal_every_filter_its_own_mask(pkg, pipeline_mode):
    """256 filters x 256 landmarks (the fused one-workgroup pass): each filter a different mask, one keeping all and one keeping
    none.  Every filter bitwise against np.delete; then a scripted continuation against a twin batch loaded with set_state per
    index: decisions and states bitwise equal."""
    B, cap, N = 256, 256, 240
    states = [pkg.scenarios.injected_state(N, seed=400 + k, extent=30.0) for k in range(4)]
    f = pkg.FilterBatch(B, cap)
    for b in range(B):
        f.set_state(*states[b % 4], index=b)
    ctrl, z, R = batch_script(pkg, B, 6, 2)
    f.script_load(ctrl[:3], z[:3], R[:3])
    f.script_run(0, 3)
    before = [f.get_state(b) for b in range(B)]
    rng = np.random.default_rng(41)
    keep = np.zeros((B, cap), dtype=bool)
    for b in range(B):
        n = (before[b][0].size - 3) // 2
        keep[b, :n] = rng.random(n) > rng.uniform(0.0, 0.9)
    keep[0, :] = True
    keep[1, :] = False
    n_out = f.remove_landmarks(keep)
    counts = [int(c) for c in f.num_landmarks()]
    reduced = []
    for b in range(B):
        n = (before[b][0].size - 3) // 2
        want = reduce_state(*before[b], keep[b, :n])
        reduced.append(want)
        assert n_out[b] == counts[b] == (want[0].size - 3) // 2
        assert_bitwise(f.get_state(b), want, "filter %d" % b)
    assert counts[0] == (before[0][0].size - 3) // 2 and counts[1] == 0
    f.script_load(ctrl[3:], z[3:], R[3:])
    f.script_run(0, 3)
    ours = [(f.get_state(b), f.decisions(b, 6)) for b in range(B)]
    f.close()  # (the twin after it: a batch of 256 may hold every CU of the GPU)
    twin = pkg.FilterBatch(B, cap)
    for b in range(B):
        twin.set_state(*reduced[b], index=b)
    twin.script_load(ctrl[3:], z[3:], R[3:])
    twin.script_run(0, 3)
    for b in range(B):
        assert_bitwise(ours[b][0], twin.get_state(b), "continuation, filter %d" % b)
        assert ours[b][1] == twin.decisions(b, 6)
    twin.close()


def test_edges(pkg, pipeline_mode):
    """All-keep is the identity, removing everything leaves the robot, bad arguments and sticky statuses change nothing,
    ekf_reserve before and after, the KalmanFilter mirror's count."""
    N, cap = 60, 64
    f, x0, P0 = make_filter(pkg, N, cap, seed=51)
    sc = pkg.scenarios.steady_script(x0, steps=4, M=2, seed=52, min_separation=1.0)
    run_steps(pkg, f, sc, 0, 4, 2)
    st = f.get_state()
    assert f.remove_landmarks(np.ones(N, dtype=bool), index=0) == N
    assert_bitwise(f.get_state(), st, "all kept")
    # bad arguments
    L = f.L
    k = np.ones(N, dtype=np.uint8)
    kp = k.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))
    assert L.ekf_remove_landmarks(f.h, 1, kp, N) == pkg.ekfslam.ERR_BAD_ARG
    assert L.ekf_remove_landmarks(f.h, -1, kp, N) == pkg.ekfslam.ERR_BAD_ARG
    assert L.ekf_remove_landmarks(f.h, 0, None, N) == pkg.ekfslam.ERR_BAD_ARG
    assert L.ekf_remove_landmarks(f.h, 0, kp, -1) == pkg.ekfslam.ERR_BAD_ARG
    assert L.ekf_batch_remove_landmarks(f.h, None, N, None) == pkg.ekfslam.ERR_BAD_ARG
    assert L.ekf_get_landmark_covs(f.h, 3, None, 0) == pkg.ekfslam.ERR_BAD_ARG
    assert_bitwise(f.get_state(), st, "after bad arguments")
    # a shorter mask: landmarks without an entry are kept
    keep = np.ones(N, dtype=bool)
    keep[[2, 5]] = False
    assert f.remove_landmarks(keep[:10], index=0) == N - 2
    st = reduce_state(*st, keep)
    assert_bitwise(f.get_state(), st, "short mask")
    # removal after a reserve, reserve after a removal
    f.reserve(2 * cap)
    keep = np.ones(N - 2, dtype=bool)
    keep[-3:] = False
    assert f.remove_landmarks(keep, index=0) == N - 5
    st = reduce_state(*st, keep)
    assert_bitwise(f.get_state(), st, "after reserve")
    f.reserve(4 * cap)
    assert_bitwise(f.get_state(), st, "reserve after removal")
    # everything removed: the robot is left
    assert f.remove_landmarks(np.zeros(N - 5, dtype=bool), index=0) == 0
    x3, P3 = f.get_state()
    assert x3.size == 3 and np.array_equal(x3, st[0][:3]) and np.array_equal(P3, st[1][:3, :3])
    f.close()
    # a sticky capacity error is returned and nothing changes
    g, gx, gP = make_filter(pkg, 8, 8, seed=53)
    z, R = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    with pytest.raises(pkg.EkfError) as ei:
        g.remove_landmarks(np.zeros(8, dtype=bool), index=0)
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    xg, Pg = g.get_state()
    assert xg.size == 3 + 16
    with pytest.raises(pkg.EkfError) as ei:
        g.sync()
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    g.close()
    # the KalmanFilter mirror
    kf = pkg.KalmanFilter(capacity_landmarks=16)
    kf.set_state(x0[:3 + 2 * 10], P0[:3 + 2 * 10, :3 + 2 * 10])
    keep = np.ones(10, dtype=bool)
    keep[[1, 7]] = False
    kf.remove_landmarks(keep)
    assert kf.Num_Landmarks == 8
    assert_bitwise(kf.state(), reduce_state(x0[:23], P0[:23, :23], keep), "KalmanFilter")
    kf._f.close()


def test_a_one_filter_handle_streams_again_after_a_removal(pkg, pipeline_mode):
    """The removal stops the resident streaming launch; the next immediate calls start another, and their results equal those of a
    twin loaded with set_state."""
    N, cap = 280, 320
    a, x0, P0 = make_filter(pkg, N, cap, seed=61)
    sc = pkg.scenarios.steady_script(x0, steps=12, M=2, seed=62, min_separation=1.0)
    run_steps(pkg, a, sc, 0, 3, 2)
    keep = np.random.default_rng(63).random(N) > 0.1
    st = a.get_state()
    a.remove_landmarks(keep, index=0)
    on, starts0 = stream_starts(a)
    b = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    b.set_state(*reduce_state(*st, keep))
    sc2 = pkg.scenarios.steady_script(reduce_state(*st, keep)[0], steps=8, M=2, seed=64, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc2, 0, 8, 2)
    db, _ = run_steps(pkg, b, sc2, 0, 8, 2)
    on1, starts1 = stream_starts(a)
    if on:
        assert starts1 > starts0
    assert kinds(da) == kinds(db)
    assert_bitwise(a.get_state(), b.get_state(), "streamed continuation")
    a.close(), b.close()


@pytest.mark.parametrize("N,cap", [(280, 320), (180, 200)])
def test_landmark_covs_are_the_diagonal_blocks_and_force_no_pass(pkg, pipeline_mode, N, cap):
    f, x0, P0 = make_filter(pkg, N, cap, seed=71)
    sc = pkg.scenarios.steady_script(x0, steps=3, M=2, seed=72, min_separation=1.0)
    run_steps(pkg, f, sc, 0, 3, 2)  # 6 slots of a 16-slot window: open
    closed = windows_closed(f)
    covs = f.landmark_covs()
    assert windows_closed(f) == closed
    assert covs.shape == (N, 3)
    x, P = f.get_state()
    l = np.arange(N)
    want = np.stack([P[3 + 2 * l, 3 + 2 * l], P[3 + 2 * l, 4 + 2 * l], P[4 + 2 * l, 4 + 2 * l]], axis=1)
    assert np.array_equal(covs, want)
    f.close()
