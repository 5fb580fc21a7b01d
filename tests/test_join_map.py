"""Map joining on the device: ekf_join_map / ekf_batch_join_map append a local map, whose frame origin is the destination's estimated
pose, behind the destination's landmarks.  The reference is tests/join_ref.py (NumPy, the dense Jacobian product; checked on the
CPU in tests/test_join_map_cpu.py); tolerances are the project's own (helpers.assert_state_close) and every comparison covers the
whole exported state.  Every device buffer must be left as ekf_set_state of the joined state leaves it: a twin loaded with set_state
goes on bit for bit the same.  Sizes: a tile is 32 landmarks, capacity 256 splits the two kernel families --
A: 200 landmarks in capacity 320 (k_chain), B: 100 in capacity 200 (k_solo where the pipeline mode allows it); the source has 70
landmarks in capacity 96 (more than two tiles, a layout of its own).  Ng mod 32 != 0 in both."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_ref as jr  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, open_window_pair  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(200, 320), (100, 200)]
NS, CAP_S = 70, 96


def run_script(f, sc, steps, M):
    decs = []
    for s in range(steps):
        v, w, dt = sc["ctrl"][s]
        f.propagate(v, w, dt)
        for m in range(M):
            decs.append(f.update(sc["z"][s, m].reshape(1, 1, 2), sc["R"][s, m].reshape(2, 2, order="F").reshape(1, 1, 2, 2))[0][0])
    return decs


def measurement_of(pkg, x, l):
    """The relative Cartesian measurement that hits landmark l of state x exactly (slam.cpp:158-167 conversion)."""
    c, s = np.cos(x[2]), np.sin(x[2])
    d = x[3 + 2 * l:5 + 2 * l] - x[0:2]
    return pkg.scenarios.measurement_from_feature_mm(1000.0 * (c * d[0] + s * d[1]), 1000.0 * (-s * d[0] + c * d[1]))


def nearest_isolated(x, lo, hi, count):
    """`count` landmarks of [lo, hi), nearest to the robot first, at least 1 m from the robot and 0.5 m from every other landmark."""
    L = x[3:].reshape(-1, 2)
    d2 = ((L[:, None, :] - L[None, :, :]) ** 2).sum(-1)
    d2[np.diag_indices(L.shape[0])] = np.inf
    iso = np.sqrt(d2.min(axis=1))
    r = np.hypot(*(L - x[0:2]).T)
    ok = [l for l in range(lo, hi) if iso[l] >= 0.5 and r[l] >= 1.0]
    assert len(ok) >= count
    return sorted(ok, key=lambda l: r[l])[:count]


def continue_both(pkg, a, b, Ng, Ns):
    """The same further calls on the joined handle `a` and its set_state twin `b` (window of 8): propagations, Old matches of old and
    of joined landmarks, a far New landmark, a compass update -- ten slots, so a window closes on the way.  Bitwise equal ends."""
    x = a.get_x()
    assert np.array_equal(x, b.get_x())
    olds, news = nearest_isolated(x, 0, Ng, 4), nearest_isolated(x, Ng, Ng + Ns, 4)
    far = pkg.scenarios.measurement_from_feature_mm(90000.0, -55000.0)
    out = []
    for f in (a, b):
        decs = []
        for s in range(4):
            f.propagate(0.3, 0.05, 0.05)
            for l in (olds[s], news[s]):
                z, R = measurement_of(pkg, x, l)
                decs.append(f.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2))[0][0])
            if s == 1:
                decs.append(f.update(far[0].reshape(1, 1, 2), far[1].reshape(1, 1, 2, 2))[0][0])
            if s == 2:
                f.update_compass(x[2] + 0.01, pkg.scenarios.COMPASS_VAR)
        out.append(decs)
    da, db = out
    assert da == db
    for s in range(4):
        at = 2 * s + (1 if s > 1 else 0)
        assert (da[at][0], da[at][1]) == (pkg.ekfslam.OLD, 3 + 2 * olds[s]), (s, da[at])
        k = news[s] - Ng  # the source's landmark k: state index 2 (Ng + k + 1) + 1
        assert (da[at + 1][0], da[at + 1][1]) == (pkg.ekfslam.OLD, 2 * (Ng + k + 1) + 1), (s, da[at + 1])
    assert da[4][0] == pkg.ekfslam.NEW
    sa, sb = a.get_state(), b.get_state()
    assert sa[0].size == 3 + 2 * (Ng + Ns + 1)
    assert_bitwise(sa, sb, "joined handle vs set_state twin")
    assert a.decisions()[-9:] == b.decisions()[-9:]


# ---- 1. parity with windows open on both filters ------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_with_windows_open_on_both_filters(pkg, pipeline_mode, N, cap):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=11, steps=3)
    s, sw, _ = open_window_pair(pkg, NS, CAP_S, seed=15, extent=8.0, steps=3)
    xg, Pg = aw.get_state()
    xs, Ps = sw.get_state()
    st_a, dec_a, st_s, dec_s = aw.stats(), aw.decisions(), sw.stats(), sw.decisions()
    assert a.join_map(s) == N + NS
    after = a.get_state()
    err = assert_state_close(after[0], after[1], *jr.join(xg, Pg, xs, Ps), what="join")
    print("join %d + %d: max |dx| %.3e, max |dP| / max |P| %.3e" % (N, NS, err[0], err[1]))
    assert_bitwise_symmetric(after[1])
    e = 3 + 2 * N
    assert np.array_equal(after[1][3:e, 3:e], Pg[3:, 3:]) and np.array_equal(after[0][3:e], xg[3:])
    assert np.array_equal(a.poses()[0], after[0][:3]) and np.array_equal(a.robot_cov(), after[1][:3, :3])
    assert int(a.num_landmarks()[0]) == N + NS
    assert a.stats() == st_a and a.decisions() == dec_a
    assert_bitwise(s.get_state(), (xs, Ps), "the source after the join")
    assert s.stats() == st_s and s.decisions() == dec_s
    # the source streams on: the same further calls as its witness, the same bits
    sc = pkg.scenarios.steady_script(xs, steps=2, M=2, seed=19, min_separation=1.0)
    assert run_script(s, sc, 2, 2) == run_script(sw, sc, 2, 2)
    assert_bitwise(s.get_state(), sw.get_state(), "the source goes on")
    for f in (a, aw, s, sw):
        f.close()


# ---- 2. exact cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [320, 200])
def test_join_into_a_fresh_filter_reproduces_the_source(pkg, pipeline_mode, cap):
    s, sw, _ = open_window_pair(pkg, NS, CAP_S, seed=25, extent=8.0, steps=3)
    a = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    assert a.join_map(s) == NS
    xa, Pa = a.get_state()
    xs, Ps = sw.get_state()
    assert xa.shape == xs.shape and (xa == xs).all() and (Pa == Ps).all()
    for f in (a, s, sw):
        f.close()


@pytest.mark.parametrize("N,cap", SIZES)
def test_join_of_a_fresh_source_leaves_the_destination_unchanged(pkg, pipeline_mode, N, cap):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=31, steps=3)
    s = pkg.FilterBatch(1, CAP_S, max_pending=16, log_capacity=4096)
    assert a.join_map(s) == N
    xa, Pa = a.get_state()
    xw, Pw = aw.get_state()
    assert xa.shape == xw.shape and (xa == xw).all() and (Pa == Pw).all()
    assert np.array_equal(a.poses()[0], xw[:3]) and np.array_equal(a.robot_cov(), Pw[:3, :3])
    for f in (a, aw, s):
        f.close()


# ---- 3. buffers are left as ekf_set_state leaves them -----------------------------------------------------
@pytest.mark.parametrize("reserve_first", [False, True])
@pytest.mark.parametrize("N,cap", SIZES)
def test_set_state_twin_goes_on_bit_for_bit(pkg, pipeline_mode, N, cap, reserve_first):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=41, max_pending=8, steps=3)
    s, sw, _ = open_window_pair(pkg, NS, CAP_S, seed=45, extent=8.0, steps=3)
    aw.close(), sw.close()
    a.join_map(s)
    s.close()
    if reserve_first:  # the joined state moves to larger buffers (another tile numbering) first
        joined = a.get_state()
        a.reserve(cap + 100)
        assert_bitwise(a.get_state(), joined, "reserve after the join")
    b = pkg.FilterBatch(1, a.capacity, max_pending=8, log_capacity=4096)
    b.set_state(*a.get_state())
    continue_both(pkg, a, b, N, NS)
    a.close(), b.close()


# ---- 4. same-handle and batch forms ---------------------------------------------------------------------
def _batch(pkg, cap, counts, seed):
    f = pkg.FilterBatch(len(counts), cap, max_pending=16, log_capacity=4096)
    for b, n in enumerate(counts):
        if n:
            f.set_state(*pkg.scenarios.injected_state(n, seed=seed + b, extent=10.0 + b), index=b)
    return f


def _open_batch_window(pkg, f):
    f.propagate(0.3, 0.05, 0.05)
    z, R = pkg.scenarios.measurement_from_feature_mm(80000.0, 30000.0)
    B = f.batch
    f.update(np.tile(z, (B, 1, 1)), np.tile(R, (B, 1, 1, 1)), want_decisions=False)  # a New landmark everywhere: a slot in the open window


def test_join_inside_one_handle_changes_that_filter_only(pkg, pipeline_mode):
    counts = (60, 100, 45, 70)
    f, w = _batch(pkg, 200, counts, seed=50), _batch(pkg, 200, counts, seed=50)
    _open_batch_window(pkg, f), _open_batch_window(pkg, w)
    before = [w.get_state(b) for b in range(4)]
    assert f.join_map(f, index=1, src_index=3) == counts[1] + counts[3] + 2
    assert list(f.num_landmarks()) == [61, 172, 46, 71]
    for b in (0, 2, 3):
        assert_bitwise(f.get_state(b), before[b], "filter %d" % b)
    got = f.get_state(1)
    assert_state_close(got[0], got[1], *jr.join(*before[1], *before[3]), what="filter 1")
    assert_bitwise_symmetric(got[1])
    f.close(), w.close()


def test_batch_form_equals_single_joins(pkg, pipeline_mode):
    ng, ns = (100, 45, 0, 64), (70, 33, 20, 0)
    d1, d2, s = _batch(pkg, 200, ng, seed=60), _batch(pkg, 200, ng, seed=60), _batch(pkg, CAP_S, ns, seed=70)
    for f in (d1, d2, s):
        _open_batch_window(pkg, f)
    d1.batch_join_map(s)
    for b in range(4):
        assert d2.join_map(s, index=b, src_index=b) == ng[b] + ns[b] + 2
    assert list(d1.num_landmarks()) == list(d2.num_landmarks()) == [ng[b] + ns[b] + 2 for b in range(4)]
    for b in range(4):
        assert_bitwise(d1.get_state(b), d2.get_state(b), "filter %d" % b)
    assert np.array_equal(d1.poses(), d2.poses())
    for f in (d1, d2, s):
        f.close()


# ---- 5. errors ------------------------------------------------------------------------------------------
def test_errors_change_nothing_and_capacity_is_not_sticky(pkg, pipeline_mode):
    a, aw, _ = open_window_pair(pkg, 60, 64, seed=81, steps=3)
    s, sw, _ = open_window_pair(pkg, 10, 32, seed=85, extent=8.0, steps=3)
    aw.close(), sw.close()
    held_a, held_s = a.get_state(), s.get_state()
    n_joined = (held_a[0].size - 3) // 2 + (held_s[0].size - 3) // 2
    assert n_joined > 64
    L, E = a.L, pkg.ekfslam
    assert L.ekf_join_map(a.h, 0, s.h, 0) == E.ERR_CAPACITY  # 60 + 10 > 64
    assert_bitwise(a.get_state(), held_a, "destination after EKF_ERR_CAPACITY")
    assert_bitwise(s.get_state(), held_s, "source after EKF_ERR_CAPACITY")
    a.sync()  # EKF_OK: nothing sticky
    assert L.ekf_join_map(a.h, 0, a.h, 0) == E.ERR_BAD_ARG  # a filter into itself
    for di, si in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        assert L.ekf_join_map(a.h, di, s.h, si) == E.ERR_BAD_ARG
    assert L.ekf_join_map(None, 0, s.h, 0) == E.ERR_BAD_ARG and L.ekf_join_map(a.h, 0, None, 0) == E.ERR_BAD_ARG
    four = pkg.FilterBatch(4, 16)
    assert L.ekf_batch_join_map(a.h, four.h) == E.ERR_BAD_ARG and L.ekf_batch_join_map(four.h, four.h) == E.ERR_BAD_ARG
    assert L.ekf_batch_join_map(None, s.h) == E.ERR_BAD_ARG
    four.close()
    assert_bitwise(a.get_state(), held_a, "destination after bad arguments")
    assert_bitwise(s.get_state(), held_s, "source after bad arguments")
    a.reserve(128)
    assert a.join_map(s) == n_joined
    got = a.get_state()
    assert_state_close(got[0], got[1], *jr.join(*held_a, *held_s), what="join after reserve")
    a.close(), s.close()


# ---- 6. join after removal --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_join_after_removal_reuses_the_freed_rows(pkg, pipeline_mode, N, cap):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=91, max_pending=8, steps=3)
    s, sw, _ = open_window_pair(pkg, NS, CAP_S, seed=95, extent=8.0, steps=3)
    keep = np.ones(N, dtype=bool)
    keep[1::3] = False  # spread over every tile
    n_kept = int(keep.sum())
    assert a.remove_landmarks(keep, index=0) == n_kept and aw.remove_landmarks(keep, index=0) == n_kept
    sc = pkg.scenarios.steady_script(aw.get_x(), steps=2, M=2, seed=97, min_separation=1.0)
    assert run_script(a, sc, 2, 2) == run_script(aw, sc, 2, 2)  # a window open again, on the reduced map
    xg, Pg = aw.get_state()
    xs, Ps = sw.get_state()
    aw.close(), sw.close()
    assert a.join_map(s) == n_kept + NS
    s.close()
    after = a.get_state()
    assert_state_close(after[0], after[1], *jr.join(xg, Pg, xs, Ps), what="join after removal")
    assert_bitwise_symmetric(after[1])
    e = 3 + 2 * n_kept
    assert np.array_equal(after[1][3:e, 3:e], Pg[3:, 3:])
    b = pkg.FilterBatch(1, cap, max_pending=8, log_capacity=4096)
    b.set_state(*after)
    continue_both(pkg, a, b, n_kept, NS)
    a.close(), b.close()
