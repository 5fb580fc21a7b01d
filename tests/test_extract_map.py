"""Submap extraction on the device: ekf_extract_map / ekf_batch_extract_map replace a filter with the marginal of another filter over
the robot and chosen landmarks, ekf_get_submap returns the same marginal to the host.  There is no arithmetic, so the reference for
every comparison is NumPy indexing of ekf_get_state and every state comparison is bitwise (helpers.assert_bitwise): no tolerance
anywhere.  Every device buffer of the destination must be left as ekf_set_state of the extracted state leaves it: a twin loaded with
set_state goes on bit for bit the same.  Sizes: a tile is 32 landmarks, capacity 256 splits the two kernel families --
source A: 200 landmarks in capacity 320 (k_chain), source B: 100 in capacity 200 (k_solo where the pipeline mode allows it);
destinations of capacity 96 and 320.
No test keeps more than two handles of one capacity open at a time: a witness is read and closed before the next handle is made.
A handle's streams go back to a process-wide pool and are never destroyed, and an overlap-mode handle's dense-pass stream is a
hardware queue of its own; with up to four such handles open at once here, test_config4_full_size_batch_256_filters[overlap-32]
ran into EKF_ERR_TIMEOUT (a chain launch waiting in-kernel for its dense pass) later in the same process."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import (assert_bitwise, assert_bitwise_symmetric, index_state, make_filter, open_window_pair, run_steps, shuffled_ids,  # noqa: E402
                     stream_starts)

pytestmark = pytest.mark.gpu

SOURCES = [(200, 320), (100, 200)]
_IP = ctypes.POINTER(ctypes.c_int)
_DP = ctypes.POINTER(ctypes.c_double)


def fresh(pkg, cap, max_pending=16):
    return pkg.FilterBatch(1, cap, max_pending=max_pending, log_capacity=4096)


def int_array(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data_as(_IP)


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


def nearest_isolated(x, count):
    """`count` landmarks of state x, nearest to the robot first, at least 1 m from the robot and 0.5 m from every other landmark."""
    L = x[3:].reshape(-1, 2)
    d2 = ((L[:, None, :] - L[None, :, :]) ** 2).sum(-1)
    d2[np.diag_indices(L.shape[0])] = np.inf
    iso = np.sqrt(d2.min(axis=1))
    r = np.hypot(*(L - x[0:2]).T)
    ok = [l for l in range(L.shape[0]) if iso[l] >= 0.5 and r[l] >= 1.0]
    assert len(ok) >= count
    return sorted(ok, key=lambda l: r[l])[:count]


def continue_both(pkg, a, b, n):
    """The same further calls on the extracted handle `a` and its set_state twin `b` (window of 8): propagations, Old matches, a far
    New landmark, a compass update -- ten slots, so a window closes on the way.  Bitwise equal ends, equal decisions; the New
    landmark lands in row n."""
    x = a.get_x()
    assert np.array_equal(x, b.get_x()) and x.size == 3 + 2 * n
    olds = nearest_isolated(x, 4)
    far = pkg.scenarios.measurement_from_feature_mm(90000.0, -55000.0)
    out = []
    for f in (a, b):
        decs = []
        for s in range(4):
            f.propagate(0.3, 0.05, 0.05)
            for l in (olds[s], olds[(s + 2) % 4]):
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
        assert (da[at + 1][0], da[at + 1][1]) == (pkg.ekfslam.OLD, 3 + 2 * olds[(s + 2) % 4]), (s, da[at + 1])
    assert da[4][0] == pkg.ekfslam.NEW
    sa, sb = a.get_state(), b.get_state()
    assert sa[0].size == 3 + 2 * (n + 1) and np.all(sa[0][3 + 2 * n:] != 0.0)  # the New landmark in row n
    assert_bitwise(sa, sb, "extracted handle vs set_state twin")
    assert a.decisions()[-9:] == b.decisions()[-9:]


# ---- 1. parity with a window open on the source -----------------------------------------------------------
@pytest.mark.parametrize("N,cap", SOURCES)
def test_parity_with_a_window_open_on_the_source(pkg, pipeline_mode, N, cap):
    s, sw, _ = open_window_pair(pkg, N, cap, seed=111, steps=3)
    ids = shuffled_ids(N, 70, seed=112)
    held = sw.get_state()
    st_s, dec_s = sw.stats(), sw.decisions()
    d = fresh(pkg, 96)
    assert d.extract_map(s, ids) == 70
    got = d.get_state()
    assert_bitwise(got, index_state(held, ids), "extracted state")
    assert_bitwise_symmetric(got[1])
    assert np.array_equal(d.poses()[0], held[0][:3]) and np.array_equal(d.robot_cov(), held[1][:3, :3])
    assert int(d.num_landmarks()[0]) == 70
    assert_bitwise(s.get_state(), held, "the source after the extraction")
    assert s.stats() == st_s and s.decisions() == dec_s
    # the source goes on as its untouched twin does
    sc = pkg.scenarios.steady_script(held[0], steps=2, M=2, seed=119, min_separation=1.0)
    assert run_script(s, sc, 2, 2) == run_script(sw, sc, 2, 2)
    assert_bitwise(s.get_state(), sw.get_state(), "the source goes on")
    assert s.stats() == sw.stats() and s.decisions() == sw.decisions()
    for f in (d, s, sw):
        f.close()


# ---- 2. buffers are left as ekf_set_state leaves them ------------------------------------------------------
@pytest.mark.parametrize("cap_d", [96, 320])
def test_set_state_twin_goes_on_bit_for_bit(pkg, pipeline_mode, cap_d):
    s, sw, _ = open_window_pair(pkg, 200, 320, seed=121, steps=3)
    ids = shuffled_ids(200, 70, seed=122)
    want = index_state(sw.get_state(), ids)
    sw.close()
    a = fresh(pkg, cap_d, max_pending=8)
    assert a.extract_map(s, ids) == 70
    s.close()
    b = fresh(pkg, cap_d, max_pending=8)
    b.set_state(*want)
    continue_both(pkg, a, b, 70)
    a.close(), b.close()


# ---- 3. a destination that held a larger map ---------------------------------------------------------------
def test_shrinking_destination(pkg, pipeline_mode):
    s, sw, _ = open_window_pair(pkg, 100, 200, seed=131, steps=3)
    held = sw.get_state()
    sw.close()
    ids = np.array(nearest_isolated(held[0], 10), dtype=np.int32)
    np.random.default_rng(132).shuffle(ids)
    a, x0, _ = make_filter(pkg, 90, 96, seed=133, max_pending=8)
    run_steps(pkg, a, pkg.scenarios.steady_script(x0, steps=3, M=2, seed=134, min_separation=1.0), 0, 3, 2)  # a window open on the destination
    assert a.extract_map(s, ids) == 10
    assert_bitwise(a.get_state(), index_state(held, ids), "10 landmarks over 90")
    s.close()
    b = fresh(pkg, 96, max_pending=8)
    b.set_state(*index_state(held, ids))
    continue_both(pkg, a, b, 10)
    a.close(), b.close()


# ---- 4. copy and fork --------------------------------------------------------------------------------------
def test_copy_between_capacities_and_back(pkg, pipeline_mode):
    s, sw, _ = open_window_pair(pkg, 200, 320, seed=141, steps=3)
    held = sw.get_state()
    sw.close()
    t, u = fresh(pkg, 256), fresh(pkg, 320)
    assert t.extract_map(s) == 200
    assert_bitwise(t.get_state(), held, "320 -> 256")
    assert u.extract_map(t) == 200
    assert_bitwise(u.get_state(), held, "256 -> 320")
    assert_bitwise(s.get_state(), held, "the source")
    for f in (s, t, u):
        f.close()


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


def test_fork_inside_one_handle_changes_that_filter_only(pkg, pipeline_mode):
    counts = (60, 100, 45, 70)
    f, w = _batch(pkg, 200, counts, seed=150), _batch(pkg, 200, counts, seed=150)
    _open_batch_window(pkg, f), _open_batch_window(pkg, w)
    before = [w.get_state(b) for b in range(4)]
    assert f.extract_map(f, index=2, src_index=0) == counts[0] + 1
    assert list(f.num_landmarks()) == [61, 101, 61, 71]
    for b in (0, 1, 3):
        assert_bitwise(f.get_state(b), before[b], "filter %d" % b)
    assert_bitwise(f.get_state(2), before[0], "the fork")
    f.close(), w.close()


# ---- 5. against the existing removal -----------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SOURCES)
def test_increasing_ids_give_the_bits_of_the_removal(pkg, pipeline_mode, N, cap):
    s, sw, _ = open_window_pair(pkg, N, cap, seed=161, steps=3)
    keep = np.ones(N, dtype=bool)
    keep[1::3] = False  # spread over every tile
    n_kept = int(keep.sum())
    assert sw.remove_landmarks(keep, index=0) == n_kept
    want = sw.get_state()
    sw.close()
    d = fresh(pkg, 320)
    assert d.extract_map(s, np.flatnonzero(keep)) == n_kept
    assert_bitwise(d.get_state(), want, "extraction vs removal")
    d.close(), s.close()


# ---- 6. composition ----------------------------------------------------------------------------------------
def test_two_extractions_compose(pkg, pipeline_mode):
    s, sw, _ = open_window_pair(pkg, 200, 320, seed=171, steps=3)
    ids1 = shuffled_ids(200, 70, seed=172)
    ids2 = shuffled_ids(70, 30, seed=173)
    want = index_state(sw.get_state(), ids1[ids2])
    sw.close()
    t, u, v = fresh(pkg, 96), fresh(pkg, 320), fresh(pkg, 96)
    assert t.extract_map(s, ids1) == 70 and u.extract_map(t, ids2) == 30 and v.extract_map(s, ids1[ids2]) == 30
    assert_bitwise(u.get_state(), v.get_state(), "src -> t -> u vs src -> u")
    assert_bitwise(u.get_state(), want, "the composed selection")
    for f in (s, t, u, v):
        f.close()


# ---- 7. batch form -----------------------------------------------------------------------------------------
def test_batch_form_equals_single_extractions(pkg, pipeline_mode):
    ns = (70, 33, 20, 64, 50, 0, 95, 40)  # (+ 1 each: the open window's New landmark)
    nd = (10, 90, 0, 64, 33, 50, 5, 96)
    s = _batch(pkg, 128, ns, seed=180)
    _open_batch_window(pkg, s)
    n_src = [n + 1 for n in ns]
    rng = np.random.default_rng(181)
    lists = [np.array([], dtype=np.int32),                       # the pose and P_RR alone
             np.arange(n_src[1], dtype=np.int32),                # the full map
             np.arange(n_src[2], dtype=np.int32)[::-1].copy(),   # ... reversed
             shuffled_ids(n_src[3], 40, seed=182), shuffled_ids(n_src[4], 33, seed=183), np.array([0], dtype=np.int32),
             shuffled_ids(n_src[6], 96, seed=184), rng.permutation(n_src[7]).astype(np.int32)[:7]]
    want = [len(v) for v in lists]
    # the batch form on one destination, then the one-filter calls on a destination with the same history
    d1 = _batch(pkg, 96, nd, seed=190)
    _open_batch_window(pkg, d1)
    assert list(d1.batch_extract_map(s, lists)) == want
    assert list(d1.num_landmarks()) == want
    got, poses = [d1.get_state(b) for b in range(8)], d1.poses().copy()
    assert list(d1.batch_extract_map(s)) == n_src  # every landmark of every filter: the source's largest map (96) just fits
    got_all = [d1.get_state(b) for b in range(8)]
    d1.close()
    d2 = _batch(pkg, 96, nd, seed=190)
    _open_batch_window(pkg, d2)
    for b in range(8):
        assert d2.extract_map(s, lists[b], index=b, src_index=b) == want[b]
    assert list(d2.num_landmarks()) == want
    src_states = [s.get_state(b) for b in range(8)]
    for b in range(8):
        assert_bitwise(got[b], d2.get_state(b), "filter %d" % b)
        assert_bitwise(got[b], index_state(src_states[b], lists[b]), "filter %d against the source" % b)
    assert np.array_equal(poses, d2.poses())
    for b in range(8):
        assert d2.extract_map(s, index=b, src_index=b) == n_src[b]
        assert_bitwise(got_all[b], d2.get_state(b), "copy of filter %d" % b)
        assert_bitwise(got_all[b], src_states[b], "copy of filter %d against the source" % b)
    s.close(), d2.close()


# ---- 8. the dense partial readout --------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SOURCES)
def test_get_submap(pkg, pipeline_mode, N, cap):
    a, w, _ = open_window_pair(pkg, N, cap, seed=201, steps=3)
    ids = shuffled_ids(N, 70, seed=202)
    idv, idp = int_array(ids)
    L = a.L
    assert L.ekf_get_submap(a.h, 0, idp, 70, None, None, 0) == 143  # the size alone
    got = a.get_submap(ids)
    held = w.get_state()  # the twin exports where the submap was read
    assert_bitwise(got, index_state(held, ids), "submap")
    assert_bitwise_symmetric(got[1])
    assert_bitwise(a.get_submap(ids), got, "a second call")
    n, ld = 143, 150
    xo, Po = np.full(n, np.nan), np.full((n, ld), np.nan)  # column j at Po[j]: rows n..ld-1 are the padding
    assert L.ekf_get_submap(a.h, 0, idp, 70, xo.ctypes.data_as(_DP), Po.ctypes.data_as(_DP), ld) == n
    assert np.array_equal(xo, got[0]) and np.array_equal(Po[:, :n], got[1]) and np.isnan(Po[:, n:]).all()
    x0, P0 = a.get_submap([])
    assert np.array_equal(x0, held[0][:3]) and np.array_equal(P0, held[1][:3, :3])
    assert a.stats() == w.stats() and a.decisions() == w.decisions()
    sc = pkg.scenarios.steady_script(held[0], steps=2, M=2, seed=209, min_separation=1.0)
    assert run_script(a, sc, 2, 2) == run_script(w, sc, 2, 2)
    assert_bitwise(a.get_state(), w.get_state(), "after get_submap vs after get_state")
    a.close(), w.close()


# ---- 9. errors ---------------------------------------------------------------------------------------------
def test_errors_change_nothing_and_capacity_is_not_sticky(pkg, pipeline_mode):
    a, aw, _ = open_window_pair(pkg, 60, 64, seed=211, steps=3)
    s, sw, _ = open_window_pair(pkg, 100, 200, seed=215, steps=3)
    aw.close(), sw.close()
    held_a, held_s = a.get_state(), s.get_state()
    L, E = a.L, pkg.ekfslam
    for bad in ([3, 7, 3], [5, 100], [-1, 2]):  # repeated, id = N, negative
        v, p = int_array(bad)
        assert L.ekf_extract_map(a.h, 0, s.h, 0, p, len(bad)) == E.ERR_BAD_ARG, bad
        assert L.ekf_get_submap(s.h, 0, p, len(bad), None, None, 0) == E.ERR_BAD_ARG, bad
    v, p = int_array([1, 2, 3])
    assert L.ekf_extract_map(a.h, 0, s.h, 0, p, -1) == E.ERR_BAD_ARG
    assert L.ekf_extract_map(a.h, 0, a.h, 0, p, 3) == E.ERR_BAD_ARG  # a filter into itself
    assert L.ekf_extract_map(a.h, 0, a.h, 0, None, 0) == E.ERR_BAD_ARG
    for di, si in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        assert L.ekf_extract_map(a.h, di, s.h, si, p, 3) == E.ERR_BAD_ARG
    assert L.ekf_extract_map(None, 0, s.h, 0, p, 3) == E.ERR_BAD_ARG and L.ekf_extract_map(a.h, 0, None, 0, p, 3) == E.ERR_BAD_ARG
    assert L.ekf_get_submap(None, 0, p, 3, None, None, 0) == E.ERR_BAD_ARG and L.ekf_get_submap(s.h, 1, p, 3, None, None, 0) == E.ERR_BAD_ARG
    assert L.ekf_get_submap(s.h, 0, p, -1, None, None, 0) == E.ERR_BAD_ARG
    four = pkg.FilterBatch(4, 16)
    assert L.ekf_batch_extract_map(a.h, four.h, None, 0, None, None) == E.ERR_BAD_ARG  # batch sizes
    assert L.ekf_batch_extract_map(four.h, four.h, None, 0, None, None) == E.ERR_BAD_ARG  # one handle
    assert L.ekf_batch_extract_map(None, s.h, None, 0, None, None) == E.ERR_BAD_ARG
    four.close()
    assert_bitwise(a.get_state(), held_a, "destination after bad arguments")
    assert_bitwise(s.get_state(), held_s, "source after bad arguments")
    ids = shuffled_ids(100, 70, seed=216)
    v, p = int_array(ids)
    assert L.ekf_extract_map(a.h, 0, s.h, 0, p, 70) == E.ERR_CAPACITY  # 70 > 64
    assert L.ekf_extract_map(a.h, 0, s.h, 0, None, 0) == E.ERR_CAPACITY  # 100 > 64
    a.sync()  # EKF_OK: nothing sticky
    assert_bitwise(a.get_state(), held_a, "destination after EKF_ERR_CAPACITY")
    assert_bitwise(s.get_state(), held_s, "source after EKF_ERR_CAPACITY")
    a.reserve(128)
    assert a.extract_map(s, ids) == 70
    assert_bitwise(a.get_state(), index_state(held_s, ids), "extraction after reserve")
    a.close(), s.close()


def test_a_sticky_capacity_status_of_the_source_does_not_block_the_call(pkg, pipeline_mode):
    g, _, _ = make_filter(pkg, 8, 8, seed=221)
    z, R = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    d = fresh(pkg, 16)
    assert d.extract_map(g, [5, 0, 7]) == 3
    sub = g.get_submap([5, 0, 7])
    held = g.get_state()
    assert_bitwise(d.get_state(), index_state(held, [5, 0, 7]), "from a full source")
    assert_bitwise(sub, index_state(held, [5, 0, 7]), "submap of a full source")
    d.sync()
    with pytest.raises(pkg.EkfError) as ei:
        g.sync()
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    d.close(), g.close()


# ---- 10. streaming -----------------------------------------------------------------------------------------
def test_both_handles_stream_again_after_the_call(pkg, pipeline_mode):
    s, sw, _ = open_window_pair(pkg, 200, 320, seed=231, steps=3)
    ids = np.array(nearest_isolated(sw.get_x(), 40), dtype=np.int32)[::-1].copy()
    d = fresh(pkg, 320)
    d.propagate(0.3, 0.05, 0.05)  # a streaming launch resident on the destination too
    on_s, s0 = stream_starts(s)
    on_d, d0 = stream_starts(d)
    assert d.extract_map(s, ids) == 40
    held = sw.get_state()
    sc_s = pkg.scenarios.steady_script(held[0], steps=2, M=2, seed=232, min_separation=1.0)
    assert run_script(s, sc_s, 2, 2) == run_script(sw, sc_s, 2, 2)
    if on_s:
        assert stream_starts(s)[1] > s0
    assert_bitwise(s.get_state(), sw.get_state(), "the source streams on")
    s.close(), sw.close()
    b = fresh(pkg, 320)
    b.set_state(*index_state(held, ids))
    sc_d = pkg.scenarios.steady_script(b.get_x(), steps=2, M=2, seed=233, min_separation=1.0)
    assert run_script(d, sc_d, 2, 2) == run_script(b, sc_d, 2, 2)
    if on_d:
        assert stream_starts(d)[1] > d0
    assert_bitwise(d.get_state(), b.get_state(), "the destination streams on")
    d.close(), b.close()
