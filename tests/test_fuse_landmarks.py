"""Landmark fusion on the device: ekf_fuse_landmarks / ekf_batch_fuse_landmarks (the equality constraint L_i = L_j of a pair list as
an update of the whole state in rounds of ekf_window pairs, then the removal of every j).  The reference is tests/fuse_ref.py (NumPy
on the dense export, rounds as the device takes them; checked on the CPU in tests/test_fuse_landmarks_cpu.py, where the same inputs
agree with their extended-precision restatement to 1/20 of the bounds used here), and the states come from its builder: a
destination map joined on the device with a source map whose first 24 landmarks re-observe destination landmarks.
Sizes follow tests/test_join_map.py: 200 landmarks in capacity 320 (k_chain), 100 in capacity 200 (k_solo where the pipeline mode
allows it), 70 source landmarks -- 270 and 170 joined, neither a multiple of 32."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref as fr  # noqa: E402
import map_model as mm  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, open_window_pair, stream_starts, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(200, 320), (100, 200)]
NS, CAP_S, N_DUP = 70, 96, 24


@functools.lru_cache(maxsize=None)
def built(pkg, N, seed=7, extent=7.0):
    out = fr.joined_with_duplicates(pkg, N, NS, N_DUP, seed, extent)
    for a in out[:6]:
        a.setflags(write=False)
    return out


def joined(pkg, N, cap, seed=7, max_pending=16, extent=7.0):
    """A handle that has joined the source map on the device, and the true pairs."""
    xg, Pg, xs, Ps, _, _, truth = built(pkg, N, seed, extent)
    a = pkg.FilterBatch(1, cap, max_pending=max_pending, log_capacity=4096)
    a.set_state(xg, Pg)
    s = pkg.FilterBatch(1, CAP_S, max_pending=16, log_capacity=4096)
    s.set_state(xs, Ps)
    assert a.join_map(s) == N + NS
    s.close()
    return a, truth


def loaded(pkg, x, P, cap, max_pending=16):
    f = pkg.FilterBatch(1, cap, max_pending=max_pending, log_capacity=4096)
    f.set_state(x, P)
    return f


def check(f, pre, pairs, slack, got, what, round_size=None):
    """The handle after fuse_landmarks(pairs) returned `got`, against the reference on the export `pre`; returns the reference."""
    ref = fr.fuse(pre[0], pre[1], pairs, slack, round_size or f.window)
    after = f.get_state()
    n_ref = (ref[0].size - 3) // 2
    assert got == (n_ref, ref[2]), (what, got, n_ref, ref[2])
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=what)
    print("%s: %d pairs, %d fused, max |dx| %.3e, max |dP| / max |P| %.3e" % (what, len(pairs), ref[2], err[0], err[1]))
    assert_bitwise_symmetric(after[1])
    assert int(f.num_landmarks()[0]) == n_ref
    assert np.array_equal(f.poses()[0], after[0][:3]) and np.array_equal(f.robot_cov(), after[1][:3, :3])
    return ref


# ---- 1. parity: join, find, fuse ------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [0.0, 1e-4])
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_after_join_and_find(pkg, pipeline_mode, N, cap, slack):
    a, truth = joined(pkg, N, cap)
    pre = a.get_state()
    found, n_found, _ = a.find_duplicates(split=N)
    assert n_found == len(found)
    pairs = pkg.ekfslam.duplicate_matching(found, N + NS)
    true = set(zip(truth["i"].tolist(), truth["j"].tolist()))
    assert true <= set(zip(pairs["i"].tolist(), pairs["j"].tolist()))  # every planted duplicate is found and matched
    st, dec = a.stats(), a.decisions()
    got = a.fuse_landmarks(pairs, slack=slack)
    assert got == (N + NS - len(pairs), len(pairs))
    check(a, pre, pairs, slack, got, "N=%d slack=%g" % (N, slack))
    assert a.stats() == st and a.decisions() == dec
    a.close()


# ---- 2. with a window open --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_with_a_window_open(pkg, pipeline_mode, N, cap):
    _, _, _, _, x, P, truth = built(pkg, N)
    a, b = loaded(pkg, x, P, cap), loaded(pkg, x, P, cap)
    for f in (a, b):  # the same immediate calls: a slot in the open window, a streaming launch live
        f.propagate(0.3, 0.05, 0.05)
        z, R = pkg.scenarios.measurement_from_feature_mm(80000.0, 30000.0)
        assert f.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2))[0][0][0] == pkg.ekfslam.NEW
    pre = b.get_state()
    got = a.fuse_landmarks(truth)
    check(a, pre, truth, 0.0, got, "window open, N=%d" % N)
    a.close(), b.close()


def test_open_window_pair_of_the_helpers(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    pre = b.get_state()
    pairs = fr.as_pairs([(3, 40), (31, 32), (63, 64), (5, 99)])
    got = a.fuse_landmarks(pairs, slack=1e-4)
    check(a, pre, pairs, 1e-4, got, "helpers.open_window_pair")
    a.close(), b.close()


# ---- 3. rounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pending,order", [(8, 1), (8, -1), (1, 1)])
@pytest.mark.parametrize("N,cap", SIZES)
def test_rounds(pkg, pipeline_mode, N, cap, max_pending, order):
    _, _, _, _, x, P, truth = built(pkg, N)
    pairs = truth[::order] if max_pending > 1 else truth[:5]
    a = loaded(pkg, x, P, cap, max_pending)
    assert a.window <= max_pending and (max_pending != 8 or a.window == 8)  # 24 pairs in windows of 8: three passes
    w0 = windows_closed(a)
    got = a.fuse_landmarks(pairs)
    assert windows_closed(a) == w0  # the rounds' passes are the call's own: no window of the filter was closed
    ref = check(a, (x, P), pairs, 0.0, got, "window %d, order %d" % (a.window, order), round_size=a.window)
    joint = fr.fuse(x, P, pairs, 0.0)  # all at once: the same up to rounding
    assert_state_close(ref[0], ref[1], joint[0], joint[1], what="rounds vs joint")
    a.close()


# ---- 4. tile edges ----------------------------------------------------------------------------------------
EDGE_LISTS = [
    [(31, 32), (63, 64)],             # i and j either side of a tile edge
    [(2, 3), (40, 41), (65, 95)],     # i and j in the same tile
    [(0, 97), (1, 96), (30, 98)],     # first and last tile
    [(5, 127)],                       # the last landmark of a full-capacity map (N = capacity = 128)
]


@pytest.mark.parametrize("k", range(len(EDGE_LISTS)))
def test_tile_edges(pkg, pipeline_mode, k):
    N = 128 if k == 3 else 100
    x, P = pkg.scenarios.injected_state(N, seed=51 + k, extent=15.0)
    a = loaded(pkg, x, P, 128)
    pairs = fr.as_pairs(EDGE_LISTS[k])
    got = a.fuse_landmarks(pairs, slack=1e-4)
    check(a, (x, P), pairs, 1e-4, got, "edges %s" % EDGE_LISTS[k])
    a.close()


def test_two_landmarks_one_pair(pkg, pipeline_mode):
    x, P = pkg.scenarios.injected_state(2, seed=61, extent=5.0)
    a = loaded(pkg, x, P, 64)
    got = a.fuse_landmarks([(0, 1)])
    assert got == (1, 1)
    check(a, (x, P), fr.as_pairs([(0, 1)]), 0.0, got, "N = 1 + 1")
    a.close()


def test_no_pairs_is_a_no_op(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=71, steps=3)
    w0, s0 = windows_closed(a), stream_starts(a)
    assert a.fuse_landmarks(np.zeros(0, dtype=fr.DUP_DTYPE)) == (int(b.num_landmarks()[0]), 0)
    assert a.fuse_landmarks([], index=0) == (int(b.num_landmarks()[0]), 0)
    assert windows_closed(a) == w0 and stream_starts(a) == s0  # window and stream as they were
    assert_bitwise(a.get_state(), b.get_state(), "n_pairs = 0")
    a.close(), b.close()


# ---- 5. buffers are left as ekf_set_state leaves them -----------------------------------------------------
def isolated_of(x, candidates, count):
    L = x[3:].reshape(-1, 2)
    d2 = ((L[:, None, :] - L[None, :, :]) ** 2).sum(-1)
    d2[np.diag_indices(L.shape[0])] = np.inf
    iso = np.sqrt(d2.min(axis=1))
    r = np.hypot(*(L - x[0:2]).T)
    ok = [l for l in candidates if iso[l] >= 0.5 and r[l] >= 1.0]
    assert len(ok) >= count, (len(ok), count)
    return sorted(ok, key=lambda l: r[l])[:count]


def measurement_of(pkg, x, l):
    c, s = np.cos(x[2]), np.sin(x[2])
    d = x[3 + 2 * l:5 + 2 * l] - x[0:2]
    return pkg.scenarios.measurement_from_feature_mm(1000.0 * (c * d[0] + s * d[1]), 1000.0 * (-s * d[0] + c * d[1]))


def continue_both(pkg, a, b, fused, renumbered):
    """The same further calls on the fused handle `a` and its set_state twin `b` (window of 8): propagations, Old matches of fused and
    of renumbered landmarks, a far New landmark, a compass update -- ten slots, so a window closes on the way.  Bitwise equal ends."""
    x = a.get_x()
    assert np.array_equal(x, b.get_x())
    olds, news = isolated_of(x, fused, 4), isolated_of(x, renumbered, 4)
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
        assert (da[at + 1][0], da[at + 1][1]) == (pkg.ekfslam.OLD, 3 + 2 * news[s]), (s, da[at + 1])
    assert da[4][0] == pkg.ekfslam.NEW
    assert_bitwise(a.get_state(), b.get_state(), "fused handle vs set_state twin")


@pytest.mark.parametrize("N,cap", SIZES)
def test_set_state_twin_goes_on_bit_for_bit(pkg, pipeline_mode, N, cap):
    a, truth = joined(pkg, N, cap, seed=9, max_pending=8, extent=20.0)
    n, nf = a.fuse_landmarks(truth, slack=1e-4)
    assert (n, nf) == (N + NS - N_DUP, N_DUP)
    b = loaded(pkg, *a.get_state(), cap, 8)
    first_gone = int(truth["j"].min())
    continue_both(pkg, a, b, truth["i"].tolist(), range(first_gone, n))
    a.close(), b.close()


# ---- 6. determinism and the batch form --------------------------------------------------------------------
def test_same_call_same_bits_and_batch_equals_single_calls(pkg, pipeline_mode):
    counts = (100, 45, 64, 33)
    lists = [[(0, 99), (31, 32), (63, 64), (5, 6), (40, 80)], [], [(1, 63)], [(k, 32 - k) for k in range(10)]]
    hs = []
    for _ in range(3):
        f = pkg.FilterBatch(4, 128, max_pending=4, log_capacity=4096)
        for b, n in enumerate(counts):
            f.set_state(*pkg.scenarios.injected_state(n, seed=80 + b, extent=10.0 + b), index=b)
        hs.append(f)
    before = [hs[0].get_state(b) for b in range(4)]
    n1, f1 = hs[0].fuse_landmarks(lists, slack=1e-5, index=None)
    n2, f2 = hs[1].fuse_landmarks(lists, slack=1e-5, index=None)
    want = [counts[b] - len(lists[b]) for b in range(4)]
    assert list(n1) == list(n2) == want and list(f1) == list(f2) == [len(p) for p in lists]
    for b in range(4):
        got = hs[2].fuse_landmarks(lists[b], slack=1e-5, index=b)
        assert got == (want[b], len(lists[b]))
        s1 = hs[0].get_state(b)
        assert_bitwise(s1, hs[1].get_state(b), "two identical handles, filter %d" % b)
        assert_bitwise(s1, hs[2].get_state(b), "batch form vs single call, filter %d" % b)
        ref = fr.fuse(*before[b], fr.as_pairs(lists[b]), 1e-5, hs[0].window)
        assert_state_close(s1[0], s1[1], ref[0], ref[1], what="filter %d" % b)
    assert_bitwise(hs[0].get_state(1), before[1], "the filter without a pair")
    for f in hs:
        f.close()


# ---- 7. S not positive definite ---------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [0.0, 1e-4])
def test_exact_copy_in_the_second_round(pkg, pipeline_mode, slack):
    x0, P0 = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    x, P = fr.with_exact_copy(x0, P0, 17)  # landmark 60 is landmark 17 again
    pairs = fr.as_pairs([(0, 33), (1, 50), (31, 32), (2, 59), (17, 60), (3, 40), (4, 41)])
    a = loaded(pkg, x, P, 128, max_pending=4)
    got = a.fuse_landmarks(pairs, slack=slack)
    ref = check(a, (x, P), pairs, slack, got, "exact copy, slack %g" % slack, round_size=4)
    if slack == 0.0:  # round 1 is applied, round 2 is not: exactly the first four j are gone
        assert got == (57, 4) and ref[2] == 4
        keep = np.ones(61, dtype=bool)
        keep[pairs["j"][:4]] = False
        only_removed = mm.reduce_state(x, P, keep)
        assert only_removed[0].shape == a.get_x().shape  # (the copy and the pairs of rounds 2 stay two landmarks each)
    else:
        assert got == (54, 7)
    a.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=101, steps=3)
    held = b.get_state()
    N = (held[0].size - 3) // 2
    L, E = a.L, pkg.ekfslam
    import ctypes
    P_ = ctypes.POINTER(E.EkfDupPair)

    def call(rows, slack=0.0, index=0, n=None, null=False):
        buf = fr.as_pairs(rows)
        return L.ekf_fuse_landmarks(a.h, index, None if null else buf.ctypes.data_as(P_), len(buf) if n is None else n, slack, None)

    assert call([(1, 2), (2, 3)]) == E.ERR_BAD_ARG        # a repeated landmark
    assert call([(1, 2), (0, 1)]) == E.ERR_BAD_ARG
    assert call([(3, 3)]) == E.ERR_BAD_ARG                # i >= j
    assert call([(5, 4)]) == E.ERR_BAD_ARG
    assert call([(-1, 4)]) == E.ERR_BAD_ARG
    assert call([(0, N)]) == E.ERR_BAD_ARG                # j >= N
    assert call([(0, 1)], slack=-1e-9) == E.ERR_BAD_ARG
    assert call([(0, 1)], slack=float("nan")) == E.ERR_BAD_ARG
    assert call([(0, 1)], slack=float("inf")) == E.ERR_BAD_ARG
    assert call([(0, 1)], index=1) == E.ERR_BAD_ARG and call([(0, 1)], index=-1) == E.ERR_BAD_ARG
    assert call([(0, 1)], null=True) == E.ERR_BAD_ARG     # a null list with n_pairs > 0
    assert call([(0, 1)], n=-1) == E.ERR_BAD_ARG
    assert L.ekf_fuse_landmarks(None, 0, None, 0, 0.0, None) == E.ERR_BAD_ARG
    cnt, out = np.array([1], dtype=np.int32), np.zeros(1, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    assert L.ekf_batch_fuse_landmarks(a.h, None, 1, cnt.ctypes.data_as(ip), 0.0, None, out.ctypes.data_as(ip)) == E.ERR_BAD_ARG
    assert L.ekf_batch_fuse_landmarks(a.h, None, 1, None, 0.0, None, out.ctypes.data_as(ip)) == E.ERR_BAD_ARG
    with pytest.raises(ValueError):
        a.fuse_landmarks([(0, 1)], slack=-1.0)
    assert_bitwise(a.get_state(), held, "after the refusals")
    got = a.fuse_landmarks([(0, 1), (2, 59)])  # the next valid call works
    check(a, held, fr.as_pairs([(0, 1), (2, 59)]), 0.0, got, "after the refusals")
    a.close(), b.close()


# ---- 9. after ekf_reserve -----------------------------------------------------------------------------------
def test_fuse_reserve_fuse(pkg, pipeline_mode):
    _, _, _, _, x, P, truth = built(pkg, 100)
    a = loaded(pkg, x, P, 200)
    bytes0 = a.device_bytes()
    got = a.fuse_landmarks(truth[:12])
    check(a, (x, P), truth[:12], 0.0, got, "before the reserve")
    bytes1 = a.device_bytes()
    assert bytes1 > bytes0  # the scratch is counted
    mid = a.get_state()
    a.reserve(320)  # the other side of 256: another kernel family, another tile numbering
    assert_bitwise(a.get_state(), mid, "reserve after the fuse")
    assert a.device_bytes() > bytes1
    # the remaining twelve true pairs in the reduced numbering: their j moved down by the number of removed j in front of them
    gone = np.sort(truth["j"][:12])
    rest = truth[12:].copy()
    rest["j"] -= np.searchsorted(gone, rest["j"]).astype(np.int32)
    got = a.fuse_landmarks(rest, slack=1e-4)
    check(a, mid, rest, 1e-4, got, "after the reserve")
    a.close()


# ---- 10. the KalmanFilter shim --------------------------------------------------------------------------------
def test_kalman_filter_shim_refreshes_its_mirror(pkg, pipeline_mode):
    _, _, _, _, x, P, truth = built(pkg, 100)
    kf = pkg.KalmanFilter(capacity_landmarks=200)
    kf.set_state(x, P)
    assert kf.Num_Landmarks == 100 + NS
    assert kf.fuse_landmarks(truth, slack=1e-4) == (100 + NS - N_DUP, N_DUP)
    xa, _ = kf.state()
    ref = fr.fuse(x, P, truth, 1e-4, kf._f.window)
    assert kf.Num_Landmarks == 100 + NS - N_DUP
    assert (kf.X, kf.Y, kf.Phi) == (xa[0], xa[1], xa[2])
    assert abs(kf.X - ref[0][0]) <= 1e-9 and abs(kf.Y - ref[0][1]) <= 1e-9 and abs(kf.Phi - ref[0][2]) <= 1e-9
    assert (kf.X, kf.Y, kf.Phi) != (x[0], x[1], x[2])  # the fusion moved the pose
