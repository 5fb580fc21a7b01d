"""Polar measurements on the device: ekf_update_polar / ekf_polar_compat and their batch forms (range, bearing and range-bearing
measurements of known landmarks as joint updates in rounds of ekf_window entries; the read-only score of one list).  The reference
is tests/polar_ref.py (NumPy on the dense export, rounds as the device takes them, the inert row of a one-component entry kept;
checked on the CPU in tests/test_update_polar_cpu.py, where the same inputs agree with the textbook form and with their
extended-precision restatement to 1/20 of the bounds used here).  The inputs are polar_ref.gpu_inputs': 200 landmarks in capacity 320
(k_chain) and 100 in capacity 200 (k_solo where the pipeline mode allows it).
d2 is compared relatively within polar_ref.D2_REL = 6.89e-12: 20 times the 3.444e-13 the CPU test measures between the double
reference and its extended-precision restatement over these inputs."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
import polar_ref as pr  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, open_window_pair, run_steps, stream_starts, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = pr.SIZES
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
RG, BR, BO = pr.RANGE, pr.BEARING, pr.BOTH


@functools.lru_cache(maxsize=None)
def mixed(pkg, N):
    x, P = pkg.scenarios.injected_state(N, seed=pr.STATE_SEED[N], extent=mr.map_extent(N))
    out = (x, P) + pr.mixed_list(pkg, x, P, pr.STATE_SEED[N])
    for a in out:
        a.setflags(write=False)
    return out


def loaded(pkg, x, P, cap, max_pending=16):
    f = pkg.FilterBatch(1, cap, max_pending=max_pending, log_capacity=4096)
    f.set_state(x, P)
    return f


def assert_d2_close(got, want, what):
    mr.assert_d2_close(got, want, what, pr.D2_REL)


def check(f, pre, lst, got, name, round_size=None, index=0):
    """Filter `index` after update_polar(*lst) answered `got`, against the reference on the export `pre`; returns the reference."""
    ref = pr.update(pre[0], pre[1], *lst, round_size or f.window)
    after = f.get_state(index)
    n, applied, d2 = got
    assert (n, applied) == ((pre[0].size - 3) // 2, ref[2]), (name, n, applied, ref[2])
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=name)
    print("%s: %d entries, %d applied, max |dx| %.3e, max |dP| / max |P| %.3e" % (name, len(lst[2]), applied, err[0], err[1]))
    assert_d2_close(d2, ref[3], name)
    assert_bitwise_symmetric(after[1])
    assert np.all(np.isfinite(after[0])) and np.all(np.isfinite(after[1]))
    assert int(f.num_landmarks()[index]) == n
    assert np.array_equal(f.poses()[index], after[0][:3])
    if f.batch == 1:
        assert np.array_equal(f.robot_cov(), after[1][:3, :3])
    return ref


# ---- 1. parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_on_the_mixed_list(pkg, pipeline_mode, N, cap):
    x, P, z, R, ids, kind = mixed(pkg, N)
    a = loaded(pkg, x, P, cap)
    st, dec = a.stats(), a.decisions()
    got = a.update_polar(z, R, ids, kind)
    assert got[1] == 22
    check(a, (x, P), (z, R, ids, kind), got, "N=%d" % N)
    assert a.stats() == st and a.decisions() == dec
    a.close()


# ---- 2. rounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_rounds(pkg, pipeline_mode, N, cap):
    """Each window against the reference with the same round size: the model is linearised at every round's entry state, so the
    windows are not compared with each other."""
    x, P, z, R, ids, kind = mixed(pkg, N)
    kept = np.flatnonzero(ids >= 0)
    for mp in (1, 5, 16, 32):
        a = loaded(pkg, x, P, cap, max_pending=mp)
        assert a.window == mp
        w0 = windows_closed(a)
        got = a.update_polar(z, R, ids, kind)
        assert windows_closed(a) == w0  # the rounds' passes are the call's own: no window of the filter was closed
        assert check(a, (x, P), (z, R, ids, kind), got, "N=%d, window %d" % (N, mp))[2] == 22
        for r0 in range(0, len(kept), mp):  # a running distance per round
            assert np.all(np.diff(got[2][kept[r0:r0 + mp]]) >= 0.0)
        a.close()
    a = loaded(pkg, x, P, cap)  # 9 entries in a window of 16: 18 columns, into the second chunk of k_fuse_apply
    nine = pr.list_of_nine(z, R, ids, kind)
    assert a.window == 16 and int((nine[2] >= 0).sum()) == 9
    assert check(a, (x, P), nine, a.update_polar(*nine), "N=%d, list of 9" % N)[2] == 9
    a.close()


@pytest.mark.parametrize("N,cap", SIZES)
def test_a_round_of_the_whole_factor(pkg, pipeline_mode, N, cap):
    """32 BOTH entries in a window of 32: all 64 columns live, every chunk of k_fuse_apply and the whole of FUSE_MAX_COLS."""
    x, P = mixed(pkg, N)[:2]
    lst = pr.uniform_list(x, BO, 32, 400 + N)
    a = loaded(pkg, x, P, cap, max_pending=32)
    assert a.window == 32
    jc = a.polar_compat(*lst)
    got = a.update_polar(*lst)
    assert got[1] == 32 and got[2].tobytes() == jc.tobytes()
    check(a, (x, P), lst, got, "32 BOTH N=%d" % N)
    a.close()


# ---- 3. kinds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kd", [RG, BR])
@pytest.mark.parametrize("N,cap", SIZES)
def test_one_component_lists(pkg, pipeline_mode, N, cap, kd):
    """A list of RANGE entries alone and one of BEARING entries alone: every second column is inert.  The kernel writes the inert
    row's entries of S, d and W as constants, so its pivot is 1 and its y an exact zero, and fuse_prefix_d2 adds 0.0 * 0.0.  From
    outside that shows as the running distance of the reference, whose inert increments are exactly 0.0 (asserted on the CPU),
    within D2_REL, entry by entry -- one inert y of the size of a live one would miss it by orders --, and in the score of a list
    being bit for bit that of each of its prefixes."""
    x, P = mixed(pkg, N)[:2]
    lst = pr.uniform_list(x, kd, 12, (500 if kd == RG else 600) + N)
    z, R, ids, kind = lst
    a = loaded(pkg, x, P, cap)
    jc = a.polar_compat(*lst)
    for k in (1, 5, 12):   # the inert columns in front of entry k - 1 have added exactly 0.0 to its distance
        head = a.polar_compat(z[:k], R[:k], ids[:k], kind[:k])
        assert head.tobytes() == jc[:k].tobytes()
    ref = pr.compat(x, P, *lst)
    assert_d2_close(jc, ref, "polar_compat, one kind")
    assert np.all(np.diff(np.concatenate([[0.0], ref])) > 0.0) and np.all(np.diff(np.concatenate([[0.0], jc])) > 0.0)   # (every live column adds something)
    got = a.update_polar(*lst)
    assert got[1] == 12 and got[2].tobytes() == jc.tobytes()
    check(a, (x, P), lst, got, "%s only N=%d" % ("RANGE" if kd == RG else "BEARING", N))
    a.close()


def test_a_both_entry_split_into_its_components_scores_the_same(pkg, pipeline_mode):
    """BOTH with a diagonal R against the same landmark as a RANGE and a BEARING entry: the same two live rows with an inert column
    between and behind them.  The inert columns' y are exact zeros, so the two distances differ by the rounding of the elimination's
    other order alone (D2_REL)."""
    x, P, z, R, ids, kind = mixed(pkg, 100)
    i = int(ids[0])
    assert kind[0] == BO
    Rd = np.diag(np.diag(R[0]))
    a = loaded(pkg, x, P, 200)
    both = a.polar_compat(z[:1], Rd[None], [i], [BO])
    split = a.polar_compat(np.array([z[0], z[0]]), np.array([Rd, Rd]), [i, i], [RG, BR])
    assert abs(split[1] - both[0]) <= pr.D2_REL * both[0] and 0.0 < split[0] < split[1]
    assert_bitwise(a.get_state(), (x, P), "polar_compat only reads")
    a.close()


# ---- 4. compat ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_polar_compat(pkg, pipeline_mode, N, cap):
    x, P, z, R, ids, kind = mixed(pkg, N)
    a = loaded(pkg, x, P, cap, max_pending=8)
    before, st, dec = a.get_state(), a.stats(), a.decisions()
    w0 = windows_closed(a)
    d2 = a.polar_compat(z, R, ids, kind)  # 22 entries on a window of 8
    assert_d2_close(d2, pr.compat(x, P, z, R, ids, kind), "polar_compat N=%d" % N)
    assert d2.tobytes() == a.polar_compat(z, R, ids, kind).tobytes()  # two calls, the same bits
    z32, R32, i32, k32 = (np.concatenate([v, v[8:18]]) for v in (z, R, ids, kind))
    assert int((i32 >= 0).sum()) == 32
    d32 = a.polar_compat(z32, R32, i32, k32)
    assert_d2_close(d32, pr.compat(x, P, z32, R32, i32, k32), "list of 32")
    assert d32[:24].tobytes() == d2.tobytes()  # extending a list leaves its prefix as it was
    z33, R33, i33, k33 = (np.concatenate([v, w[:1]]) for v, w in ((z32, z), (R32, R), (i32, ids), (k32, kind)))
    i33, k33 = i33.astype(np.int32), k33.astype(np.int32)
    Rc = np.ascontiguousarray(np.swapaxes(R33, 1, 2).reshape(-1, 4))
    out = np.zeros(len(i33))
    assert a.L.ekf_polar_compat(a.h, 0, z33.ctypes.data_as(DP), Rc.ctypes.data_as(DP), i33.ctypes.data_as(IP), k33.ctypes.data_as(IP), len(i33),
                                out.ctypes.data_as(DP)) == pkg.ekfslam.ERR_BAD_ARG   # 33 entries
    with pytest.raises(ValueError):
        a.polar_compat(z33, R33, i33, k33)
    i33[5] = -1  # 32 entries and a skip more: accepted
    assert np.isnan(a.polar_compat(z33, R33, i33, k33)[5])
    assert_bitwise(a.get_state(), before, "polar_compat only reads")
    assert windows_closed(a) == w0 and a.stats() == st and a.decisions() == dec
    # the same list in one round of update_polar: the same bits
    b = loaded(pkg, x, P, cap, max_pending=16)
    k8 = a.polar_compat(z[:9], R[:9], ids[:9], kind[:9])   # (8 entries and a skip)
    assert a.update_polar(z[:9], R[:9], ids[:9], kind[:9])[2].tobytes() == k8.tobytes()
    k16 = b.polar_compat(z[:17], R[:17], ids[:17], kind[:17])
    assert b.update_polar(z[:17], R[:17], ids[:17], kind[:17])[2].tobytes() == k16.tobytes()
    assert k16[:9].tobytes() == k8.tobytes()
    a.close(), b.close()


# ---- 5. refusal -----------------------------------------------------------------------------------------
def test_singular_round_is_not_applied(pkg, pipeline_mode):
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    a, b = loaded(pkg, x, P, 128, max_pending=4), loaded(pkg, x, P, 128, max_pending=4)
    lst = pr.singular_list(pkg, x, P)  # the same landmark's range twice with R = 0 at the head of round two of three
    z, R, ids, kind = lst
    n, applied, d2 = a.update_polar(*lst)
    assert (n, applied) == (60, 4) and not np.isnan(d2[:4]).any() and np.isnan(d2[4:]).all()
    check(a, (x, P), lst, (n, applied, d2), "singular second round", round_size=4)
    assert b.update_polar(z[:4], R[:4], ids[:4], kind[:4])[:2] == (60, 4)
    assert_bitwise(a.get_state(), b.get_state(), "the state after the completed round")
    bad = a.polar_compat(z[4:7], R[4:7], ids[4:7], kind[4:7])
    assert not np.isnan(bad[0]) and np.isnan(bad[1:]).all()
    pre = a.get_state()  # the handle works on: the rest without the copy
    rest = [4, 6, 7, 8, 9]
    sub = tuple(v[rest] for v in lst)
    got = a.update_polar(*sub)
    assert got[1] == 5
    check(a, pre, sub, got, "behind the refusal")
    a.close(), b.close()


@pytest.mark.parametrize("kd", [RG, BR, BO])
def test_a_landmark_on_the_pose_is_refused(pkg, pipeline_mode, kd):
    """q == 0 at the entry state of round one (behind a completed round the pose and the landmark have moved apart): the round is
    refused like a non-positive pivot, nothing is applied, and no NaN or Inf reaches the filter."""
    x, P = pr.on_pose_state(pkg)
    a = loaded(pkg, x, P, 128, max_pending=4)
    before = a.get_state()
    assert np.array_equal(before[0][3 + 2 * pr.ON_POSE:5 + 2 * pr.ON_POSE], before[0][0:2])
    lst = pr.on_pose_list(pkg, x, P, kd)
    z, R, ids, kind = lst
    jc = a.polar_compat(*lst)
    assert not np.isnan(jc[0]) and np.isnan(jc[1:]).all()   # the entry in front of it keeps its distance
    n, applied, d2 = a.update_polar(*lst)
    assert (n, applied) == (60, 0) and np.isnan(d2).all()
    after = a.get_state()
    assert np.all(np.isfinite(after[0])) and np.all(np.isfinite(after[1]))
    assert_bitwise(after, before, "a call with no completed round")
    assert np.array_equal(a.poses()[0], before[0][:3]) and np.array_equal(a.robot_cov(), before[1][:3, :3])
    rest = np.arange(10) != 1   # the handle works on: the list without that entry
    sub = tuple(v[rest] for v in lst)
    got = a.update_polar(*sub)
    assert got[1] == 9
    check(a, before, sub, got, "behind the refusal, kind %d" % kd)
    a.close()


# ---- 6. batch -------------------------------------------------------------------------------------------
def test_batch_equals_single_calls_bit_for_bit(pkg, pipeline_mode):
    """Three filters of 100, 45 and 64 landmarks in capacity 128, window 4, ragged lists padded with -1."""
    states = mr.batch_states(pkg, pr.BATCH_COUNTS, 80)
    hs = []
    for _ in range(3):
        f = pkg.FilterBatch(3, 128, max_pending=4, log_capacity=4096)
        for b, (x, P) in enumerate(states):
            f.set_state(x, P, index=b)
        hs.append(f)
    before = [hs[0].get_state(b) for b in range(3)]
    z, R, ids, kind = pr.batch_lists(pkg, before)
    want = [int((ids[b] >= 0).sum()) for b in range(3)]
    assert want == [8, 3, 8] and hs[0].window == 4
    ap1, d1 = hs[0].update_polar(z, R, ids, kind, index=None)
    ap2, d2 = hs[1].update_polar(z, R, ids, kind, index=None)
    jc = hs[2].polar_compat(z, R, ids, kind, index=None)
    assert list(ap1) == list(ap2) == want and d1.tobytes() == d2.tobytes()
    assert np.array_equal(np.isnan(d1), ids < 0)
    for b in range(3):
        n, ap, db = hs[2].update_polar(z[b], R[b], ids[b], kind[b], index=b)
        assert (n, ap) == (pr.BATCH_COUNTS[b], want[b])
        s1 = hs[0].get_state(b)
        assert_bitwise(s1, hs[1].get_state(b), "two identical handles, filter %d" % b)
        assert_bitwise(s1, hs[2].get_state(b), "batch form vs single call, filter %d" % b)
        assert db.tobytes() == d1[b].tobytes()
        check(hs[0], before[b], (z[b], R[b], ids[b], kind[b]), (pr.BATCH_COUNTS[b], int(ap1[b]), d1[b]), "batch filter %d" % b, index=b)
        assert_d2_close(jc[b], pr.compat(*before[b], z[b], R[b], ids[b], kind[b]), "polar_compat, filter %d" % b)
    for f in hs:
        f.close()


# ---- 7. window open, streaming launch live --------------------------------------------------------------
def test_with_a_window_open(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    pre = b.get_state()
    ids = np.array(pr.OPEN_WINDOW_IDS, dtype=np.int32)
    kind = pr.cycle(len(ids))
    lst = pr.entries_for(pre[0], ids, kind, 313) + (ids, kind)
    st, dec = b.stats(), b.decisions()
    t = loaded(pkg, pre[0], pre[1], 200)   # a settled copy of the witness's state
    got = a.update_polar(*lst)
    check(a, pre, lst, got, "helpers.open_window_pair")
    gt = t.update_polar(*lst)
    assert gt[:2] == got[:2] and gt[2].tobytes() == got[2].tobytes()
    assert_bitwise(a.get_state(), t.get_state(), "the call behind an open window vs on a settled copy")
    assert a.stats() == st and a.decisions() == dec
    # immediate calls go on, streaming again where the handle streams, exactly as on the twin
    on, starts0 = stream_starts(a)
    sc = pkg.scenarios.steady_script(a.get_state()[0], steps=6, M=2, seed=104, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc, 0, 6, 2)
    dt, _ = run_steps(pkg, t, sc, 0, 6, 2)
    if on:
        assert stream_starts(a)[1] > starts0
    assert da == dt
    assert_bitwise(a.get_state(), t.get_state(), "streamed continuation")
    a.close(), b.close(), t.close()


def test_only_skips_is_a_no_op(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=71, steps=3)
    w0, s0 = windows_closed(a), stream_starts(a)
    N = int(b.num_landmarks()[0])
    nan3 = np.full((3, 2), np.nan)
    n, applied, d2 = a.update_polar(nan3, np.full((3, 2, 2), np.nan), [-1, -1, -1], [0, 7, -3])
    assert (n, applied) == (N, 0) and np.all(np.isnan(d2))
    n, applied, d2 = a.update_polar(np.zeros((0, 2)), np.zeros((0, 2, 2)), [], [])
    assert (n, applied, d2.size) == (N, 0, 0)
    assert windows_closed(a) == w0 and stream_starts(a) == s0  # window and stream as they were
    assert np.all(np.isnan(a.polar_compat(nan3, np.full((3, 2, 2), np.nan), [-1, -1, -1], [BO, BO, BO])))
    assert windows_closed(a) == w0
    assert_bitwise(a.get_state(), b.get_state(), "no entry")
    a.close(), b.close()


# ---- 8. bad arguments -----------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=101, steps=3)
    held = b.get_state()
    N = (held[0].size - 3) // 2
    L, BAD = a.L, pkg.ekfslam.ERR_BAD_ARG
    i0 = np.array([2, 5, 7], dtype=np.int32)
    k0 = np.array([BO, RG, BR], dtype=np.int32)
    z0, R0 = pr.entries_for(held[0], i0, k0, 5)
    z0, R0 = np.nan_to_num(z0, nan=1.0), np.nan_to_num(R0, nan=0.0)   # (finite everywhere: each refusal below has one cause)

    def raw(z, R, ids, kind, index=0, n=None, null=None):
        z, Rc = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(np.swapaxes(np.asarray(R, dtype=np.float64), 1, 2).reshape(-1, 4))
        ids, kind = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(kind, dtype=np.int32)
        ptr = [z.ctypes.data_as(DP), Rc.ctypes.data_as(DP), ids.ctypes.data_as(IP), kind.ctypes.data_as(IP)]
        if null is not None:
            ptr[null] = None
        n = len(ids) if n is None else n
        out = np.zeros(max(len(ids), 1))
        return (L.ekf_update_polar(a.h, index, *ptr, n, None, None), L.ekf_polar_compat(a.h, index, *ptr, n, out.ctypes.data_as(DP)))

    assert raw(z0, R0, [2, 5, N], k0) == (BAD, BAD)           # id >= N
    assert raw(z0, R0, [2, -2, 7], k0) == (BAD, BAD)          # id < -1
    assert raw(z0, R0, i0, [BO, 0, BR]) == (BAD, BAD)         # a kind of 0
    assert raw(z0, R0, i0, [BO, RG, 4]) == (BAD, BAD)         # a kind of 4
    for at in ((0, 0), (0, 1), (1, 0), (2, 1)):
        zb = z0.copy()
        zb[at] = np.nan
        assert raw(zb, R0, i0, k0) == (BAD, BAD)              # NaN in a z that is read
    for at in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (2, 1, 1)):
        Rb = R0.copy()
        Rb[at] = np.inf
        assert raw(z0, Rb, i0, k0) == (BAD, BAD)              # inf in an R that is read
    for at in ((1, 0, 0), (2, 1, 1)):
        Rb = R0.copy()
        Rb[at] = -1e-6
        assert raw(z0, Rb, i0, k0) == (BAD, BAD)              # a negative variance of a one-component entry
    for null in range(4):
        assert raw(z0, R0, i0, k0, null=null) == (BAD, BAD)   # a null list with n > 0
    assert raw(z0, R0, i0, k0, n=-1) == (BAD, BAD)
    assert raw(z0, R0, i0, k0, index=1) == (BAD, BAD) and raw(z0, R0, i0, k0, index=-1) == (BAD, BAD)
    assert L.ekf_update_polar(None, 0, None, None, None, None, 0, None, None) == BAD and L.ekf_batch_update_polar(None, None, None, None, None, 0, None, None) == BAD
    assert L.ekf_polar_compat(None, 0, None, None, None, None, 0, None) == BAD and L.ekf_batch_polar_compat(None, None, None, None, None, 0, None) == BAD
    assert L.ekf_polar_compat(a.h, 0, z0.ctypes.data_as(DP), z0.ctypes.data_as(DP), i0.ctypes.data_as(IP), k0.ctypes.data_as(IP), 1, None) == BAD  # no d2_out
    assert_bitwise(a.get_state(), held, "after the refusals")
    # what a kind does not read may be anything; the next valid call works
    zn, Rn = z0.copy(), R0.copy()
    zn[1, 1], Rn[1, 0, 1], Rn[1, 1, 0], Rn[1, 1, 1] = np.nan, np.nan, np.inf, -1.0
    zn[2, 0], Rn[2, 0, 0], Rn[2, 0, 1], Rn[2, 1, 0] = np.inf, -1.0, np.nan, np.nan
    jc = a.polar_compat(zn, Rn, i0, k0)
    got = a.update_polar(zn, Rn, i0, k0)
    assert got[1] == 3 and got[2].tobytes() == jc.tobytes()
    check(a, held, (z0, R0, i0, k0), got, "after the refusals")
    a.close(), b.close()


# ---- 9. surrounding state -------------------------------------------------------------------------------
def test_kalman_filter_shim_refreshes_its_mirror(pkg, pipeline_mode):
    x, P, z, R, ids, kind = mixed(pkg, 100)
    kf = pkg.KalmanFilter(capacity_landmarks=200)
    kf.set_state(x, P)
    d2 = kf.polar_compat(z[:17], R[:17], ids[:17], kind[:17])
    n, applied, got = kf.update_polar(z, R, ids, kind)
    assert (n, applied) == (100, 22) and kf.Num_Landmarks == 100
    if kf._f.window == 16:
        assert got[:17].tobytes() == d2.tobytes()
    xa, _ = kf.state()
    assert (kf.X, kf.Y, kf.Phi) == (xa[0], xa[1], xa[2]) and (kf.X, kf.Y, kf.Phi) != (x[0], x[1], x[2])
