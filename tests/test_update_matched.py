"""Matched updates on the device: ekf_update_matched / ekf_joint_compat and their batch forms (a scan with the caller's own data
association as joint updates in rounds of ekf_window measurements; the read-only score of one hypothesis).  The reference is
tests/match_ref.py (NumPy on the dense export, rounds as the device takes them; checked on the CPU in
tests/test_update_matched_cpu.py, where the same inputs agree with their extended-precision restatement to 1/20 of the bounds used
here), the inputs are match_ref.gpu_inputs' : 24 planted measurements of the landmarks nearest the robot on 200 landmarks in capacity
320 (k_chain) and 100 in capacity 200 (k_solo where the pipeline mode allows it), as tests/test_fuse_landmarks.py.
d2 is compared relatively within match_ref.D2_REL = 5e-12: 20 times the 2.48e-13 the CPU test measures between the double reference
and its extended-precision restatement over these inputs.
The batch form where the filters diverge (match_ref.divergent_batch_inputs): one filter of four whose second round is refused while
its siblings go on to a third (the `stopped` path of k_match_factor), lists of 70 entries on a fresh handle (a table of 128 entries
per filter under arrays of 70) with a list of 9 behind them, and filters of 257, 0, 33 and 64 landmarks in one call.  The grid, tile
and chunk edges of a single filter are in tests/test_map_edges.py, matched updates in random operation sequences in
tests/test_map_sequences.py."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, open_window_pair, run_steps, stream_starts, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = mr.SIZES
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@functools.lru_cache(maxsize=None)
def planted(pkg, N):
    out = mr.planted_scan(pkg, N, mr.SCAN_SEED[N])
    for a in out:
        a.setflags(write=False)
    return out


def loaded(pkg, x, P, cap, max_pending=16, batch=1):
    f = pkg.FilterBatch(batch, cap, max_pending=max_pending, log_capacity=4096)
    f.set_state(x, P)
    return f


def assert_d2_close(got, want, what):
    mr.assert_d2_close(got, want, what, mr.D2_REL)


def check(f, pre, z, R, ids, got, what, round_size=None):
    """The handle after update_matched(z, R, ids) returned `got`, against the reference on the export `pre`; returns the reference."""
    ref = mr.update(pre[0], pre[1], z, R, ids, round_size or f.window)
    after = f.get_state()
    n, applied, d2 = got
    assert (n, applied) == ((pre[0].size - 3) // 2, ref[2]), (what, n, applied, ref[2])
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=what)
    print("%s: %d measurements, %d applied, max |dx| %.3e, max |dP| / max |P| %.3e" % (what, len(ids), applied, err[0], err[1]))
    assert_d2_close(d2, ref[3], what)
    assert_bitwise_symmetric(after[1])
    assert int(f.num_landmarks()[0]) == n
    assert np.array_equal(f.poses()[0], after[0][:3]) and np.array_equal(f.robot_cov(), after[1][:3, :3])
    return ref


# ---- 1. parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_on_the_planted_scan(pkg, pipeline_mode, N, cap):
    x, P, z, R, ids = planted(pkg, N)
    a = loaded(pkg, x, P, cap)
    st, dec = a.stats(), a.decisions()
    got = a.update_matched(z, R, ids)
    assert got[1] == 24
    check(a, (x, P), z, R, ids, got, "N=%d" % N)
    assert a.stats() == st and a.decisions() == dec
    a.close()


# ---- 2. against the reference's own path ----------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_window_of_one_is_the_sequence_of_old_updates(pkg, pipeline_mode, N, cap):
    x, P, z, R, ids = planted(pkg, N)
    a, b = loaded(pkg, x, P, cap, max_pending=1), loaded(pkg, x, P, cap, max_pending=1)
    assert a.window == 1
    n, applied, d2 = a.update_matched(z, R, ids)
    dec = [b.update(z[k].reshape(1, 1, 2), R[k].reshape(1, 1, 2, 2))[0][0] for k in range(len(ids))]
    assert [(d[0], d[1]) for d in dec] == [(pkg.ekfslam.OLD, 2 * int(i) + 3) for i in ids]  # a precondition: Old, as planted
    assert (n, applied) == (N, len(ids))
    sa, sb = a.get_state(), b.get_state()
    err = assert_state_close(sa[0], sa[1], sb[0], sb[1], what="update_matched vs update, N=%d" % N)
    print("N=%d: update_matched vs update(): max |dx| %.3e, max |dP| / max |P| %.3e" % (N, err[0], err[1]))
    assert_d2_close(d2, np.array([d[2] for d in dec]), "d2 vs mahal, N=%d" % N)
    check(a, (x, P), z, R, ids, (n, applied, d2), "window 1, N=%d" % N, round_size=1)
    a.close(), b.close()


# ---- 3. rounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, -1])
@pytest.mark.parametrize("N,cap", SIZES)
def test_rounds(pkg, pipeline_mode, N, cap, order):
    x, P, z, R, ids = planted(pkg, N)
    z, R, ids = z[::order], R[::order], ids[::order]
    a = loaded(pkg, x, P, cap, max_pending=8)
    assert a.window == 8  # 24 measurements in windows of 8: three passes
    w0 = windows_closed(a)
    got = a.update_matched(z, R, ids)
    assert windows_closed(a) == w0  # the rounds' passes are the call's own: no window of the filter was closed
    ref = check(a, (x, P), z, R, ids, got, "window 8, order %d" % order, round_size=8)
    for r0 in (0, 8, 16):  # a running distance per round
        assert np.all(np.diff(got[2][r0:r0 + 8]) >= 0.0)
    assert ref[2] == 24
    a.close()


# ---- 4. window open, streaming launch live --------------------------------------------------------------
def test_with_a_window_open(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    pre = b.get_state()
    ids = [3, 40, 31, 32, 63, 64, 5, 99]
    z, R = mr.scan_of(pkg, pre[0], ids, 313)
    st, dec = b.stats(), b.decisions()
    got = a.update_matched(z, R, ids)
    check(a, pre, z, R, ids, got, "helpers.open_window_pair")
    assert a.stats() == st and a.decisions() == dec
    # immediate calls go on, streaming again where the handle streams, exactly as on a twin loaded with set_state
    on, starts0 = stream_starts(a)
    st = a.get_state()
    t = loaded(pkg, st[0], st[1], 200)
    sc = pkg.scenarios.steady_script(st[0], steps=6, M=2, seed=104, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc, 0, 6, 2)
    dt, _ = run_steps(pkg, t, sc, 0, 6, 2)
    if on:
        assert stream_starts(a)[1] > starts0
    assert da == dt
    assert_bitwise(a.get_state(), t.get_state(), "streamed continuation")
    a.close(), b.close(), t.close()


# ---- 5. tile edges and repeats --------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3))
def test_tile_edges_repeats_and_skips(pkg, pipeline_mode, k):
    name, ids = mr.edge_lists()[k]
    x, P = pkg.scenarios.injected_state(100, seed=51, extent=15.0)
    z, R = mr.scan_of(pkg, x, ids, 510 + k)  # (NaN in z and R of the skipped entries: they are not looked at)
    a = loaded(pkg, x, P, 128)
    got = a.update_matched(z, R, ids)
    assert got[1] == sum(1 for i in ids if i >= 0)
    check(a, (x, P), z, R, ids, got, name)
    a.close()


def test_only_skips_is_a_no_op(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=71, steps=3)
    w0, s0 = windows_closed(a), stream_starts(a)
    N = int(b.num_landmarks()[0])
    nan3 = np.full((3, 2), np.nan)
    n, applied, d2 = a.update_matched(nan3, np.full((3, 2, 2), np.nan), [-1, -1, -1])
    assert (n, applied) == (N, 0) and np.all(np.isnan(d2))
    n, applied, d2 = a.update_matched(np.zeros((0, 2)), np.zeros((0, 2, 2)), [])
    assert (n, applied, d2.size) == (N, 0, 0)
    assert windows_closed(a) == w0 and stream_starts(a) == s0  # window and stream as they were
    assert np.all(np.isnan(a.joint_compat(nan3, np.full((3, 2, 2), np.nan), [-1, -1, -1])))
    assert windows_closed(a) == w0
    assert_bitwise(a.get_state(), b.get_state(), "no measurement")
    a.close(), b.close()


# ---- 6. determinism and the batch form ------------------------------------------------------------------
def test_batch_equals_single_calls_bit_for_bit(pkg, pipeline_mode):
    counts, lists = mr.BATCH_COUNTS, mr.BATCH_IDS
    hs = []
    for _ in range(3):
        f = pkg.FilterBatch(4, 128, max_pending=4, log_capacity=4096)
        for b, n in enumerate(counts):
            f.set_state(*pkg.scenarios.injected_state(n, seed=80 + b, extent=10.0 + b), index=b)
        hs.append(f)
    before = [hs[0].get_state(b) for b in range(4)]
    zs, Rs = zip(*[mr.scan_of(pkg, before[b][0], lists[b], 800 + b) for b in range(4)])
    z, R, ids = np.stack(zs), np.stack(Rs), np.array(lists)
    want = [sum(1 for i in l if i >= 0) for l in lists]
    ap1, d1 = hs[0].update_matched(z, R, ids, index=None)
    ap2, d2 = hs[1].update_matched(z, R, ids, index=None)
    jc = hs[2].joint_compat(z, R, ids, index=None)
    assert list(ap1) == list(ap2) == want and d1.tobytes() == d2.tobytes()
    for b in range(4):
        n, ap, db = hs[2].update_matched(z[b], R[b], ids[b], index=b)
        assert (n, ap) == (counts[b], want[b])
        s1 = hs[0].get_state(b)
        assert_bitwise(s1, hs[1].get_state(b), "two identical handles, filter %d" % b)
        assert_bitwise(s1, hs[2].get_state(b), "batch form vs single call, filter %d" % b)
        assert db.tobytes() == d1[b].tobytes()
        ref = mr.update(*before[b], z[b], R[b], ids[b], hs[0].window)
        assert_state_close(s1[0], s1[1], ref[0], ref[1], what="filter %d" % b)
        assert_d2_close(d1[b], ref[3], "filter %d" % b)
        assert_d2_close(jc[b], mr.joint_compat(*before[b], z[b], R[b], ids[b]), "joint_compat, filter %d" % b)
    assert_bitwise(hs[0].get_state(1), before[1], "the filter whose list is all -1")
    assert list(hs[0].num_landmarks()) == list(counts)
    for f in hs:
        f.close()


def batch_handle(pkg, states, cap, max_pending):
    f = pkg.FilterBatch(len(states), cap, max_pending=max_pending, log_capacity=4096)
    for b, (x, P) in enumerate(states):
        if x.size > 3:
            f.set_state(x, P, index=b)
    return f


def check_filter(f, b, pre, z, R, ids, applied, d2, what):
    """Filter b of a batch handle after a matched update that answered (applied, d2), against the reference on the export `pre`."""
    ref = mr.update(pre[0], pre[1], z, R, ids, f.window)
    after = f.get_state(b)
    assert applied == ref[2], (what, applied, ref[2])
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=what)
    print("%s: %d applied, max |dx| %.3e, max |dP| / max |P| %.3e" % (what, applied, err[0], err[1]))
    assert_d2_close(d2, ref[3], what)
    assert_bitwise_symmetric(after[1])
    return ref


def test_one_refused_filter_among_four(pkg, pipeline_mode):
    """Filter 2's second round is refused (the same exact measurement twice, R = 0) while its siblings go on to their second and third
    rounds: it stays at the state after its first round, bit for bit, and takes no part in the later rounds' gather, apply and pass;
    the siblings are what single calls on a second handle give."""
    states = mr.batch_states(pkg, mr.BATCH_COUNTS, 80)
    f, g = batch_handle(pkg, states, 128, 4), batch_handle(pkg, states, 128, 4)
    assert f.window == 4
    f.anchor_at_robot(index=2), g.anchor_at_robot(index=2)
    before = [f.get_state(b) for b in range(4)]
    assert not before[2][1][:3].any() and not before[2][0][:3].any()
    ids = np.array(mr.REFUSED_IDS)
    z, R = mr.refused_scan(pkg, before)
    want = [sum(1 for i in l if i >= 0) for l in mr.REFUSED_IDS]
    want[2] = 4
    assert [-(-w // 4) for w in want] == [3, 3, 1, 3]
    applied, d2 = f.update_matched(z, R, ids, index=None)
    assert list(applied) == want
    assert not np.isnan(d2[2, :4]).any() and np.isnan(d2[2, 4:]).all()
    for b in range(4):
        check_filter(f, b, before[b], z[b], R[b], ids[b], int(applied[b]), d2[b], "one refused among four, filter %d" % b)
    for b in (0, 1, 3):
        n, ap, db = g.update_matched(z[b], R[b], ids[b], index=b)
        assert (n, ap) == (mr.BATCH_COUNTS[b], want[b]) and db.tobytes() == d2[b].tobytes()
    n, ap, db = g.update_matched(z[2, :4], R[2, :4], ids[2, :4], index=2)  # filter 2's first round alone
    assert (n, ap) == (64, 4) and db.tobytes() == d2[2, :4].tobytes()
    for b in range(4):
        assert_bitwise(f.get_state(b), g.get_state(b), "batch form with a refused filter vs single calls, filter %d" % b)
    # a following valid batch call works, the refused filter included
    mid = [f.get_state(b) for b in range(4)]
    ids2 = np.array(mr.FOLLOW_IDS)
    z2, R2 = (np.stack(a) for a in zip(*[mr.scan_of(pkg, mid[b][0], mr.FOLLOW_IDS[b], 840 + b) for b in range(4)]))
    applied, d2 = f.update_matched(z2, R2, ids2, index=None)
    assert list(applied) == [sum(1 for i in l if i >= 0) for l in mr.FOLLOW_IDS]
    for b in range(4):
        check_filter(f, b, mid[b], z2[b], R2[b], ids2[b], int(applied[b]), d2[b], "behind the refusal, filter %d" % b)
    assert list(f.num_landmarks()) == list(mr.BATCH_COUNTS)
    f.close(), g.close()


def test_lists_longer_than_the_table_in_the_batch_form(pkg, pipeline_mode):
    """70 entries per filter on a fresh handle: the measurement table is made for 128 per filter, not 64, so every [B][zcap] offset of
    the upload, of the kernels and of the way back has that stride while the caller's arrays have 70; then 9 entries in the same
    table.  Both against single-index calls on a twin handle, bit for bit, and against the reference."""
    states = mr.batch_states(pkg, mr.LONG_COUNTS, 80)
    f, g = batch_handle(pkg, states, 128, 16), batch_handle(pkg, states, 128, 16)
    assert f.window == 16
    bytes0 = f.device_bytes()
    grew = []
    for name, lists, seed in (("list of 70", mr.long_lists(), 870), ("list of 9 behind it", np.array(mr.LONG_NINE), mr.NINE_SCAN_SEED)):
        pre = [f.get_state(b) for b in range(3)]
        z, R = (np.stack(a) for a in zip(*[mr.scan_of(pkg, pre[b][0], lists[b], seed + b) for b in range(3)]))
        want = [int((lists[b] >= 0).sum()) for b in range(3)]
        applied, d2 = f.update_matched(z, R, lists, index=None)
        grew.append(f.device_bytes())
        assert list(applied) == want
        assert np.array_equal(np.isnan(d2), lists < 0)
        jc = g.joint_compat(z[:, :9], R[:, :9], lists[:, :9], index=None)  # (the twin's table: made for 64 by this score, replaced by one for 128 in its long call)
        for b in range(3):
            check_filter(f, b, pre[b], z[b], R[b], lists[b], int(applied[b]), d2[b], "%s, filter %d" % (name, b))
            n, ap, db = g.update_matched(z[b], R[b], lists[b], index=b)
            assert (n, ap) == (mr.LONG_COUNTS[b], want[b]) and db.tobytes() == d2[b].tobytes(), (name, b)
            assert_bitwise(f.get_state(b), g.get_state(b), "%s: batch form vs single calls, filter %d" % (name, b))
            assert_d2_close(jc[b], mr.joint_compat(*pre[b], z[b, :9], R[b, :9], lists[b, :9]), "%s: score of the first 9, filter %d" % (name, b))
    assert max(int((mr.long_lists()[b] >= 0).sum()) for b in range(3)) > 64
    assert grew[0] > bytes0 and grew[1] == grew[0]  # the table grows once and not again
    f.close(), g.close()


def test_no_landmarks_beside_257(pkg, pipeline_mode):
    """Counts (257, 0, 33, 64) in capacity 320: k_match_gather's grid has two blocks of 256 landmarks for every filter, filter 0
    measures landmark 256, filter 1 has nothing to measure and stays bit for bit."""
    states = mr.batch_states(pkg, mr.WIDE_COUNTS, 90)
    f, g = batch_handle(pkg, states, 320, 8), batch_handle(pkg, states, 320, 8)
    assert f.window == 8 and list(f.num_landmarks()) == list(mr.WIDE_COUNTS)
    f.propagate(0.3, 0.05, 0.05), g.propagate(0.3, 0.05, 0.05)  # (filter 1 away from the all-zero state of a fresh filter)
    before = [f.get_state(b) for b in range(4)]
    assert before[1][0].size == 3 and before[1][1].any()
    ids = np.array(mr.WIDE_IDS)
    assert ids[0, 0] == 256 and (ids[1] == -1).all()
    z, R = (np.stack(a) for a in zip(*[mr.scan_of(pkg, before[b][0], mr.WIDE_IDS[b], 890 + b) for b in range(4)]))
    applied, d2 = f.update_matched(z, R, ids, index=None)
    assert list(applied) == [int((ids[b] >= 0).sum()) for b in range(4)] and applied[1] == 0
    assert np.array_equal(np.isnan(d2), ids < 0)
    jc = g.joint_compat(z, R, ids, index=None)
    for b in range(4):
        check_filter(f, b, before[b], z[b], R[b], ids[b], int(applied[b]), d2[b], "0 beside 257, filter %d" % b)
        assert_d2_close(jc[b], mr.joint_compat(*before[b], z[b], R[b], ids[b]), "0 beside 257: the score, filter %d" % b)
        if b != 1:
            n, ap, db = g.update_matched(z[b], R[b], ids[b], index=b)
            assert (n, ap) == (mr.WIDE_COUNTS[b], int(applied[b])) and db.tobytes() == d2[b].tobytes()
        assert_bitwise(f.get_state(b), g.get_state(b), "batch form vs single calls, filter %d" % b)
    assert_bitwise(f.get_state(1), before[1], "the filter without a landmark")
    assert list(f.num_landmarks()) == list(mr.WIDE_COUNTS)
    f.close(), g.close()


# ---- 7. joint_compat ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_joint_compat(pkg, pipeline_mode, N, cap):
    x, P, z, R, ids = planted(pkg, N)
    a = loaded(pkg, x, P, cap, max_pending=8)
    before, st = a.get_state(), a.stats()
    w0 = windows_closed(a)
    d2 = a.joint_compat(z, R, ids)  # 24 pairings on a window of 8
    assert_d2_close(d2, mr.joint_compat(x, P, z, R, ids), "joint_compat N=%d" % N)
    assert d2.tobytes() == a.joint_compat(z, R, ids).tobytes()  # two calls, the same bits
    wrong = a.joint_compat(z, R, mr.wrong_pairing(ids))
    assert wrong[-1] > d2[-1] and wrong[1] > d2[1]  # a wrong pairing is a larger joint distance
    z32, R32, ids32 = mr.hypothesis_of_32(pkg, x, z, R, ids)
    d32 = a.joint_compat(z32, R32, ids32)
    assert_d2_close(d32, mr.joint_compat(x, P, z32, R32, ids32), "hypothesis of 32")
    assert d32[:24].tobytes() == d2.tobytes()  # extending a hypothesis leaves its prefix as it was
    z33, R33, ids33 = np.concatenate([z32, z[:1]]), np.concatenate([R32, R[:1]]), np.concatenate([ids32, ids[:1]]).astype(np.int32)
    Rc = np.ascontiguousarray(np.swapaxes(R33, 1, 2).reshape(-1, 4))
    out = np.zeros(33)
    assert a.L.ekf_joint_compat(a.h, 0, z33.ctypes.data_as(DP), Rc.ctypes.data_as(DP), ids33.ctypes.data_as(IP), 33, out.ctypes.data_as(DP)) == pkg.ekfslam.ERR_BAD_ARG
    with pytest.raises(ValueError):
        a.joint_compat(z33, R33, ids33)
    assert_bitwise(a.get_state(), before, "joint_compat only reads")
    assert windows_closed(a) == w0 and a.stats() == st
    # the same hypothesis in one round of update_matched: the same bits
    b = loaded(pkg, x, P, cap, max_pending=16)
    k8 = a.joint_compat(z[:8], R[:8], ids[:8])
    assert a.update_matched(z[:8], R[:8], ids[:8])[2].tobytes() == k8.tobytes()
    k16 = b.joint_compat(z[:16], R[:16], ids[:16])
    assert b.update_matched(z[:16], R[:16], ids[:16])[2].tobytes() == k16.tobytes()
    assert k16[:8].tobytes() == k8.tobytes()
    a.close(), b.close()


# ---- 8. S not positive definite -------------------------------------------------------------------------
def test_singular_round_is_not_applied(pkg, pipeline_mode):
    x0, P0 = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    a, b = loaded(pkg, x0, P0, 128, max_pending=4), loaded(pkg, x0, P0, 128, max_pending=4)
    a.anchor_at_robot(0), b.anchor_at_robot(0)
    pre = a.get_state()
    assert not pre[1][:3].any() and not pre[0][:3].any()  # P_RR = 0 and with it every robot row
    ids = [3, 40, 31, 32, 17, 17, 5]
    z, R = mr.scan_of(pkg, pre[0], ids, 91)
    R[4:6] = 0.0
    z[5] = z[4]  # the same exact measurement of landmark 17 twice: S of round 2 is exactly singular
    n, applied, d2 = a.update_matched(z, R, ids)
    assert (n, applied) == (60, 4) and not np.isnan(d2[:4]).any() and np.isnan(d2[4:]).all()
    check(a, pre, z, R, ids, (n, applied, d2), "singular second round", round_size=4)
    assert b.update_matched(z[:4], R[:4], ids[:4])[:2] == (60, 4)
    assert_bitwise(a.get_state(), b.get_state(), "the state after the completed round")
    jc = a.joint_compat(z[4:6], R[4:6], ids[4:6])
    assert not np.isnan(jc[0]) and np.isnan(jc[1])
    # the handle works on
    zf, Rf = pkg.scenarios.measurement_from_feature_mm(80000.0, 30000.0)
    assert a.update(zf.reshape(1, 1, 2), Rf.reshape(1, 1, 2, 2))[0][0][0] == pkg.ekfslam.NEW
    assert a.fuse_landmarks([(0, 1)], slack=1e-4) == (60, 1)
    assert a.update_matched(z[6:], R[6:], ids[6:])[:2] == (60, 1)
    a.close(), b.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=101, steps=3)
    held = b.get_state()
    N = (held[0].size - 3) // 2
    L, E = a.L, pkg.ekfslam
    BAD = E.ERR_BAD_ARG
    ids0 = [0, 1, 2]
    z0, R0 = mr.scan_of(pkg, held[0], ids0, 5)

    def raw(z, R, ids, index=0, n=None, null=None):
        z, Rc = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(np.swapaxes(np.asarray(R, dtype=np.float64), 1, 2).reshape(-1, 4))
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        ptr = [z.ctypes.data_as(DP), Rc.ctypes.data_as(DP), ids.ctypes.data_as(IP)]
        if null is not None:
            ptr[null] = None
        n = len(ids) if n is None else n
        out = np.zeros(max(len(ids), 1))
        return (L.ekf_update_matched(a.h, index, ptr[0], ptr[1], ptr[2], n, None, None),
                L.ekf_joint_compat(a.h, index, ptr[0], ptr[1], ptr[2], n, out.ctypes.data_as(DP)))

    assert raw(z0, R0, [0, N, 2]) == (BAD, BAD)            # id >= N
    assert raw(z0, R0, [0, -2, 2]) == (BAD, BAD)           # id < -1
    for at in ((0, 0), (2, 1)):
        zb = z0.copy()
        zb[at] = np.nan
        assert raw(zb, R0, ids0) == (BAD, BAD)             # NaN in z
    Rb = R0.copy()
    Rb[1, 0, 1] = np.inf
    assert raw(z0, Rb, ids0) == (BAD, BAD)
    for null in range(3):
        assert raw(z0, R0, ids0, null=null) == (BAD, BAD)  # a null list with n_z > 0
    assert raw(z0, R0, ids0, n=-1) == (BAD, BAD)
    assert raw(z0, R0, ids0, index=1) == (BAD, BAD) and raw(z0, R0, ids0, index=-1) == (BAD, BAD)
    assert L.ekf_update_matched(None, 0, None, None, None, 0, None, None) == BAD and L.ekf_batch_update_matched(None, None, None, None, 0, None, None) == BAD
    assert L.ekf_joint_compat(None, 0, None, None, None, 0, None) == BAD and L.ekf_batch_joint_compat(None, None, None, None, 0, None) == BAD
    assert L.ekf_joint_compat(a.h, 0, z0.ctypes.data_as(DP), z0.ctypes.data_as(DP), np.zeros(3, dtype=np.int32).ctypes.data_as(IP), 3, None) == BAD  # no d2_out
    assert_bitwise(a.get_state(), held, "after the refusals")
    got = a.update_matched(z0, R0, ids0)  # the next valid call works
    check(a, held, z0, R0, ids0, got, "after the refusals")
    a.close(), b.close()


def test_sticky_capacity_blocks_the_update_but_not_the_score(pkg, pipeline_mode):
    g = pkg.FilterBatch(1, 8, max_pending=16, log_capacity=4096)
    g.set_state(*pkg.scenarios.injected_state(8, seed=93, extent=8.0))
    zf, Rf = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(zf.reshape(1, 1, 2), Rf.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    held = g.get_state()
    ids = [2, 5]
    z, R = mr.scan_of(pkg, held[0], ids, 7)
    with pytest.raises(pkg.EkfError) as ei:
        g.update_matched(z, R, ids)
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    assert_bitwise(g.get_state(), held, "sticky capacity")
    assert_d2_close(g.joint_compat(z, R, ids), mr.joint_compat(held[0], held[1], z, R, ids), "the score under a sticky capacity status")
    g.close()


# ---- 10. ekf_reserve ------------------------------------------------------------------------------------
def test_update_reserve_update(pkg, pipeline_mode):
    x, P, z, R, ids = planted(pkg, 100)
    a = loaded(pkg, x, P, 200)
    bytes0 = a.device_bytes()
    d_before = a.joint_compat(z[:12], R[:12], ids[:12])
    bytes1 = a.device_bytes()
    assert bytes1 > bytes0  # the measurement table is counted
    got = a.update_matched(z[:12], R[:12], ids[:12])
    assert got[2].tobytes() == d_before.tobytes()
    check(a, (x, P), z[:12], R[:12], ids[:12], got, "before the reserve")
    bytes2 = a.device_bytes()
    assert bytes2 > bytes1  # ... and so is the round's factor
    mid = a.get_state()
    a.reserve(320)  # the other side of 256: another kernel family, another tile numbering
    assert_bitwise(a.get_state(), mid, "reserve after the update")
    assert a.device_bytes() > bytes2
    got = a.update_matched(z[12:], R[12:], ids[12:])
    check(a, mid, z[12:], R[12:], ids[12:], got, "after the reserve")
    bytes3 = a.device_bytes()
    long_ids = np.concatenate([ids[:12]] * 9)
    zl, Rl = mr.scan_of(pkg, a.get_state()[0], long_ids, 77)
    pre = a.get_state()
    got = a.update_matched(zl, Rl, long_ids)  # 108 > 64 measurements: a larger table, seven rounds
    check(a, pre, zl, Rl, long_ids, got, "a list longer than the table")
    assert a.device_bytes() > bytes3
    a.close()


# ---- 11. the KalmanFilter shim --------------------------------------------------------------------------
def test_kalman_filter_shim_refreshes_its_mirror(pkg, pipeline_mode):
    x, P, z, R, ids = planted(pkg, 100)
    kf = pkg.KalmanFilter(capacity_landmarks=200)
    kf.set_state(x, P)
    d2 = kf.joint_compat(z[:16], R[:16], ids[:16])
    n, applied, got = kf.update_matched(z, R, ids)
    assert (n, applied) == (100, 24) and kf.Num_Landmarks == 100
    if kf._f.window == 16:
        assert got[:16].tobytes() == d2.tobytes()
    xa, _ = kf.state()
    assert (kf.X, kf.Y, kf.Phi) == (xa[0], xa[1], xa[2]) and (kf.X, kf.Y, kf.Phi) != (x[0], x[1], x[2])
