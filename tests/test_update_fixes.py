"""Absolute fixes on the device: ekf_update_fixes / ekf_fix_compat and their batch forms (position, heading and landmark fixes as
joint updates in rounds of ekf_window entries; the read-only score of one list).  The reference is tests/fix_ref.py (NumPy on the
dense export, rounds as the device takes them, the inert row of a heading entry kept; checked on the CPU in
tests/test_update_fixes_cpu.py, where the same inputs agree with the textbook form and with their extended-precision restatement to
1/20 of the bounds used here).  The inputs are fix_ref.gpu_inputs': 200 landmarks in capacity 320 (k_chain) and 100 in capacity 200
(k_solo where the pipeline mode allows it).
d2 is compared relatively within fix_ref.D2_REL = 1.52e-12: 20 times the 7.59e-14 the CPU test measures between the double reference
and its extended-precision restatement over these inputs."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fix_ref as fx  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, open_window_pair, run_steps, stream_starts, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = fx.SIZES
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
P_, H_, S_ = fx.POSITION, fx.HEADING, fx.SKIP


@functools.lru_cache(maxsize=None)
def mixed(pkg, N):
    x, P = pkg.scenarios.injected_state(N, seed=fx.STATE_SEED[N], extent=mr.map_extent(N))
    out = (x, P) + fx.mixed_list(pkg, x, P, fx.STATE_SEED[N])
    for a in out:
        a.setflags(write=False)
    return out


def loaded(pkg, x, P, cap, max_pending=16, batch=1):
    f = pkg.FilterBatch(batch, cap, max_pending=max_pending, log_capacity=4096)
    if x.size > 3:
        f.set_state(x, P)
    return f


def assert_d2_close(got, want, what):
    mr.assert_d2_close(got, want, what, fx.D2_REL)


def check(f, pre, z, R, what, got, name, round_size=None, index=0):
    """Filter `index` after update_fixes(z, R, what) answered `got`, against the reference on the export `pre`; returns the reference."""
    ref = fx.update(pre[0], pre[1], z, R, what, round_size or f.window)
    after = f.get_state(index)
    n, applied, d2 = got
    assert (n, applied) == ((pre[0].size - 3) // 2, ref[2]), (name, n, applied, ref[2])
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=name)
    print("%s: %d entries, %d applied, max |dx| %.3e, max |dP| / max |P| %.3e" % (name, len(what), applied, err[0], err[1]))
    assert_d2_close(d2, ref[3], name)
    assert_bitwise_symmetric(after[1])
    assert int(f.num_landmarks()[index]) == n
    assert np.array_equal(f.poses()[index], after[0][:3])
    if f.batch == 1:
        assert np.array_equal(f.robot_cov(), after[1][:3, :3])
    return ref


# ---- 1. parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_on_the_mixed_list(pkg, pipeline_mode, N, cap):
    x, P, z, R, what = mixed(pkg, N)
    assert len(what) == 24 and list(what[:2]) == [P_, H_] and list(what[-2:]) == [P_, H_]
    a = loaded(pkg, x, P, cap)
    st, dec = a.stats(), a.decisions()
    got = a.update_fixes(z, R, what)
    assert got[1] == 24
    check(a, (x, P), z, R, what, got, "N=%d" % N)
    assert a.stats() == st and a.decisions() == dec
    a.close()


# ---- 2. the compass -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_heading_in_a_round_of_one_is_the_compass_update(pkg, pipeline_mode, N, cap):
    x, P, _, _, _ = mixed(pkg, N)
    a, b = loaded(pkg, x, P, cap), loaded(pkg, x, P, cap)
    zc, Rc = x[2] + 0.07, 4e-4
    n, applied, d2 = a.update_fixes(zc, Rc, H_)
    b.update_compass(zc, Rc)
    assert (n, applied) == (N, 1)
    sa, sb = a.get_state(), b.get_state()
    err = assert_state_close(sa[0], sa[1], sb[0], sb[1], what="update_fixes vs update_compass, N=%d" % N)
    print("N=%d: heading fix vs update_compass: max |dx| %.3e, max |dP| / max |P| %.3e" % (N, err[0], err[1]))
    want = fx.wrap(x[2] - zc) ** 2 / (P[2, 2] + Rc)
    assert abs(d2[0] - want) <= fx.D2_REL * want
    a.close(), b.close()


# ---- 3. rounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_rounds(pkg, pipeline_mode, N, cap):
    x, P, z, R, what = mixed(pkg, N)
    states = []
    for mp in (1, 5, 16):
        a = loaded(pkg, x, P, cap, max_pending=mp)
        assert a.window == mp
        w0 = windows_closed(a)
        got = a.update_fixes(z, R, what)
        assert windows_closed(a) == w0  # the rounds' passes are the call's own: no window of the filter was closed
        assert check(a, (x, P), z, R, what, got, "N=%d, window %d" % (N, mp))[2] == 24
        for r0 in range(0, 24, mp):  # a running distance per round
            assert np.all(np.diff(got[2][r0:r0 + mp]) >= 0.0)
        states.append(a.get_state())
        a.close()
    for s in states[1:]:  # nothing is linearised: the cut into rounds changes the rounding alone
        assert_state_close(s[0], s[1], states[0][0], states[0][1], what="N=%d: the windows against each other" % N)
    a = loaded(pkg, x, P, cap)  # 9 entries in a window of 16: 18 columns, into the second chunk of k_fuse_apply
    assert a.window == 16
    check(a, (x, P), z[:9], R[:9], what[:9], a.update_fixes(z[:9], R[:9], what[:9]), "N=%d, list of 9" % N)
    a.close()


@pytest.mark.parametrize("count", [17, 32])
def test_rounds_up_to_the_whole_factor(pkg, pipeline_mode, count):
    """Window 32 on the map of 100: 34 and 64 columns, every chunk of k_fuse_apply and the whole of FUSE_MAX_COLS."""
    x, P = pkg.scenarios.injected_state(100, seed=fx.STATE_SEED[100], extent=mr.map_extent(100))
    z, R, what = fx.long_list(pkg, x, P, count, 40 + count)
    a = loaded(pkg, x, P, 200, max_pending=32)
    assert a.window == 32 and len(what) == count
    jc = a.fix_compat(z, R, what)
    got = a.update_fixes(z, R, what)
    assert got[1] == count and got[2].tobytes() == jc.tobytes()
    check(a, (x, P), z, R, what, got, "list of %d, window 32" % count)
    a.close()


# ---- 4. tile and grid edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,what", [(257, fx.EDGE_WHAT_257), (256, fx.EDGE_WHAT_256)])
def test_tile_and_grid_edges(pkg, pipeline_mode, N, what):
    x, P = pkg.scenarios.injected_state(N, seed=1500 + N, extent=mr.map_extent(N))
    z, R = fx.entries_for(x, P, what, 1600 + N)
    a = loaded(pkg, x, P, 320, max_pending=8)
    assert a.window == 8
    got = a.update_fixes(z, R, what)
    assert got[1] == len(what)
    check(a, (x, P), z, R, what, got, "tile edges N=%d" % N)
    a.close()


# ---- 5. no landmarks ------------------------------------------------------------------------------------
def test_a_filter_without_landmarks(pkg, pipeline_mode):
    a = pkg.FilterBatch(1, 64, max_pending=16, log_capacity=4096)
    a.propagate(0.3, 0.05, 0.05)
    pre = a.get_state()
    assert pre[0].size == 3 and pre[1].any()
    what = [P_, H_]
    z, R = fx.entries_for(pre[0], pre[1], what, 61, R_scale=1e-2)
    jc = a.fix_compat(z, R, what)
    assert_bitwise(a.get_state(), pre, "fix_compat only reads")
    got = a.update_fixes(z, R, what)
    assert got[:2] == (0, 2) and got[2].tobytes() == jc.tobytes()
    check(a, pre, z, R, what, got, "no landmarks")
    held = a.get_state()
    with pytest.raises(pkg.EkfError) as ei:
        a.update_fixes(z, R, [P_, 0])
    assert ei.value.code == pkg.ekfslam.ERR_BAD_ARG
    with pytest.raises(pkg.EkfError):
        a.fix_compat(z, R, [0, H_])
    assert_bitwise(a.get_state(), held, "a landmark id on a filter without landmarks")
    zf, Rf = pkg.scenarios.measurement_from_feature_mm(2500.0, 400.0)
    assert a.update(zf.reshape(1, 1, 2), Rf.reshape(1, 1, 2, 2))[0][0][0] == pkg.ekfslam.NEW  # a landmark is added as usual
    pre = a.get_state()
    what = [0, P_, H_]
    z, R = fx.entries_for(pre[0], pre[1], what, 62, R_scale=1e-2)
    check(a, pre, z, R, what, a.update_fixes(z, R, what), "behind the first landmark")
    a.close()


# ---- 6. window open, streaming launch live --------------------------------------------------------------
def test_with_a_window_open(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    pre = b.get_state()
    what = fx.OPEN_WINDOW_WHAT
    z, R = fx.entries_for(pre[0], pre[1], what, 313)
    st, dec = b.stats(), b.decisions()
    got = a.update_fixes(z, R, what)
    check(a, pre, z, R, what, got, "helpers.open_window_pair")
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


# ---- 7. determinism and the batch form ------------------------------------------------------------------
def batch_handle(pkg, states, cap, max_pending):
    f = pkg.FilterBatch(len(states), cap, max_pending=max_pending, log_capacity=4096)
    for b, (x, P) in enumerate(states):
        if x.size > 3:
            f.set_state(x, P, index=b)
    return f


def test_batch_equals_single_calls_bit_for_bit(pkg, pipeline_mode):
    """Filters of 257, 0, 33 and 64 landmarks in capacity 320, window 4, ragged lists padded with FIX_SKIP: the filter without a
    landmark takes a heading and a position fix while k_fix_gather's grid has two blocks for every filter."""
    states = fx.batch_states(pkg, fx.WIDE_COUNTS, 90)
    hs = [batch_handle(pkg, states, 320, 4) for _ in range(3)]
    for f in hs:
        assert f.window == 4
        f.propagate(0.3, 0.05, 0.05)  # (filter 1 away from the all-zero state of a fresh filter)
    before = [hs[0].get_state(b) for b in range(4)]
    assert before[1][0].size == 3 and before[1][1].any()
    zs, Rs = zip(*[fx.entries_for(*before[b], fx.WIDE_WHAT[b], 900 + b) for b in range(4)])
    z, R, what = np.stack(zs), np.stack(Rs), np.array(fx.WIDE_WHAT, dtype=np.int32)
    want = [int((what[b] != S_).sum()) for b in range(4)]
    assert want[1] == 2 and what[0, 0] == 256
    ap1, d1 = hs[0].update_fixes(z, R, what, index=None)
    ap2, d2 = hs[1].update_fixes(z, R, what, index=None)
    jc = hs[2].fix_compat(z, R, what, index=None)
    assert list(ap1) == list(ap2) == want and d1.tobytes() == d2.tobytes()
    assert np.array_equal(np.isnan(d1), what == S_)
    for b in range(4):
        n, ap, db = hs[2].update_fixes(z[b], R[b], what[b], index=b)
        assert (n, ap) == (fx.WIDE_COUNTS[b], want[b])
        s1 = hs[0].get_state(b)
        assert_bitwise(s1, hs[1].get_state(b), "two identical handles, filter %d" % b)
        assert_bitwise(s1, hs[2].get_state(b), "batch form vs single call, filter %d" % b)
        assert db.tobytes() == d1[b].tobytes()
        check(hs[0], before[b], z[b], R[b], what[b], (fx.WIDE_COUNTS[b], int(ap1[b]), d1[b]), "wide batch, filter %d" % b, index=b)
        assert_d2_close(jc[b], fx.compat(*before[b], z[b], R[b], what[b]), "fix_compat, filter %d" % b)
    assert list(hs[0].num_landmarks()) == list(fx.WIDE_COUNTS)
    for f in hs:
        f.close()


def test_one_refused_filter_among_four(pkg, pipeline_mode):
    """Filter 2's second round is refused (landmark 17 fixed twice with R = 0) while its siblings go on to a third round: it stays at
    the state after its first round, bit for bit; the siblings are what single calls on a second handle give."""
    states = mr.batch_states(pkg, fx.REFUSED_COUNTS, 80)
    f, g = batch_handle(pkg, states, 128, 4), batch_handle(pkg, states, 128, 4)
    assert f.window == 4
    before = [f.get_state(b) for b in range(4)]
    z, R, what = fx.refused_lists(pkg, before)
    want = [int((what[b] != S_).sum()) for b in range(4)]
    want[2] = 4
    assert [-(-w // 4) for w in want] == [3, 3, 1, 3]
    applied, d2 = f.update_fixes(z, R, what, index=None)
    assert list(applied) == want
    assert not np.isnan(d2[2, :4]).any() and np.isnan(d2[2, 4:]).all()
    for b in range(4):
        check(f, before[b], z[b], R[b], what[b], (fx.REFUSED_COUNTS[b], int(applied[b]), d2[b]), "one refused among four, filter %d" % b, index=b)
    for b in (0, 1, 3):
        n, ap, db = g.update_fixes(z[b], R[b], what[b], index=b)
        assert (n, ap) == (fx.REFUSED_COUNTS[b], want[b]) and db.tobytes() == d2[b].tobytes()
    n, ap, db = g.update_fixes(z[2, :4], R[2, :4], what[2, :4], index=2)  # filter 2's first round alone
    assert (n, ap) == (64, 4) and db.tobytes() == d2[2, :4].tobytes()
    for b in range(4):
        assert_bitwise(f.get_state(b), g.get_state(b), "batch form with a refused filter vs single calls, filter %d" % b)
    f.close(), g.close()


# ---- 8. fix_compat --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_fix_compat(pkg, pipeline_mode, N, cap):
    x, P, z, R, what = mixed(pkg, N)
    a = loaded(pkg, x, P, cap, max_pending=8)
    before, st, dec = a.get_state(), a.stats(), a.decisions()
    w0 = windows_closed(a)
    d2 = a.fix_compat(z, R, what)  # 24 entries on a window of 8
    assert_d2_close(d2, fx.compat(x, P, z, R, what), "fix_compat N=%d" % N)
    assert d2.tobytes() == a.fix_compat(z, R, what).tobytes()  # two calls, the same bits
    z32, R32, w32 = (np.concatenate([v, v[2:10]]) for v in (z, R, what))
    d32 = a.fix_compat(z32, R32, w32)
    assert_d2_close(d32, fx.compat(x, P, z32, R32, w32), "list of 32")
    assert d32[:24].tobytes() == d2.tobytes()  # extending a list leaves its prefix as it was
    z33, R33, w33 = np.concatenate([z32, z[2:3]]), np.concatenate([R32, R[2:3]]), np.concatenate([w32, what[2:3]]).astype(np.int32)
    Rc = np.ascontiguousarray(np.swapaxes(R33, 1, 2).reshape(-1, 4))
    out = np.zeros(33)
    assert a.L.ekf_fix_compat(a.h, 0, z33.ctypes.data_as(DP), Rc.ctypes.data_as(DP), w33.ctypes.data_as(IP), 33, out.ctypes.data_as(DP)) == pkg.ekfslam.ERR_BAD_ARG
    with pytest.raises(ValueError):
        a.fix_compat(z33, R33, w33)
    w33[5] = S_  # 32 entries and a skip: accepted
    assert np.isnan(a.fix_compat(z33, R33, w33)[5])
    assert_bitwise(a.get_state(), before, "fix_compat only reads")
    assert windows_closed(a) == w0 and a.stats() == st and a.decisions() == dec
    # NaN from the refused pivot on: the position twice with R = 0
    zs, Rs, ws = z[[2, 0, 0, 3]].copy(), R[[2, 0, 0, 3]].copy(), what[[2, 0, 0, 3]]
    Rs[1:3] = 0.0
    bad = a.fix_compat(zs, Rs, ws)
    assert not np.isnan(bad[:2]).any() and np.isnan(bad[2:]).all()
    assert np.array_equal(np.isnan(bad), np.isnan(fx.compat(x, P, zs, Rs, ws)))
    # the same list in one round of update_fixes: the same bits
    b = loaded(pkg, x, P, cap, max_pending=16)
    k8 = a.fix_compat(z[:8], R[:8], what[:8])
    assert a.update_fixes(z[:8], R[:8], what[:8])[2].tobytes() == k8.tobytes()
    k16 = b.fix_compat(z[:16], R[:16], what[:16])
    assert b.update_fixes(z[:16], R[:16], what[:16])[2].tobytes() == k16.tobytes()
    assert k16[:8].tobytes() == k8.tobytes()
    a.close(), b.close()


def test_fix_compat_folds_an_open_window_and_nothing_else(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    pre, st, dec = b.get_state(), b.stats(), b.decisions()
    z, R = fx.entries_for(pre[0], pre[1], fx.OPEN_WINDOW_WHAT, 313)
    d2 = a.fix_compat(z, R, fx.OPEN_WINDOW_WHAT)
    assert_d2_close(d2, fx.compat(pre[0], pre[1], z, R, fx.OPEN_WINDOW_WHAT), "fix_compat behind an open window")
    assert_bitwise(a.get_state(), pre, "fix_compat behind an open window")
    assert a.stats() == st and a.decisions() == dec
    a.close(), b.close()


# ---- 9. S not positive definite -------------------------------------------------------------------------
def test_singular_round_is_not_applied(pkg, pipeline_mode):
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    a, b = loaded(pkg, x, P, 128, max_pending=4), loaded(pkg, x, P, 128, max_pending=4)
    z, R, what = fx.singular_list(pkg, x, P)  # the position twice with R = 0 in round two of three
    assert len(what) == 10 and list(what[4:6]) == [P_, P_]
    n, applied, d2 = a.update_fixes(z, R, what)
    assert (n, applied) == (60, 4) and not np.isnan(d2[:4]).any() and np.isnan(d2[4:]).all()
    check(a, (x, P), z, R, what, (n, applied, d2), "singular second round", round_size=4)
    assert b.update_fixes(z[:4], R[:4], what[:4])[:2] == (60, 4)
    assert_bitwise(a.get_state(), b.get_state(), "the state after the completed round")
    pre = a.get_state()  # the handle works on: the rest without the copy
    rest = [4, 6, 7, 8, 9]
    got = a.update_fixes(z[rest], R[rest], what[rest])
    assert got[1] == 5
    check(a, pre, z[rest], R[rest], what[rest], got, "behind the refusal")
    s = a.get_state()  # the hard position fix: the position is z, its rows of P are rounding noise
    assert np.abs(s[0][:2] - z[4]).max() <= 1e-12 and np.abs(s[1][:2]).max() <= 1e-12 * np.abs(P).max()
    a.close(), b.close()


# ---- 10. refusals ---------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=101, steps=3)
    held = b.get_state()
    N = (held[0].size - 3) // 2
    L, E = a.L, pkg.ekfslam
    BAD = E.ERR_BAD_ARG
    w0 = [P_, H_, 2]
    z0, R0 = fx.entries_for(held[0], held[1], w0, 5)
    z0[1, 1], R0[1, 0, 1], R0[1, 1, 0], R0[1, 1, 1] = 0.0, 0.0, 0.0, 0.0

    def raw(z, R, what, index=0, n=None, null=None):
        z, Rc = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(np.swapaxes(np.asarray(R, dtype=np.float64), 1, 2).reshape(-1, 4))
        what = np.ascontiguousarray(what, dtype=np.int32)
        ptr = [z.ctypes.data_as(DP), Rc.ctypes.data_as(DP), what.ctypes.data_as(IP)]
        if null is not None:
            ptr[null] = None
        n = len(what) if n is None else n
        out = np.zeros(max(len(what), 1))
        return (L.ekf_update_fixes(a.h, index, ptr[0], ptr[1], ptr[2], n, None, None),
                L.ekf_fix_compat(a.h, index, ptr[0], ptr[1], ptr[2], n, out.ctypes.data_as(DP)))

    assert raw(z0, R0, [P_, H_, N]) == (BAD, BAD)          # id >= N
    assert raw(z0, R0, [P_, -4, 2]) == (BAD, BAD)          # what < -3
    for at in ((0, 0), (0, 1), (1, 0), (2, 1)):
        zb = z0.copy()
        zb[at] = np.nan
        assert raw(zb, R0, w0) == (BAD, BAD)               # NaN in a z that is read
    for at in ((0, 0, 1), (2, 1, 1), (1, 0, 0)):
        Rb = R0.copy()
        Rb[at] = np.inf
        assert raw(z0, Rb, w0) == (BAD, BAD)
    Rb = R0.copy()
    Rb[1, 0, 0] = -1e-6
    assert raw(z0, Rb, w0) == (BAD, BAD)                   # a negative heading variance
    for null in range(3):
        assert raw(z0, R0, w0, null=null) == (BAD, BAD)    # a null list with n > 0
    assert raw(z0, R0, w0, n=-1) == (BAD, BAD)
    assert raw(z0, R0, w0, index=1) == (BAD, BAD) and raw(z0, R0, w0, index=-1) == (BAD, BAD)
    assert L.ekf_update_fixes(None, 0, None, None, None, 0, None, None) == BAD and L.ekf_batch_update_fixes(None, None, None, None, 0, None, None) == BAD
    assert L.ekf_fix_compat(None, 0, None, None, None, 0, None) == BAD and L.ekf_batch_fix_compat(None, None, None, None, 0, None) == BAD
    assert L.ekf_fix_compat(a.h, 0, z0.ctypes.data_as(DP), z0.ctypes.data_as(DP), np.full(3, P_, dtype=np.int32).ctypes.data_as(IP), 3, None) == BAD  # no d2_out
    assert_bitwise(a.get_state(), held, "after the refusals")
    # what a heading entry does not read may be anything; the next valid call works
    zn, Rn = z0.copy(), R0.copy()
    zn[1, 1], Rn[1, 0, 1], Rn[1, 1, 0], Rn[1, 1, 1] = np.nan, np.nan, np.inf, np.nan
    jc = a.fix_compat(zn, Rn, w0)
    got = a.update_fixes(zn, Rn, w0)
    assert got[2].tobytes() == jc.tobytes()
    check(a, held, z0, R0, w0, got, "after the refusals")
    a.close(), b.close()


def test_only_skips_is_a_no_op(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=71, steps=3)
    w0, s0 = windows_closed(a), stream_starts(a)
    N = int(b.num_landmarks()[0])
    nan3 = np.full((3, 2), np.nan)
    n, applied, d2 = a.update_fixes(nan3, np.full((3, 2, 2), np.nan), [S_, S_, S_])
    assert (n, applied) == (N, 0) and np.all(np.isnan(d2))
    n, applied, d2 = a.update_fixes(np.zeros((0, 2)), np.zeros((0, 2, 2)), [])
    assert (n, applied, d2.size) == (N, 0, 0)
    assert windows_closed(a) == w0 and stream_starts(a) == s0  # window and stream as they were
    assert np.all(np.isnan(a.fix_compat(nan3, np.full((3, 2, 2), np.nan), [S_, S_, S_])))
    assert windows_closed(a) == w0
    assert_bitwise(a.get_state(), b.get_state(), "no entry")
    a.close(), b.close()


# ---- 11. surrounding state ------------------------------------------------------------------------------
def test_sticky_capacity_blocks_the_update_but_not_the_score(pkg, pipeline_mode):
    g = pkg.FilterBatch(1, 8, max_pending=16, log_capacity=4096)
    g.set_state(*pkg.scenarios.injected_state(8, seed=93, extent=8.0))
    zf, Rf = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(zf.reshape(1, 1, 2), Rf.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    held = g.get_state()
    what = [P_, 5, H_]
    z, R = fx.entries_for(held[0], held[1], what, 7)
    with pytest.raises(pkg.EkfError) as ei:
        g.update_fixes(z, R, what)
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    assert_bitwise(g.get_state(), held, "sticky capacity")
    assert_d2_close(g.fix_compat(z, R, what), fx.compat(held[0], held[1], z, R, what), "the score under a sticky capacity status")
    g.close()


def test_update_reserve_update(pkg, pipeline_mode):
    x, P, z, R, what = mixed(pkg, 100)
    a = loaded(pkg, x, P, 200)
    bytes0 = a.device_bytes()
    got = a.update_fixes(z[:12], R[:12], what[:12])
    check(a, (x, P), z[:12], R[:12], what[:12], got, "before the reserve")
    assert a.device_bytes() > bytes0  # the tables and the round's factor are counted
    mid = a.get_state()
    a.reserve(320)  # the other side of 256: another kernel family, another tile numbering
    assert_bitwise(a.get_state(), mid, "reserve after the update")
    got = a.update_fixes(z[12:], R[12:], what[12:])
    check(a, mid, z[12:], R[12:], what[12:], got, "after the reserve")
    a.close()


def test_kalman_filter_shim_refreshes_its_mirror(pkg, pipeline_mode):
    x, P, z, R, what = mixed(pkg, 100)
    kf = pkg.KalmanFilter(capacity_landmarks=200)
    kf.set_state(x, P)
    d2 = kf.fix_compat(z[:16], R[:16], what[:16])
    n, applied, got = kf.update_fixes(z, R, what)
    assert (n, applied) == (100, 24) and kf.Num_Landmarks == 100
    if kf._f.window == 16:
        assert got[:16].tobytes() == d2.tobytes()
    xa, _ = kf.state()
    assert (kf.X, kf.Y, kf.Phi) == (xa[0], xa[1], xa[2]) and (kf.X, kf.Y, kf.Phi) != (x[0], x[1], x[2])


# ---- 12. a short mixed sequence -------------------------------------------------------------------------
def test_a_short_mixed_sequence(pkg, pipeline_mode, oc):
    """update_fixes -> update_matched -> add_landmarks -> remove_landmarks -> update_fixes on one handle, the dense references
    (fix_ref, match_ref, the oracle's New, NumPy indexing) on each step's own export."""
    x, P = fx.sequence_start(pkg)
    a = loaded(pkg, x, P, 200)
    pre = a.get_state()
    z, R = fx.entries_for(pre[0], pre[1], fx.SEQ_FIX_1, 71)
    check(a, pre, z, R, fx.SEQ_FIX_1, a.update_fixes(z, R, fx.SEQ_FIX_1), "sequence, step 1")
    pre = a.get_state()
    z, R = mr.scan_of(pkg, pre[0], fx.SEQ_MATCH, 72)
    n, applied, d2 = a.update_matched(z, R, fx.SEQ_MATCH)
    ref = mr.update(pre[0], pre[1], z, R, fx.SEQ_MATCH, a.window)
    s = a.get_state()
    assert (n, applied) == (100, 4)
    assert_state_close(s[0], s[1], ref[0], ref[1], what="sequence, step 2")
    mr.assert_d2_close(d2, ref[3], "sequence, step 2")
    pre = s
    zf, Rf = fx.sequence_add_measurement(pkg)
    n, ids = a.add_landmarks(zf.reshape(1, 2), Rf.reshape(1, 2, 2))
    assert n == 101 and list(ids) == [100]
    xo, Po, dec, _, _ = oc.update(pre[0], pre[1], zf.reshape(2, 1), Rf)
    assert dec == [oc.NEW]
    s = a.get_state()
    assert_state_close(s[0], s[1], xo, Po, what="sequence, step 3")
    keep = np.ones(101, dtype=bool)
    keep[fx.SEQ_REMOVE] = False
    assert a.remove_landmarks(keep, 0) == 98
    want = fx.remove(s[0], s[1], fx.SEQ_REMOVE)
    pre = a.get_state()
    assert_bitwise(pre, want, "sequence, step 4")
    z, R = fx.entries_for(pre[0], pre[1], fx.SEQ_FIX_2, 73)
    check(a, pre, z, R, fx.SEQ_FIX_2, a.update_fixes(z, R, fx.SEQ_FIX_2), "sequence, step 5")
    a.close()
