"""The iterated matched update on the device: ekf_update_matched_iter and its batch form (a round of ekf_update_matched relinearised,
inside its one factor kernel, until the step vanishes).  The reference is tests/iter_ref.py (NumPy on the dense export, rounds as the
device takes them), the inputs are iter_ref.gpu_inputs': planted scans on 200 landmarks in capacity 320 (k_chain) and 100 in
capacity 200 (k_solo where the pipeline mode allows it) whose pose has been displaced by 0.02, 0.1 and 0.3 m / rad.
tests/test_update_matched_iter_cpu.py runs the same inputs on the CPU: x, P, d2 and step are compared within iter_ref.BOUND_X
(1.08e-13 m / rad), BOUND_P (6.8e-13 of max |P|), BOUND_D2 (2.7e-12, relative) and BOUND_STEP (1.2e-13), 20 times what the double
reference and its extended-precision restatement differ by there; `iters` is asked for exactly, every step of the reference lying a
factor of 4 and more from tol."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iter_ref as ir  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, open_window_pair, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@functools.lru_cache(maxsize=None)
def inputs(pkg):
    """name -> (x, P, z, R, ids, round_size, max_iter), read-only"""
    out = {}
    for t in ir.gpu_inputs(pkg):
        for a in t[1:5]:
            a.setflags(write=False)
        out[t[0]] = t[1:]
    return out


@functools.lru_cache(maxsize=None)
def reference(pkg, name):
    """iter_ref.update on a named input, computed once for both pipeline modes."""
    x, P, z, R, ids, rs, mi = inputs(pkg)[name]
    out = ir.update(x, P, z, R, ids, mi, ir.tol_of(name), rs)
    for a in (out[0], out[1], out[3], out[4], out[5]):
        a.setflags(write=False)
    return out


def loaded(pkg, x, P, cap, max_pending=16):
    f = pkg.FilterBatch(1, cap, max_pending=max_pending, log_capacity=4096)
    f.set_state(x, P)
    return f


def assert_close(after, got, ref, what):
    """The exported state `after` and the per-measurement results got = (applied, d2, iters, step) of one filter against a run of
    iter_ref.update."""
    applied, d2, iters, step = got
    assert applied == ref[2], (what, applied, ref[2])
    dx = float(np.abs(after[0] - ref[0]).max())
    dP = float(np.abs(after[1] - ref[1]).max() / np.abs(ref[1]).max())
    print("%s: %d applied, iters %s, max |dx| %.3e, max |dP| / max |P| %.3e" % (what, applied, sorted(set(int(i) for i in iters)), dx, dP))
    assert dx <= ir.BOUND_X and dP <= ir.BOUND_P, (what, dx, dP)
    mr.assert_d2_close(d2, ref[3], what, ir.BOUND_D2)
    assert np.array_equal(iters, ref[4]), (what, iters, ref[4])
    assert np.array_equal(np.isnan(step), np.isnan(ref[5])), (what, step, ref[5])
    ok = ~np.isnan(ref[5])
    if ok.any():
        ds = float(np.abs(step[ok] - ref[5][ok]).max())
        print("%s: max |dstep| %.3e" % (what, ds))
        assert ds <= ir.BOUND_STEP, (what, ds)
    assert_bitwise_symmetric(after[1])


def run_named(pkg, name, cap):
    """A fresh handle loaded with the named input, the iterated update, the comparison; returns (handle, result)."""
    x, P, z, R, ids, rs, mi = inputs(pkg)[name]
    a = loaded(pkg, x, P, cap, max_pending=rs)
    assert a.window == rs
    st, dec, w0 = a.stats(), a.decisions(), windows_closed(a)
    got = a.update_matched_iter(z, R, ids, mi, ir.tol_of(name))
    after = a.get_state()
    assert got[0] == (x.size - 3) // 2 == int(a.num_landmarks()[0])
    assert_close(after, got[1:], reference(pkg, name), name)
    assert np.array_equal(a.poses()[0], after[0][:3]) and np.array_equal(a.robot_cov(), after[1][:3, :3])  # the mirror
    assert a.stats() == st and a.decisions() == dec and windows_closed(a) == w0  # counters, log and the filter's own windows untouched
    return a, got


# ---- 1. parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", ir.HEADINGS)
@pytest.mark.parametrize("N,cap", mr.SIZES)
def test_parity_on_the_displaced_planted_scan(pkg, pipeline_mode, N, cap, e):
    a, got = run_named(pkg, "planted N=%d, heading off by %g" % (N, e), cap)
    assert got[1] == 24 and got[3].min() >= 3
    a.close()


# ---- 2. one iteration is the single-step update ---------------------------------------------------------
@pytest.mark.parametrize("window", [8, 32])
@pytest.mark.parametrize("N,cap", mr.SIZES)
def test_one_iteration_is_update_matched_bit_for_bit(pkg, pipeline_mode, N, cap, window):
    x, P, z, R, ids = inputs(pkg)["planted N=%d, heading off by 0.1" % N][:5]
    a = loaded(pkg, x, P, cap, max_pending=window)
    b = pkg.FilterBatch(1, cap, max_pending=window, log_capacity=4096)
    assert b.extract_map(a, ids=None) == N  # a fork
    assert_bitwise(a.get_state(), b.get_state(), "the fork")
    n, applied, d2, iters, step = a.update_matched_iter(z, R, ids, 1, 1e-8)
    nb, appliedb, d2b = b.update_matched(z, R, ids)
    assert (n, applied) == (nb, appliedb) == (N, 24)
    assert d2.tobytes() == d2b.tobytes()
    assert_bitwise(a.get_state(), b.get_state(), "max_iter = 1 against ekf_update_matched")
    assert (iters == 1).all() and (step > 1e-8).all()  # one factorisation each, and the step says that it was not the last word
    a.close(), b.close()


# ---- 3. m = 1, repeats, tile edges, a full round, rounds that iterate on their own, tol = 0 --------------
@pytest.mark.parametrize("name,cap", [("one measurement", 200), ("one landmark three times in a round", 200), ("tile edges", 128),
                                      ("a full round of 32", 200), ("9 entries in rounds of 4", 200), ("tol = 0", 200)])
def test_named_inputs(pkg, pipeline_mode, name, cap):
    a, (n, applied, d2, iters, step) = run_named(pkg, name, cap)
    ids, mi = inputs(pkg)[name][4], inputs(pkg)[name][6]
    assert applied == len(ids)
    if name == "9 entries in rounds of 4":
        assert len({int(iters[0]), int(iters[4]), int(iters[8])}) > 1 and (iters[:4] == iters[0]).all() and (iters[4:8] == iters[4]).all()
    if name == "tol = 0":
        assert (iters == mi).all() and (step > 0.0).all()  # ran out of iterations, and step_out > tol says so
    else:
        assert (step <= ir.tol_of(name)).all() and iters.max() < mi
    a.close()


# ---- 4. d2 is the prior's compatibility -----------------------------------------------------------------
@pytest.mark.parametrize("N,cap", mr.SIZES)
def test_d2_is_joint_compat_at_the_entry_state(pkg, pipeline_mode, N, cap):
    name = "planted N=%d, heading off by 0.3" % N
    x, P, z, R, ids, rs, mi = inputs(pkg)[name]
    a = loaded(pkg, x, P, cap, max_pending=rs)
    jc = a.joint_compat(z, R, ids)  # 24 pairings, one round at window 32
    n, applied, d2, iters, step = a.update_matched_iter(z, R, ids, mi, ir.tol_of(name))
    assert applied == 24 and iters.min() > 1
    assert d2.tobytes() == jc.tobytes()
    a.close()


# ---- 5. determinism and the batch form ------------------------------------------------------------------
def test_batch_equals_single_calls_bit_for_bit(pkg, pipeline_mode):
    """match_ref.WIDE_COUNTS' shapes: 257 landmarks (k_match_gather's second block), a filter without a landmark, ragged lists."""
    wide = ir.wide_inputs(pkg)
    hs = []
    for _ in range(3):
        f = pkg.FilterBatch(4, 320, max_pending=8, log_capacity=4096)
        for b, t in enumerate(wide):
            if mr.WIDE_COUNTS[b]:
                f.set_state(t[0], t[1], index=b)
        hs.append(f)
    assert hs[0].window == 8 and list(hs[0].num_landmarks()) == list(mr.WIDE_COUNTS)
    before1 = hs[0].get_state(1)
    z, R, ids = np.stack([t[2] for t in wide]), np.stack([t[3] for t in wide]), np.array([t[4] for t in wide])
    got1 = hs[0].update_matched_iter(z, R, ids, ir.MAX_ITER, ir.WIDE_TOL, index=None)
    got2 = hs[1].update_matched_iter(z, R, ids, ir.MAX_ITER, ir.WIDE_TOL, index=None)
    for u, v in zip(got1, got2):
        assert u.tobytes() == v.tobytes()
    assert list(got1[0]) == [int((ids[b] >= 0).sum()) for b in range(4)] and got1[0][1] == 0
    assert np.array_equal(np.isnan(got1[1]), ids < 0) and np.array_equal(got1[2] == 0, ids < 0) and np.array_equal(np.isnan(got1[3]), ids < 0)
    for b in range(4):
        s1 = hs[0].get_state(b)
        assert_bitwise(s1, hs[1].get_state(b), "two identical handles, filter %d" % b)
        if mr.WIDE_COUNTS[b]:
            n, ap, d2, iters, step = hs[2].update_matched_iter(z[b], R[b], ids[b], ir.MAX_ITER, ir.WIDE_TOL, index=b)
            assert (n, ap) == (mr.WIDE_COUNTS[b], got1[0][b])
            assert d2.tobytes() == got1[1][b].tobytes() and iters.tobytes() == got1[2][b].tobytes() and step.tobytes() == got1[3][b].tobytes()
            assert_close(s1, (int(got1[0][b]), got1[1][b], got1[2][b], got1[3][b]), reference(pkg, "0 beside 257, filter %d" % b), "0 beside 257, filter %d" % b)
        assert_bitwise(s1, hs[2].get_state(b), "batch form vs single call, filter %d" % b)
    assert_bitwise(hs[0].get_state(1), before1, "the filter without a landmark")
    assert list(hs[0].num_landmarks()) == list(mr.WIDE_COUNTS)
    for f in hs:
        f.close()


# ---- 6. a refused round ---------------------------------------------------------------------------------
def test_refused_later_round_leaves_the_completed_rounds(pkg, pipeline_mode):
    """Window 4; the second round starts with the same exact measurement of landmark 17 twice (R = 0): S is singular in its first
    factorisation.  The first round has iterated to its end and stays; the call reports 4 applied, 0 iterations and NaN behind."""
    name = "refused second round"
    x, P, z, R, ids, rs, mi = inputs(pkg)[name]
    a, (n, applied, d2, iters, step) = run_named(pkg, name, 128)
    assert (n, applied) == (60, 4)
    assert iters[0] > 1 and list(iters) == [iters[0]] * 4 + [0] * 3
    assert not np.isnan(d2[:4]).any() and np.isnan(d2[4:]).all() and np.isnan(step[4:]).all()
    b = loaded(pkg, x, P, 128, max_pending=4)
    got = b.update_matched_iter(z[:4], R[:4], ids[:4], mi, ir.tol_of(name))  # the first round alone
    assert got[1] == 4 and got[3].tobytes() == iters[:4].tobytes() and got[4].tobytes() == step[:4].tobytes()
    assert_bitwise(a.get_state(), b.get_state(), "the state after the completed round")
    # the handle works on: the last entry, iterated, against the reference on what the handle holds
    mid = a.get_state()
    got = a.update_matched_iter(z[6:], R[6:], ids[6:], 2, 0.0)
    assert_close(a.get_state(), got[1:], ir.update(mid[0], mid[1], z[6:], R[6:], ids[6:], 2, 0.0, 4), "behind the refusal")
    a.close(), b.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=101, steps=3)
    held = b.get_state()
    N = (held[0].size - 3) // 2
    L, BAD = a.L, pkg.ekfslam.ERR_BAD_ARG
    ids0 = np.array([0, 1, 2], dtype=np.int32)
    z0, R0 = mr.scan_of(pkg, held[0], ids0, 5)
    Rc = np.ascontiguousarray(np.swapaxes(R0, 1, 2).reshape(-1, 4))
    w0 = windows_closed(a)

    def raw(max_iter, tol, ids=ids0, n=3):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        return (L.ekf_update_matched_iter(a.h, 0, z0.ctypes.data_as(DP), Rc.ctypes.data_as(DP), ids.ctypes.data_as(IP), n, max_iter, tol, None, None, None, None),
                L.ekf_batch_update_matched_iter(a.h, z0.ctypes.data_as(DP), Rc.ctypes.data_as(DP), ids.ctypes.data_as(IP), n, max_iter, tol, None, None, None, None))

    for max_iter in (0, -1, pkg.ITER_MAX + 1):
        assert raw(max_iter, 1e-8) == (BAD, BAD)
    for tol in (-1e-12, np.nan, np.inf, -np.inf):
        assert raw(4, tol) == (BAD, BAD)
    for kw in (dict(max_iter=0), dict(max_iter=17), dict(tol=-1.0), dict(tol=np.nan)):
        with pytest.raises(ValueError):
            a.update_matched_iter(z0, R0, ids0, **kw)
    assert windows_closed(a) == w0  # found before the handle is touched: the window is still open
    assert raw(4, 1e-8, ids=[0, N, 2]) == (BAD, BAD)   # what ekf_update_matched refuses: an id >= N, ...
    assert raw(4, 1e-8, ids=[0, -2, 2]) == (BAD, BAD)  # ... an id < -1, ...
    assert raw(4, 1e-8, n=-1) == (BAD, BAD)            # ... a negative count, ...
    for index in (1, -1):                              # ... a filter that is not there
        assert L.ekf_update_matched_iter(a.h, index, z0.ctypes.data_as(DP), Rc.ctypes.data_as(DP), ids0.ctypes.data_as(IP), 3, 4, 1e-8, None, None, None, None) == BAD
    assert L.ekf_update_matched_iter(None, 0, None, None, None, 0, 4, 1e-8, None, None, None, None) == BAD
    assert L.ekf_batch_update_matched_iter(None, None, None, None, 0, 4, 1e-8, None, None, None, None) == BAD
    assert_bitwise(a.get_state(), held, "after the refusals")
    n, applied, d2, iters, step = a.update_matched_iter(z0, R0, [-1, -1, -1])  # only skips: a no-op with its outputs filled
    assert (n, applied) == (N, 0) and np.isnan(d2).all() and (iters == 0).all() and np.isnan(step).all()
    got = a.update_matched_iter(z0, R0, ids0, 3, 0.0)  # the next valid call works
    assert_close(a.get_state(), got[1:], ir.update(held[0], held[1], z0, R0, ids0, 3, 0.0, a.window), "after the refusals")
    a.close(), b.close()


# ---- 8. window open, streaming launch live --------------------------------------------------------------
def test_with_a_window_open(pkg, pipeline_mode):
    """The call folds the open window first: its result is the reference's on the witness's export.  tol lies between two successive
    steps of the reference's run on that export (iter_ref.tol_between)."""
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    pre = b.get_state()
    ids = [3, 40, 31, 32, 63, 64, 5, 99]
    z, R = ir.seen_from(pkg, pre[0], ids, 313, 0.02)
    tol, ratio = ir.tol_between(pre[0], pre[1], z, R, ids, a.window)
    assert ratio >= 16.0, ratio  # a precondition: both neighbours a factor of 4 away
    st, dec = b.stats(), b.decisions()
    got = a.update_matched_iter(z, R, ids, ir.MAX_ITER, tol)
    assert got[0] == 100 and got[3].min() >= 3
    assert_close(a.get_state(), got[1:], ir.update(pre[0], pre[1], z, R, ids, ir.MAX_ITER, tol, a.window), "helpers.open_window_pair")
    assert a.stats() == st and a.decisions() == dec
    a.close(), b.close()


# ---- 9. the kept scratch and ekf_reserve ----------------------------------------------------------------
def test_scratch_is_counted_and_rebuilt_by_reserve(pkg, pipeline_mode):
    name = "planted N=100, heading off by 0.1"
    x, P, z, R, ids, rs, mi = inputs(pkg)[name]
    a = loaded(pkg, x, P, 200, max_pending=rs)
    bytes0 = a.device_bytes()
    a.joint_compat(z[:4], R[:4], ids[:4])
    bytes1 = a.device_bytes()
    n, applied, d2, iters, step = a.update_matched_iter(z, R, ids, mi, ir.tol_of(name))
    bytes2 = a.device_bytes()
    # the measurement table, then the round's factor AND the iterations' block: 12 bytes per measurement, 64 of them
    fork = loaded(pkg, x, P, 200, max_pending=rs)
    fork.update_matched(z, R, ids)
    assert bytes1 > bytes0 and bytes2 - bytes0 == fork.device_bytes() - bytes0 + 64 * 12
    assert_close(a.get_state(), (applied, d2, iters, step), reference(pkg, name), "before the reserve")
    mid = a.get_state()
    a.reserve(320)  # the other side of 256: another kernel family, another tile numbering
    assert_bitwise(a.get_state(), mid, "reserve after the update")
    bytes3 = a.device_bytes()
    got = a.update_matched_iter(z[:8], R[:8], ids[:8], 3, 0.0)  # the same landmarks once more: three factorisations
    assert a.device_bytes() == bytes3  # built again by the reserve: nothing left to allocate
    assert_close(a.get_state(), got[1:], ir.update(mid[0], mid[1], z[:8], R[:8], ids[:8], 3, 0.0, rs), "after the reserve")
    a.close(), fork.close()
