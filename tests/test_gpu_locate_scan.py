"""The scan-to-map pose search on the device: ekf_locate_scan and its batch form, and ekf_relocalize, which ends in ekf_reset_pose and
ekf_update_matched.  The reference is tests/locate_ref.py (NumPy on the exported x; checked on the CPU in
tests/test_locate_scan_cpu.py, where every input used here is shown to lie at least 1e-9 off every threshold, so that the integer
fields, the ids, the candidate count and the order of the hypotheses are asked for EXACTLY).  The floats are compared within
locate_ref.POSE_ABS / SSR_REL / RMS_REL: 20 times what the CPU test measures between the double reference and its extended-precision
restatement over these inputs.  The inputs: match_ref.planted_scan's twelve measurements with two replaced by spurious ones on 200
landmarks in capacity 320 and 100 in capacity 200; scans planted on the LAST landmarks of maps either side of the wave of 64 and the
workgroup of 256, and on 2, 1 and 0 landmarks; scans of 2, 32 and 33 measurements and a valid mask with holes; a tolerance that
finds more candidates than the list starts with; a batch of 257, 0, 33 and 64 landmarks.
No test keeps more than two handles open at a time, and the module's name sorts behind tests/test_gpu_configs.py: the docstring of
tests/test_gpu_gate_candidates.py says why."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_ref as lr  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import assert_bitwise, assert_state_close, make_filter, open_window_pair, stream_starts, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

P_RR = np.diag([0.04, 0.04, 0.01])


@functools.lru_cache(maxsize=None)
def reference(pkg):
    """name -> (Input, Result) of locate_ref.inputs, computed once and left unchanged."""
    out = {}
    for t in lr.inputs(pkg):
        for a in (t.x, t.P, t.z):
            a.setflags(write=False)
        out[t.name] = (t, lr.reference_of(t))
    return out


def loaded(pkg, x, P, cap, batch=1, **params):
    params.setdefault("max_pending", 16)
    f = pkg.FilterBatch(batch, cap, log_capacity=4096, **params)
    if batch == 1:
        f.set_state(x, P)
    return f


def search(f, t, **kw):
    return f.locate_scan(t.z, t.args.tol, t.args.min_sep, t.args.max_base, t.args.max_out, **kw)


def same_bits(a, b):
    return a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- 1. parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", [("planted N=200, tol 0.1", 320), ("planted N=100, tol 0.05", 200), ("planted N=100, tol 0.1", 200),
                                      ("planted N=200, one base pair", 320)])
def test_parity_on_the_planted_scan(pkg, pipeline_mode, name, cap):
    t, ref = reference(pkg)[name]
    a = loaded(pkg, t.x, t.P, cap)
    st, dec, pre = a.stats(), a.decisions(), a.get_state()
    got = search(a, t)
    lr.check(got, ref, name)
    if "one base pair" in name:
        assert got[0]["inliers"][0] < 6   # the farthest-apart pair holds a spurious measurement: the pose is not found
    else:
        assert got[0]["inliers"][0] == 10 and got[1][0].tolist() == t.ids.tolist()
        assert np.hypot(*(got[0]["pose"][0][:2] - t.x[:2])) <= t.args.tol
    assert same_bits(search(a, t), got)   # two calls on an unchanged state
    assert a.stats() == st and a.decisions() == dec
    assert_bitwise(a.get_state(), pre, "the state behind the calls")
    a.close()


# ---- 2. edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", lr.EDGE_SIZES)
def test_map_sizes_around_the_wave_and_the_workgroup(pkg, pipeline_mode, N, cap):
    t, ref = reference(pkg)["edge N=%d" % N]
    a = loaded(pkg, t.x, t.P, cap)
    bytes0 = a.device_bytes()
    got = search(a, t)
    lr.check(got, ref, t.name, ordered=t.ordered)
    if N < 2:
        assert len(got[0]) == 0 and got[2] == 0 and a.device_bytes() == bytes0   # nothing to search: no scratch either
    elif N == 2:
        assert sorted(zip(got[0]["lm_i"].tolist(), got[0]["lm_j"].tolist())) == [(0, 1), (1, 0)]
    else:
        assert N - 1 in (int(got[0]["lm_i"][0]), int(got[0]["lm_j"][0])) and got[1][0].tolist() == t.ids.tolist()
        assert a.device_bytes() > bytes0
    a.close()


def test_scan_lengths_and_a_valid_mask(pkg, pipeline_mode):
    two, ref2 = reference(pkg)["two measurements"]
    many, ref32 = reference(pkg)["32 measurements"]
    a = loaded(pkg, two.x, two.P, 200)
    hyps, ids, n_cand = a.locate_scan(two.z[:0], 0.1)
    assert (len(hyps), ids.shape, n_cand) == (0, (0, 0), 0)
    assert len(a.locate_scan(two.z[:1], 0.1)[0]) == 0   # one measurement: no base pair
    lr.check(search(a, two), ref2, two.name, ordered=False)
    got = search(a, many)
    lr.check(got, ref32, many.name)
    assert got[0]["inliers"][0] == 24 and (got[1][0] >= 0).sum() == 24   # of 32: eight landmarks are measured twice, one of each pair keeps it
    z33 = np.concatenate([many.z, many.z[:1]])
    with pytest.raises(ValueError):
        a.locate_scan(z33, 0.1)
    room, idr = (pkg.ekfslam.EkfLocateHyp * 16)(), (ctypes.c_int * (16 * 33))()
    zp = z33.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert a.L.ekf_locate_scan(a.h, 0, zp, 33, 0.1, 1.0, 2, 16, room, idr, None) == pkg.ekfslam.ERR_BAD_ARG
    # the batch form on the one filter with holes in the mask (their z is not looked at); then 33 entries of which 32 are valid
    t, ref = reference(pkg)["a valid mask with holes"]
    got = search(a, lr.Input(t.name, t.x, t.P, t.z[None], None, None, None, t.args, True), index=None, valid=t.valid[None])[0]
    lr.check(got, ref, t.name)
    assert not np.isin(got[0]["meas_a"], np.flatnonzero(t.valid == 0)).any() and (got[1][:, t.valid == 0] == -1).all()
    valid = np.ones((1, 33), dtype=np.uint8)
    valid[0, 32] = 0
    masked = a.locate_scan(z33[None], many.args.tol, many.args.min_sep, many.args.max_base, many.args.max_out, index=None, valid=valid)[0]
    assert masked[0].tobytes() == search(a, many)[0].tobytes() and masked[1][:, :32].tobytes() == search(a, many)[1].tobytes()
    a.close()


# ---- 3. overflow ----------------------------------------------------------------------------------------
def test_a_list_that_grows(pkg, pipeline_mode):
    t, ref = reference(pkg)["overflow N=200, tol %g" % lr.OVERFLOW_TOL]
    assert ref.n_cand > lr.LIST_FLOOR
    a = loaded(pkg, t.x, t.P, 320)
    small, ref_small = reference(pkg)["planted N=200, tol 0.1"]
    assert ref_small.n_cand > lr.LIST_FLOOR   # (the planted scan itself outgrows the first list at this tolerance)
    bytes0 = a.device_bytes()
    got = search(a, t)
    lr.check(got, ref, t.name)
    assert a.device_bytes() >= bytes0 + 16 * ref.n_cand   # a score, a key and a count per candidate
    assert same_bits(search(a, t), got)
    lr.check(search(a, small), ref_small, small.name)   # the larger list serves a smaller call
    a.close()


def test_too_many_candidates_are_refused_and_nothing_sticks(pkg, pipeline_mode):
    # 2100 landmarks on a grid of pitch 0.5 (23 m across): with tol 5 most of the 4.4 million ordered pairs pass the length filter of each base pair
    side = 46
    g = np.stack(np.meshgrid(np.arange(side) * 0.5, np.arange(side) * 0.5), axis=-1).reshape(-1, 2)[:2100]
    x = np.concatenate([[0.0, 0.0, 0.0], g.reshape(-1)])
    a = loaded(pkg, x, np.eye(len(x)) * 0.01, 2100)
    z = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]])
    cnt = ctypes.c_longlong(0)
    room, idr = (pkg.ekfslam.EkfLocateHyp * 4)(), (ctypes.c_int * 12)(*([7] * 12))
    zp = z.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = a.L.ekf_locate_scan(a.h, 0, zp, 3, 5.0, 1.0, 3, 4, room, idr, ctypes.byref(cnt))
    assert rc == pkg.ekfslam.ERR_CAPACITY and cnt.value > lr.MAX_CAND and list(idr) == [7] * 12
    assert b"tol too loose" in a.L.ekf_last_error()
    a.sync()   # not sticky
    assert len(a.locate_scan(z, 0.01, max_base=1)[0]) > 0
    a.close()


# ---- 4. the batch form ----------------------------------------------------------------------------------
def test_batch_equals_single_calls_bit_for_bit(pkg, pipeline_mode):
    ref = [reference(pkg)["wide batch, filter %d" % b] for b in range(4)]
    f = loaded(pkg, None, None, 320, batch=4, max_pending=8)
    for b, (t, _) in enumerate(ref):
        if lr.WIDE_COUNTS[b]:
            f.set_state(t.x, t.P, index=b)
    z, valid = np.stack([t.z for t, _ in ref]), np.stack([t.valid for t, _ in ref])
    args = ref[0][0].args
    assert np.isnan(z[valid == 0]).all() and list(f.num_landmarks()) == list(lr.WIDE_COUNTS)
    one = f.locate_scan(z, args.tol, args.min_sep, args.max_base, args.max_out, index=None, valid=valid)
    two = f.locate_scan(z, args.tol, args.min_sep, args.max_base, args.max_out, index=None, valid=valid)
    for b, (t, r) in enumerate(ref):
        assert same_bits(one[b], two[b])
        lr.check(one[b], r, t.name)
        at = np.flatnonzero(valid[b])
        hyps, ids, n_cand = f.locate_scan(z[b][at], args.tol, args.min_sep, args.max_base, args.max_out, index=b)   # the one-filter call on the valid entries
        assert n_cand == one[b][2] and ids.tobytes() == np.ascontiguousarray(one[b][1][:, at]).tobytes()
        mapped = hyps.copy()
        mapped["meas_a"], mapped["meas_b"] = at[hyps["meas_a"]], at[hyps["meas_b"]]
        assert mapped.tobytes() == one[b][0].tobytes()
        if lr.WIDE_COUNTS[b]:
            assert lr.WIDE_COUNTS[b] - 1 in (int(hyps["lm_i"][0]), int(hyps["lm_j"][0]))
    assert len(one[1][0]) == 0 and one[1][2] == 0
    f.close()


# ---- 5. read-only, window open --------------------------------------------------------------------------
def test_read_only_with_a_window_open(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    xb = b.get_x()
    L = xb[3:].reshape(-1, 2)
    lms = np.argsort(np.hypot(L[:, 0] - xb[0], L[:, 1] - xb[1]), kind="stable")[:8]
    z = lr.scan_of_landmarks(xb, lms, 3130)
    w0 = windows_closed(a)
    on, _ = stream_starts(a)
    opened = a.locate_scan(z, 0.1, max_out=2)   # (behind the hits of the true pose come hypotheses of two inliers, whose (i, j) and (j, i) tie)
    assert windows_closed(a) == w0   # nothing folded, no pass: the window stays open
    assert a.stats() == b.stats() and a.decisions() == b.decisions()
    ref = lr.locate(xb, z, 0.1, max_out=2)
    lr.check_margins(ref, "open window")
    lr.check(opened, ref, "open window")
    assert opened[0]["inliers"][0] == 8 and opened[1][0].tolist() == lms.tolist()
    a.flush()
    assert same_bits(a.locate_scan(z, 0.1, max_out=2), opened)   # x is current inside the open window
    assert_bitwise(a.get_state(), b.get_state(), "the handle behind the calls against its twin")
    assert a.stats() == b.stats() and a.decisions() == b.decisions()
    a.close(), b.close()


def test_bad_arguments_leave_the_handle_untouched(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 60, 64, seed=71, steps=3)
    L, E = a.L, pkg.ekfslam
    w0, s0 = windows_closed(a), stream_starts(a)
    z = np.array([[2.0, 0.5], [1.0, -0.5], [0.0, 3.0]])
    zn = z.copy()
    zn[1, 0] = np.nan
    dp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    room, idr = (E.EkfLocateHyp * 4)(), (ctypes.c_int * 12)()
    nan, inf = float("nan"), float("inf")
    bad = [(0, dp(z), -1, 0.1, 1.0, 4, 4, room, idr), (0, None, 3, 0.1, 1.0, 4, 4, room, idr), (0, dp(zn), 3, 0.1, 1.0, 4, 4, room, idr),
           (0, dp(z), 3, 0.0, 1.0, 4, 4, room, idr), (0, dp(z), 3, nan, 1.0, 4, 4, room, idr), (0, dp(z), 3, inf, 1.0, 4, 4, room, idr),
           (0, dp(z), 3, 0.1, -1.0, 4, 4, room, idr), (0, dp(z), 3, 0.1, nan, 4, 4, room, idr), (0, dp(z), 3, 0.1, 1.0, 0, 4, room, idr),
           (0, dp(z), 3, 0.1, 1.0, 17, 4, room, idr), (0, dp(z), 3, 0.1, 1.0, 4, 0, room, idr), (0, dp(z), 3, 0.1, 1.0, 4, 65, room, idr),
           (0, dp(z), 3, 0.1, 1.0, 4, 4, None, idr), (0, dp(z), 3, 0.1, 1.0, 4, 4, room, None), (1, dp(z), 3, 0.1, 1.0, 4, 4, room, idr),
           (-1, dp(z), 3, 0.1, 1.0, 4, 4, room, idr)]
    for args in bad:
        assert L.ekf_locate_scan(a.h, *args, None) == E.ERR_BAD_ARG, args[2:7]
    found = (ctypes.c_int * 1)()
    assert L.ekf_batch_locate_scan(a.h, dp(z), None, 3, 0.1, 1.0, 4, 4, room, idr, None, None) == E.ERR_BAD_ARG
    assert L.ekf_locate_scan(None, 0, dp(z), 3, 0.1, 1.0, 4, 4, room, idr, None) == E.ERR_BAD_ARG
    mask = (ctypes.c_ubyte * 3)(1, 0, 1)
    assert L.ekf_batch_locate_scan(a.h, dp(zn), mask, 3, 0.1, 1.0, 4, 4, room, idr, found, None) == 0   # a NaN in a masked entry is not looked at
    R = np.tile(np.array([0.01, 0.0, 0.0, 0.01]), (3, 1))
    prr, hyp, d2 = np.zeros(9), E.EkfLocateHyp(), (ctypes.c_double * 3)()
    Ri, pneg = R.copy(), np.zeros(9)
    Ri[2, 3], pneg[4] = inf, -1.0
    for zz, RR, mi, lead, pp in ((z, R, 1, 0, prr), (z, R, 2, -1, prr), (z, Ri, 2, 0, prr), (zn, R, 2, 0, prr), (z, R, 2, 0, pneg), (z, None, 2, 0, prr)):
        rc = L.ekf_relocalize(a.h, 0, dp(zz), dp(RR) if RR is not None else None, 3, 0.1, 1.0, 4, 4, mi, lead, dp(pp), ctypes.byref(hyp), idr, d2)
        assert rc == E.ERR_BAD_ARG, (mi, lead)
    assert L.ekf_relocalize(a.h, 0, dp(z), dp(R), 3, 0.1, 1.0, 4, 4, 2, 0, None, ctypes.byref(hyp), idr, d2) == E.ERR_BAD_ARG
    assert windows_closed(a) == w0 and stream_starts(a) == s0
    assert a.stats() == b.stats() and a.decisions() == b.decisions()
    assert_bitwise(a.get_state(), b.get_state(), "behind the refused calls")
    a.close(), b.close()


def test_a_sticky_capacity_status_does_not_block_the_search(pkg, pipeline_mode):
    g, x0, _ = make_filter(pkg, 8, 8, seed=73)
    zf, Rf = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(zf.reshape(1, 1, 2), Rf.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    z = lr.scan_of_landmarks(x0, [0, 7, 3], 730)
    got = g.locate_scan(z, 0.1, max_out=1)
    ref = lr.locate(g.get_x(), z, 0.1, max_out=1)
    lr.check_margins(ref, "sticky EKF_ERR_CAPACITY")
    lr.check(got, ref, "sticky EKF_ERR_CAPACITY")
    with pytest.raises(pkg.EkfError) as ei:
        g.reset_pose(np.zeros(3), P_RR)   # ... but blocks the reset, as it blocks ekf_transform_frame
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    g.close()


# ---- 6. ekf_relocalize ----------------------------------------------------------------------------------
def lost(x):
    """The planted state with the pose far off."""
    y = x.copy()
    y[0], y[1], y[2] = x[0] + lr.LOST[0], x[1] + lr.LOST[0], x[2] + lr.LOST[1]
    return y


@pytest.mark.parametrize("N,cap", lr.SIZES)
def test_relocalize_against_the_reference_and_the_three_calls(pkg, pipeline_mode, N, cap):
    t, _ = reference(pkg)["planted N=%d, tol 0.1" % N]
    xl = lost(t.x)
    a = loaded(pkg, xl, t.P, cap)
    fork = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    assert fork.extract_map(a) == N
    st, dec = a.stats(), a.decisions()
    n, hyp, ids, d2 = a.relocalize(t.z, t.R, 0.1, P_RR, min_inliers=6, lead=2)
    want = lr.relocalize(xl, t.P, t.z, t.R, 0.1, P_RR, min_inliers=6, lead=2, window=16)
    assert n == want[0] == 10 and ids.tolist() == want[4].tolist() == t.ids.tolist()
    assert a.stats() == st and a.decisions() == dec
    xg, Pg = a.get_state()
    assert np.hypot(*(xg[:2] - t.x[:2])) < 0.05 and abs(xg[2] - t.x[2]) < 0.02   # found again
    mr.assert_d2_close(d2, want[5], "relocalize N=%d" % N, mr.D2_REL)
    err = assert_state_close(xg, Pg, want[1], want[2], what="relocalize N=%d" % N)
    print("relocalize N=%d: x %.3e, P %.3e of its largest entry" % ((N,) + err))
    # the three public calls in sequence on the fork: the same bits
    hyps, idl, _ = fork.locate_scan(t.z, 0.1)
    assert hyps[0].tobytes() == hyp.tobytes() and idl[0].tobytes() == ids.tobytes()
    fork.reset_pose(hyps["pose"][0], P_RR)
    res = fork.update_matched(t.z, t.R, idl[0])
    assert res[:2] == (N, 10) and res[2].tobytes() == d2.tobytes()
    assert_bitwise(a.get_state(), fork.get_state(), "relocalize against the three calls")
    a.close(), fork.close()


def test_relocalize_refused_inside_an_open_window(pkg, pipeline_mode):
    a, b, _ = open_window_pair(pkg, 100, 200, seed=13, steps=3)
    xb = b.get_x()
    L = xb[3:].reshape(-1, 2)
    lms = np.argsort(np.hypot(L[:, 0] - xb[0], L[:, 1] - xb[1]), kind="stable")[:8]
    z = lr.scan_of_landmarks(xb, lms, 3130)
    R = np.tile(np.eye(2) * 1e-4, (8, 1, 1))
    w0 = windows_closed(a)
    n, hyp, ids, d2 = a.relocalize(z, R, 0.1, P_RR, min_inliers=9, lead=2)   # eight measurements cannot give nine inliers
    assert n == 0 and hyp["inliers"] == 8 and ids.tolist() == lms.tolist() and np.isnan(d2).all()
    assert windows_closed(a) == w0   # refused behind the search, which only reads: the window is still open
    assert a.stats() == b.stats() and a.decisions() == b.decisions()
    assert_bitwise(a.get_state(), b.get_state(), "behind the refused call")
    a.close(), b.close()


def test_relocalize_refuses_the_issue_case(pkg, pipeline_mode):
    """N = 200 at tol 0.05 with one base pair: the farthest-apart pair holds a spurious measurement, the best hypothesis has 4
    inliers; returns 0, the state bit for bit."""
    t, ref = reference(pkg)["planted N=200, one base pair"]
    a = loaded(pkg, lost(t.x), t.P, 320)
    pre, st, dec = a.get_state(), a.stats(), a.decisions()
    for tol in (0.05, 0.1):
        n, hyp, ids, d2 = a.relocalize(t.z, t.R, tol, P_RR, max_base=1, min_inliers=6, lead=2)
        want = lr.locate(t.x, t.z, tol, max_base=1)
        assert n == 0 and hyp["inliers"] == want.hyps["inliers"][0] < 6 and ids.tolist() == want.ids[0].tolist() and np.isnan(d2).all()
    assert a.stats() == st and a.decisions() == dec
    assert_bitwise(a.get_state(), pre, "behind the refused calls")
    n, _, ids, _ = a.relocalize(t.z, t.R, 0.1, P_RR, max_base=4, min_inliers=6, lead=2)   # four base pairs succeed where one fails
    assert n == 10 and ids.tolist() == t.ids.tolist()
    a.close()


def test_batch_relocalize_leaves_the_refused_filters_alone(pkg, pipeline_mode):
    t, _ = reference(pkg)["planted N=100, tol 0.1"]
    f = loaded(pkg, None, None, 200, batch=2)
    g = loaded(pkg, lost(t.x), t.P, 200)
    for b in range(2):
        f.set_state(lost(t.x), t.P, index=b)
    z, R = np.stack([t.z, t.z]), np.stack([t.R, t.R])
    z[1, [0, 1, 2, 4, 5, 6]] += 40.0   # filter 1's scan fits nowhere
    pre1 = f.get_state(1)
    n, hyps, ids, d2 = f.relocalize(z, R, 0.1, np.stack([P_RR, P_RR]), min_inliers=6, lead=2, index=None)
    one = g.relocalize(t.z, t.R, 0.1, P_RR, min_inliers=6, lead=2)
    assert n.tolist() == [10, 0] and one[0] == 10
    assert hyps[0].tobytes() == one[1].tobytes() and ids[0].tobytes() == one[2].tobytes() and d2[0].tobytes() == one[3].tobytes()
    assert_bitwise(f.get_state(0), g.get_state(), "the accepted filter against the one-filter call")
    assert_bitwise(f.get_state(1), pre1, "the refused filter")
    assert np.isnan(d2[1]).all()
    f.close(), g.close()
