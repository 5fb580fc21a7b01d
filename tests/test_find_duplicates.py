"""Duplicate search on the device: ekf_find_duplicates / ekf_batch_find_duplicates (the pairwise gate d^T S^-1 d <= gate with
S = P_ii + P_jj - P_ij - P_ij^T read from the settled tile layout).  The reference is tests/dup_ref.py (NumPy on the dense export;
checked on the CPU in tests/test_find_duplicates_cpu.py) and the states come from its builder: eight planted pairs with d2 =
0, 1e-6, 0.5, 3, 9.0, 9.4, 12, 30 against the gate 9.21, renumbered by a fixed permutation, beside the natural close pairs of the
injected maps.  The LIST of (i, j) must equal the reference's exactly -- under the precondition, asserted on the reference, that no
pair lies within 1e-3 relative of the gate or of max_dist -- and d2 within REL_TOL relative + 1e-9 absolute (the observed errors are
printed; the kernel evaluates the reference's operations in the reference's order, so they are expected around 1e-16 .. 1e-12).
The call only reads the filter: a witness handle that exported at the same point stays bit for bit the same.
Sizes (N, capacity): a partial tile, exactly one tile, one landmark in a second tile, an off-diagonal tile beside diagonal ones,
the one-workgroup and the several-workgroup chain kernel."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dup_ref as dr  # noqa: E402
import join_ref as jr  # noqa: E402
from helpers import assert_bitwise, assert_state_close, ij, make_filter, run_steps, stream_starts  # noqa: E402
from helpers import check_duplicates as check  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(31, 64), (32, 64), (33, 64), (100, 128), (180, 200), (280, 320)]


@functools.lru_cache(maxsize=None)
def built_state(pkg, N, seed, exact=0):
    """N landmarks after the builder: N - 8 - exact injected ones, eight planted duplicates (and `exact` exact copies)."""
    n0 = N - len(dr.TARGETS) - exact
    x, P = pkg.scenarios.injected_state(n0, seed=seed, extent=12.0 * (n0 / 64.0) ** 0.5 + 8.0)
    x, P, planted = dr.with_duplicates(x, P, seed=seed + 1, exact=exact)
    x.setflags(write=False), P.setflags(write=False)
    return x, P, tuple(planted)


def loaded(pkg, N, cap, seed, exact=0):
    x, P, planted = built_state(pkg, N, seed, exact)
    f = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    f.set_state(x, P)
    return f, x, P, planted


def open_window_pair(pkg, N, cap, seed, steps):
    """helpers.open_window_pair on the built state: handles A and B after the same immediate calls (window open, streaming launch
    live on both); B is the witness."""
    a, x0, _, planted = loaded(pkg, N, cap, seed)
    b = loaded(pkg, N, cap, seed)[0]
    sc = pkg.scenarios.steady_script(x0, steps=steps, M=2, seed=seed + 1, min_separation=1.0)
    da, _ = run_steps(pkg, a, sc, 0, steps, 2)
    db, _ = run_steps(pkg, b, sc, 0, steps, 2)
    assert da == db
    return a, b, planted


# ---- 1. parity with a window open ---------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", CASES)
def test_parity_with_a_window_open(pkg, pipeline_mode, N, cap):
    a, b, planted = open_window_pair(pkg, N, cap, seed=11, steps=5)
    x, P = b.get_state()
    got = a.find_duplicates()
    worst = check(got, x, P, what="N=%d" % N)
    listed = set(ij(got[0]))
    for i, j, target in planted:  # (the updates of other landmarks move both copies alike: the planted d2 stay where they were)
        assert ((i, j) in listed) == (target <= dr.GATE), (i, j, target)
    blind, _ = dr.find(x, dr.without_cross_blocks(P))
    assert ij(blind) != ij(got[0])  # a gate that ignores P_ij answers something else
    print("N=%d: %d pairs (%d planted below the gate), worst error of d2 %.3e (relative, floor 1e-9)" % (N, got[1], 5, worst))
    again = a.find_duplicates()
    assert again[0].tobytes() == got[0].tobytes() and again[1:] == got[1:]  # an unchanged state: the same bits
    a.close(), b.close()


# ---- 2. splits and the Euclidean bound ----------------------------------------------------------------
@pytest.mark.parametrize("N,cap", CASES)
def test_splits_and_max_dist(pkg, pipeline_mode, N, cap):
    f, x, P, _ = loaded(pkg, N, cap, seed=21)
    assert_bitwise(f.get_state(), (x, P), "the loaded state")
    worst = 0.0
    for split in (0, 1, 31, 32, 33, N - 1, N):
        if split > N:
            continue
        free = f.find_duplicates(split=split)
        for max_dist in (0.05, 1.0, None):
            got = free if max_dist is None else f.find_duplicates(max_dist=max_dist, split=split)
            worst = max(worst, check(got, x, P, max_dist=max_dist, split=split, what="N=%d split=%d max_dist=%s" % (N, split, max_dist)))
            if max_dist is not None:  # with the culling = the unbounded call, filtered
                L = x[3:].reshape(-1, 2)
                d = L[free[0]["i"]] - L[free[0]["j"]]
                near = free[0][np.hypot(d[:, 0], d[:, 1]) <= max_dist]
                assert got[0].tobytes() == near.tobytes() and got[1] == len(near), (N, split, max_dist)
    print("N=%d: worst error of d2 over all splits and bounds %.3e" % (N, worst))
    f.close()


def test_culling_on_a_map_numbered_along_a_path(pkg, pipeline_mode):
    """Landmarks numbered along a path: most tiles' bounding boxes are further apart than max_dist and return unread.  The same
    pairs as the unbounded call, filtered."""
    N = 200
    x, P, _ = built_state(pkg, N, 25)
    order = np.argsort(x[3::2], kind="stable")  # renumber by x: groups of 32 become strips
    rows = np.concatenate([np.arange(3), np.stack([3 + 2 * order, 4 + 2 * order], axis=1).reshape(-1)])
    x, P = x[rows].copy(), P[np.ix_(rows, rows)].copy()
    f = pkg.FilterBatch(1, 256)
    f.set_state(x, P)
    free = f.find_duplicates()
    check(free, x, P, what="path")
    for max_dist in (0.05, 0.3, 2.0):
        got = f.find_duplicates(max_dist=max_dist)
        check(got, x, P, max_dist=max_dist, what="path max_dist=%s" % max_dist)
        L = x[3:].reshape(-1, 2)
        d = L[free[0]["i"]] - L[free[0]["j"]]
        assert got[0].tobytes() == free[0][np.hypot(d[:, 0], d[:, 1]) <= max_dist].tobytes()
    f.close()


# ---- 3. truncation and count-only ---------------------------------------------------------------------
def test_truncation_and_count_only(pkg, pipeline_mode):
    f, x, P, _ = loaded(pkg, 100, 128, seed=31)
    full = f.find_duplicates()
    found = full[1]
    assert found >= 3 and len(full[0]) == found
    check(full, x, P, what="full")
    for max_pairs in (0, 1, found - 1):
        got = f.find_duplicates(max_pairs=max_pairs)
        assert got[1] == found and got[2] == full[2] and len(got[0]) == max_pairs
        assert got[0].tobytes() == full[0][:max_pairs].tobytes()
    E = pkg.ekfslam
    assert f.L.ekf_find_duplicates(f.h, 0, dr.GATE, 0.0, 0, None, 0, None) == found  # count only, no degenerate counter either
    # a gate that lets thousands of pairs through: more than the device list held so far (the search runs again), the first ones out
    many = f.find_duplicates(gate=1e12, max_pairs=7)
    assert many[1] == 100 * 99 // 2 and ij(many[0]) == [(0, j) for j in range(1, 8)]
    allp = f.find_duplicates(gate=1e12, max_pairs=5000)
    assert allp[1] == 4950 and ij(allp[0]) == [(i, j) for i in range(100) for j in range(i + 1, 100)]
    assert allp[0][:7].tobytes() == many[0].tobytes()
    assert f.find_duplicates()[0].tobytes() == full[0].tobytes()
    assert E.DUP_DTYPE.itemsize == 16
    f.close()


# ---- 4. degenerate pairs --------------------------------------------------------------------------------
def test_an_exact_copy_is_counted_not_listed(pkg, pipeline_mode):
    f, x, P, planted = loaded(pkg, 100, 128, seed=41, exact=1)
    i, j, target = planted[-1]
    assert target is None
    got = f.find_duplicates()
    check(got, x, P, what="exact copy")
    assert got[2] == 1 and (i, j) not in set(ij(got[0]))
    listed = set(ij(got[0]))
    for a, b, t in planted[:-1]:  # the other pairs are not disturbed
        assert ((a, b) in listed) == (t <= dr.GATE)
    assert f.find_duplicates(split=j)[2] == 1 and f.find_duplicates(split=i)[2] == 0  # (i < split <= j is what a split considers)
    f.close()


# ---- 5. read-only ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", [(33, 64), (100, 128), (280, 320), (180, 200)])
def test_the_filter_is_only_read(pkg, pipeline_mode, N, cap):
    a, b, _ = open_window_pair(pkg, N, cap, seed=52, steps=5)
    on, starts0 = stream_starts(a)
    x, P = b.get_state()  # B exports at the point where A is searched
    bytes0 = a.device_bytes()
    r = a.find_duplicates(max_dist=1.0)
    check(r, x, P, max_dist=1.0, what="N=%d" % N)
    assert a.device_bytes() > bytes0  # the scratch is counted
    assert a.stats() == b.stats() and a.decisions() == b.decisions() and np.array_equal(a.poses(), b.poses())
    assert np.array_equal(a.robot_cov(), b.robot_cov()) and np.array_equal(a.num_landmarks(), b.num_landmarks())
    assert_bitwise(a.get_state(), (x, P), "after the call")
    sc2 = pkg.scenarios.steady_script(x, steps=12, M=2, seed=54, min_separation=1.0)
    da, ka = run_steps(pkg, a, sc2, 0, 12, 2, new_every=2)
    db, kb = run_steps(pkg, b, sc2, 0, 12, 2, new_every=2)
    assert da == db and ka == kb == 6 and int(a.num_landmarks()[0]) >= N + 6
    if on:
        assert stream_starts(a)[1] > starts0  # immediate-mode calls stream again
    xb, Pb = b.get_state()
    r2 = a.find_duplicates()
    check(r2, xb, Pb, what="N=%d after 12 more steps" % N)
    assert_bitwise(a.get_state(), (xb, Pb), "after 12 more steps")
    assert a.stats() == b.stats() and a.decisions() == b.decisions()
    bytes1 = a.device_bytes()
    a.reserve(2 * cap + 40)
    assert a.device_bytes() > bytes1  # the scratch has followed the capacity
    bytes2 = a.device_bytes()
    r3 = a.find_duplicates()
    assert r3[0].tobytes() == r2[0].tobytes() and r3[1:] == r2[1:]
    assert a.device_bytes() == bytes2  # no second allocation
    assert_bitwise(a.get_state(), (xb, Pb), "after the growth and the call")
    a.close(), b.close()


# ---- 6. batches -----------------------------------------------------------------------------------------
def test_batch_equals_the_single_calls(pkg, pipeline_mode):
    f = pkg.FilterBatch(3, 128)
    sizes, splits = (40, 100, 17), (17, 64, 0)
    states = []
    for b, N in enumerate(sizes):
        x, P, _ = built_state(pkg, N, 60 + b)
        f.set_state(x, P, index=b)
        states.append((x, P))
    rows = f.find_duplicates(split=splits, index=None)
    for b in range(3):
        one = f.find_duplicates(split=splits[b], index=b)
        assert one[0].tobytes() == rows[b][0].tobytes() and one[1:] == rows[b][1:], b
        check(rows[b], *states[b], split=splits[b], what="filter %d" % b)
    assert sum(r[1] for r in rows) >= 3
    rows0 = f.find_duplicates(index=None, max_dist=1.0)  # split NULL-equivalent: all 0
    for b in range(3):
        one = f.find_duplicates(index=b, max_dist=1.0)
        assert one[0].tobytes() == rows0[b][0].tobytes() and one[1:] == rows0[b][1:], b
        check(rows0[b], *states[b], max_dist=1.0, what="filter %d, all pairs" % b)
    short = f.find_duplicates(index=None, max_pairs=2)
    for b in range(3):
        full_b = f.find_duplicates(index=b)
        assert short[b][0].tobytes() == full_b[0][:2].tobytes() and short[b][1] == full_b[1]
    # an empty filter and a filter of one landmark find nothing
    g = pkg.FilterBatch(2, 16)
    x1, P1 = pkg.scenarios.injected_state(1, seed=66)
    g.set_state(x1, P1, index=1)
    assert [(len(r[0]), r[1], r[2]) for r in g.find_duplicates(index=None)] == [(0, 0, 0), (0, 0, 0)]
    assert g.find_duplicates(index=1, split=1)[1:] == (0, 0)
    f.close(), g.close()


# ---- 7. bad arguments and sticky statuses ---------------------------------------------------------------
def test_bad_arguments_leave_the_handle_untouched(pkg, pipeline_mode):
    E = pkg.ekfslam
    f, x, P, _ = loaded(pkg, 33, 64, seed=71)
    L, h = f.L, f.h
    out = (E.EkfDupPair * 4)()
    nd = ctypes.c_int(-7)
    nf = (ctypes.c_int * 1)()
    nan, inf = float("nan"), float("inf")
    bad = [(1, dr.GATE, 0.0, 0, out, 4), (-1, dr.GATE, 0.0, 0, out, 4), (0, nan, 0.0, 0, out, 4), (0, inf, 0.0, 0, out, 4), (0, -1.0, 0.0, 0, out, 4),
           (0, dr.GATE, nan, 0, out, 4), (0, dr.GATE, 0.0, -1, out, 4), (0, dr.GATE, 0.0, 34, out, 4), (0, dr.GATE, 0.0, 0, out, -1), (0, dr.GATE, 0.0, 0, None, 4)]
    for index, gate, md, split, po, mp in bad:
        assert L.ekf_find_duplicates(h, index, gate, md, split, po, mp, ctypes.byref(nd)) == E.ERR_BAD_ARG, (index, gate, md, split, mp)
    assert L.ekf_find_duplicates(None, 0, dr.GATE, 0.0, 0, out, 4, None) == E.ERR_BAD_ARG
    assert L.ekf_batch_find_duplicates(h, dr.GATE, 0.0, None, out, 4, None, None) == E.ERR_BAD_ARG  # n_found_out is not optional
    assert L.ekf_batch_find_duplicates(h, dr.GATE, 0.0, None, None, 4, nf, None) == E.ERR_BAD_ARG
    assert L.ekf_batch_find_duplicates(h, nan, 0.0, None, out, 4, nf, None) == E.ERR_BAD_ARG
    assert L.ekf_batch_find_duplicates(h, dr.GATE, 0.0, (ctypes.c_int * 1)(34), out, 4, nf, None) == E.ERR_BAD_ARG
    assert L.ekf_batch_find_duplicates(None, dr.GATE, 0.0, None, out, 4, nf, None) == E.ERR_BAD_ARG
    assert nd.value == -7
    assert_bitwise(f.get_state(), (x, P), "after the refused calls")
    check(f.find_duplicates(), x, P, what="after the refused calls")
    check(f.find_duplicates(max_dist=inf), x, P, what="an infinite bound is no bound")
    check(f.find_duplicates(max_dist=-1.0, split=33), x, P, split=33, what="a negative bound is no bound; split = N considers nothing")
    check(f.find_duplicates(gate=0.0), x, P, gate=0.0, what="gate 0")
    f.close()


def test_a_sticky_capacity_status_does_not_block_the_call(pkg, pipeline_mode):
    g, _, _ = make_filter(pkg, 8, 8, seed=73)
    z, R = pkg.scenarios.measurement_from_feature_mm(60000.0, 10000.0)
    g.update(z.reshape(1, 1, 2), R.reshape(1, 1, 2, 2), want_decisions=False)  # New, no room
    got = g.find_duplicates(gate=1e9)
    x, P = g.get_state()
    assert got[1] == 28
    check(got, x, P, gate=1e9, what="sticky EKF_ERR_CAPACITY")
    with pytest.raises(pkg.EkfError) as ei:
        g.sync()
    assert ei.value.code == pkg.ekfslam.ERR_CAPACITY
    g.close()


_TIMEOUT_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import __graft_entry__ as ge
pkg = ge.load_package()
N, M, steps = 700, 4, 40
x0, P0 = pkg.scenarios.injected_state(N, seed=5)
sc = pkg.scenarios.steady_script(x0, steps=steps, M=M, seed=6)
f = pkg.FilterBatch(1, N, max_pending=8)
assert f.overlap
f.set_state(x0, P0)
f.script_load(sc["ctrl"][:, None, :], sc["z"][:, :, None, :], sc["R"][:, :, None, :])
f.script_run(0, steps)
for call in (f.sync, f.find_duplicates, lambda: f.find_duplicates(index=None), f.find_duplicates):
    try:
        call()
    except pkg.ekfslam.EkfError as e:
        assert e.code == pkg.ekfslam.ERR_TIMEOUT, e
    else:
        raise AssertionError("no timeout reported")
os.environ.pop("EKF_DEBUG_DROP_MARKS_FROM"); os.environ.pop("EKF_DEBUG_SPIN_LIMIT")
f.set_state(x0, P0)
assert f.find_duplicates(gate=0.0)[1] == 0
f.close()
print("timeout child ok")
"""


@functools.lru_cache(maxsize=None)
def timeout_child():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "2d-ekf-slam_amd", "lib", "libekfslam_hip_debug.so")
    assert os.path.exists(dbg), "build the debug variant: make -C 2d-ekf-slam_amd/csrc debug"
    env = dict(os.environ, EKFSLAM_LIB=dbg, EKF_OVERLAP="1", EKF_DEBUG_DROP_MARKS_FROM="3", EKF_DEBUG_SPIN_LIMIT=str(1 << 13))
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout[-2000:], r.stderr[-4000:]


def test_a_sticky_timeout_is_returned_unchanged(pkg, pipeline_mode):
    """A dense pass that never reports (a hook of the debug variant of the library, loaded in a child process as
    tests/test_gpu_parity.py does) leaves EKF_ERR_TIMEOUT sticky: both forms return it, and the handle works again after
    ekf_set_state.  The child runs in overlap mode whatever this test's mode is, once for both."""
    rc, out, err = timeout_child()
    assert rc == 0 and "timeout child ok" in out, (out, err)


# ---- 8. the workflow: join, find with split = Ng, keep mask, remove ---------------------------------------
def joined_pair(pkg):
    """A destination of 100 landmarks and a local map of 12 in the frame of the destination's pose: 8 re-observations of isolated
    destination landmarks (the estimate moved by a fraction of its standard deviation) and 4 landmarks far away from everything."""
    Ng, Ns, cap = 100, 12, 200
    rng = np.random.default_rng(81)
    xg, Pg = pkg.scenarios.injected_state(Ng, seed=82, extent=23.0)
    L = xg[3:].reshape(-1, 2)
    d2 = ((L[:, None, :] - L[None, :, :]) ** 2).sum(-1)
    d2[np.diag_indices(Ng)] = np.inf
    seen = np.flatnonzero(np.sqrt(d2.min(axis=1)) >= 2.0)[:8]
    assert len(seen) == 8
    xs, Ps = pkg.scenarios.injected_state(Ns, seed=83, extent=6.0)
    xs[0:3] = (0.4, -0.3, 0.2)
    c, s = np.cos(xg[2]), np.sin(xg[2])
    C = np.array([[c, -s], [s, c]])
    at = rng.permutation(Ns)[:8]  # the local numbers of the re-observed landmarks
    for k, l in zip(at, seen):
        xs[3 + 2 * k:5 + 2 * k] = C.T @ (L[l] - xg[0:2]) + rng.normal(0.0, 0.03, size=2)
    for q, k in enumerate(sorted(set(range(Ns)) - set(at.tolist()))):
        xs[3 + 2 * k:5 + 2 * k] = (300.0 + 40.0 * q, -200.0 - 35.0 * q)
    want = sorted((int(l), Ng + int(k)) for k, l in zip(at, seen))
    return Ng, Ns, cap, (xg, Pg), (xs, Ps), want


def test_join_find_and_remove(pkg, pipeline_mode):
    Ng, Ns, cap, (xg, Pg), (xs, Ps), want = joined_pair(pkg)
    handles = []
    for _ in range(2):  # the handle under test and its witness: the same join
        f, src = pkg.FilterBatch(1, cap), pkg.FilterBatch(1, 32)
        f.set_state(xg, Pg)
        src.set_state(xs, Ps)
        assert f.join_map(src) == Ng + Ns
        src.close()
        handles.append(f)
    a, w = handles
    x, P = w.get_state()
    assert_state_close(x, P, *jr.join(xg, Pg, xs, Ps), what="the joined state")
    got = a.find_duplicates(split=Ng)
    worst = check(got, x, P, split=Ng, what="old x new")
    print("join %d + %d: %d pairs across the split, d2 %s, worst error %.3e" % (Ng, Ns, got[1], np.round(got[0]["d2"], 3).tolist(), worst))
    # every re-observed landmark is listed with its original; a joined landmark's covariance carries the lever arm of the pose it was
    # joined at, so its gate may let further old landmarks a few metres away through: the one-to-one matching by ascending d2 sorts
    # them out, the accepted pairs are exactly the 8 re-observations
    assert set(want) <= set(ij(got[0])) and {j for _, j in ij(got[0])} == {j for _, j in want}
    best = {}
    for p in got[0]:
        if int(p["j"]) not in best or p["d2"] < best[int(p["j"])][1]:
            best[int(p["j"])] = (int(p["i"]), float(p["d2"]))
    assert sorted((i, j) for j, (i, _) in best.items()) == want
    blind, _ = dr.find(x, dr.without_cross_blocks(P), split=Ng)
    print("without the cross blocks: %d pairs" % len(blind))
    keep = pkg.duplicate_keep_mask(got[0], Ng + Ns)
    assert np.flatnonzero(~keep).tolist() == sorted(j for _, j in want)
    assert a.remove_landmarks(keep, index=0) == Ng + Ns - 8
    assert w.remove_landmarks(keep, index=0) == Ng + Ns - 8
    assert_bitwise(a.get_state(), w.get_state(), "after removing the duplicates")
    assert a.find_duplicates(split=Ng)[1] == 0
    kf = pkg.KalmanFilter(capacity_landmarks=cap)  # the mirror class: the same call on the same state
    kf.set_state(x, P)
    m = kf.find_duplicates(split=Ng)
    assert m[0].tobytes() == got[0].tobytes() and m[1:] == got[1:]
    kf._f.close(), a.close(), w.close()
