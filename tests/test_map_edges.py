"""The map rewrites at the edges of the tile layout.  P_LL is stored as 64 x 64 tiles of 32 landmarks, the dense vectors are walked
in chunks of 1024 elements, capacity 256 splits the two kernel families; the other GPU tests of removal, frame change, joining and
joint consistency sit in the middle of all that.  Here: maps of 0, 1, 31, 32, 33, 63, 64, 65 landmarks, maps that end on a tile or
on the capacity, removals that lose a tile or move every row across a tile edge, joins that start on a tile edge (no straddling
old x new tile) or fit into the straddling tile altogether, filters of one batch with different tile counts.

Every case: a window is left open by a few immediate steps, a witness handle that ran the same steps exports what the handle under
test held; parity against the NumPy reference (tests/reframe_ref.py, tests/join_ref.py, tests/factor_ref.py; helpers' tolerances) or
bit for bit where the contract says so (np.delete, theta = 0, the old x old block); bitwise symmetry; and a set_state twin that goes
on for three steps with a far New landmark, bit for bit -- the check that sees the zeros behind the map (not the places of a
diagonal tile that are nobody's home, a landmark's own block and the blocks below the diagonal: nothing reads those).  A map that fills its capacity is given room by ekf_reserve first (which must not change a bit).

The same for the three newer map operations.  Fusion (tests/fuse_ref.py, rounds of the handle's window): a pair whose j is alone in
the last tile, 32 pairs over four rounds that give a whole tile back, and maps of 511 / 512 / 513 landmarks, whose columns of
3 + 2 N = 1025 / 1027 / 1029 elements end either side of the 1024-element chunk.  Duplicate search (tests/dup_ref.py, the contract
of tests/test_find_duplicates.py): 0, 1, 2, 63, 64, 65 landmarks and a map that fills its capacity, one planted pair whose later
landmark is the map's last.  Extraction (NumPy indexing, bit for bit): sources of 0 / 1 / 31 / 32 / 33 / 65 landmarks into a
destination of another tile count, a destination that held 65 and receives 1, selections of 511 / 512 / 513 landmarks.  And each of
the three straight behind a window in which a far New landmark has just started a second tile (32 -> 33): they read the settled
tile layout and must close that window themselves.

And for the matched updates (ekf_update_matched / ekf_joint_compat; tests/match_ref.py on the witness' export, rounds of the handle's
window, the scan from match_ref.scan_of on that export; d2 within match_ref.D2_REL_EDGES, which tests/test_update_matched_cpu.py
derives for exactly these inputs): k_match_gather's grid of 256 landmarks per block at 256 and 257 landmarks, the chunk edge at 511 /
512 / 513 as an update of two rounds and as a score of 32 pairings, a full round of 32 (and of 24) measurements applied with one more
behind it in both kernel families, one landmark measured three times in one round, maps that fill their capacity, a landmark alone in
the last tile, and the landmark the open window has just created."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dup_ref as dr  # noqa: E402
import factor_ref as fr  # noqa: E402
import fuse_ref as fu  # noqa: E402
import join_ref as jr  # noqa: E402
import map_model as mm  # noqa: E402
import match_ref as mr  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import (ABS_P, REL_TOL, assert_bitwise, assert_bitwise_symmetric, assert_state_close, batch_script, check_duplicates,  # noqa: E402
                     check_joint, ij, index_state, open_window_pair, run_steps, windows_closed)

pytestmark = pytest.mark.gpu

FRAME = (3.0, -2.0, 0.7)
WINDOW = 8


def opened_pair(pkg, N, cap, seed, extent=None, window=WINDOW):
    """The handle under test and its witness after the same immediate steps, a window open on both.  N = 0: fresh filters that
    have been propagated twice."""
    if N:
        a, w, _ = open_window_pair(pkg, N, cap, seed=seed, steps=2, extent=extent, M=min(2, N), max_pending=window)
        return a, w
    pair = [pkg.FilterBatch(1, cap, max_pending=WINDOW, log_capacity=4096) for _ in range(2)]
    for f in pair:
        f.propagate(0.3, 0.05, 0.05)
        f.propagate(0.2, -0.1, 0.1)
    return pair


def witnessed(pkg, N, cap, seed, extent=None, window=WINDOW):
    """(handle with its window open and its streaming launch live, what it holds as its witness exported it, the witness' stats and
    decision log).  Nothing is asked of the handle itself: reading its counters would have the resident launch leave."""
    a, w = opened_pair(pkg, N, cap, seed, extent, window)
    before, logs = w.get_state(), (w.stats(), w.decisions())
    w.close()
    return a, before, logs


def settled_checks(a, after, logs, N):
    assert_bitwise_symmetric(after[1])
    assert int(a.num_landmarks()[0]) == N == (after[0].size - 3) // 2
    assert np.array_equal(a.poses()[0], after[0][:3]) and np.array_equal(a.robot_cov(), after[1][:3, :3])
    assert (a.stats(), a.decisions()) == logs  # counters and decision log do not move


def twin_goes_on(pkg, a, what, window=WINDOW):
    """Three more steps on the handle and on a twin loaded with set_state of its export: propagations, Old matches where there are
    landmarks, far New landmarks (steps 0 and 2).  Decisions with their distances and the final exports are equal bit for bit."""
    st = a.get_state()
    N = (st[0].size - 3) // 2
    if N + 2 > a.capacity:
        a.reserve(N + 8)
        assert_bitwise(a.get_state(), st, "%s: reserve behind the call" % what)
    b = pkg.FilterBatch(1, a.capacity, max_pending=window, log_capacity=4096)
    b.set_state(*st)
    M = min(2, N)
    if M:
        sc = pkg.scenarios.steady_script(st[0], steps=3, M=M, seed=7 + N, min_separation=1.0)
    else:
        sc = dict(ctrl=np.tile(np.array([0.3, 0.05, 0.05]), (3, 1)), z=np.empty((3, 0, 2)), R=np.empty((3, 0, 4)))
    da, ka = run_steps(pkg, a, sc, 0, 3, M, new_every=2)
    db, kb = run_steps(pkg, b, sc, 0, 3, M, new_every=2)
    assert da == db and ka == kb == 2, what
    assert sum(1 for d in da if d[0] == pkg.ekfslam.NEW) >= 2, (what, da)
    assert_bitwise(a.get_state(), b.get_state(), "%s: handle vs set_state twin" % what)
    b.close()


def mask(N, drop=None, keep_only=None):
    k = np.ones(N, dtype=bool)
    if keep_only is not None:
        k[:] = False
        k[keep_only] = True
    else:
        k[drop] = False
    return k


# ---- removal ------------------------------------------------------------------------------------------
REMOVALS = {
    "the only landmark": (1, 8, mask(1, drop=0)),
    "full single tile, first": (32, 32, mask(32, drop=0)),
    "full single tile, last": (32, 32, mask(32, drop=31)),
    "full single tile, keep only the last": (32, 32, mask(32, keep_only=31)),
    "33 drop 32: the map loses a tile": (33, 64, mask(33, drop=32)),
    "33 drop 0: every row crosses the tile edge": (33, 64, mask(33, drop=0)),
    "64 drop 0..31: a whole-tile shift": (64, 64, mask(64, drop=slice(0, 32))),
    "64 drop the odd ones": (64, 64, mask(64, drop=slice(1, None, 2))),
    "65 keep only the last": (65, 96, mask(65, keep_only=64)),
    "511 drop 0: 3 + 2 N = 1025 -> 1023": (511, 520, mask(511, drop=0)),
    "512 drop 0: 3 + 2 N = 1027 -> 1025": (512, 520, mask(512, drop=0)),
}


@pytest.mark.parametrize("case", list(REMOVALS))
def test_removal(pkg, pipeline_mode, case):
    N, cap, keep = REMOVALS[case]
    a, before, logs = witnessed(pkg, N, cap, seed=100 + N)
    n_new = int(keep.sum())
    assert a.remove_landmarks(keep, index=0) == n_new
    after = a.get_state()
    assert_bitwise(after, mm.reduce_state(*before, keep), case)
    settled_checks(a, after, logs, n_new)
    twin_goes_on(pkg, a, case)
    a.close()


# ---- frame change ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["rigid", "anchor"])
@pytest.mark.parametrize("N,cap", [(0, 8), (1, 8), (31, 32), (32, 32), (33, 64), (64, 64), (65, 96), (128, 128)])
def test_frame_change(pkg, pipeline_mode, N, cap, call):
    a, before, logs = witnessed(pkg, N, cap, seed=200 + N)
    if call == "rigid":
        a.transform_frame(FRAME, index=0)
        want = rr.rigid(*before, FRAME)
    else:
        a.anchor_at_robot(index=0)
        want = rr.anchor(*before)
    after = a.get_state()
    err = assert_state_close(after[0], after[1], *want, what=call)
    print("%s N=%d: max |dx| %.3e, max |dP| / max |P| %.3e" % (call, N, err[0], err[1]))
    settled_checks(a, after, logs, N)
    if call == "anchor":
        assert not after[0][:3].any() and not after[1][:3, :].any() and not after[1][:, :3].any()
    twin_goes_on(pkg, a, "%s N=%d" % (call, N))
    a.close()


def loaded_batch(pkg, cap, counts, seed):
    f = pkg.FilterBatch(len(counts), cap, max_pending=WINDOW, log_capacity=4096)
    for b, n in enumerate(counts):
        if n:
            f.set_state(*pkg.scenarios.injected_state(n, seed=seed + b, extent=3.0 if n == 1 else 6.0 + b), index=b)  # (a lone landmark close by: a distant one is no match)
    return f


def open_batch_window(pkg, f, counts):
    """A propagation on every filter and a measurement of its landmark nearest to the robot, but a metre away at least, where it
    has one (the others are masked out): a slot in the open window, no new landmark."""
    B = f.batch
    z, R = np.zeros((B, 1, 2)), np.tile(np.eye(2), (B, 1, 1, 1))
    for b in range(B):
        if counts[b]:
            x = f.get_x(b)
            c, s = np.cos(x[2]), np.sin(x[2])
            r = np.hypot(*(x[3:].reshape(-1, 2) - x[0:2]).T)
            l = int(np.argmin(np.where(r >= 1.0, r, np.inf)))
            d = x[3 + 2 * l:5 + 2 * l] - x[0:2]
            z[b, 0], R[b, 0] = pkg.scenarios.measurement_from_feature_mm(1000.0 * (c * d[0] + s * d[1]), 1000.0 * (-s * d[0] + c * d[1]))
    f.propagate(0.3, 0.05, 0.05)
    f.update(z, R, valid=(np.array(counts) > 0).reshape(B, 1), want_decisions=False)
    assert list(f.num_landmarks()) == list(counts)


def batch_twin_goes_on(pkg, f, what):
    """Three more batch steps (a measurement near the robot, a far New landmark) on the handle and on a set_state twin: bit for bit."""
    B = f.batch
    states = [f.get_state(b) for b in range(B)]
    g = pkg.FilterBatch(B, f.capacity, max_pending=WINDOW, log_capacity=4096)
    for b in range(B):
        g.set_state(*states[b], index=b)
    ctrl, z, R = batch_script(pkg, B, 3, 2)
    decs = []
    for h in (f, g):
        d = []
        for s in range(3):
            h.propagate(ctrl[s, :, 0], ctrl[s, :, 1], ctrl[s, :, 2])
            d.append(h.update(z[s].transpose(1, 0, 2), R[s].transpose(1, 0, 2).reshape(B, 2, 2, 2)))  # (R is symmetric: either order)
        decs.append(d)
    assert decs[0] == decs[1], what
    for b in range(B):
        assert_bitwise(f.get_state(b), g.get_state(b), "%s: handle vs set_state twin, filter %d" % (what, b))
    g.close()


def test_frame_change_in_a_batch_of_different_tile_counts(pkg, pipeline_mode):
    """Five filters of one handle with 0, 1, 32, 33 and 65 landmarks (0, 1, 1, 2 and 3 tile rows): the batch form with a frame per
    filter (one with theta = 0), then single-index calls on filter 3 that leave the other four bit for bit."""
    counts, cap = (0, 1, 32, 33, 65), 96
    f, w = loaded_batch(pkg, cap, counts, seed=300), loaded_batch(pkg, cap, counts, seed=300)
    open_batch_window(pkg, f, counts), open_batch_window(pkg, w, counts)
    before = [w.get_state(b) for b in range(5)]
    w.close()
    frames = np.array([[1.0, 2.0, 0.4], [-3.0, 0.5, -2.9], [4.0, -1.0, 0.0], [0.0, 0.0, 1.3], [-2.0, -2.0, 3.1]])
    f.transform_frame(frames)
    mid = [f.get_state(b) for b in range(5)]
    for b in range(5):
        err = assert_state_close(mid[b][0], mid[b][1], *rr.rigid(*before[b], frames[b]), what="batch rigid, filter %d" % b)
        print("batch rigid, filter %d (N=%d): max |dx| %.3e, max |dP| / max |P| %.3e" % (b, counts[b], err[0], err[1]))
        assert_bitwise_symmetric(mid[b][1])
    assert np.array_equal(mid[2][1], before[2][1])  # theta = 0: P bit for bit
    assert np.array_equal(f.poses(), np.stack([m[0][:3] for m in mid]))
    f.transform_frame(FRAME, index=3)
    end = [f.get_state(b) for b in range(5)]
    assert_state_close(end[3][0], end[3][1], *rr.rigid(*mid[3], FRAME), what="rigid on filter 3")
    for b in (0, 1, 2, 4):
        assert_bitwise(end[b], mid[b], "rigid on filter 3: filter %d" % b)
    f.anchor_at_robot(index=3)
    last = [f.get_state(b) for b in range(5)]
    assert_state_close(last[3][0], last[3][1], *rr.anchor(*end[3]), what="anchor on filter 3")
    assert_bitwise_symmetric(last[3][1])
    assert not last[3][0][:3].any() and not last[3][1][:3, :].any()
    for b in (0, 1, 2, 4):
        assert_bitwise(last[b], mid[b], "anchor on filter 3: filter %d" % b)
    f.anchor_at_robot()
    for b in range(5):
        got = f.get_state(b)
        assert_state_close(got[0], got[1], *rr.anchor(*last[b]), what="batch anchor, filter %d" % b)
        assert_bitwise_symmetric(got[1])
    assert list(f.num_landmarks()) == list(counts)
    batch_twin_goes_on(pkg, f, "batch frame changes")
    f.close()


# ---- join ---------------------------------------------------------------------------------------------
# (Ng, Ns, destination capacity, source capacity): the source's tile count differs from the destination's; capacity 300 is the
# several-workgroup kernel family joining into a one-workgroup destination, (256, 33, 320, 40) the other way round
JOINS = [(0, 1, 8, 40), (1, 1, 8, 40), (31, 1, 32, 96), (31, 2, 64, 300), (32, 1, 64, 8), (32, 32, 64, 96), (33, 31, 64, 96),
         (40, 24, 64, 300), (63, 1, 64, 8), (64, 64, 128, 96), (256, 33, 320, 40)]


@pytest.mark.parametrize("Ng,Ns,cap,cap_s", JOINS)
def test_join(pkg, pipeline_mode, Ng, Ns, cap, cap_s):
    assert (cap + 31) // 32 != (cap_s + 31) // 32
    a, xPg, logs = witnessed(pkg, Ng, cap, seed=400 + Ng)
    s, xPs, logs_s = witnessed(pkg, Ns, cap_s, seed=450 + Ns, extent=8.0)
    assert a.join_map(s) == Ng + Ns
    after = a.get_state()
    err = assert_state_close(after[0], after[1], *jr.join(*xPg, *xPs), what="join")
    print("join %d + %d: max |dx| %.3e, max |dP| / max |P| %.3e" % (Ng, Ns, err[0], err[1]))
    settled_checks(a, after, logs, Ng + Ns)
    e = 3 + 2 * Ng
    assert np.array_equal(after[1][3:e, 3:e], xPg[1][3:, 3:]) and np.array_equal(after[0][3:e], xPg[0][3:])
    assert_bitwise(s.get_state(), xPs, "the source after the join")
    assert (s.stats(), s.decisions()) == logs_s
    s.close()
    twin_goes_on(pkg, a, "join %d + %d" % (Ng, Ns))
    a.close()


def test_batch_join_of_different_tile_positions(pkg, pipeline_mode):
    """(Ng, Ns) per filter: a fresh destination, a fresh source behind a full tile, a join that straddles and ends on a tile edge, a
    join that starts on one."""
    ng, ns = (0, 32, 31, 64), (5, 0, 33, 1)
    d, dw = loaded_batch(pkg, 96, ng, seed=500), loaded_batch(pkg, 96, ng, seed=500)
    s, sw = loaded_batch(pkg, 40, ns, seed=520), loaded_batch(pkg, 40, ns, seed=520)
    for f, counts in ((d, ng), (dw, ng), (s, ns), (sw, ns)):
        open_batch_window(pkg, f, counts)
    xPg, xPs = [dw.get_state(b) for b in range(4)], [sw.get_state(b) for b in range(4)]
    dw.close(), sw.close()
    d.batch_join_map(s)
    assert list(d.num_landmarks()) == [5, 32, 64, 65]
    for b in range(4):
        got = d.get_state(b)
        err = assert_state_close(got[0], got[1], *jr.join(*xPg[b], *xPs[b]), what="batch join, filter %d" % b)
        print("batch join, filter %d: max |dx| %.3e, max |dP| / max |P| %.3e" % (b, err[0], err[1]))
        assert_bitwise_symmetric(got[1])
        e = xPg[b][0].size
        assert np.array_equal(got[1][3:e, 3:e], xPg[b][1][3:, 3:]) and np.array_equal(got[0][3:e], xPg[b][0][3:])
        assert_bitwise(s.get_state(b), xPs[b], "the source after the join, filter %d" % b)
    assert np.array_equal(d.poses(), np.stack([d.get_state(b)[0][:3] for b in range(4)]))
    s.close()
    batch_twin_goes_on(pkg, d, "batch join")
    d.close()


# ---- joint consistency --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cap", [(63, 64), (64, 64), (65, 96), (32, 32)])
def test_joint_consistency(pkg, pipeline_mode, N, cap):
    """Beside tests/test_joint_consistency.py's 31 / 32 / 33: two tiles less a landmark, exactly two, two and one, and a map that
    fills its capacity; the record and the factor, with a window open."""
    a, (x, P), _ = witnessed(pkg, N, cap, seed=600 + N)
    xt = fr.draw_truth(x, P, seed=700 + N)
    xt[2] += 2.0 * np.pi
    r = a.joint_consistency(xt, 0)[0]
    ref = fr.lapack(x, P, xt)
    assert ref["info"] == 0
    print("N=%d: worst relative error %.3e" % (N, check_joint(r, ref, P, "N=%d" % N)))
    assert a.joint_consistency(xt, 0).tobytes() == r.tobytes()
    U, Ur = a.joint_factor(0), scipy.linalg.cholesky(P[3:, 3:], lower=False)
    assert U.shape == Ur.shape == (2 * N, 2 * N)
    assert np.all(np.abs(U - Ur) <= REL_TOL * np.abs(Ur) + ABS_P * np.abs(Ur).max())
    assert np.abs(U.T @ U - P[3:, 3:]).max() <= REL_TOL * np.abs(P[3:, 3:]).max()
    assert not np.tril(U, -1).any()
    assert_bitwise(a.get_state(), (x, P), "the call only reads")
    twin_goes_on(pkg, a, "joint consistency N=%d" % N)
    a.close()


# ---- duplicate search, fusion, extraction ------------------------------------------------------------------------
def witnessed_state(pkg, x, P, cap, seed, new_every=0):
    """witnessed() for a state of the caller's: two handles loaded with (x, P), the same two immediate steps on both (two Old-type
    measurements each; new_every: a far New landmark as well), the witness exported and closed."""
    N = (x.size - 3) // 2
    M = min(2, N)
    pair = [pkg.FilterBatch(1, cap, max_pending=WINDOW, log_capacity=4096) for _ in range(2)]
    sc = pkg.scenarios.steady_script(x, steps=2, M=M, seed=seed, min_separation=1.0)
    decs = []
    for f in pair:
        f.set_state(x, P)
        decs.append(run_steps(pkg, f, sc, 0, 2, M, new_every=new_every))
    assert decs[0] == decs[1]
    a, w = pair
    before, logs = w.get_state(), (w.stats(), w.decisions())
    w.close()
    return a, before, logs


def k_pairs(N):
    return [(0, N - 1), (255, 256)]


FUSES = {
    "33, pair (0, 32): the map loses a tile": (33, 64, [(0, 32)]),
    "64, the 32 pairs (k, k + 32): four rounds, a whole tile goes": (64, 64, [(k, k + 32) for k in range(32)]),
    "65, pair (31, 64)": (65, 96, [(31, 64)]),
    "511: columns of 1025": (511, 520, k_pairs(511)),
    "512: columns of 1027": (512, 520, k_pairs(512)),
    "513: columns of 1029": (513, 520, k_pairs(513)),
}


@pytest.mark.parametrize("slack", [0.0, 1e-4])
@pytest.mark.parametrize("case", list(FUSES))
def test_fuse(pkg, pipeline_mode, case, slack):
    N, cap, rows = FUSES[case]
    pairs = fu.as_pairs(rows)
    x0, P0 = pkg.scenarios.injected_state(N, seed=800 + N, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
    a, before, logs = witnessed_state(pkg, *fu.with_noisy_copies(x0, P0, pairs, seed=801 + N), cap, seed=802 + N)
    assert a.window == WINDOW
    closed0 = windows_closed(a)
    got = a.fuse_landmarks(pairs, slack=slack)
    assert windows_closed(a) - closed0 <= 1  # the open window; the rounds' passes are the call's own
    ref = fu.fuse(*before, pairs, slack, WINDOW)
    assert got == (N - len(rows), len(rows)) and ref[2] == len(rows), (got, ref[2])
    after = a.get_state()
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=case)
    print("fuse %s, slack %g: %d rounds, max |dx| %.3e, max |dP| / max |P| %.3e" % (case, slack, -(-len(rows) // WINDOW), err[0], err[1]))
    settled_checks(a, after, logs, N - len(rows))
    twin_goes_on(pkg, a, case)
    a.close()


def planted_at_the_end(pkg, N, seed):
    """N landmarks, the last one a planted duplicate (d2 = 3) of a landmark of an earlier tile where there is one: the pair lies
    across the last tile edge.  dup_ref.with_duplicates without the renumbering; the seed moves on until the copied landmark is one
    of an earlier tile (a property of the builder's draw alone)."""
    while True:
        x, P = pkg.scenarios.injected_state(N - 1, seed=seed, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
        x, P, planted = dr.with_duplicates(x, P, targets=(3.0,), seed=seed + 1, permute=False)
        (i, j, _), = planted
        assert j == N - 1
        if i // 32 < j // 32 or j < 33:
            return x, P, (i, j)
        seed += 2


@pytest.mark.parametrize("N,cap", [(0, 8), (1, 8), (2, 8), (63, 64), (64, 64), (65, 96)])
def test_find_duplicates(pkg, pipeline_mode, N, cap):
    """(64, 64) is the map that fills its capacity."""
    if N >= 2:
        x, P, pair = planted_at_the_end(pkg, N, seed=900 + N)
        a, before, logs = witnessed_state(pkg, x, P, cap, seed=950 + N)
    else:
        a, before, logs = witnessed(pkg, N, cap, seed=900 + N)
        pair = None
    got = a.find_duplicates()
    worst = check_duplicates(got, *before, what="N=%d" % N)
    assert len(got[0]) == got[1] and (pair is None and got[1] == 0 or pair in ij(got[0])), (pair, ij(got[0]))
    again = a.find_duplicates()
    assert again[0].tobytes() == got[0].tobytes() and again[1:] == got[1:]
    for split, max_dist in ((max(N - 1, 0), None), (0, 1.0), (N, 0.05)):  # old x last, a Euclidean bound, a split that considers nothing
        r = a.find_duplicates(split=split, max_dist=max_dist)
        worst = max(worst, check_duplicates(r, *before, split=split, max_dist=max_dist, what="N=%d split=%d max_dist=%s" % (N, split, max_dist)))
        if pair is not None and split == N - 1:
            assert pair in ij(r[0])
    if pair is not None:  # a gate that ignores P_ij answers something else: another list, or another distance for the planted pair
        blind, _ = dr.find(before[0], dr.without_cross_blocks(before[1]))
        d2 = dict(zip(ij(got[0]), got[0]["d2"].tolist()))[pair]
        assert ij(blind) != ij(got[0]) or abs(dict(zip(ij(blind), blind["d2"].tolist()))[pair] / d2 - 1.0) > 0.1
    print("find N=%d: %d pairs, worst error of d2 %.3e (relative, floor 1e-9)" % (N, got[1], worst))
    after = a.get_state()
    assert_bitwise(after, before, "the call only reads")
    settled_checks(a, after, logs, N)
    twin_goes_on(pkg, a, "find N=%d" % N)
    a.close()


def id_lists(N):
    return {"None": None, "[]": np.zeros(0, dtype=np.int32), "the last only": np.array([N - 1] if N else [], dtype=np.int32),
            "all reversed": np.arange(N, dtype=np.int32)[::-1].copy()}


def extraction_checks(pkg, s, held, logs_s, d, logs_d, ids, what):
    """d.extract_map(s, ids) and s.get_submap(ids) against NumPy indexing of what the source's witness exported; the source only read."""
    want = index_state(held, ids)
    n = (want[0].size - 3) // 2
    assert d.extract_map(s, ids) == n, what
    got = d.get_state()
    assert_bitwise(got, want, "%s: ekf_extract_map" % what)
    assert_bitwise(s.get_submap(np.arange((held[0].size - 3) // 2, dtype=np.int32) if ids is None else ids), want, "%s: ekf_get_submap" % what)
    settled_checks(d, got, logs_d, n)
    after_s = s.get_state()
    assert_bitwise(after_s, held, "%s: the source" % what)
    settled_checks(s, after_s, logs_s, (held[0].size - 3) // 2)


@pytest.mark.parametrize("which", ["None", "[]", "the last only", "all reversed"])
@pytest.mark.parametrize("N,cap,cap_d", [(0, 8, 40), (1, 8, 40), (31, 32, 64), (32, 32, 96), (33, 64, 96), (65, 96, 200)])
def test_extract(pkg, pipeline_mode, N, cap, cap_d, which):
    """A source with its window open into a fresh destination of another tile count."""
    assert mm.lm_tiles(cap) != mm.lm_tiles(cap_d)
    ids = id_lists(N)[which]
    s, held, logs_s = witnessed(pkg, N, cap, seed=1000 + N)
    d = pkg.FilterBatch(1, cap_d, max_pending=WINDOW, log_capacity=4096)
    extraction_checks(pkg, s, held, logs_s, d, (d.stats(), d.decisions()), ids, "N=%d ids %s" % (N, which))
    s.close()
    twin_goes_on(pkg, d, "extract N=%d ids %s" % (N, which))
    d.close()


@pytest.mark.parametrize("Ns,ids", [(33, [32]), (1, [0]), (65, [64]), (33, None)])
def test_extract_into_a_destination_that_held_65(pkg, pipeline_mode, Ns, ids):
    """Three tile rows, a window open on them, replaced by one landmark (or by 33): the tiles of the larger map are zeroed."""
    d, _, logs_d = witnessed(pkg, 65, 96, seed=1100)
    s, held, logs_s = witnessed(pkg, Ns, 64 if Ns <= 33 else 128, seed=1101 + Ns)
    extraction_checks(pkg, s, held, logs_s, d, logs_d, None if ids is None else np.array(ids, dtype=np.int32), "65 <- %s of %d" % (ids, Ns))
    s.close()
    twin_goes_on(pkg, d, "65 <- %s of %d" % (ids, Ns))
    d.close()


@pytest.mark.parametrize("Ns,count", [(512, 511), (512, 512), (513, 513)])
def test_extract_across_the_chunk(pkg, pipeline_mode, Ns, count):
    """Selections of 511 / 512 / 513 landmarks: 3 + 2 count = 1025 / 1027 / 1029 (a source of 512 has no 513 to give: that one is
    taken from 513), shuffled, into a destination of another tile count."""
    s, held, logs_s = witnessed(pkg, Ns, 520, seed=1200 + Ns)
    ids = np.random.default_rng(1201 + count).permutation(Ns).astype(np.int32)[:count]
    d = pkg.FilterBatch(1, 600, max_pending=WINDOW, log_capacity=4096)
    extraction_checks(pkg, s, held, logs_s, d, (d.stats(), d.decisions()), ids, "%d of %d" % (count, Ns))
    s.close()
    twin_goes_on(pkg, d, "%d of %d" % (count, Ns))
    d.close()


# ---- behind a window in which the map grew into a new tile ---------------------------------------------------------
def grown(pkg):
    """A handle of 32 landmarks (capacity 64) whose open window holds a far New landmark: 33 landmarks, the 33rd in a tile row that the
    settled layout does not have yet.  Nothing is read from the handle; its witness says what it holds."""
    x, P = pkg.scenarios.injected_state(32, seed=1300, extent=12.0 * 0.5 ** 0.5 + 8.0)
    a, before, logs = witnessed_state(pkg, x, P, 64, seed=1301, new_every=2)
    assert before[0].size == 3 + 2 * 33 and logs[0][0]["n_new"] == 1
    assert windows_closed(a) == 0  # (a host counter: five slots of eight, the New landmark among them, still deferred)
    return a, before, logs


def test_find_duplicates_behind_a_grown_window(pkg, pipeline_mode):
    a, before, logs = grown(pkg)
    got = a.find_duplicates(gate=1e12)  # every pair passes: the 32 pairs of the new landmark are in the list
    check_duplicates(got, *before, gate=1e12, what="grown window")
    assert got[1] == 33 * 32 // 2 and ij(got[0])[-1] == (31, 32)
    check_duplicates(a.find_duplicates(split=32), *before, split=32, what="grown window, old x new")
    after = a.get_state()
    assert_bitwise(after, before, "the call only reads")
    settled_checks(a, after, logs, 33)
    twin_goes_on(pkg, a, "find behind a grown window")
    a.close()


def test_fuse_behind_a_grown_window(pkg, pipeline_mode):
    a, before, logs = grown(pkg)
    pairs = fu.as_pairs([(31, 32), (0, 5)])
    got = a.fuse_landmarks(pairs, slack=1e-4)
    ref = fu.fuse(*before, pairs, 1e-4, WINDOW)
    assert got == (31, 2) and ref[2] == 2
    after = a.get_state()
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what="grown window")
    print("fuse behind a grown window: max |dx| %.3e, max |dP| / max |P| %.3e" % err)
    settled_checks(a, after, logs, 31)
    twin_goes_on(pkg, a, "fuse behind a grown window")
    a.close()


def test_extract_behind_a_grown_window(pkg, pipeline_mode):
    a, before, logs = grown(pkg)
    ids = np.arange(33, dtype=np.int32)[::-1].copy()
    d = pkg.FilterBatch(1, 96, max_pending=WINDOW, log_capacity=4096)
    logs_d = (d.stats(), d.decisions())
    assert d.extract_map(a, ids) == 33  # the first call on the handle: it closes the window itself
    got = d.get_state()
    assert_bitwise(got, index_state(before, ids), "ekf_extract_map behind a grown window")
    settled_checks(d, got, logs_d, 33)
    d.close()
    a.close()
    a, before, logs = grown(pkg)
    assert_bitwise(a.get_submap(ids), index_state(before, ids), "ekf_get_submap behind a grown window")
    after = a.get_state()
    assert_bitwise(after, before, "the call only reads")
    settled_checks(a, after, logs, 33)
    twin_goes_on(pkg, a, "get_submap behind a grown window")
    a.close()


# ---- matched updates -----------------------------------------------------------------------------------------------------
def matched_checks(pkg, a, before, logs, z, R, ids, what, window=WINDOW):
    """a.update_matched(z, R, ids) on the handle whose witness exported `before`: the reference in rounds of the handle's window,
    the checks every rewrite of this file gets, the twin.  Returns the device's d2."""
    N = (before[0].size - 3) // 2
    assert a.window == window
    closed0 = windows_closed(a)
    got = a.update_matched(z, R, ids)
    assert windows_closed(a) - closed0 <= 1  # the open window; the rounds' passes are the call's own
    ref = mr.update(*before, z, R, ids, window)
    n_z = sum(1 for i in ids if i >= 0)
    assert got[:2] == (N, n_z) and ref[2] == n_z, (what, got[:2], ref[2])
    after = a.get_state()
    err = assert_state_close(after[0], after[1], ref[0], ref[1], what=what)
    rel = mr.assert_d2_close(got[2], ref[3], what, mr.D2_REL_EDGES)
    print("matched %s: %d rounds, max |dx| %.3e, max |dP| / max |P| %.3e, d2 relative %.3e" % (what, -(-n_z // window), err[0], err[1], rel))
    settled_checks(a, after, logs, N)
    twin_goes_on(pkg, a, what, window)
    return got[2]


@pytest.mark.parametrize("case", [k for k in mr.MAP_EDGES if k not in mr.FULL_ROUND_CASES])
def test_update_matched(pkg, pipeline_mode, case):
    N, cap, window, _, seed = mr.MAP_EDGES[case]
    a, before, logs = witnessed(pkg, N, cap, seed=seed)
    ids = mr.map_edge_ids(case, before[0])
    z, R = mr.scan_of(pkg, before[0], ids, seed + mr.SCAN_OFFSET)
    matched_checks(pkg, a, before, logs, z, R, ids, case)
    a.close()


@pytest.mark.parametrize("case", mr.FULL_ROUND_CASES)
def test_update_matched_full_round(pkg, pipeline_mode, case):
    """A round of as many measurements as the window holds (32: EKF_MAX_PENDING, M = 64 = FUSE_MAX_COLS columns) and a round of one
    behind it, on the chain kernel's geometry (capacity 320) and on the one-workgroup family's (capacity 200).  Then, on a handle
    loaded with the same state, the prefixes of 8 / 16 / 24 / 32 measurements that fit one round: ekf_joint_compat and
    ekf_update_matched give the same bits."""
    N, cap, window, count, seed = mr.MAP_EDGES[case]
    assert all(mm.planned_window(1, cap, window, ov) == window for ov in (False, True))  # the window asked for, in either pipeline mode
    a, before, logs = witnessed(pkg, N, cap, seed=seed, window=window)
    # capacity 200 is run by the one-workgroup kernel where the dense pass is in place, by the chain kernel in overlap mode; 320 never is
    assert a.overlap == (pipeline_mode == "overlap")
    assert mm.planned_geometry(1, cap, window, a.overlap)[:2] == ((1, True) if cap <= 256 and not a.overlap else (5 if cap > 256 else 4, False))
    ids = mr.map_edge_ids(case, before[0])
    assert len(ids) == count == window + 1 and len(set(ids.tolist())) == 24
    z, R = mr.scan_of(pkg, before[0], ids, seed + mr.SCAN_OFFSET)
    d2 = matched_checks(pkg, a, before, logs, z, R, ids, case, window)
    a.close()
    assert np.all(np.diff(d2[:window]) >= 0.0)  # a running distance within the round
    for p in (8, 16, 24, 32):
        if p > window:
            continue
        h = pkg.FilterBatch(1, cap, max_pending=window, log_capacity=4096)
        h.set_state(*before)
        score = h.joint_compat(z[:p], R[:p], ids[:p])
        mr.assert_d2_close(score, mr.joint_compat(*before, z[:p], R[:p], ids[:p]), "%s, score of %d" % (case, p), mr.D2_REL_EDGES)
        n, applied, dp = h.update_matched(z[:p], R[:p], ids[:p])
        assert (n, applied) == (N, p) and dp.tobytes() == score.tobytes(), (case, p)
        assert d2[:p].tobytes() == dp.tobytes(), (case, p)  # ... and the bits the call behind the open window gave for its first round
        h.close()


@pytest.mark.parametrize("case", mr.CHUNK_CASES)
def test_joint_compat_across_the_chunk(pkg, pipeline_mode, case):
    """The score alone on 511 / 512 / 513 landmarks: 32 pairings (M = 64, NC = 68), the last landmark among them."""
    N, cap, _, _, seed = mr.MAP_EDGES[case]
    a, before, logs = witnessed(pkg, N, cap, seed=seed)
    ids = mr.chunk_hypothesis(N)
    assert len(ids) == 32 and N - 1 in ids
    z, R = mr.scan_of(pkg, before[0], ids, seed + mr.SCAN_OFFSET + 1)
    d2 = a.joint_compat(z, R, ids)
    rel = mr.assert_d2_close(d2, mr.joint_compat(*before, z, R, ids), case, mr.D2_REL_EDGES)
    print("joint_compat %s: d2 relative %.3e" % (case, rel))
    assert not np.isnan(d2).any() and np.all(np.diff(d2) >= 0.0)
    assert a.joint_compat(z, R, ids).tobytes() == d2.tobytes()  # two calls, the same bits
    after = a.get_state()
    assert_bitwise(after, before, "the call only reads")
    settled_checks(a, after, logs, N)
    twin_goes_on(pkg, a, case)
    a.close()


def test_update_matched_behind_a_grown_window(pkg, pipeline_mode):
    """Landmark 32 measured straight behind the window in which it was created (a second tile just started), and an old one."""
    a, before, logs = grown(pkg)
    z, R = mr.scan_of(pkg, before[0], mr.GROWN_IDS, mr.GROWN_SCAN_SEED)
    matched_checks(pkg, a, before, logs, z, R, mr.GROWN_IDS, mr.GROWN_NAME)
    a.close()
