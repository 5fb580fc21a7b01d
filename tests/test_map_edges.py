"""The map rewrites at the edges of the tile layout.  P_LL is stored as 64 x 64 tiles of 32 landmarks, the dense vectors are walked
in chunks of 1024 elements, capacity 256 splits the two kernel families; the other GPU tests of removal, frame change, joining and
joint consistency sit in the middle of all that.  Here: maps of 0, 1, 31, 32, 33, 63, 64, 65 landmarks, maps that end on a tile or
on the capacity, removals that lose a tile or move every row across a tile edge, joins that start on a tile edge (no straddling
old x new tile) or fit into the straddling tile altogether, filters of one batch with different tile counts.

Every case: a window is left open by a few immediate steps, a witness handle that ran the same steps exports what the handle under
test held; parity against the NumPy reference (tests/reframe_ref.py, tests/join_ref.py, tests/factor_ref.py; helpers' tolerances) or
bit for bit where the contract says so (np.delete, theta = 0, the old x old block); bitwise symmetry; and a set_state twin that goes
on for three steps with a far New landmark, bit for bit -- the check that sees the zeros behind the map (not the places of a
diagonal tile that are nobody's home, a landmark's own block and the blocks below the diagonal: nothing reads those).  A map that fills its capacity is given room by ekf_reserve first (which must not change a bit)."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ref as fr  # noqa: E402
import join_ref as jr  # noqa: E402
import map_model as mm  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import (ABS_P, REL_TOL, assert_bitwise, assert_bitwise_symmetric, assert_state_close, batch_script, check_joint,  # noqa: E402
                     open_window_pair, run_steps)

pytestmark = pytest.mark.gpu

FRAME = (3.0, -2.0, 0.7)
WINDOW = 8


def opened_pair(pkg, N, cap, seed, extent=None):
    """The handle under test and its witness after the same immediate steps, a window open on both.  N = 0: fresh filters that
    have been propagated twice."""
    if N:
        a, w, _ = open_window_pair(pkg, N, cap, seed=seed, steps=2, extent=extent, M=min(2, N), max_pending=WINDOW)
        return a, w
    pair = [pkg.FilterBatch(1, cap, max_pending=WINDOW, log_capacity=4096) for _ in range(2)]
    for f in pair:
        f.propagate(0.3, 0.05, 0.05)
        f.propagate(0.2, -0.1, 0.1)
    return pair


def witnessed(pkg, N, cap, seed, extent=None):
    """(handle with its window open and its streaming launch live, what it holds as its witness exported it, the witness' stats and
    decision log).  Nothing is asked of the handle itself: reading its counters would have the resident launch leave."""
    a, w = opened_pair(pkg, N, cap, seed, extent)
    before, logs = w.get_state(), (w.stats(), w.decisions())
    w.close()
    return a, before, logs


def settled_checks(a, after, logs, N):
    assert_bitwise_symmetric(after[1])
    assert int(a.num_landmarks()[0]) == N == (after[0].size - 3) // 2
    assert np.array_equal(a.poses()[0], after[0][:3]) and np.array_equal(a.robot_cov(), after[1][:3, :3])
    assert (a.stats(), a.decisions()) == logs  # counters and decision log do not move


def twin_goes_on(pkg, a, what):
    """Three more steps on the handle and on a twin loaded with set_state of its export: propagations, Old matches where there are
    landmarks, far New landmarks (steps 0 and 2).  Decisions with their distances and the final exports are equal bit for bit."""
    st = a.get_state()
    N = (st[0].size - 3) // 2
    if N + 2 > a.capacity:
        a.reserve(N + 8)
        assert_bitwise(a.get_state(), st, "%s: reserve behind the call" % what)
    b = pkg.FilterBatch(1, a.capacity, max_pending=WINDOW, log_capacity=4096)
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
