"""update_polar among the other list and map calls: one seeded random sequence of 12 operations per size -- update_polar, update_matched,
update_fixes, remove_landmarks, add_landmarks -- on one handle, every step checked against the NumPy references (polar_ref,
match_ref, fix_ref, the oracle's New, NumPy indexing for the removal) on that step's own export, as tests/test_map_sequences.py does
for the map operations.  The first and the last operation are update_polar, and no operation is missing from a sequence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fix_ref as fx  # noqa: E402
import match_ref as mr  # noqa: E402
import polar_ref as pr  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close, far_feature  # noqa: E402

pytestmark = pytest.mark.gpu

OPS = ("polar", "matched", "fixes", "remove", "add")
STEPS = 12


def d2_bound(module_bound, ref, ext):
    """The relative agreement asked of a step's d2: the reference module's bound, which is 20 times the difference between the double
    reference and its extended-precision restatement on that module's own inputs -- or 20 times that difference on THIS step's
    input where it is larger (the states here are a dozen updates, removals and far additions away from those inputs)."""
    ok = ~np.isnan(ref[3])
    assert np.array_equal(np.isnan(ext[3]), ~ok)
    own = float((np.abs(ref[3][ok] - ext[3][ok]) / np.abs(ext[3][ok])).max()) if ok.any() else 0.0
    return max(module_bound, 20.0 * own)


def plan(seed):
    """12 operations: update_polar first and last, each of the others at least once, the rest drawn."""
    rng = np.random.default_rng(seed)
    middle = list(OPS[1:]) + ["polar", "polar"] + list(rng.choice(OPS, size=STEPS - 2 - 6))
    return ["polar"] + [middle[i] for i in rng.permutation(len(middle))] + ["polar"]


@pytest.mark.parametrize("N,cap", pr.SIZES)
def test_a_random_sequence(pkg, pipeline_mode, oc, N, cap):
    x, P = pkg.scenarios.injected_state(N, seed=pr.STATE_SEED[N], extent=mr.map_extent(N))
    a = pkg.FilterBatch(1, cap, max_pending=16, log_capacity=4096)
    a.set_state(x, P)
    rng = np.random.default_rng(7000 + N)
    ops = plan(7100 + N)
    assert len(ops) == STEPS and set(ops) == set(OPS) and ops[0] == ops[-1] == "polar"
    added = 0
    for step, op in enumerate(ops):
        pre = a.get_state()
        n = (pre[0].size - 3) // 2
        name = "N=%d, step %d: %s" % (N, step, op)
        if op == "polar":
            count = int(rng.integers(3, 21))   # up to two rounds of the window of 16
            ids = rng.choice(pr.nearest(pre[0], 24), size=count).astype(np.int32)
            ids[1:][rng.random(count - 1) < 0.15] = -1
            kind = rng.integers(1, 4, size=count).astype(np.int32)
            z, R = pr.entries_for(pre[0], ids, kind, 7200 + 20 * N + step)
            got = a.update_polar(z, R, ids, kind)
            ref = pr.update(pre[0], pre[1], z, R, ids, kind, a.window)
            bound = d2_bound(pr.D2_REL, ref, pr.update_extended(pre[0], pre[1], z, R, ids, kind, a.window))
        elif op == "matched":
            ids = rng.choice(pr.nearest(pre[0], 24), size=int(rng.integers(2, 9))).astype(np.int32)
            z, R = mr.scan_of(pkg, pre[0], ids, 7300 + 20 * N + step)
            got = a.update_matched(z, R, ids)
            ref = mr.update(pre[0], pre[1], z, R, ids, a.window)
            bound = d2_bound(mr.D2_REL, ref, mr.update_extended(pre[0], pre[1], z, R, ids, a.window))
        elif op == "fixes":
            what = np.array([fx.POSITION, fx.HEADING] + list(rng.choice(n, size=3)), dtype=np.int32)[rng.permutation(5)]
            z, R = fx.entries_for(pre[0], pre[1], what, 7400 + 20 * N + step)
            got = a.update_fixes(z, R, what)
            ref = fx.update(pre[0], pre[1], z, R, what, a.window)
            bound = d2_bound(fx.D2_REL, ref, fx.update_extended(pre[0], pre[1], z, R, what, a.window))
        elif op == "remove":
            gone = sorted(int(i) for i in rng.choice(n, size=3, replace=False))
            keep = np.ones(n, dtype=bool)
            keep[gone] = False
            assert a.remove_landmarks(keep, 0) == n - 3
            assert_bitwise(a.get_state(), fx.remove(pre[0], pre[1], gone), name)
            continue
        else:
            zf, Rf = far_feature(pkg, added)
            added += 1
            cnt, new_ids = a.add_landmarks(zf.reshape(1, 2), Rf.reshape(1, 2, 2))
            assert cnt == n + 1 and list(new_ids) == [n]
            xo, Po, dec, _, _ = oc.update(pre[0], pre[1], zf.reshape(2, 1), Rf)
            assert dec == [oc.NEW]
            s = a.get_state()
            assert_state_close(s[0], s[1], xo, Po, what=name)
            continue
        s = a.get_state()
        assert got[:2] == (n, ref[2]) and ref[2] == int((np.asarray(ids if op != "fixes" else what) != -1).sum()), (name, got[:2], ref[2])
        err = assert_state_close(s[0], s[1], ref[0], ref[1], what=name)
        print("%s: %d applied, max |dx| %.3e, max |dP| / max |P| %.3e" % (name, got[1], err[0], err[1]))
        mr.assert_d2_close(got[2], ref[3], name, bound)
        assert_bitwise_symmetric(s[1])
        assert np.array_equal(a.poses()[0], s[0][:3]) and np.array_equal(a.robot_cov(), s[1][:3, :3])
    assert a.num_landmarks()[0] == (a.get_state()[0].size - 3) // 2
    a.close()
