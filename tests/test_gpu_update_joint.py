"""The scan step on the device: ekf_update_joint / ekf_batch_update_joint are ekf_associate_joint, ekf_update_matched and
ekf_add_landmarks of one scan as one call.  The contract is bit for bit: state and every output equal those of the three public
calls made in sequence with the same arguments.  The kinds and the ids are held to the NumPy composition of the three references
(add_ref.update_joint_ref; its scenarios and their margins are checked on the CPU in tests/test_add_landmarks_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import add_ref as ad  # noqa: E402
from helpers import assert_bitwise, assert_bitwise_symmetric, assert_state_close  # noqa: E402

pytestmark = pytest.mark.gpu

N0, CAP = 60, 96


def loaded(pkg, x, P, cap=CAP, batch=1, index=0, f=None):
    f = f or pkg.FilterBatch(batch, cap, max_pending=16, log_capacity=4096)
    f.set_state(x, P, index=index)
    return f


def three_calls(pkg, f, z, R, index=0):
    """associate_joint -> update_matched -> add_landmarks on filter `index`; (n, ids, kinds, d2, info) as update_joint returns them."""
    E = pkg.ekfslam
    ids, _, info, near, _ = f.associate_joint(z, R, index=index)
    kinds = np.where(ids >= 0, E.OLD, np.where(near["decision"] == E.NEW, E.NEW, E.IGNORE)).astype(np.int32)
    _, applied, d2 = f.update_matched(z, R, ids, index=index)
    ids = ids.copy()
    for q in np.flatnonzero(ids >= 0)[applied:]:
        ids[q], kinds[q] = -1, E.IGNORE
    n, new = f.add_landmarks(z, R, add=(kinds == E.NEW), index=index)
    ids[kinds == E.NEW] = new[kinds == E.NEW]
    return n, ids, kinds, d2, info


def same_outputs(a, b, what):
    assert a[0] == b[0], what
    assert a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist(), (what, a[1], b[1], a[2], b[2])
    assert np.array_equal(a[3], b[3], equal_nan=True), (what, a[3], b[3])
    assert a[4].tobytes() == b[4].tobytes(), (what, a[4], b[4])


def test_one_call_equals_the_three_calls_bit_for_bit(pkg, pipeline_mode):
    x, P, z, R, kinds, _ = ad.scan_with_kinds(pkg, N0)
    a, b = loaded(pkg, x, P), loaded(pkg, x, P)
    st, dec = a.stats(), a.decisions()
    got, seq = a.update_joint(z, R), three_calls(pkg, b, z, R)
    same_outputs(got, seq, "update_joint vs the three calls")
    sa = a.get_state()
    assert_bitwise(sa, b.get_state(), "update_joint vs the three calls")
    assert_bitwise_symmetric(sa[1])
    ref = ad.update_joint_ref(x, P, z, R, pkg.ekfslam.joint_gates(0.99), window=a.window)
    assert got[2].tolist() == kinds.tolist() == ref.kinds.tolist()
    assert got[1].tolist() == ref.ids.tolist() and got[0] == N0 + 2
    err = assert_state_close(sa[0], sa[1], ref.x, ref.P, what="update_joint vs its reference")
    print("update_joint, %d measurements: max |dx| %.3e, max |dP| / max |P| %.3e" % (len(z), err[0], err[1]))
    assert a.stats() == st and a.decisions() == dec  # counters and decision log stay as they are
    a.close(), b.close()


def test_batch_form_equals_one_filter_calls(pkg, pipeline_mode):
    x, P, z, R, _, _ = ad.scan_with_kinds(pkg, N0)
    n_z = len(z)
    valid = np.ones((3, n_z), dtype=np.uint8)
    valid[0, [1, n_z - 1]] = 0   # a pairing and a far feature masked
    valid[2, :] = 0
    valid[2, [0, n_z - 3, n_z - 2]] = 1
    f, w = pkg.FilterBatch(3, CAP, max_pending=16, log_capacity=4096), pkg.FilterBatch(3, CAP, max_pending=16, log_capacity=4096)
    for h in (f, w):
        loaded(pkg, x, P, index=0, f=h), loaded(pkg, x, P, index=2, f=h)   # filter 1 stays fresh: everything New
    zb, Rb = np.tile(z, (3, 1, 1)), np.tile(R, (3, 1, 1, 1))
    zb[0, 1] = np.nan  # a masked entry is not looked at
    n, ids, kinds, d2, info = f.update_joint(zb, Rb, index=None, valid=valid)
    for b in range(3):
        keep = valid[b] != 0
        one = w.update_joint(z[keep], R[keep], index=b)
        assert one[0] == n[b], b
        assert ids[b][keep].tolist() == one[1].tolist() and kinds[b][keep].tolist() == one[2].tolist(), (b, ids[b], one[1])
        assert np.array_equal(d2[b][keep], one[3], equal_nan=True)
        assert (ids[b][~keep] == -1).all() and (kinds[b][~keep] == 0).all() and np.isnan(d2[b][~keep]).all()
        assert info[b].tobytes() == one[4].tobytes()
        assert_bitwise(f.get_state(b), w.get_state(b), "filter %d" % b)
    assert n.tolist() == [N0 + 1, n_z, N0 + 1] and kinds[1].tolist() == [pkg.ekfslam.NEW] * n_z
    f.close(), w.close()


def test_capacity_short_by_one_applies_nothing(pkg, pipeline_mode):
    x, P, z, R, _, _ = ad.scan_with_kinds(pkg, N0)
    a = loaded(pkg, x, P, cap=N0 + 1)
    held = a.get_state()
    with pytest.raises(pkg.ekfslam.EkfError) as e:
        a.update_joint(z, R)
    assert e.value.code == pkg.ekfslam.ERR_CAPACITY
    assert_bitwise(a.get_state(), held, "after EKF_ERR_CAPACITY")
    a.sync()  # nothing sticky
    a.reserve(N0 + 2)
    assert a.update_joint(z, R)[0] == N0 + 2
    a.close()


def test_twenty_step_loop_builds_the_map_with_update_joint_alone(pkg, pipeline_mode):
    """The reference is re-seeded from the device's exported state at every step, so that one flipped decision could not cascade;
    the scenario's margins are asserted on the CPU for the same seed."""
    world, script = ad.loop_script(pkg)
    jg = pkg.ekfslam.joint_gates(0.99)
    f = pkg.FilterBatch(1, 64, max_pending=16, log_capacity=4096)
    worst = (0.0, 0.0)
    for s, (v, w, dt, z, R) in enumerate(script):
        f.propagate(v, w, dt)
        x, P = f.get_state()
        ref = ad.update_joint_ref(x, P, z, R, jg, window=f.window)
        n, ids, kinds, d2, info = f.update_joint(z, R)
        assert ids.tolist() == ref.ids.tolist() and kinds.tolist() == ref.kinds.tolist(), (s, ids, ref.ids, kinds, ref.kinds)
        assert n == (ref.x.size - 3) // 2 and int(info["complete"]) == 1
        xa, Pa = f.get_state()
        err = assert_state_close(xa, Pa, ref.x, ref.P, what="step %d" % s)
        worst = (max(worst[0], err[0]), max(worst[1], err[1]))
    print("20 steps: max |dx| %.3e, max |dP| / max |P| %.3e" % worst)
    assert n == len(world) == 40
    L = xa[3:].reshape(-1, 2)
    nearest = [int(np.argmin(np.hypot(*(world - l).T))) for l in L]
    assert sorted(nearest) == list(range(40))  # every landmark of the world exactly once: no duplicates
    assert_bitwise_symmetric(Pa)
    f.close()
