"""CPU tests of ekf_add_landmarks / ekf_update_joint: the header declares the calls and the binding lists them; the host-side
planning (tests/cpp/add_plan_check.cpp) refuses what the header says, lays the table out and walks exactly the tiles that hold a
new column; and the NumPy references the GPU tests compare with (tests/add_ref.py) are themselves checked -- the add against the
join of a block-diagonal source, against the oracle's sequential New and against central differences of the map; the scan step on
a small scenario with every kind in it; the 20-step loop's margins."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import add_ref as ad  # noqa: E402
import gate_ref as gr  # noqa: E402
import join_ref as jr  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import assert_bitwise_symmetric, assert_state_close, run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state(pkg, N=23, seed=7):
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=10.0)
    x[0:3] = (1.5, -0.7, 0.3)
    return x, P


def _far_scan(pkg, count):
    """`count` features far from the injected maps and 9 m or more from each other, with R of slam.cpp made slightly unsymmetric."""
    z, R = np.empty((count, 2)), np.empty((count, 2, 2))
    for k in range(count):
        zz, RR = pkg.scenarios.measurement_from_feature_mm(70000.0 + 9000.0 * (k % 7), -40000.0 + 11000.0 * (k // 7))
        z[k], R[k] = zz.reshape(2), RR.reshape(2, 2)
    return z, R


def test_header_declares_and_binding_lists_the_calls(pkg):
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ekf_add_landmarks", "ekf_batch_add_landmarks", "ekf_update_joint", "ekf_batch_update_joint"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        for meth in ("add_landmarks", "update_joint"):
            assert callable(getattr(cls, meth)), meth


def test_plan_refusals_table_and_tiles(tmp_path):
    out = run_cpp_check(tmp_path, "add_plan_check")
    assert out.returncode == 0 and "add plan ok" in out.stdout, out.stdout + out.stderr


def test_add_equals_the_join_of_a_block_diagonal_source(pkg):
    for N, m in ((23, 5), (0, 3), (40, 1), (33, 40)):
        x, P = _state(pkg, N) if N else (np.array([0.4, -0.2, 0.9]), np.zeros((3, 3)))
        z, R = _far_scan(pkg, m + 2)
        R[0, 0, 1] += 1e-7  # only the symmetric part may enter
        mask = np.ones(m + 2, dtype=bool)
        mask[[1, m + 1]] = False
        xa, Pa = ad.add(x, P, z, R, mask)
        xj, Pj = jr.join(x, P, *ad.as_join_source(z, R, mask))
        err = assert_state_close(xa, Pa, xj, Pj, what="N=%d m=%d" % (N, m))
        print("N=%d m=%d: add vs join, max |dx| %.3e, max |dP| / max |P| %.3e" % (N, m, err[0], err[1]))
        assert list(ad.new_ids(N, mask, m + 2)[mask]) == list(range(N, N + m))


def test_add_equals_the_oracles_sequential_new(pkg, npo):
    x, P = _state(pkg, 23)
    z, R = _far_scan(pkg, 6)
    zc, Rc = mr.as_oracle_chunk(z, R)
    xo, Po, dec, mat, _ = npo.update(x, P, zc, Rc)
    assert list(dec) == [gr.NEW] * 6, dec  # every one of them, no case left out
    xa, Pa = ad.add(x, P, z, R)
    err = assert_state_close(xa, Pa, xo, Po, what="sequential New")
    print("add vs sequential New: max |dx| %.3e, max |dP| / max |P| %.3e" % err)


def test_grid_scan_is_new_for_the_oracle_on_the_gpu_tests_maps(pkg, npo):
    """The scans of tests/test_gpu_landmark_add.py on its maps: the oracle decides New for each, one after the other."""
    for N, seed in ((200, 11), (100, 11), (200, 41), (100, 41), (200, 61), (100, 61)):
        x, P = pkg.scenarios.injected_state(N, seed=seed, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
        z, R = ad.grid_scan(pkg, 40)
        _, _, dec, _, mahal = npo.update(x, P, *mr.as_oracle_chunk(z, R))
        assert list(dec) == [gr.NEW] * 40 and min(mahal) > 1.5 * gr.GAMMA_MAX, (N, seed, min(mahal))


def test_new_rows_equal_the_central_difference_jacobian(pkg):
    x, P = _state(pkg, 9)
    z, R = _far_scan(pkg, 3)
    n = x.size
    num = jr.central_difference(lambda v: ad.add_g(v[:n], v[n:].reshape(-1, 2)), np.concatenate([x, z.reshape(-1)]), h=1e-5)
    big = np.zeros((n + 6, n + 6))
    big[:n, :n] = P
    for k in range(3):
        big[n + 2 * k:n + 2 * k + 2, n + 2 * k:n + 2 * k + 2] = R[k]
    want = num @ big @ num.T
    _, Pa = ad.add(x, P, z, R)
    scale = np.abs(want).max()
    err = np.abs(Pa[n:, :n] - want[n:, :n]).max() / scale  # new x robot and new x old
    print("new rows vs J P J^T by central differences: relative %.3e" % err)
    assert err < 1e-8  # (h^2 of the difference quotient on entries of order 1e2 in J)


def test_old_rows_are_bitwise_unchanged_and_P_is_bitwise_symmetric(pkg):
    x, P = _state(pkg, 33)
    z, R = _far_scan(pkg, 40)
    xa, Pa = ad.add(x, P, z, R)
    n = x.size
    assert np.array_equal(xa[:n], x) and np.array_equal(Pa[:n, :n], P)
    assert_bitwise_symmetric(Pa)
    assert np.linalg.eigvalsh(Pa).min() >= -1e-12 * np.abs(Pa).max()


def test_update_joint_ref_gives_every_kind_on_the_small_scenario(pkg):
    x, P, z, R, kinds, pair = ad.scan_with_kinds(pkg)
    N = (x.size - 3) // 2
    j = ad.update_joint_ref(x, P, z, R, pkg.ekfslam.joint_gates(0.99), window=16)
    print("kinds", j.kinds.tolist(), "ids", j.ids.tolist(), "pair", pair, "margin %.3e" % ad.decision_margin(j))
    assert j.kinds.tolist() == kinds.tolist()
    n_pair = int((kinds == ad.OLD).sum())
    assert (j.ids[:n_pair] >= 0).all() and (j.ids[:n_pair] < N).all() and len(set(j.ids[:n_pair].tolist())) == n_pair
    assert j.ids[n_pair:].tolist() == [N, -1, N + 1]       # the two fresh features end as the last two landmarks
    assert j.x.size == x.size + 4
    k = n_pair + 1  # the in-between measurement: inside gamma_max of something (not New), outside every joint gate (not paired)
    assert j.nearest["matched"][k] in (3 + 2 * pair[0], 3 + 2 * pair[1]) and j.nearest["mahal"][k] <= gr.GAMMA_MAX
    assert ad.decision_margin(j) > gr.EDGE
    assert_bitwise_symmetric(0.5 * (j.P + j.P.T))


def test_loop_scenario_has_wide_margins_and_grows_the_whole_map(pkg):
    """The CPU run of the 20-step loop of tests/test_gpu_update_joint.py, the same seed: no decision of the reference within
    gate_ref.EDGE = 1e-6 relative of its threshold, the map grows from 0 to the world's 40 landmarks, every landmark once."""
    world, script = ad.loop_script(pkg)
    jg = pkg.ekfslam.joint_gates(0.99)
    x, P = np.zeros(3), np.zeros((3, 3))
    worst = np.inf
    for v, w, dt, z, R in script:
        x, P = _propagate(x, P, v, w, dt)
        j = ad.update_joint_ref(x, P, z, R, jg, window=16)
        worst = min(worst, ad.decision_margin(j))
        assert ad.IGNORE not in j.kinds.tolist(), j.kinds
        x, P = j.x, j.P
    print("smallest decision margin of the loop: %.3e" % worst)
    assert worst > gr.EDGE
    N = (x.size - 3) // 2
    assert N == len(world) == 40
    L = x[3:].reshape(-1, 2)
    nearest = [int(np.argmin(np.hypot(*(world - l).T))) for l in L]
    assert sorted(nearest) == list(range(40))  # no duplicates: every world landmark exactly once
    assert max(np.hypot(*(world[nearest] - L).T)) < 0.5


def _propagate(x, P, v, w, dt):
    from oracle import ekf_numpy as en
    return en.propagate(x, P, v, w, en.make_Q(v), dt)
