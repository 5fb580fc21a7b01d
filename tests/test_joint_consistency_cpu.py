"""CPU tests of whole-state consistency (ekf_joint_consistency): the header declares the calls and the binding lists them; the index
functions the trailing-update kernel runs (ekf_device.h: chol_trail_ij, chol_operand_offset) agree with brute force; the two NumPy
references the GPU tests compare with (tests/factor_ref.py: LAPACK on the whole P, and a restatement of the device algorithm in
64-row tile steps with the robot last) agree with each other and with an np.longdouble Cholesky; `info` follows LAPACK's potrf; and
montecarlo.joint_consistency_report is checked against scipy.stats.chi2 on drawn errors."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_ref as fr  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import correlated_state, run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The references against the longdouble yardstick: the issue's own measurements are <= 3e-12 relative on the NEES values and <= 5e-10
# absolute on the log-determinants for states of condition 1e9 .. 4e10; the states here are far better conditioned (<= 1e6), for
# which n * eps * cond <= 203 * 2.2e-16 * 1e6 = 5e-8 bounds any of the factorisations and 1e-9 is what they are expected to keep.
REF_REL = 1e-9
REF_LOGDET = 1e-9


def test_header_declares_and_binding_lists_the_calls(pkg):
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ekf_joint_consistency", "ekf_batch_joint_consistency", "ekf_debug_joint_factor"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    assert "typedef struct ekf_joint" in src
    assert callable(pkg.FilterBatch.joint_consistency) and callable(pkg.KalmanFilter.joint_consistency)
    assert callable(pkg.montecarlo.joint_consistency_report)
    assert pkg.ekfslam.JOINT_DTYPE.itemsize == 128  # two ints, six doubles, nine doubles: no padding


def test_index_functions_agree_with_brute_force(tmp_path):
    out = run_cpp_check(tmp_path, "factor_map_check")
    assert out.returncode == 0 and "factor map ok (105 grids)" in out.stdout, out.stdout + out.stderr


def _compare(x, P, what):
    xt = fr.draw_truth(x, P, seed=17)
    a, b, c = fr.lapack(x, P, xt), fr.tiled(x, P, xt), fr.longdouble(x, P, xt)
    assert a["info"] == b["info"] == 0, what
    for r, name in ((a, "lapack"), (b, "tiled")):
        for k in ("nees_map", "nees_joint", "min_pivot", "max_pivot"):
            err = fr.rel_err(r[k], c[k])
            print("%s %s %s: %.3e" % (what, name, k, err))
            assert err <= REF_REL, (what, name, k, r[k], c[k])
        for k in ("logdet_map", "logdet_joint"):
            err = abs(r[k] - c[k])
            print("%s %s %s: %.3e" % (what, name, k, err))
            assert err <= REF_LOGDET * (3 + len(x)), (what, name, k)
        scale = np.abs(P).max()
        assert np.abs(r["cov_robot_given_map"] - c["cov_robot_given_map"]).max() <= REF_REL * scale, (what, name)
        assert np.abs(r["U"] - c["U"]).max() <= REF_REL * np.abs(c["U"]).max(), (what, name)
        assert not np.tril(r["U"], -1).any()
    for k in fr.FIELDS:  # (a) and (b) with each other
        assert abs(a[k] - b[k]) <= REF_REL * max(abs(a[k]), 1.0), (what, k, a[k], b[k])


@pytest.mark.parametrize("N", [31, 32, 33, 100])
def test_references_agree_on_injected_states(pkg, N):
    x, P = pkg.scenarios.injected_state(N, seed=900 + N)
    _compare(x, P, "injected N=%d" % N)


@pytest.fixture(scope="module")
def correlated(pkg, oc):
    return correlated_state(pkg, oc, copies=4, n_landmarks=24, steps=400)


def test_references_agree_on_the_correlated_state(correlated):
    x, P = correlated
    N = (len(x) - 3) // 2
    print("correlated state: N = %d, cond %.2e" % (N, np.linalg.cond(P)))
    assert N > 32  # more than one tile step
    _compare(x, P, "correlated N=%d" % N)


def test_without_truth_the_nees_fields_are_nan(pkg):
    x, P = pkg.scenarios.injected_state(33, seed=5)
    for f in (fr.lapack, fr.tiled):
        r = f(x, P, None)
        assert r["info"] == 0 and np.isnan(r["nees_map"]) and np.isnan(r["nees_joint"])
        assert np.isfinite(r["logdet_map"]) and np.isfinite(r["logdet_joint"]) and r["min_pivot"] > 0


def test_info_follows_potrf_on_a_zeroed_landmark(pkg):
    x, P = pkg.scenarios.injected_state(100, seed=6)
    a = 3 + 2 * 40
    P[a:a + 2, :] = 0.0
    P[:, a:a + 2] = 0.0
    want = fr.potrf_info(P[3:, 3:])
    assert want == 81
    for f in (fr.lapack, fr.tiled):
        r = f(x, P, x)
        assert r["info"] == want, f.__name__
        for k in ("nees_map", "nees_joint", "logdet_map", "logdet_joint"):
            assert np.isnan(r[k]), (f.__name__, k)
    assert fr.tiled(x, P, x)["min_pivot"] == 0.0


def test_fresh_and_anchored_states_give_info_minus_one(pkg):
    for f in (fr.lapack, fr.tiled):
        r = f(np.zeros(3), np.zeros((3, 3)), np.array([0.1, 0.2, 0.3]))
        assert r["info"] == -1 and r["n_landmarks"] == 0 and r["nees_map"] == 0.0 and r["logdet_map"] == 0.0
        assert np.isnan(r["nees_joint"]) and np.isnan(r["logdet_joint"])
    x, P = pkg.scenarios.injected_state(40, seed=8)
    xa, Pa = rr.anchor(x, P)
    assert not Pa[:3, :].any()
    xt = xa.copy()
    xt[3:] += 0.01
    Pm = np.eye(83)  # the map alone under the yardstick: an identity robot block, uncorrelated
    Pm[3:, 3:] = Pa[3:, 3:]
    want = fr.longdouble(xa, Pm, xt)
    for f in (fr.lapack, fr.tiled):
        r = f(xa, Pa, xt)
        assert r["info"] == -1, f.__name__
        assert fr.rel_err(r["nees_map"], want["nees_map"]) <= REF_REL and abs(r["logdet_map"] - want["logdet_map"]) <= REF_LOGDET * 83
        assert np.isnan(r["nees_joint"]) and np.isnan(r["logdet_joint"])
        assert np.abs(r["cov_robot_given_map"]).max() <= 1e-12 * np.abs(Pa).max()


def test_joint_consistency_report_against_chi2(pkg):
    from scipy.stats import chi2
    rng = np.random.default_rng(3)
    rows = np.zeros(40, dtype=pkg.ekfslam.JOINT_DTYPE)
    dof_j = dof_m = 0
    for i in range(40):
        N = 5 + i % 7
        x, P = pkg.scenarios.injected_state(N, seed=100 + i)
        L = np.linalg.cholesky(P)
        r = fr.lapack(x, P, x - L @ rng.standard_normal(len(x)))
        rows[i]["n_landmarks"], rows[i]["info"] = N, 0
        rows[i]["nees_joint"], rows[i]["nees_map"] = r["nees_joint"], r["nees_map"]
        dof_j += 3 + 2 * N
        dof_m += 2 * N
    rows[7]["info"], rows[7]["nees_joint"] = -1, np.nan
    rows[9]["info"] = 12
    dof_j -= (3 + 2 * rows[7]["n_landmarks"]) + (3 + 2 * rows[9]["n_landmarks"])
    dof_m -= 2 * rows[7]["n_landmarks"] + 2 * rows[9]["n_landmarks"]
    rep = pkg.montecarlo.joint_consistency_report(rows, alpha=0.05)
    assert rep["skipped"] == 2
    keep = rows[rows["info"] == 0]
    for name, field, dof in (("joint", "nees_joint", dof_j), ("map", "nees_map", dof_m)):
        r = rep[name]
        assert r["dof"] == dof and r["samples"] == 38
        assert r["sum"] == pytest.approx(float(keep[field].sum()), rel=1e-14)
        assert r["lower"] == pytest.approx(chi2.ppf(0.025, dof)) and r["upper"] == pytest.approx(chi2.ppf(0.975, dof))
        assert r["consistent"] == bool(r["lower"] <= r["sum"] <= r["upper"])
        assert r["consistent"]  # errors drawn from P itself (fixed seed)
    # an over-confident filter (P ten times too small) is caught
    bad = keep.copy()
    bad["nees_joint"] *= 10.0
    assert not pkg.montecarlo.joint_consistency_report(bad)["joint"]["consistent"]
    assert pkg.montecarlo.joint_consistency_report(rows[[7, 9]])["joint"] is None
