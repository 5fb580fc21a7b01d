"""CPU tests of the iterated matched update (ekf_update_matched_iter and its batch form): the header declares the calls and the
binding lists them; the argument checks and the new scratch block's carving (tests/cpp/iter_plan_check.cpp); and the NumPy reference
tests/iter_ref.py on every input the GPU tests of tests/test_update_matched_iter.py compare with it (iter_ref.gpu_inputs):
  * with max_iter = 1 it is match_ref.update, bit for bit;
  * the double run and its extended-precision restatement agree -- the differences MEASURED here, with cos phi and sin phi from libm
    and moved by an ulp either way, are iter_ref's MEASURED_ constants, and the GPU tests' bounds are 20 times them;
  * every step of both runs lies outside [tol / 4, 4 tol], which lets the GPU tests ask for `iters` exactly;
  * the converged result has a lower MAP cost than the single-step result, and in extended precision the cost's gradient at the
    converged result is at rounding level relative to its two terms."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iter_ref as ir  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_update_matched_iter", "ekf_batch_update_matched_iter")
ULPS = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def differences(a, e):
    """(max |dx|, max |dP| / max |P|, worst relative d2, max |dstep|) of two runs of iter_ref.update."""
    assert a[2] == e[2] and np.array_equal(a[4], e[4]), (a[2], e[2], a[4], e[4])
    assert np.array_equal(np.isnan(a[3]), np.isnan(e[3])) and np.array_equal(np.isnan(a[5]), np.isnan(e[5]))
    ok = ~np.isnan(a[3])
    d2 = float((np.abs(a[3][ok] - e[3][ok]) / np.abs(e[3][ok])).max()) if ok.any() else 0.0
    st = float(np.abs(a[5][ok] - e[5][ok]).max()) if ok.any() else 0.0
    return float(np.abs(a[0] - e[0]).max()), float(np.abs(a[1] - e[1]).max() / np.abs(e[1]).max()), d2, st


@pytest.fixture(scope="module")
def runs(pkg):
    """[(input, double run, extended run, double trace, extended trace)]"""
    out = []
    for t in ir.gpu_inputs(pkg):
        name, x, P, z, R, ids, rs, mi = t
        tr, tre = [], []
        a = ir.update(x, P, z, R, ids, mi, ir.tol_of(name), rs, trace=tr)
        e = ir.update_extended(x, P, z, R, ids, mi, ir.tol_of(name), rs, trace=tre)
        out.append((t, a, e, tr, tre))
    return out


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    assert re.search(r"#define\s+EKF_ITER_MAX\s+16\s", src)
    assert pkg.ITER_MAX == pkg.ekfslam.ITER_MAX == ir.ITER_MAX == 16
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        assert callable(cls.update_matched_iter)


def test_the_kernel_has_a_name_inside_no_other_kernels_name():
    csrc = os.path.join(ROOT, "2d-ekf-slam_amd", "csrc")
    every = []
    for f in os.listdir(csrc):
        if f.endswith(".hip"):
            every += re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", open(os.path.join(csrc, f)).read())
    own = re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", open(os.path.join(csrc, "ekf_match_iter.hip")).read())
    assert own == ["k_match_factor_iter"]
    assert sorted(k for k in set(every) if "k_match_factor" in k) == ["k_match_factor", "k_match_factor_iter"]


def test_argument_checks_and_the_scratch_block(tmp_path):
    out = run_cpp_check(tmp_path, "iter_plan_check")
    assert out.returncode == 0 and "iter plan ok" in out.stdout, out.stdout + out.stderr


def test_python_layer_refuses_what_the_library_refuses(pkg):
    call = pkg.FilterBatch.update_matched_iter
    for bad in (dict(max_iter=0), dict(max_iter=17), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf)):
        with pytest.raises(ValueError):
            call(None, np.zeros((1, 2)), np.zeros((1, 2, 2)), [0], **bad)  # (refused before the handle is looked at)


def test_one_iteration_is_the_single_step_update_bit_for_bit(pkg):
    for name, x, P, z, R, ids, rs, _ in ir.gpu_inputs(pkg):
        a = ir.update(x, P, z, R, ids, 1, ir.tol_of(name), rs)
        b = mr.update(x, P, z, R, ids, rs)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], name
        assert a[3].tobytes() == b[3].tobytes(), name
        kept = ~np.isnan(b[3])
        assert np.array_equal(a[4], kept.astype(np.int32)) and np.array_equal(np.isnan(a[5]), ~kept), name


def test_inputs_are_what_the_gpu_tests_take_them_for(pkg, runs):
    by = {t[0]: (t, a) for t, a, _, _, _ in runs}
    assert len(by) == len(runs) == len(ir.TOL_OF)
    t, a = by["refused second round"]
    assert a[2] == 4 and list(a[4]) == [a[4][0]] * 4 + [0] * 3 and a[4][0] > 1 and np.isnan(a[5][4:]).all()   # the second round refused
    assert np.isnan(mr.joint_compat(a[0], a[1], t[3][4:6], t[4][4:6], t[5][4:6])[1])  # ... in its first factorisation
    t, a = by["9 entries in rounds of 4"]
    assert a[2] == 9 and len({int(a[4][0]), int(a[4][4]), int(a[4][8])}) > 1   # three rounds, each with its own count
    t, a = by["tol = 0"]
    assert (a[4] == t[7]).all() and (a[5] > 0.0).all()
    t, a = by["a full round of 32"]
    assert a[2] == 32 and t[6] == 32
    for name, (t, a) in by.items():
        if name != "tol = 0":
            assert (a[5][~np.isnan(a[5])] <= ir.tol_of(name)).all() and a[4].max() < t[7], name   # converged, iterations to spare
        assert a[4].max() >= 3, name   # and every input iterates


def test_double_and_extended_runs_agree_within_the_written_constants(pkg, runs):
    worst = np.zeros(4)
    for (name, x, P, z, R, ids, rs, mi), a, e, _, _ in runs:
        d = np.array(differences(a, e))
        for dc, ds in ULPS:
            d = np.maximum(d, differences(ir.update(x, P, z, R, ids, mi, ir.tol_of(name), rs, trig=mr.ulp_trig(dc, ds)), e))
        print("%-40s x %.2e  P %.2e  d2 %.2e  step %.2e" % (name, *d))
        worst = np.maximum(worst, d)
    print("worst: x %.3e  P %.3e  d2 %.3e  step %.3e" % tuple(worst))
    written = np.array([ir.MEASURED_X, ir.MEASURED_P, ir.MEASURED_D2, ir.MEASURED_STEP])
    assert (worst <= written).all() and (written <= 1.5 * worst).all(), (worst, written)   # the constants are what is measured
    assert (ir.BOUND_X, ir.BOUND_P, ir.BOUND_D2, ir.BOUND_STEP) == tuple(20 * written)


def test_every_step_lies_a_factor_of_four_from_tol(runs):
    for (name, *_), _, _, tr, tre in runs:
        tol = ir.tol_of(name)
        assert len(tr) == len(tre), name
        for s in tr + tre:
            assert not (tol / 4 <= s <= 4 * tol), (name, float(s), tol)


SINGLE_ROUND = [n for n in ir.TOL_OF if n.startswith("planted N=100") or n in ("one measurement", "a full round of 32", "tile edges")]


def test_converged_result_has_the_lower_map_cost(pkg, runs):
    for (name, x, P, z, R, ids, rs, _), a, _, _, _ in runs:
        if name not in SINGLE_ROUND:
            continue
        single = mr.update(x, P, z, R, ids, rs)
        c1, cn = ir.map_cost(single[0], x, P, z, R, ids), ir.map_cost(a[0], x, P, z, R, ids)
        print("%-40s MAP cost: single step %.4g, iterated %.4g" % (name, c1, cn))
        assert cn < c1, (name, c1, cn)


def test_gradient_vanishes_at_the_converged_result_in_extended_precision(pkg, runs):
    """Run to a standstill (tol = 0, 16 iterations; the step shrinks about 100 times per iteration), the two terms of P grad / 2
    cancel to rounding level in the maximum norm: within n units of the extended format's rounding (2^-63) of the products they are summed from
    (iter_ref.map_gradient's scale), n = 3 + 2 N the length of those sums -- the textbook bound of a sum of n products."""
    eps = np.finfo(np.longdouble).eps
    for (name, x, P, z, R, ids, rs, _), _, _, _, _ in runs:
        if name not in SINGLE_ROUND:
            continue
        e = ir.update_extended(x, P, z, R, ids, ir.ITER_MAX, 0.0, rs)
        prior, meas, scale = ir.map_gradient(e[0], x, P, z, R, ids)
        rel = float(np.abs(prior + meas).max() / (np.abs(prior) + scale).max())
        print("%-40s |P grad| / |terms| = %.2e (%.1f eps, n = %d)" % (name, rel, rel / eps, len(x)))
        assert rel <= len(x) * eps, (name, rel)
