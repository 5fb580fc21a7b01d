"""CPU tests of the matched updates (ekf_update_matched / ekf_joint_compat and their batch forms): the header declares the calls and
the binding lists them; the plan functions refuse what they must (tests/cpp/match_plan_check.cpp); and, for every input a GPU test
of tests/test_update_matched.py or a matched update of tests/test_map_edges.py uses (match_ref.gpu_inputs), the NumPy reference (tests/match_ref.py) is checked against its
restatement in extended precision within 1/20 of each bound of helpers.assert_state_close -- with libm's cos / sin and with values
an ulp either side, which is what the device's own cos() / sin() may return --, against the oracle's sequence of Old updates when
the rounds hold one measurement, for the prefix property of d2, and for what an update must do: a positive semidefinite result, no
variance grown.  The Python layer's argument checks."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
from helpers import ABS_P, ABS_X, FRO_TOL, REL_TOL, assert_state_close, run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_update_matched", "ekf_batch_update_matched", "ekf_joint_compat", "ekf_batch_joint_compat")


@pytest.fixture(scope="module")
def inputs(pkg):
    return mr.gpu_inputs(pkg)


def fractions_of_the_bounds(a, b):
    """(x, P, Frobenius) differences of state a from state b as fractions of the bounds of helpers.assert_state_close."""
    xb, Pb = np.asarray(b[0], dtype=np.float64), np.asarray(b[1], dtype=np.float64)
    xa, Pa = np.asarray(a[0], dtype=np.float64), np.asarray(a[1], dtype=np.float64)
    scale = np.abs(Pb).max()
    ex = float((np.abs(xa - xb) / (REL_TOL * np.abs(xb) + ABS_X)).max())
    eP = float((np.abs(Pa - Pb) / (REL_TOL * np.abs(Pb) + ABS_P * scale)).max())
    fro = float(np.linalg.norm(Pa - Pb) / np.linalg.norm(Pb) / FRO_TOL)
    return ex, eP, fro


def rel_d2(a, b):
    both = ~np.isnan(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float((np.abs(a[both] - b[both]) / np.abs(b[both])).max()) if both.any() else 0.0


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        assert callable(cls.update_matched) and callable(cls.joint_compat)


def test_plan_functions_refuse_and_build_the_table(tmp_path):
    out = run_cpp_check(tmp_path, "match_plan_check")
    assert out.returncode == 0 and "match plan ok" in out.stdout, out.stdout + out.stderr


def test_reference_against_extended_precision(inputs):
    """1/20 of each bound of helpers.assert_state_close, and d2 within 1/20 of the bound its GPU test uses (match_ref.d2_bound:
    D2_REL, or D2_REL_EDGES for the inputs of tests/test_map_edges.py).  An input that fails this is badly scaled: change the input."""
    worst = {mr.D2_REL: 0.0, mr.D2_REL_EDGES: 0.0}
    for name, x, P, z, R, ids, rs in inputs:
        a, b = mr.update(x, P, z, R, ids, rs), mr.update_extended(x, P, z, R, ids, rs)
        n = int((np.asarray(ids) >= 0).sum())
        assert a[2] == b[2] == n, name
        ex, eP, fro = fractions_of_the_bounds(a, b)
        rd = rel_d2(a[3], b[3])
        worst[mr.d2_bound(name)] = max(worst[mr.d2_bound(name)], rd)
        print("%s: fractions of the bounds: x %.3e, P %.3e, Frobenius %.3e; d2 relative %.3e" % (name, ex, eP, fro, rd))
        assert max(ex, eP, fro) <= 1.0 / 20.0, (name, ex, eP, fro)
        assert rd <= mr.d2_bound(name) / 20.0, (name, rd)
    print("worst relative difference of d2, double against extended: %.3e under D2_REL, %.3e under D2_REL_EDGES" % (worst[mr.D2_REL], worst[mr.D2_REL_EDGES]))


def test_an_ulp_in_cos_and_sin_is_absorbed(inputs):
    """The device takes cos phi and sin phi from its own library: the reference with libm's values moved by an ulp, in every
    combination of directions, stays within 1/20 of the bounds of the extended-precision result."""
    for name, x, P, z, R, ids, rs in inputs:
        if "rounds of 8 reversed" in name or "of 32" in name:
            continue  # (the same states and lists as their neighbours)
        b = mr.update_extended(x, P, z, R, ids, rs)
        for dc, ds in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            a = mr.update(x, P, z, R, ids, rs, trig=mr.ulp_trig(dc, ds))
            ex, eP, fro = fractions_of_the_bounds(a, b)
            assert max(ex, eP, fro) <= 1.0 / 20.0, (name, dc, ds, ex, eP, fro)
            assert rel_d2(a[3], b[3]) <= mr.d2_bound(name) / 10.0, (name, dc, ds)  # (one more rounding error than libm's: a tenth)


def test_rounds_of_one_are_the_oracles_old_updates(pkg, oc):
    for N, _ in mr.SIZES:
        x, P, z, R, ids = mr.planted_scan(pkg, N, mr.SCAN_SEED[N])
        xo, Po, dec, matched, mahal = oc.update(x, P, *mr.as_oracle_chunk(z, R))
        assert dec == [pkg.ekfslam.OLD] * len(ids), dec                   # preconditions: every decision Old ...
        assert matched == [2 * int(i) + 3 for i in ids], (matched, ids)   # ... on the planted landmark
        x1, P1, applied, d2 = mr.update(x, P, z, R, ids, 1)
        assert applied == len(ids)
        err = assert_state_close(x1, P1, xo, Po, what="N=%d" % N)
        rd = float((np.abs(d2 - np.array(mahal)) / np.array(mahal)).max())
        print("N=%d: rounds of 1 vs oracle: max |dx| %.3e, max |dP| / max |P| %.3e, d2 vs mahal relative %.3e" % (N, err[0], err[1], rd))
        assert rd <= mr.D2_REL, rd


def test_d2_is_the_joint_distance_of_the_prefix_hypothesis(pkg):
    for N, _ in mr.SIZES:
        x, P, z, R, ids = mr.planted_scan(pkg, N, mr.SCAN_SEED[N])
        d2 = mr.update(x, P, z, R, ids)[3]
        assert np.all(np.diff(d2) >= 0.0)
        assert np.array_equal(d2, mr.joint_compat(x, P, z, R, ids))
        for k in range(len(ids)):  # computed separately: the distance d^T S^-1 d of the first k + 1 pairings
            _, S, d = mr.linearise(x, P, z[:k + 1], R[:k + 1], ids[:k + 1])
            want = float(d @ np.linalg.solve(S, d))
            assert abs(d2[k] - want) <= mr.D2_REL * want, (N, k, d2[k], want)
        wrong = mr.joint_compat(x, P, z, R, mr.wrong_pairing(ids))
        assert wrong[-1] > d2[-1] and wrong[1] > d2[1]


def test_result_is_psd_and_no_variance_has_grown(inputs):
    for name, x, P, z, R, ids, rs in inputs:
        x1, P1, _, _ = mr.update(x, P, z, R, ids, rs)
        scale = np.abs(P).max()
        assert np.linalg.eigvalsh(0.5 * (P1 + P1.T)).min() >= -1e-12 * scale, name
        assert np.all(np.diag(P1) <= np.diag(P) * (1.0 + 1e-12)), name
        diff = P - P1
        ev = np.linalg.eigvalsh(0.5 * (diff + diff.T))
        assert ev.min() >= -1e-12 * scale, (name, ev.min())
        if (np.asarray(ids) >= 0).any():
            assert ev.max() > 1e-6 * scale, (name, ev.max())
        else:
            assert np.array_equal(P1, P) and np.array_equal(x1, x), name


def test_a_singular_round_is_refused_in_either_precision(pkg):
    """The state of the GPU test: no robot uncertainty, one landmark measured twice with R = 0 behind a regular round of 4."""
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    P = P.copy()
    P[0:3, :] = 0.0
    P[:, 0:3] = 0.0
    ids = [3, 40, 31, 32, 17, 17]
    z, R = mr.scan_of(pkg, x, ids, 91)
    R[4:] = 0.0
    z[5] = z[4]
    for dtype in (np.float64, np.longdouble):
        x1, P1, applied, d2 = mr.update(x, P, z, R, ids, 4, dtype=dtype)
        assert applied == 4 and np.all(np.isnan(d2[4:])) and not np.any(np.isnan(d2[:4]))
        first = mr.update(x, P, z[:4], R[:4], ids[:4], 4, dtype=dtype)
        assert np.array_equal(x1, first[0]) and np.array_equal(P1, first[1])
        jc = mr.joint_compat(x, P, z[4:], R[4:], ids[4:], dtype=dtype)
        assert not np.isnan(jc[0]) and np.isnan(jc[1])  # the first of the pair is regular, the copy is where the pivot fails


def test_the_refused_filter_of_the_batch_is_refused_in_either_precision(pkg):
    """Filter 2 of match_ref.REFUSED_IDS (the GPU test of one refused filter among four): anchored, rounds of 4, the exact copy at the
    head of the second round with two regular measurements behind it.  gpu_inputs holds its first round and its siblings' lists."""
    import reframe_ref as rr
    states = mr.batch_states(pkg, mr.BATCH_COUNTS, 80)
    states[2] = rr.anchor(*states[2])
    z, R = mr.refused_scan(pkg, states)
    ids = mr.REFUSED_IDS[2]
    assert not states[2][1][:3].any() and not R[2, 4:6].any() and np.array_equal(z[2, 4], z[2, 5]) and ids[4] == ids[5]
    for dtype in (np.float64, np.longdouble):
        x1, P1, applied, d2 = mr.update(*states[2], z[2], R[2], ids, 4, dtype=dtype)
        assert applied == 4 and np.all(np.isnan(d2[4:])) and not np.any(np.isnan(d2[:4]))
        first = mr.update(*states[2], z[2, :4], R[2, :4], ids[:4], 4, dtype=dtype)
        assert np.array_equal(x1, first[0]) and np.array_equal(P1, first[1])
    for b in (0, 1, 3):  # the siblings: three rounds each
        n = sum(1 for i in mr.REFUSED_IDS[b] if i >= 0)
        assert 8 < n <= 12 and mr.update(*states[b], z[b], R[b], mr.REFUSED_IDS[b], 4)[2] == n


class _NoLibrary:
    """Stands where the C library would: the Python layer must refuse before it gets here."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_python_layer_validates_its_arguments(pkg):
    f = pkg.FilterBatch.__new__(pkg.FilterBatch)
    f.L, f.h, f.batch = _NoLibrary(), None, 2
    z, R = np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1))
    for call in (f.update_matched, f.joint_compat):
        with pytest.raises(ValueError):
            call(z, R, [0, 1])                   # fewer ids than measurements
        with pytest.raises(ValueError):
            call(z, R[:2], [0, 1, 2])
        with pytest.raises(ValueError):
            call(z, R, [0, -2, 1])               # below -1
        with pytest.raises(ValueError):
            call(z, R, [[0, 1, 2]])              # a batch axis with an index
        with pytest.raises(ValueError):
            call(z, R, [0, 1, 2], index=None)    # no batch axis without one
        with pytest.raises(ValueError):
            call(np.zeros((1, 3, 2)), R[None], [[0, 1, 2]], index=None)  # one list for a batch of two
    with pytest.raises(ValueError):
        f.joint_compat(np.zeros((33, 2)), np.tile(np.eye(2), (33, 1, 1)), list(range(33)))
    zz, Rc, a, n_z = f._matched_lists(z, [[[1.0, 2.0], [3.0, 4.0]]] * 3, [5, -1, 7], 0)
    assert n_z == 3 and a.dtype == np.int32 and a.tolist() == [5, -1, 7] and zz.shape == (3, 2)
    assert Rc.shape == (3, 4) and Rc[0].tolist() == [1.0, 3.0, 2.0, 4.0]  # column-major blocks
