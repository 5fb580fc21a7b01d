"""CPU tests of landmark fusion (ekf_fuse_landmarks / ekf_batch_fuse_landmarks): the header declares the calls and the binding lists
them; the index functions the kernels run (ekf_device.h: fuse_source, fuse_slot_offset) are checked against bm_offset and pair_offset
(tests/cpp/fuse_map_check.cpp); and, for every input a GPU test of tests/test_fuse_landmarks.py uses, the NumPy reference
(tests/fuse_ref.py) is checked against itself in rounds, against its restatement in extended precision within 1/20 of each bound of
helpers.assert_state_close, and for what a fusion must do: equal rows with slack = 0, a positive semidefinite result, no landmark's
variance grown, more information than removal keeps.  duplicate_matching and the Python layer's argument checks."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dup_ref as dr  # noqa: E402
import fuse_ref as fr  # noqa: E402
import map_model as mm  # noqa: E402
from helpers import ABS_P, ABS_X, FRO_TOL, REL_TOL, assert_state_close, run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, N_DUP = 70, 24
EDGE_LISTS = [[(31, 32), (63, 64)], [(2, 3), (40, 41), (65, 95)], [(0, 97), (1, 96), (30, 98)], [(5, 127)]]
BATCH_COUNTS = (100, 45, 64, 33)
BATCH_LISTS = [[(0, 99), (31, 32), (63, 64), (5, 6), (40, 80)], [], [(1, 63)], [(k, 32 - k) for k in range(10)]]


def gpu_inputs(pkg):
    """(name, x, P, pairs, slack, round_size) of every fusion the GPU tests ask for (states with an open window differ from these by
    a propagation and a far New landmark; the exact-copy state is taken with the slack that makes it regular)."""
    out = []
    for N in (200, 100):
        _, _, _, _, x, P, truth = fr.joined_with_duplicates(pkg, N, NS, N_DUP, 7)
        found, _ = dr.find(x, P, split=N)
        matched = pkg.ekfslam.duplicate_matching(found, N + NS)
        for slack in (0.0, 1e-4):
            out.append(("join-find-fuse N=%d slack=%g" % (N, slack), x, P, matched, slack, 16))
        out.append(("rounds of 8 N=%d" % N, x, P, truth, 0.0, 8))
        out.append(("rounds of 8 reversed N=%d" % N, x, P, truth[::-1], 0.0, 8))
        out.append(("rounds of 1 N=%d" % N, x, P, truth[:5], 0.0, 1))
        _, _, _, _, x, P, truth = fr.joined_with_duplicates(pkg, N, NS, N_DUP, 9, extent=20.0)
        out.append(("twin N=%d" % N, x, P, truth, 1e-4, 8))
    x, P = pkg.scenarios.injected_state(100, seed=13, extent=12.0 * (100 / 64.0) ** 0.5 + 8.0)
    out.append(("open window pair", x, P, fr.as_pairs([(3, 40), (31, 32), (63, 64), (5, 99)]), 1e-4, 16))
    for k, rows in enumerate(EDGE_LISTS):
        x, P = pkg.scenarios.injected_state(128 if k == 3 else 100, seed=51 + k, extent=15.0)
        out.append(("edges %d" % k, x, P, fr.as_pairs(rows), 1e-4, 16))
    x, P = pkg.scenarios.injected_state(2, seed=61, extent=5.0)
    out.append(("two landmarks", x, P, fr.as_pairs([(0, 1)]), 0.0, 16))
    for b, n in enumerate(BATCH_COUNTS):
        if BATCH_LISTS[b]:
            x, P = pkg.scenarios.injected_state(n, seed=80 + b, extent=10.0 + b)
            out.append(("batch filter %d" % b, x, P, fr.as_pairs(BATCH_LISTS[b]), 1e-5, 4))
    x0, P0 = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    x, P = fr.with_exact_copy(x0, P0, 17)
    out.append(("exact copy, slack", x, P, fr.as_pairs([(0, 33), (1, 50), (31, 32), (2, 59), (17, 60), (3, 40), (4, 41)]), 1e-4, 4))
    x, P = pkg.scenarios.injected_state(60, seed=101, extent=12.0 * (60 / 64.0) ** 0.5 + 8.0)
    out.append(("after the refusals", x, P, fr.as_pairs([(0, 1), (2, 59)]), 0.0, 16))
    return out


@pytest.fixture(scope="module")
def inputs(pkg):
    return gpu_inputs(pkg)


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("ekf_fuse_landmarks", "ekf_batch_fuse_landmarks"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    assert callable(pkg.FilterBatch.fuse_landmarks) and callable(pkg.KalmanFilter.fuse_landmarks)
    assert callable(pkg.ekfslam.duplicate_matching) and callable(pkg.duplicate_matching)


def test_index_functions_agree_with_the_layout(tmp_path):
    out = run_cpp_check(tmp_path, "fuse_map_check")
    assert out.returncode == 0 and "fuse map ok (4 layouts)" in out.stdout, out.stdout + out.stderr


def test_joint_and_round_wise_references_agree(inputs):
    for name, x, P, pairs, slack, rs in inputs:
        fr.check_pairs(pairs, (len(x) - 3) // 2)
        joint, rounds = fr.fuse(x, P, pairs, slack), fr.fuse(x, P, pairs, slack, rs)
        assert joint[2] == rounds[2] == len(pairs), name
        err = assert_state_close(rounds[0], rounds[1], joint[0], joint[1], what=name)
        print("%s: rounds of %d vs joint: max |dx| %.3e, max |dP| / max |P| %.3e" % (name, rs, err[0], err[1]))


def test_reference_against_extended_precision(inputs):
    """1/20 of each bound of helpers.assert_state_close.  An input that fails this is badly scaled: change the input."""
    for name, x, P, pairs, slack, rs in inputs:
        a, b = fr.fuse(x, P, pairs, slack, rs), fr.fuse_extended(x, P, pairs, slack, rs)
        assert a[2] == b[2] == len(pairs), name
        xb, Pb = b[0].astype(np.float64), b[1].astype(np.float64)
        scale = np.abs(Pb).max()
        ex = float((np.abs(a[0] - xb) / (REL_TOL * np.abs(xb) + ABS_X)).max())
        eP = float((np.abs(a[1] - Pb) / (REL_TOL * np.abs(Pb) + ABS_P * scale)).max())
        fro = float(np.linalg.norm(a[1] - Pb) / np.linalg.norm(Pb) / FRO_TOL)
        print("%s: fractions of the bounds: x %.3e, P %.3e, Frobenius %.3e" % (name, ex, eP, fro))
        assert max(ex, eP, fro) <= 1.0 / 20.0, (name, ex, eP, fro)


def test_exact_constraint_makes_the_rows_coincide(inputs):
    for name, x, P, pairs, slack, rs in inputs:
        x1, P1, fused = fr.fuse(x, P, pairs, 0.0, rs, reduce=False)
        if fused < len(pairs):  # (the exact-copy state: see test_exact_copy_stops_the_second_round)
            continue
        ij = fr.as_ij(pairs)
        scale = np.abs(P).max()
        for e in range(2):
            ri, rj = 3 + 2 * ij[:, 0] + e, 3 + 2 * ij[:, 1] + e
            assert np.all(np.abs(x1[ri] - x1[rj]) <= 1e-9 * np.maximum(np.abs(x1[ri]), 1.0)), name
            assert np.abs(P1[ri] - P1[rj]).max() <= 1e-10 * scale, (name, np.abs(P1[ri] - P1[rj]).max())


def test_fused_covariance_is_psd_and_no_block_has_grown(inputs):
    for name, x, P, pairs, slack, rs in inputs:
        x1, P1, fused = fr.fuse(x, P, pairs, slack, rs)
        keep = np.ones((len(x) - 3) // 2, dtype=bool)
        keep[fr.as_ij(pairs)[:, 1]] = False
        _, P0 = mm.reduce_state(np.asarray(x), np.asarray(P), keep)
        scale = np.abs(P).max()
        assert np.linalg.eigvalsh(P1).min() >= -1e-12 * scale, name
        t0 = np.diag(P0)[3::2] + np.diag(P0)[4::2]
        t1 = np.diag(P1)[3::2] + np.diag(P1)[4::2]
        assert np.all(t1 <= t0 * (1.0 + 1e-12)), name
        # fusing is strictly more informative than removing: P_removed - P_fused is PSD to rounding and not zero
        diff = P0 - P1
        ev = np.linalg.eigvalsh(0.5 * (diff + diff.T))
        assert ev.min() >= -1e-12 * scale and ev.max() > 1e-6 * scale, (name, ev.min(), ev.max())


def test_exact_copy_stops_the_second_round(pkg):
    x0, P0 = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    x, P = fr.with_exact_copy(x0, P0, 17)
    pairs = fr.as_pairs([(0, 33), (1, 50), (31, 32), (2, 59), (17, 60), (3, 40), (4, 41)])
    for dtype in (np.float64, np.longdouble):
        x1, P1, fused = fr.fuse(x, P, pairs, 0.0, 4, dtype=dtype)
        assert fused == 4 and len(x1) == 3 + 2 * 57
        first = fr.fuse(x, P, pairs[:4], 0.0, 4, dtype=dtype)
        assert np.array_equal(x1, first[0]) and np.array_equal(P1, first[1])  # exactly round 1, exactly its j removed
    assert fr.fuse(x, P, pairs, 0.0)[2] == 0  # jointly: nothing
    assert fr.fuse(x, P, pairs, 1e-4, 4)[2] == 7


def test_duplicate_matching_accepts_what_the_keep_mask_drops(pkg):
    E = pkg.ekfslam
    rows = [(0, 4, 3.0), (1, 4, 0.1), (2, 3, 0.2), (0, 3, 0.15)]
    for lst in (rows, rows[::-1], sorted(rows)[:2], [], [(1, 2, 1.0), (0, 2, 1.0), (1, 3, 1.0)]):
        pairs = np.array(lst, dtype=dr.DUP_DTYPE)
        m = E.duplicate_matching(pairs, 6)
        keep = E.duplicate_keep_mask(pairs, 6)
        assert m.dtype == E.DUP_DTYPE and sorted(m["j"].tolist()) == np.flatnonzero(~keep).tolist()
        fr.check_pairs(m, 6)
        assert list(zip(m["i"].tolist(), m["j"].tolist())) == sorted(zip(m["i"].tolist(), m["j"].tolist()))
        for p in m:  # an accepted pair is one of the list, d2 and all
            assert p in pairs
    assert [tuple(p) for p in E.duplicate_matching(np.array(rows, dtype=dr.DUP_DTYPE), 6)] == [(0, 3, 0.15), (1, 4, 0.1)]
    with pytest.raises(ValueError):
        E.duplicate_matching(np.array([(2, 2, 0.0)], dtype=dr.DUP_DTYPE), 4)
    for N in (200, 100):  # on the GPU tests' joined maps: every planted pair is matched
        _, _, _, _, x, P, truth = fr.joined_with_duplicates(pkg, N, NS, N_DUP, 7)
        found, _ = dr.find(x, P, split=N)
        m = E.duplicate_matching(found, N + NS)
        assert set(zip(truth["i"].tolist(), truth["j"].tolist())) <= set(zip(m["i"].tolist(), m["j"].tolist()))
        assert np.flatnonzero(~E.duplicate_keep_mask(found, N + NS)).tolist() == sorted(m["j"].tolist())


class _NoLibrary:
    """Stands where the C library would: the Python layer must refuse before it gets here."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_python_layer_validates_its_arguments(pkg):
    f = pkg.FilterBatch.__new__(pkg.FilterBatch)
    f.L, f.h, f.batch = _NoLibrary(), None, 2
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            f.fuse_landmarks([(0, 1)], slack=bad)
    with pytest.raises(ValueError):
        f.fuse_landmarks([[(0, 1)]], index=None)  # one list for a batch of two
    with pytest.raises(ValueError):
        f.fuse_landmarks([(0, 1, 2, 3, 4)])       # rows that are no pairs
    buf = pkg.ekfslam._pair_buffer([(3, 4), (5, 9)])
    assert buf.dtype == pkg.ekfslam.DUP_DTYPE and buf["i"].tolist() == [3, 5] and buf["j"].tolist() == [4, 9]
    same = np.array([(1, 2, 0.5)], dtype=pkg.ekfslam.DUP_DTYPE)
    assert pkg.ekfslam._pair_buffer(same).tobytes() == same.tobytes()
