"""CPU tests of the absolute fixes (ekf_update_fixes / ekf_fix_compat and their batch forms): the header declares the calls and the
binding lists them; the plan functions refuse what they must (tests/cpp/fix_plan_check.cpp); and, for every input a GPU test of
tests/test_update_fixes.py uses (fix_ref.gpu_inputs), the NumPy reference (tests/fix_ref.py) is checked against the textbook form
K = P H^T S^-1, P - K S K^T with unpadded heading rows, against its restatement in extended precision within 1/20 of each bound of
helpers.assert_state_close (d2 within 1/20 of fix_ref.D2_REL), for linearity in the rounds, for the heading wrap, against the
oracle's compass update, and for what an update must do: a positive semidefinite result, no variance grown, a hard fix that pins
its landmark, a singular round refused.  The Python layer's argument checks."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fix_ref as fx  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import assert_state_close, run_cpp_check  # noqa: E402
from test_update_matched_cpu import fractions_of_the_bounds, rel_d2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_update_fixes", "ekf_batch_update_fixes", "ekf_fix_compat", "ekf_batch_fix_compat")
P_, H_, S_ = fx.POSITION, fx.HEADING, fx.SKIP
# d2 against np.linalg.solve on S (another algorithm): its error is of the order of cond(S) 2^-52, and S = H P H^T + R of these
# lists has a condition number below 1e4 (asserted) -- 1e-9 is three orders above that and three below the state bound REL_TOL
TEXTBOOK_D2_REL = 1e-9


@pytest.fixture(scope="module")
def inputs(pkg):
    return fx.gpu_inputs(pkg)


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for macro, value in (("EKF_FIX_SKIP", -1), ("EKF_FIX_POSITION", -2), ("EKF_FIX_HEADING", -3)):
        assert re.search(r"#define\s+%s\s+\(%d\)" % (macro, value), src), macro
    E = pkg.ekfslam
    assert (E.FIX_SKIP, E.FIX_POSITION, E.FIX_HEADING) == (-1, -2, -3) == (fx.SKIP, fx.POSITION, fx.HEADING)
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        assert callable(cls.update_fixes) and callable(cls.fix_compat)


def test_plan_functions_refuse_and_build_the_table(tmp_path):
    out = run_cpp_check(tmp_path, "fix_plan_check")
    assert out.returncode == 0 and "fix plan ok" in out.stdout, out.stdout + out.stderr


def test_reference_against_the_textbook_form(inputs):
    for name, x, P, z, R, what, rs in inputs:
        a = fx.update(x, P, z, R, what, rs)
        assert a[2] == int((np.asarray(what) != S_).sum()), name
        t = fx.textbook(x, P, z, R, what, rs)
        err = assert_state_close(a[0], a[1], t[0], t[1], what=name)
        kept = np.flatnonzero(np.asarray(what) != S_)
        rows = [r for k in kept for r in fx.state_rows(what[k]) if r is not None]
        assert np.linalg.cond(P[np.ix_(rows, rows)] + 1e-5 * np.eye(len(rows))) < 1e4, name  # (R adds at least 1e-5 to the diagonal)
        rd = rel_d2(a[3], t[2])
        print("%s: vs the textbook form: max |dx| %.3e, max |dP| / max |P| %.3e, d2 relative %.3e" % (name, err[0], err[1], rd))
        assert rd <= TEXTBOOK_D2_REL, (name, rd)


def test_reference_against_extended_precision(inputs):
    """1/20 of each bound of helpers.assert_state_close, and d2 within 1/20 of fix_ref.D2_REL: D2_REL is 20 times the worst value
    printed here.  An input that fails this is badly scaled: change the input."""
    worst, at = 0.0, None
    for name, x, P, z, R, what, rs in inputs:
        a, b = fx.update(x, P, z, R, what, rs), fx.update_extended(x, P, z, R, what, rs)
        assert a[2] == b[2] == int((np.asarray(what) != S_).sum()), name
        ex, eP, fro = fractions_of_the_bounds(a, b)
        rd = rel_d2(a[3], b[3])
        rc = rel_d2(fx.compat(x, P, z[:32], R[:32], what[:32]), fx.compat(x, P, z[:32], R[:32], what[:32], dtype=np.longdouble))
        if max(rd, rc) > worst:
            worst, at = max(rd, rc), name
        print("%s: fractions of the bounds: x %.3e, P %.3e, Frobenius %.3e; d2 relative %.3e, one round %.3e" % (name, ex, eP, fro, rd, rc))
        assert max(ex, eP, fro) <= 1.0 / 20.0, (name, ex, eP, fro)
    print("worst relative difference of d2, double against extended: %.3e (%s)" % (worst, at))
    assert worst <= fx.D2_REL / 20.0 and fx.D2_REL <= 21.0 * worst, (worst, fx.D2_REL)


def test_the_inert_column_is_exact(pkg):
    """A heading entry's second column: pivot 1, a unit row of U, y and V's column exact zeros, and x bit-identical with and without
    the padding (the heading fix as ONE column)."""
    x, P = pkg.scenarios.injected_state(100, seed=fx.STATE_SEED[100], extent=mr.map_extent(100))
    z, R, what = fx.mixed_list(pkg, x, P, fx.STATE_SEED[100])
    sel = [0, 1, 2, 3]
    W, S, d = fx.assemble(x, P, z[sel], R[sel], what[sel])
    U, y, bad = fx.cholesky_upper(S, d)
    assert bad is None and U[3, 3] == 1.0 and not U[3, 4:].any() and not U[:3, 3].any() and y[3, 0] == 0.0
    keep = [0, 1, 2, 4, 5, 6, 7]
    U1, y1, _ = fx.cholesky_upper(S[np.ix_(keep, keep)], d[keep])
    assert np.array_equal(U1, U[np.ix_(keep, keep)]) and np.array_equal(y1[:, 0], y[keep, 0])
    x1 = fx.round_update(x, P, z[sel], R[sel], what[sel])[0]
    V = np.linalg.solve(U1.T, W[:, keep].T).T
    assert np.allclose(x1, x - V @ y1[:, 0], rtol=0, atol=1e-12)


def test_linearity_in_the_rounds(pkg):
    """Nothing is linearised: the same list in rounds of 1, 5, 16, all at once, and reversed, is the same state within the bounds."""
    for N, _ in fx.SIZES:
        x, P = pkg.scenarios.injected_state(N, seed=fx.STATE_SEED[N], extent=mr.map_extent(N))
        z, R, what = fx.mixed_list(pkg, x, P, fx.STATE_SEED[N])
        base = fx.update(x, P, z, R, what, None)
        for rs in (1, 5, 16):
            got = fx.update(x, P, z, R, what, rs)
            assert_state_close(got[0], got[1], base[0], base[1], what="N=%d, rounds of %d" % (N, rs))
        got = fx.update(x, P, z[::-1], R[::-1], what[::-1], 5)
        assert_state_close(got[0], got[1], base[0], base[1], what="N=%d, reversed" % N)
        assert abs(got[3][0] - base[3][-1]) > 0  # (the distances do depend on the cut)


def test_heading_wrap(pkg):
    x, P = pkg.scenarios.injected_state(100, seed=fx.STATE_SEED[100], extent=mr.map_extent(100))
    for sign in (1.0, -1.0):
        base = fx.update(x, P, [[x[2] + sign * 0.1, np.nan]], np.full((1, 2, 2), 4e-4), [H_])
        assert base[2] == 1 and abs(base[0][2] - x[2]) > 1e-3
        for k in (-2, 3):
            got = fx.update(x, P, [[x[2] + fx.TWO_PI * k + sign * 0.1, np.nan]], np.full((1, 2, 2), 4e-4), [H_])
            assert_state_close(got[0], got[1], base[0], base[1], what="heading shifted by %d turns" % k)
            assert abs(got[3][0] - base[3][0]) <= 1e-9 * base[3][0]
    # a residual of exactly -pi stays, +pi goes to -pi, one just below +pi stays: [-pi, pi)
    assert fx.wrap(-fx.PI) == -fx.PI and fx.wrap(fx.PI) == -fx.PI
    below = fx.PI - 2.0 ** -40
    assert fx.wrap(below) == below and fx.wrap(below - fx.TWO_PI) == below - fx.TWO_PI + fx.TWO_PI
    for e in np.linspace(-20.0, 20.0, 4001):
        assert -fx.PI <= fx.wrap(e) < fx.PI
    # (the last ulp below +pi: (e + pi) / (2 pi) rounds to 1 there and the expression gives e - 2 pi, one ulp BELOW -pi -- the
    # interval is [-pi, pi) up to that rounding, the residual's magnitude is right to an ulp either way)
    last = np.nextafter(fx.PI, 0.0)
    assert abs(fx.wrap(last)) <= fx.PI * (1.0 + 2.0 ** -51)


def test_heading_fix_in_a_round_of_one_is_the_oracles_compass(pkg, oc):
    """phi in (0.1, 6.2) and |z - phi| < 3: the reference's three-way minimum and its truncated 2 pi add nothing there."""
    x0, P = pkg.scenarios.injected_state(100, seed=fx.STATE_SEED[100], extent=mr.map_extent(100))
    for phi, dz in ((0.3, 0.1), (0.11, -0.09), (3.1, 2.9), (6.19, -2.9), (4.0, 0.02)):
        x = x0.copy()
        x[2] = phi
        xo, Po = oc.compass(x, P, phi + dz, 4e-4)
        got = fx.update(x, P, [[phi + dz, np.nan]], np.full((1, 2, 2), 4e-4), [H_], 1)
        err = assert_state_close(got[0], got[1], xo, Po, what="phi %.2f" % phi)
        print("phi %.2f, z - phi %.2f: vs the oracle's compass: max |dx| %.3e, max |dP| / max |P| %.3e" % (phi, dz, err[0], err[1]))
        want = dz * dz / (P[2, 2] + 4e-4)
        assert abs(got[3][0] - want) <= 1e-12 * want  # d2 = wrap(phi - z)^2 / (P_phiphi + R)


def test_result_is_psd_and_no_variance_has_grown(inputs):
    for name, x, P, z, R, what, rs in inputs:
        x1, P1, _, _ = fx.update(x, P, z, R, what, rs)
        scale = np.abs(P).max()
        assert np.linalg.eigvalsh(0.5 * (P1 + P1.T)).min() >= -1e-12 * scale, name
        assert np.all(np.diag(P1) <= np.diag(P) * (1.0 + 1e-12) + 1e-300), name
        diff = P - P1
        ev = np.linalg.eigvalsh(0.5 * (diff + diff.T))
        assert ev.min() >= -1e-12 * scale, (name, ev.min())
        assert ev.max() > 1e-6 * scale, (name, ev.max())


def test_a_hard_fix_pins_its_landmark(pkg):
    x, P = pkg.scenarios.injected_state(100, seed=fx.STATE_SEED[100], extent=mr.map_extent(100))
    i = 31
    z = x[3 + 2 * i:5 + 2 * i] + np.array([0.05, -0.08])
    for dtype in (np.float64, np.longdouble):
        x1, P1, applied, _ = fx.update(x, P, [z], np.zeros((1, 2, 2)), [i], dtype=dtype)
        assert applied == 1
        rows = [3 + 2 * i, 4 + 2 * i]
        assert np.abs(x1[rows] - z).max() <= 1e-14 * np.abs(z).max()
        assert np.abs(P1[rows, :]).max() <= 1e-15 * np.abs(P).max() and np.abs(P1[:, rows]).max() <= 1e-15 * np.abs(P).max()


def test_a_singular_round_is_refused_in_either_precision(pkg):
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    z, R, what = fx.singular_list(pkg, x, P)
    assert list(what[4:6]) == [P_, P_] and not R[4:6].any() and np.array_equal(z[4], z[5])
    twice5 = [3, 40, 31, 32, 5, 5, 17]
    z5, R5 = fx.entries_for(x, P, twice5, 77)
    R5[4:6] = 0.0
    z5[5] = z5[4]
    for zz, RR, ww in ((z, R, what), (z5, R5, twice5)):
        for dtype in (np.float64, np.longdouble):
            x1, P1, applied, d2 = fx.update(x, P, zz, RR, ww, 4, dtype=dtype)
            assert applied == 4 and np.all(np.isnan(d2[4:])) and not np.any(np.isnan(d2[:4]))
            first = fx.update(x, P, zz[:4], RR[:4], ww[:4], 4, dtype=dtype)
            assert np.array_equal(x1, first[0]) and np.array_equal(P1, first[1])
            jc = fx.compat(x, P, zz[4:6], RR[4:6], ww[4:6], dtype=dtype)
            assert not np.isnan(jc[0]) and np.isnan(jc[1])  # the first of the pair is regular, the copy is where the pivot fails
    # the refused filter of the batch test: its siblings run three rounds
    states = mr.batch_states(pkg, fx.REFUSED_COUNTS, 80)
    z, R, what = fx.refused_lists(pkg, states)
    for dtype in (np.float64, np.longdouble):
        assert fx.update(*states[2], z[2], R[2], what[2], 4, dtype=dtype)[2] == 4
    for b in (0, 1, 3):
        n = int((what[b] != S_).sum())
        assert 8 < n <= 12 and fx.update(*states[b], z[b], R[b], what[b], 4)[2] == n


class _NoLibrary:
    """Stands where the C library would: the Python layer must refuse before it gets here."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_python_layer_validates_its_arguments(pkg):
    f = pkg.FilterBatch.__new__(pkg.FilterBatch)
    f.L, f.h, f.batch = _NoLibrary(), None, 2
    z, R = np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1))
    for call in (f.update_fixes, f.fix_compat):
        with pytest.raises(ValueError):
            call(z, R, [0, 1])                   # fewer kinds than entries
        with pytest.raises(ValueError):
            call(z, R[:2], [0, 1, 2])
        with pytest.raises(ValueError):
            call(z, R, [0, -4, 1])               # below FIX_HEADING
        with pytest.raises(ValueError):
            call(z, R, [[0, 1, 2]])              # a batch axis with an index
        with pytest.raises(ValueError):
            call(z, R, [0, 1, 2], index=None)    # no batch axis without one
        with pytest.raises(ValueError):
            call(np.zeros((1, 3, 2)), R[None], [[0, 1, 2]], index=None)  # one list for a batch of two
        with pytest.raises(ValueError):
            call([[0.0, 0.0], 1.0], [np.eye(2), 0.1], [P_, 4])           # a scalar z for a landmark entry
        with pytest.raises(ValueError):
            call([[0.0, 0.0], [1.0, 2.0, 3.0]], [np.eye(2), np.eye(2)], [P_, 4])
    with pytest.raises(ValueError):
        f.fix_compat(np.zeros((33, 2)), np.tile(np.eye(2), (33, 1, 1)), [P_] * 33)
    zz, Rc, a, n = f._fix_lists(z, [[[1.0, 2.0], [3.0, 4.0]]] * 3, [5, S_, P_], 0)
    assert n == 3 and a.dtype == np.int32 and a.tolist() == [5, -1, -2] and zz.shape == (3, 2)
    assert Rc.shape == (3, 4) and Rc[0].tolist() == [1.0, 3.0, 2.0, 4.0]  # column-major blocks
    # a heading entry as a scalar z with a scalar variance, among entries of two values and alone
    zz, Rc, a, n = f._fix_lists([[1.0, 2.0], 0.25, [3.0, 4.0]], [[[1.0, 2.0], [3.0, 4.0]], 0.5, np.eye(2)], [P_, H_, 7], 0)
    assert n == 3 and zz.tolist() == [[1.0, 2.0], [0.25, 0.0], [3.0, 4.0]]
    assert Rc.tolist() == [[1.0, 3.0, 2.0, 4.0], [0.5, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0]]
    zz, Rc, a, n = f._fix_lists(0.25, 0.5, H_, 0)
    assert n == 1 and a.tolist() == [H_] and zz.tolist() == [[0.25, 0.0]] and Rc.tolist() == [[0.5, 0.0, 0.0, 0.0]]
    zz, Rc, a, n = f._fix_lists([0.25, 0.3], [0.5, 0.6], [H_, H_], 0)
    assert n == 2 and zz.tolist() == [[0.25, 0.0], [0.3, 0.0]] and Rc[:, 0].tolist() == [0.5, 0.6]
    # landmark ids alone on rectangular lists, single and batch: the lists of _matched_lists, byte for byte
    rng = np.random.default_rng(7)
    for lead, index in (((), 0), ((2,), None)):
        zr, Rr, ids = rng.normal(size=lead + (3, 2)), rng.normal(size=lead + (3, 2, 2)), rng.integers(0, 9, size=lead + (3,))
        fixes, matched = f._fix_lists(zr, Rr, ids, index), f._matched_lists(zr, Rr, ids, index)
        for got, want in zip(fixes[:3], matched[:3]):
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
        assert fixes[3] == matched[3] == 3
