"""CPU tests of the polar measurements (ekf_update_polar / ekf_polar_compat and their batch forms): the header declares the calls and
the binding lists them; the plan functions refuse what they must (tests/cpp/polar_plan_check.cpp, plain and under the address and
undefined-behaviour sanitizers); H of the NumPy reference (tests/polar_ref.py) against central differences of h; and, for every
input a GPU test of tests/test_update_polar.py uses (polar_ref.gpu_inputs), the reference against the textbook form K = P H^T S^-1,
P - K S K^T with unpadded one-row entries, against its restatement in extended precision within 1/20 of each bound of
helpers.assert_state_close (d2 within 1/20 of polar_ref.D2_REL), and for what an update must do: the inert column exact, whole turns
of a bearing immaterial, a positive semidefinite result, no variance grown, the singular round and the landmark on the pose refused.
The Python layer's argument checks, and polar_to_cartesian against differences."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr  # noqa: E402
import polar_ref as pr  # noqa: E402
from helpers import assert_state_close, run_cpp_check  # noqa: E402
from test_update_matched_cpu import fractions_of_the_bounds, rel_d2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_update_polar", "ekf_batch_update_polar", "ekf_polar_compat", "ekf_batch_polar_compat")
RG, BR, BO = pr.RANGE, pr.BEARING, pr.BOTH
# d2 against np.linalg.solve on S (another algorithm): its error is of the order of cond(S) 2^-52; S = H P H^T + R of these lists
# mixes metres^2 and radians^2 and has a condition number below 1e7 (asserted) -- 1e-8 is an order above that and two below REL_TOL
TEXTBOOK_D2_REL = 1e-8


@pytest.fixture(scope="module")
def inputs(pkg):
    return pr.gpu_inputs(pkg)


def mixed(pkg, N):
    x, P = pkg.scenarios.injected_state(N, seed=pr.STATE_SEED[N], extent=mr.map_extent(N))
    return (x, P) + pr.mixed_list(pkg, x, P, pr.STATE_SEED[N])


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for macro, value in (("EKF_POLAR_RANGE", 1), ("EKF_POLAR_BEARING", 2), ("EKF_POLAR_BOTH", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), src), macro
    assert (pkg.POLAR_RANGE, pkg.POLAR_BEARING, pkg.POLAR_BOTH) == (1, 2, 3) == (RG, BR, BO)
    assert (pkg.ekfslam.POLAR_RANGE, pkg.ekfslam.POLAR_BEARING, pkg.ekfslam.POLAR_BOTH) == (1, 2, 3)
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        assert callable(cls.update_polar) and callable(cls.polar_compat)
    assert callable(pkg.polar_to_cartesian)


def test_plan_functions_refuse_and_build_the_table(tmp_path):
    out = run_cpp_check(tmp_path, "polar_plan_check")
    assert out.returncode == 0 and "polar plan ok" in out.stdout, out.stdout + out.stderr


def test_plan_functions_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with the address and undefined-behaviour sanitizers compiled in."""
    exe = str(tmp_path / "polar_plan_check_san")
    src = os.path.join(ROOT, "tests", "cpp", "polar_plan_check.cpp")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "polar plan ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_mixed_list_is_what_the_gpu_tests_need(pkg):
    for N, _ in pr.SIZES:
        x, P, z, R, ids, kind = mixed(pkg, N)
        assert len(ids) == 24 and list(kind) == [pr.KIND_CYCLE[k % 3] for k in range(24)]
        assert int((ids == pr.SKIP).sum()) == 2 and {0, 15, 16, N - 1} <= set(int(i) for i in ids)
        assert ids[1] == ids[2] and (kind[1], kind[2]) == (RG, BR)            # one landmark by range and by bearing, one round
        west = pr.behind(x)
        assert np.pi - abs(pr.predict(x, west, BR)[0] + x[2]) < 0.2 and west in ids[kind != RG]   # atan2 near +-pi
        kept = ids >= 0
        assert pr.ranges(x)[ids[kept]].min() >= 1.0
        # the wrap acts: some bearing residual leaves [-pi, pi) before it
        raw = np.array([pr.predict(x, ids[k], BR)[0] - z[k, 1] for k in range(24) if kept[k] and kind[k] != RG])
        assert np.any(np.abs(raw) > np.pi) and np.abs(pr.wrap(raw)).max() < 0.2
        # what a kind does not read is NaN: the reference and the device must not look at it
        assert np.all(np.isnan(z[kind == RG, 1])) and np.all(np.isnan(z[kept & (kind == BR), 0]))
        for rs in (1, 5, 16, 32):
            got = pr.update(x, P, z, R, ids, kind, rs)
            assert got[2] == 22 and np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])), (N, rs)
            assert np.array_equal(np.isnan(got[3]), ~kept)


def test_jacobian_against_central_differences(pkg):
    """Step s = 1e-5 (m, rad): the truncation error of a central difference is s^2 / 6 times the third derivative, at most about
    2 / r^3 for the bearing and 1 / r^2 for the range of a landmark r >= 1 m away -- below 4e-11 --, its rounding error about
    2^-52 |h| / s <= 40 m * 2.2e-16 / 1e-5 = 9e-10.  The bound asked is 1e-8."""
    s = 1e-5
    for N, _ in pr.SIZES:
        x, _, _, _, ids, kind = mixed(pkg, N)
        for i, kd in zip(ids, kind):
            if i < 0:
                continue
            H = pr.jacobian(x, i, kd)
            assert H.shape == ((2 if kd == BO else 1), len(x))
            touched = [0, 1, 2, 3 + 2 * i, 4 + 2 * i]
            assert not np.delete(H, touched, axis=1).any()
            for c in touched:
                e = np.zeros(len(x))
                e[c] = s
                num = (pr.predict(x + e, i, kd) - pr.predict(x - e, i, kd)) / (2 * s)
                assert np.abs(num - H[:, c]).max() <= 1e-8, (N, i, kd, c, num, H[:, c])


def test_reference_against_the_textbook_form(inputs):
    for name, x, P, z, R, ids, kind, rs in inputs:
        a = pr.update(x, P, z, R, ids, kind, rs)
        kept = np.flatnonzero(np.asarray(ids) >= 0)
        assert a[2] == len(kept), name
        t = pr.textbook(x, P, z, R, ids, kind, rs)
        err = assert_state_close(a[0], a[1], t[0], t[1], what=name)
        H = np.concatenate([pr.jacobian(x, ids[k], kind[k]) for k in kept[:rs]])
        S = H @ P @ H.T + np.diag(np.concatenate([np.diag(pr.noise_of(R[k], kind[k]))[:2 if kind[k] == BO else 1] for k in kept[:rs]]))
        assert np.linalg.cond(S) < 1e7, (name, np.linalg.cond(S))
        rd = rel_d2(a[3], t[2])
        print("%s: vs the textbook form: max |dx| %.3e, max |dP| / max |P| %.3e, d2 relative %.3e" % (name, err[0], err[1], rd))
        assert rd <= TEXTBOOK_D2_REL, (name, rd)


def test_reference_against_extended_precision(inputs):
    """1/20 of each bound of helpers.assert_state_close, and d2 within 1/20 of polar_ref.D2_REL: D2_REL is 20 times the worst value
    printed here -- measured: 3.444e-13, on "mixed N=100, rounds of 1".  An input that fails this is badly scaled: change the input."""
    worst, at = 0.0, None
    for name, x, P, z, R, ids, kind, rs in inputs:
        a, b = pr.update(x, P, z, R, ids, kind, rs), pr.update_extended(x, P, z, R, ids, kind, rs)
        assert a[2] == b[2] == int((np.asarray(ids) >= 0).sum()), name
        ex, eP, fro = fractions_of_the_bounds(a, b)
        rd = rel_d2(a[3], b[3])
        head = np.flatnonzero(np.cumsum(np.asarray(ids) >= 0) <= 32)
        one = [v[head] for v in (np.asarray(z), np.asarray(R), np.asarray(ids), np.asarray(kind))]
        rc = rel_d2(pr.compat(x, P, *one), pr.compat(x, P, *one, dtype=np.longdouble))
        if max(rd, rc) > worst:
            worst, at = max(rd, rc), name
        print("%s: fractions of the bounds: x %.3e, P %.3e, Frobenius %.3e; d2 relative %.3e, one round %.3e" % (name, ex, eP, fro, rd, rc))
        assert max(ex, eP, fro) <= 1.0 / 20.0, (name, ex, eP, fro)
    print("worst relative difference of d2, double against extended: %.3e (%s)" % (worst, at))
    assert worst <= pr.D2_REL / 20.0 and pr.D2_REL <= 21.0 * worst, (worst, pr.D2_REL)


def test_the_inert_column_is_exact(pkg):
    """A one-component entry's second column: pivot 1, a unit row of U, y and W's column exact zeros, and the factor of the live
    rows bit-identical with and without the padding."""
    x, P, z, R, ids, kind = mixed(pkg, 100)
    sel = [0, 1, 2, 3]   # BOTH, RANGE, BEARING, BOTH: columns 3 and 5 are inert
    W, S, d = pr.assemble(x, P, z[sel], R[sel], ids[sel], kind[sel])
    U, y, bad = pr.cholesky_upper(S, d)
    assert bad is None
    for c in (3, 5):
        assert U[c, c] == 1.0 and not U[c, c + 1:].any() and not U[:c, c].any() and y[c, 0] == 0.0 and d[c] == 0.0 and not W[:, c].any()
    keep = [0, 1, 2, 4, 6, 7]
    U1, y1, _ = pr.cholesky_upper(S[np.ix_(keep, keep)], d[keep])
    assert np.array_equal(U1, U[np.ix_(keep, keep)]) and np.array_equal(y1[:, 0], y[keep, 0])
    d2 = pr.prefix_d2(y[:, 0], None)
    assert d2[1] == d2[0] + y[2, 0] ** 2 and d2[2] == d2[1] + y[4, 0] ** 2   # the inert columns add exactly 0
    x1 = pr.round_update(x, P, z[sel], R[sel], ids[sel], kind[sel])[0]
    V = np.linalg.solve(U1.T, W[:, keep].T).T
    assert np.allclose(x1, x - V @ y1[:, 0], rtol=0, atol=1e-12)


def test_whole_turns_of_a_bearing_change_nothing(pkg):
    x, P, z, R, ids, kind = mixed(pkg, 100)
    base = pr.update(x, P, z, R, ids, kind, 16)
    for k in (-2, 3):
        zk = z.copy()
        zk[:, 1] += pr.TWO_PI * k
        got = pr.update(x, P, zk, R, ids, kind, 16)
        assert_state_close(got[0], got[1], base[0], base[1], what="bearings shifted by %d turns" % k)
        ok = ~np.isnan(base[3])
        assert np.abs(got[3][ok] - base[3][ok]).max() <= 1e-8 * base[3][ok].max()   # (2 pi k rounds at 1e-15: 1e-15 / sigma 0.02 on d)


def test_a_lone_range_entry(pkg):
    x, P, z, R, ids, kind = mixed(pkg, 100)
    k = 1
    assert kind[k] == RG
    for dtype in (np.float64, np.longdouble):
        got = pr.update(x, P, z[k:k + 1], R[k:k + 1], ids[k:k + 1], kind[k:k + 1], dtype=dtype)
        H = pr.jacobian(x, ids[k], RG)
        want = (pr.predict(x, ids[k], RG)[0] - z[k, 0]) ** 2 / (float((H @ P @ H.T)[0, 0]) + R[k, 0, 0])
        assert got[2] == 1 and abs(got[3][0] - want) <= 1e-12 * want   # d2 = (r - z)^2 / (H P H^T + R)


def test_result_is_psd_and_no_variance_has_grown(inputs):
    for name, x, P, z, R, ids, kind, rs in inputs:
        x1, P1, _, _ = pr.update(x, P, z, R, ids, kind, rs)
        scale = np.abs(P).max()
        assert np.linalg.eigvalsh(0.5 * (P1 + P1.T)).min() >= -1e-12 * scale, name
        assert np.all(np.diag(P1) <= np.diag(P) * (1.0 + 1e-12) + 1e-300), name
        diff = P - P1
        ev = np.linalg.eigvalsh(0.5 * (diff + diff.T))
        assert ev.min() >= -1e-12 * scale, (name, ev.min())
        assert ev.max() > 1e-6 * scale, (name, ev.max())


def test_a_singular_round_is_refused_in_either_precision(pkg):
    x, P = pkg.scenarios.injected_state(60, seed=91, extent=12.0)
    z, R, ids, kind = pr.singular_list(pkg, x, P)
    assert ids[4] == ids[5] and (kind[4], kind[5]) == (RG, RG) and not R[4:6, 0, 0].any() and z[4, 0] == z[5, 0]
    assert pr.ranges(x)[ids].min() >= 1.0
    for dtype in (np.float64, np.longdouble):
        x1, P1, applied, d2 = pr.update(x, P, z, R, ids, kind, 4, dtype=dtype)
        assert applied == 4 and np.all(np.isnan(d2[4:])) and not np.any(np.isnan(d2[:4]))
        first = pr.update(x, P, z[:4], R[:4], ids[:4], kind[:4], 4, dtype=dtype)
        assert np.array_equal(x1, first[0]) and np.array_equal(P1, first[1])
        jc = pr.compat(x, P, z[4:6], R[4:6], ids[4:6], kind[4:6], dtype=dtype)
        assert not np.isnan(jc[0]) and np.isnan(jc[1])  # the first of the pair is regular, the copy is where the pivot fails


def test_a_landmark_on_the_pose_is_refused_in_either_precision(pkg):
    x, P = pr.on_pose_state(pkg)
    assert np.array_equal(x[3 + 2 * pr.ON_POSE:5 + 2 * pr.ON_POSE], x[0:2])
    for kd in (RG, BR, BO):
        z, R, ids, kind = pr.on_pose_list(pkg, x, P, kd)
        assert ids[1] == pr.ON_POSE and kind[1] == kd
        for dtype in (np.float64, np.longdouble):
            x1, P1, applied, d2 = pr.update(x, P, z, R, ids, kind, 4, dtype=dtype)   # refused in round one: nothing is applied
            assert applied == 0 and np.all(np.isnan(d2))
            assert np.array_equal(x1, x.astype(dtype)) and np.array_equal(P1, P.astype(dtype))
            jc = pr.compat(x, P, z, R, ids, kind, dtype=dtype)
            assert not np.isnan(jc[0]) and np.all(np.isnan(jc[1:]))  # the entry in front of it keeps its distance
            rest = np.arange(10) != 1
            assert pr.update(x, P, z[rest], R[rest], ids[rest], kind[rest], 4, dtype=dtype)[2] == 9  # the list without it is regular


class _NoLibrary:
    """Stands where the C library would: the Python layer must refuse before it gets here."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_python_layer_validates_its_arguments(pkg):
    f = pkg.FilterBatch.__new__(pkg.FilterBatch)
    f.L, f.h, f.batch = _NoLibrary(), None, 2
    z, R = np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1))
    for call in (f.update_polar, f.polar_compat):
        with pytest.raises(ValueError):
            call(z, R, [0, 1], [BO, BO])               # fewer ids than entries
        with pytest.raises(ValueError):
            call(z, R, [0, 1, 2], [BO, BO])            # fewer kinds than ids
        with pytest.raises(ValueError):
            call(z, R[:2], [0, 1, 2], [BO, RG, BR])
        with pytest.raises(ValueError):
            call(z, R, [0, -2, 1], [BO, RG, BR])       # below -1
        with pytest.raises(ValueError):
            call(z, R, [0, 1, 2], [BO, 0, BR])         # no such kind
        with pytest.raises(ValueError):
            call(z, R, [0, 1, 2], [BO, 4, BR])
        with pytest.raises(ValueError):
            call(z, R, [[0, 1, 2]], [[BO, RG, BR]])    # a batch axis with an index
        with pytest.raises(ValueError):
            call(z, R, [0, 1, 2], [BO, RG, BR], index=None)   # no batch axis without one
        with pytest.raises(ValueError):
            call(np.zeros((1, 3, 2)), R[None], [[0, 1, 2]], [[BO, RG, BR]], index=None)  # one list for a batch of two
    with pytest.raises(ValueError):
        f.polar_compat(np.zeros((33, 2)), np.tile(np.eye(2), (33, 1, 1)), list(range(33)), [BO] * 33)
    (zz, Rc, a, n), kd = f._polar_lists(z, [[[1.0, 2.0], [3.0, 4.0]]] * 3, [5, -1, 7], [RG, 99, BO], 0)
    assert n == 3 and a.dtype == np.int32 and a.tolist() == [5, -1, 7] and kd.dtype == np.int32 and kd.tolist() == [RG, 0, BO]
    assert zz.shape == (3, 2) and Rc.shape == (3, 4) and Rc[0].tolist() == [1.0, 3.0, 2.0, 4.0]  # column-major blocks
    zn = np.full((2, 3, 2), np.nan)   # NaN passes through: what is read is the C side's to say
    (zz, Rc, a, n), kd = f._polar_lists(zn, np.full((2, 3, 2, 2), np.nan), [[0, 1, -1]] * 2, [[RG, BR, 0]] * 2, None)
    assert n == 3 and a.shape == kd.shape == (2, 3) and np.all(np.isnan(zz)) and Rc.shape == (2, 3, 4)


def test_polar_to_cartesian(pkg):
    """z against its definition, J R J^T against central differences of (r cos b, r sin b): step 1e-6, truncation s^2 / 6 * r, rounding
    2^-52 r / s -- both below 1e-8 for r <= 30 m."""
    rng = np.random.default_rng(5)
    z = np.stack([rng.uniform(1.0, 30.0, size=7), rng.uniform(-np.pi, np.pi, size=7)], axis=-1)
    R = np.tile(pr.R_BOTH, (7, 1, 1)) * rng.uniform(0.5, 2.0, size=(7, 1, 1))
    zc, Rc = pkg.polar_to_cartesian(z, R)
    assert zc.shape == (7, 2) and Rc.shape == (7, 2, 2)
    s = 1e-6

    def f(v):
        return np.array([v[0] * np.cos(v[1]), v[0] * np.sin(v[1])])

    for k in range(7):
        assert np.abs(zc[k] - f(z[k])).max() <= 1e-14 * z[k, 0]
        J = np.stack([(f(z[k] + s * e) - f(z[k] - s * e)) / (2 * s) for e in np.eye(2)], axis=1)
        want = J @ R[k] @ J.T
        assert np.abs(Rc[k] - want).max() <= 1e-7 * np.abs(want).max()
        assert np.array_equal(Rc[k], Rc[k].T)
        assert np.linalg.eigvalsh(Rc[k]).min() > 0.0
    one = pkg.polar_to_cartesian(z[0], R[0])
    assert one[0].shape == (2,) and one[1].shape == (2, 2) and np.array_equal(one[0], zc[0])
    zb, Rb = pkg.polar_to_cartesian(z.reshape(1, 7, 2), R.reshape(1, 7, 2, 2))
    assert zb.shape == (1, 7, 2) and Rb.shape == (1, 7, 2, 2)
    with pytest.raises(ValueError):
        pkg.polar_to_cartesian(z, R[:3])
    # a measurement converted and applied as a Cartesian one points where the polar one does
    assert abs(np.hypot(*zc[3]) - z[3, 0]) <= 1e-13 * z[3, 0] and abs(pr.wrap(np.arctan2(zc[3, 1], zc[3, 0]) - z[3, 1])) <= 1e-14
