"""CPU tests of map joining (ekf_join_map / ekf_batch_join_map): the header declares the calls and the binding lists them; the
destination -> source index functions the tile kernel runs (ekf_device.h: join_tile_ij, join_source) agree with a brute-force
dense model; and the NumPy reference the GPU tests compare with (tests/join_ref.py) is itself checked -- its Jacobian against
central differences of the map, the block table of include/ekfslam_c.h against the dense product, the two exact cases, symmetry
and positive semidefiniteness."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_ref as jr  # noqa: E402
from helpers import run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(pkg, Ng=23, Ns=9):
    xg, Pg = pkg.scenarios.injected_state(Ng, seed=7, extent=10.0)
    xs, Ps = pkg.scenarios.injected_state(Ns, seed=8, extent=6.0)
    xg[0:3] = (1.5, -0.7, 0.3)
    xs[0:3] = (0.4, 0.9, -1.1)
    return xg, Pg, xs, Ps


def test_header_declares_and_binding_lists_the_join_calls(pkg):
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ekf_join_map", "ekf_batch_join_map"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for meth in ("join_map", "batch_join_map"):
        assert callable(getattr(pkg.FilterBatch, meth)), meth


def test_index_function_agrees_with_a_dense_model(tmp_path):
    out = run_cpp_check(tmp_path, "join_map_check")
    assert out.returncode == 0 and "join map ok (70 cases)" in out.stdout, out.stdout + out.stderr


def test_jacobian_equals_central_differences(pkg):
    xg, _, xs, _ = _pair(pkg)
    ng = xg.size
    num = jr.central_difference(lambda v: jr.join_g(v[:ng], v[ng:]), np.concatenate([xg, xs]), h=1e-6)
    err = np.abs(num - jr.join_J(xg, xs)).max()
    print("max |J - central difference| = %.3e" % err)
    assert err < 1e-6


def test_block_table_equals_the_dense_product(pkg):
    for Ng, Ns in ((23, 9), (0, 5), (40, 1), (33, 70)):
        xg, Pg, xs, Ps = _pair(pkg, Ng, Ns)
        xd, Pd = jr.join(xg, Pg, xs, Ps)
        xb, Pb = jr.join_blocks(xg, Pg, xs, Ps)
        assert np.array_equal(xd, xb)
        err = np.abs(Pd - Pb).max() / np.abs(Pd).max()
        print("Ng=%d Ns=%d: block table vs dense, relative %.3e" % (Ng, Ns, err))
        assert err <= 1e-12
        a = 3 + 2 * Ng
        assert np.array_equal(Pb[3:a, 3:a], Pg[3:, 3:]) and np.array_equal(xb[3:a], xg[3:])


def test_joining_into_a_fresh_filter_returns_the_source_exactly(pkg):
    _, _, xs, Ps = _pair(pkg)
    for f in (jr.join, jr.join_blocks):
        x, P = f(np.zeros(3), np.zeros((3, 3)), xs, Ps)
        assert np.array_equal(x, xs) and np.array_equal(P, Ps), f.__name__


def test_joining_an_empty_source_returns_the_destination_exactly(pkg):
    xg, Pg, _, _ = _pair(pkg)
    for f in (jr.join, jr.join_blocks):
        x, P = f(xg, Pg, np.zeros(3), np.zeros((3, 3)))
        assert np.array_equal(x, xg) and np.array_equal(P, Pg), f.__name__


def test_result_is_symmetric_and_positive_semidefinite(pkg):
    xg, Pg, xs, Ps = _pair(pkg, 33, 20)
    for M in (Pg, Ps):
        assert np.linalg.eigvalsh(M).min() > 0.0  # SPD inputs
    for f in (jr.join, jr.join_blocks):
        _, P = f(xg, Pg, xs, Ps)
        assert np.array_equal(P, P.T)
        lo = np.linalg.eigvalsh(P).min()
        print("%s: smallest eigenvalue %.3e, max |P| %.3e" % (f.__name__, lo, np.abs(P).max()))
        assert lo >= -1e-12 * np.abs(P).max()
