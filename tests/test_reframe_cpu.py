"""CPU tests of the frame changes (ekf_transform_frame / ekf_anchor_at_robot and their batch forms): the header declares them and the
binding lists them; the lane -> (block, element) mapping the tile kernel runs (ekf_device.h: reframe_item) visits every element of
a tile once and groups whole 2x2 blocks; and the NumPy reference the GPU tests compare with (tests/reframe_ref.py) is itself
checked -- its Jacobians against central differences, its blockwise form against the dense J P J^T."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reframe_ref as rr  # noqa: E402
from helpers import assert_state_close, run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("ekf_transform_frame", "ekf_batch_transform_frame", "ekf_anchor_at_robot", "ekf_batch_anchor_at_robot")
FRAME = (3.0, -2.0, 0.7)


def test_header_declares_and_binding_lists_the_frame_calls(pkg):
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        for meth in ("transform_frame", "anchor_at_robot"):
            assert callable(getattr(cls, meth)), (cls, meth)


def test_tile_mapping_visits_every_element_once_in_whole_blocks(tmp_path):
    out = run_cpp_check(tmp_path, "reframe_map_check")
    assert out.returncode == 0 and "reframe map ok" in out.stdout, out.stdout + out.stderr


def _state(pkg, N, seed):
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=10.0)
    x[0:3] = (1.5, -0.7, 0.3)
    return x, P


def test_analytic_jacobians_equal_central_differences(pkg):
    x, _ = _state(pkg, 12, seed=3)
    for g, J in ((lambda v: rr.rigid_g(v, FRAME), rr.rigid_J(x, FRAME)), (rr.anchor_g, rr.anchor_J(x))):
        err = np.abs(rr.central_difference(g, x, h=1e-6) - J).max()
        print("max |J - central difference| = %.3e" % err)
        assert err < 1e-6


def test_blockwise_forms_equal_the_dense_jacobian_product(pkg):
    x, P = _state(pkg, 40, seed=4)
    xd, Pd = rr.apply_dense(x, P, lambda v: rr.rigid_g(v, FRAME), lambda v: rr.rigid_J(v, FRAME))
    xb, Pb = rr.rigid(x, P, FRAME)
    assert np.abs(xd - xb).max() <= 1e-14 * np.abs(xd).max() and np.abs(Pd - Pb).max() <= 1e-14 * np.abs(Pd).max()
    xd, Pd = rr.apply_dense(x, P, rr.anchor_g, rr.anchor_J)
    xb, Pb = rr.anchor(x, P)
    assert np.abs(xd - xb).max() <= 1e-14 * np.abs(xd).max() and np.abs(Pd - Pb).max() <= 1e-14 * np.abs(Pd).max()
    assert np.array_equal(Pb, Pb.T)


def test_anchor_zeroes_the_robot_exactly(pkg):
    x, P = _state(pkg, 40, seed=5)
    xa, Pa = rr.anchor(x, P)
    assert np.array_equal(xa[:3], np.zeros(3))
    assert not Pa[:3, :].any() and not Pa[:, :3].any()
    # the anchored blocks are the innovation covariances without R: H P H^T of the relative measurement of every landmark
    J = rr.anchor_J(x)
    for l in (0, 17, 39):
        H = J[3 + 2 * l:5 + 2 * l]
        assert np.allclose(Pa[3 + 2 * l:5 + 2 * l, 3 + 2 * l:5 + 2 * l], H @ P @ H.T, rtol=1e-12, atol=0)


def test_pure_translation_is_exact_and_the_inverse_frame_undoes_a_transform(pkg):
    x, P = _state(pkg, 40, seed=6)
    xt, Pt = rr.rigid(x, P, (3.0, -2.0, 0.0))
    assert np.array_equal(Pt, P)
    want = x.copy()
    want[0] = x[0] - 3.0
    want[1] = x[1] - (-2.0)
    want[3::2] = x[3::2] - 3.0
    want[4::2] = x[4::2] - (-2.0)
    assert np.array_equal(xt, want)
    x1, P1 = rr.rigid(x, P, FRAME)
    x2, P2 = rr.rigid(x1, P1, rr.inverse_frame(FRAME))
    assert_state_close(x2, P2, x, P, what="rigid then its inverse")
