"""CPU tests of landmark removal (ekf_remove_landmarks / ekf_batch_remove_landmarks) and the per-landmark covariance readout
(ekf_get_landmark_covs): the header declares them and the binding lists them; the destination -> source index functions the
removal kernel runs (ekf_device.h) reproduce the tile packing of the reduced matrix exactly."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("ekf_remove_landmarks", "ekf_batch_remove_landmarks", "ekf_get_landmark_covs")


def test_header_declares_and_binding_lists_the_map_management_calls(pkg):
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for meth in ("remove_landmarks", "landmark_covs"):
        assert callable(getattr(pkg.FilterBatch, meth))
    assert callable(pkg.KalmanFilter.remove_landmarks)


def test_removal_gather_reproduces_the_packing_of_the_reduced_matrix(tmp_path):
    out = run_cpp_check(tmp_path, "remove_map_check")
    assert out.returncode == 0 and "remove map ok" in out.stdout, out.stdout + out.stderr
