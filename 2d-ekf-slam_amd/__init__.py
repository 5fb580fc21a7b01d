"""MI355X-native EKF-SLAM core: host-side Python plumbing around libekfslam_hip.so.

The directory name is not a Python identifier; load it with `__graft_entry__.load_package()`
(importlib, registered as module `ekfslam_amd`).
"""
from . import ekfslam, features, montecarlo, scenarios  # noqa: F401
from .ekfslam import FilterBatch, KalmanFilter, EkfError, load, duplicate_keep_mask, duplicate_matching, candidate_matching, joint_gates, distinct_poses, same_pose, polar_to_cartesian, ITER_MAX, POLAR_RANGE, POLAR_BEARING, POLAR_BOTH  # noqa: F401
from .features import FeatureExtractor  # noqa: F401
