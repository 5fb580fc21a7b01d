"""ctypes binding of libekfslam_hip.so (include/ekfslam_c.h) plus a KalmanFilter mirror.

This is plumbing for tests/ and bench.py: every call goes straight through the C ABI to the HIP
kernels.  There is no CPU fallback -- a missing library or a missing gfx950 device raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EKFSLAM_LIB", os.path.join(_HERE, "lib", "libekfslam_hip.so"))  # override: diagnostic builds

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_HIP, ERR_NO_DEVICE, ERR_STATE, ERR_TIMEOUT = 0, -1, -2, -3, -4, -5, -6
NEW, OLD, IGNORE = 1, 2, 3
FIX_SKIP, FIX_POSITION, FIX_HEADING = -1, -2, -3  # the kinds of ekf_update_fixes beside a landmark number
POLAR_RANGE, POLAR_BEARING, POLAR_BOTH = 1, 2, 3  # the kinds of ekf_update_polar

# every symbol include/ekfslam_c.h declares
ABI_SYMBOLS = [
    "ekf_last_error", "ekf_default_params", "ekf_create", "ekf_batch_create", "ekf_destroy", "ekf_reserve", "ekf_batch_size",
    "ekf_capacity", "ekf_window", "ekf_overlap", "ekf_propagate", "ekf_propagate_q", "ekf_update", "ekf_update_compass", "ekf_get_pose",
    "ekf_num_landmarks", "ekf_get_robot_cov", "ekf_get_x", "ekf_batch_propagate", "ekf_batch_propagate_q", "ekf_batch_update",
    "ekf_batch_update_compass", "ekf_batch_get_pose", "ekf_batch_num_landmarks", "ekf_get_state", "ekf_set_state",
    "ekf_broadcast_state", "ekf_script_load", "ekf_script_run", "ekf_sync", "ekf_flush", "ekf_close_window", "ekf_timer_start",
    "ekf_timer_stop", "ekf_flush_profile", "ekf_flush_profile_read", "ekf_fused_pass", "ekf_get_decisions", "ekf_get_stats",
    "ekf_reset_stats", "ekf_stats_means_device", "ekf_record_truth", "ekf_stream", "ekf_device_bytes", "ekf_debug_windows", "ekf_debug_stream", "ekf_debug_stream_ring",
    "ekf_remove_landmarks", "ekf_batch_remove_landmarks", "ekf_get_landmark_covs",
    "ekf_transform_frame", "ekf_batch_transform_frame", "ekf_anchor_at_robot", "ekf_batch_anchor_at_robot",
    "ekf_join_map", "ekf_batch_join_map",
    "ekf_extract_map", "ekf_batch_extract_map", "ekf_get_submap",
    "ekf_joint_consistency", "ekf_batch_joint_consistency", "ekf_debug_joint_factor",
    "ekf_find_duplicates", "ekf_batch_find_duplicates",
    "ekf_fuse_landmarks", "ekf_batch_fuse_landmarks",
    "ekf_update_matched", "ekf_batch_update_matched", "ekf_joint_compat", "ekf_batch_joint_compat", "ekf_update_matched_iter", "ekf_batch_update_matched_iter",
    "ekf_update_fixes", "ekf_batch_update_fixes", "ekf_fix_compat", "ekf_batch_fix_compat",
    "ekf_update_polar", "ekf_batch_update_polar", "ekf_polar_compat", "ekf_batch_polar_compat",
    "ekf_gate_candidates", "ekf_batch_gate_candidates",
    "ekf_associate_joint", "ekf_batch_associate_joint", "ekf_joint_gates",
    "ekf_add_landmarks", "ekf_batch_add_landmarks", "ekf_update_joint", "ekf_batch_update_joint",
    "ekf_locate_scan", "ekf_batch_locate_scan", "ekf_reset_pose", "ekf_batch_reset_pose", "ekf_relocalize", "ekf_batch_relocalize",
]


class EkfParams(ctypes.Structure):
    _fields_ = [("sigma_v", ctypes.c_double), ("sigma_w", ctypes.c_double), ("gamma_max", ctypes.c_double),
                ("gamma_min", ctypes.c_double), ("cond_limit", ctypes.c_double), ("max_pending", ctypes.c_int),
                ("log_capacity", ctypes.c_int), ("overlap", ctypes.c_int)]


class EkfDecision(ctypes.Structure):
    _fields_ = [("decision", ctypes.c_int), ("matched", ctypes.c_int), ("mahal", ctypes.c_double)]


class EkfStats(ctypes.Structure):
    _fields_ = [("nis_sum", ctypes.c_double), ("nees_sum", ctypes.c_double), ("nis_count", ctypes.c_longlong),
                ("nees_count", ctypes.c_longlong), ("n_new", ctypes.c_longlong), ("n_old", ctypes.c_longlong),
                ("n_ignore", ctypes.c_longlong)]


class EkfJoint(ctypes.Structure):
    _fields_ = [("n_landmarks", ctypes.c_int), ("info", ctypes.c_int), ("nees_map", ctypes.c_double), ("nees_joint", ctypes.c_double),
                ("logdet_map", ctypes.c_double), ("logdet_joint", ctypes.c_double), ("min_pivot", ctypes.c_double),
                ("max_pivot", ctypes.c_double), ("cov_robot_given_map", ctypes.c_double * 9)]


JOINT_DTYPE = np.dtype([("n_landmarks", "i4"), ("info", "i4"), ("nees_map", "f8"), ("nees_joint", "f8"), ("logdet_map", "f8"),
                        ("logdet_joint", "f8"), ("min_pivot", "f8"), ("max_pivot", "f8"), ("cov_robot_given_map", "f8", (3, 3))])
assert JOINT_DTYPE.itemsize == ctypes.sizeof(EkfJoint)



class EkfDupPair(ctypes.Structure):
    _fields_ = [("i", ctypes.c_int), ("j", ctypes.c_int), ("d2", ctypes.c_double)]


DUP_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("d2", "f8")])
assert DUP_DTYPE.itemsize == ctypes.sizeof(EkfDupPair) == 16

class EkfCandidate(ctypes.Structure):
    _fields_ = [("meas", ctypes.c_int), ("landmark", ctypes.c_int), ("d2", ctypes.c_double)]


CAND_DTYPE = np.dtype([("meas", "i4"), ("landmark", "i4"), ("d2", "f8")])
assert CAND_DTYPE.itemsize == ctypes.sizeof(EkfCandidate) == 16


class EkfAssoc(ctypes.Structure):
    _fields_ = [("nodes", ctypes.c_longlong), ("d2", ctypes.c_double), ("n_paired", ctypes.c_int), ("complete", ctypes.c_int),
                ("n_candidates", ctypes.c_int), ("n_dropped", ctypes.c_int)]


ASSOC_DTYPE = np.dtype([("nodes", "i8"), ("d2", "f8"), ("n_paired", "i4"), ("complete", "i4"), ("n_candidates", "i4"), ("n_dropped", "i4")])
assert ASSOC_DTYPE.itemsize == ctypes.sizeof(EkfAssoc) == 32
ASSOC_MAX_MEAS, ASSOC_MAX_BRANCH, ASSOC_MAX_NODES = 32, 16, 1 << 20
DECISION_DTYPE = np.dtype([("decision", "i4"), ("matched", "i4"), ("mahal", "f8")])
assert DECISION_DTYPE.itemsize == ctypes.sizeof(EkfDecision) == 16



class EkfLocateHyp(ctypes.Structure):
    _fields_ = [("pose", ctypes.c_double * 3), ("pair_pose", ctypes.c_double * 3), ("ssr", ctypes.c_double), ("rms", ctypes.c_double),
                ("inliers", ctypes.c_int), ("meas_a", ctypes.c_int), ("meas_b", ctypes.c_int), ("lm_i", ctypes.c_int), ("lm_j", ctypes.c_int),
                ("reserved", ctypes.c_int)]


LOCATE_DTYPE = np.dtype([("pose", "f8", (3,)), ("pair_pose", "f8", (3,)), ("ssr", "f8"), ("rms", "f8"), ("inliers", "i4"), ("meas_a", "i4"),
                         ("meas_b", "i4"), ("lm_i", "i4"), ("lm_j", "i4"), ("reserved", "i4")])
assert LOCATE_DTYPE.itemsize == ctypes.sizeof(EkfLocateHyp) == 88
LOCATE_MAX_MEAS, LOCATE_MAX_BASE, LOCATE_MAX_OUT, LOCATE_MAX_CAND = 32, 16, 64, 1 << 22
ITER_MAX = 16  # EKF_ITER_MAX: the most factorisations of a round of update_matched_iter

_STATS_DTYPE = np.dtype([(n, "f8" if t is ctypes.c_double else "i8") for n, t in EkfStats._fields_])


class EkfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libekfslam_hip error %d: %s" % (code, msg))
        self.code = code


_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_up = ctypes.POINTER(ctypes.c_ubyte)
_H = ctypes.c_void_p
_lib = None


def load():
    """Load the HIP library.  Raises if it has not been built: the product path has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    L.ekf_last_error.restype = ctypes.c_char_p
    L.ekf_default_params.argtypes = [ctypes.POINTER(EkfParams)]
    L.ekf_default_params.restype = None
    L.ekf_create.argtypes = [ctypes.POINTER(_H), ctypes.c_int, ctypes.c_int, ctypes.POINTER(EkfParams)]
    L.ekf_batch_create.argtypes = [ctypes.POINTER(_H), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(EkfParams)]
    L.ekf_destroy.argtypes = [_H]
    L.ekf_reserve.argtypes = [_H, ctypes.c_int]
    L.ekf_batch_size.argtypes = [_H]
    L.ekf_capacity.argtypes = [_H]
    L.ekf_window.argtypes = [_H]
    L.ekf_overlap.argtypes = [_H]
    L.ekf_fused_pass.argtypes = [_H]
    L.ekf_propagate.argtypes = [_H, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    L.ekf_propagate_q.argtypes = [_H, ctypes.c_double, ctypes.c_double, _dp, ctypes.c_double]
    L.ekf_update.argtypes = [_H, _dp, _dp, ctypes.c_int, ctypes.POINTER(EkfDecision)]
    L.ekf_update_compass.argtypes = [_H, ctypes.c_double, ctypes.c_double]
    L.ekf_get_pose.argtypes = [_H, _dp]
    L.ekf_num_landmarks.argtypes = [_H]
    L.ekf_get_robot_cov.argtypes = [_H, _dp]
    L.ekf_get_x.argtypes = [_H, ctypes.c_int, _dp, ctypes.c_int]
    L.ekf_batch_propagate.argtypes = [_H, _dp, _dp, _dp]
    L.ekf_batch_propagate_q.argtypes = [_H, _dp, _dp, _dp, _dp]
    L.ekf_batch_update.argtypes = [_H, _dp, _dp, _up, ctypes.c_int, ctypes.POINTER(EkfDecision)]
    L.ekf_batch_update_compass.argtypes = [_H, _dp, _dp, _up]
    L.ekf_batch_get_pose.argtypes = [_H, _dp]
    L.ekf_batch_num_landmarks.argtypes = [_H, _ip]
    L.ekf_get_state.argtypes = [_H, ctypes.c_int, _dp, _dp, ctypes.c_int]
    L.ekf_set_state.argtypes = [_H, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_int]
    L.ekf_broadcast_state.argtypes = [_H]
    L.ekf_remove_landmarks.argtypes = [_H, ctypes.c_int, _up, ctypes.c_int]
    L.ekf_batch_remove_landmarks.argtypes = [_H, _up, ctypes.c_int, _ip]
    L.ekf_get_landmark_covs.argtypes = [_H, ctypes.c_int, _dp, ctypes.c_int]
    L.ekf_transform_frame.argtypes = [_H, ctypes.c_int, _dp]
    L.ekf_batch_transform_frame.argtypes = [_H, _dp]
    L.ekf_anchor_at_robot.argtypes = [_H, ctypes.c_int]
    L.ekf_batch_anchor_at_robot.argtypes = [_H]
    L.ekf_join_map.argtypes = [_H, ctypes.c_int, _H, ctypes.c_int]
    L.ekf_batch_join_map.argtypes = [_H, _H]
    L.ekf_extract_map.argtypes = [_H, ctypes.c_int, _H, ctypes.c_int, _ip, ctypes.c_int]
    L.ekf_batch_extract_map.argtypes = [_H, _H, _ip, ctypes.c_int, _ip, _ip]
    L.ekf_get_submap.argtypes = [_H, ctypes.c_int, _ip, ctypes.c_int, _dp, _dp, ctypes.c_int]
    L.ekf_joint_consistency.argtypes = [_H, ctypes.c_int, _dp, ctypes.POINTER(EkfJoint)]
    L.ekf_batch_joint_consistency.argtypes = [_H, _dp, ctypes.c_int, ctypes.POINTER(EkfJoint)]
    L.ekf_debug_joint_factor.argtypes = [_H, ctypes.c_int, _dp, ctypes.c_int]
    L.ekf_find_duplicates.argtypes = [_H, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.POINTER(EkfDupPair), ctypes.c_int, _ip]
    L.ekf_batch_find_duplicates.argtypes = [_H, ctypes.c_double, ctypes.c_double, _ip, ctypes.POINTER(EkfDupPair), ctypes.c_int, _ip, _ip]
    L.ekf_fuse_landmarks.argtypes = [_H, ctypes.c_int, ctypes.POINTER(EkfDupPair), ctypes.c_int, ctypes.c_double, _ip]
    L.ekf_batch_fuse_landmarks.argtypes = [_H, ctypes.POINTER(EkfDupPair), ctypes.c_int, _ip, ctypes.c_double, _ip, _ip]
    L.ekf_update_matched.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, ctypes.c_int, _ip, _dp]
    L.ekf_batch_update_matched.argtypes = [_H, _dp, _dp, _ip, ctypes.c_int, _ip, _dp]
    L.ekf_joint_compat.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, ctypes.c_int, _dp]
    L.ekf_update_matched_iter.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, ctypes.c_int, ctypes.c_int, ctypes.c_double, _ip, _dp, _ip, _dp]
    L.ekf_batch_update_matched_iter.argtypes = [_H, _dp, _dp, _ip, ctypes.c_int, ctypes.c_int, ctypes.c_double, _ip, _dp, _ip, _dp]
    L.ekf_batch_joint_compat.argtypes = [_H, _dp, _dp, _ip, ctypes.c_int, _dp]
    L.ekf_update_fixes.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, ctypes.c_int, _ip, _dp]
    L.ekf_batch_update_fixes.argtypes = [_H, _dp, _dp, _ip, ctypes.c_int, _ip, _dp]
    L.ekf_fix_compat.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, ctypes.c_int, _dp]
    L.ekf_batch_fix_compat.argtypes = [_H, _dp, _dp, _ip, ctypes.c_int, _dp]
    L.ekf_update_polar.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, _ip, ctypes.c_int, _ip, _dp]
    L.ekf_batch_update_polar.argtypes = [_H, _dp, _dp, _ip, _ip, ctypes.c_int, _ip, _dp]
    L.ekf_polar_compat.argtypes = [_H, ctypes.c_int, _dp, _dp, _ip, _ip, ctypes.c_int, _dp]
    L.ekf_batch_polar_compat.argtypes = [_H, _dp, _dp, _ip, _ip, ctypes.c_int, _dp]
    L.ekf_gate_candidates.argtypes = [_H, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_double, ctypes.POINTER(EkfCandidate), ctypes.c_int,
                                      ctypes.POINTER(EkfDecision), _ip]
    L.ekf_batch_gate_candidates.argtypes = [_H, _dp, _dp, _up, ctypes.c_int, ctypes.c_double, ctypes.POINTER(EkfCandidate), ctypes.c_int, _ip,
                                            ctypes.POINTER(EkfDecision), _ip]
    L.ekf_associate_joint.argtypes = [_H, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_double, _dp, ctypes.c_int, ctypes.c_longlong, _ip, _dp,
                                      ctypes.POINTER(EkfDecision), _ip, ctypes.POINTER(EkfAssoc)]
    L.ekf_batch_associate_joint.argtypes = [_H, _dp, _dp, _up, ctypes.c_int, ctypes.c_double, _dp, ctypes.c_int, ctypes.c_longlong, _ip, _dp,
                                            ctypes.POINTER(EkfDecision), _ip, ctypes.POINTER(EkfAssoc)]
    L.ekf_joint_gates.argtypes = [ctypes.c_double, _dp]
    L.ekf_add_landmarks.argtypes = [_H, ctypes.c_int, _dp, _dp, _up, ctypes.c_int, _ip]
    L.ekf_batch_add_landmarks.argtypes = [_H, _dp, _dp, _up, ctypes.c_int, _ip, _ip]
    L.ekf_update_joint.argtypes = [_H, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_double, _dp, ctypes.c_int, ctypes.c_longlong, _ip, _ip, _dp,
                                   ctypes.POINTER(EkfAssoc)]
    L.ekf_batch_update_joint.argtypes = [_H, _dp, _dp, _up, ctypes.c_int, ctypes.c_double, _dp, ctypes.c_int, ctypes.c_longlong, _ip, _ip, _dp,
                                         ctypes.POINTER(EkfAssoc), _ip]
    _hp, _llp = ctypes.POINTER(EkfLocateHyp), ctypes.POINTER(ctypes.c_longlong)
    L.ekf_locate_scan.argtypes = [_H, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, _hp, _ip, _llp]
    L.ekf_batch_locate_scan.argtypes = [_H, _dp, _up, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, _hp, _ip, _ip, _llp]
    L.ekf_reset_pose.argtypes = [_H, ctypes.c_int, _dp, _dp]
    L.ekf_batch_reset_pose.argtypes = [_H, _dp, _dp]
    L.ekf_relocalize.argtypes = [_H, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, _dp, _hp, _ip, _dp]
    L.ekf_batch_relocalize.argtypes = [_H, _dp, _dp, _up, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, _dp, _hp, _ip, _dp, _ip]
    L.ekf_script_load.argtypes =[_H, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _up, _dp]
    L.ekf_script_run.argtypes = [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ekf_sync.argtypes = [_H]
    L.ekf_flush.argtypes = [_H]
    L.ekf_close_window.argtypes = [_H]
    L.ekf_timer_start.argtypes = [_H]
    L.ekf_timer_stop.argtypes = [_H, _dp]
    L.ekf_flush_profile.argtypes = [_H, ctypes.c_int]
    L.ekf_flush_profile_read.argtypes = [_H, ctypes.POINTER(ctypes.c_longlong), _dp]
    L.ekf_get_decisions.argtypes = [_H, ctypes.c_int, ctypes.POINTER(EkfDecision), ctypes.c_int]
    L.ekf_get_stats.argtypes = [_H, ctypes.POINTER(EkfStats)]
    L.ekf_reset_stats.argtypes = [_H]
    L.ekf_stats_means_device.argtypes = [_H, ctypes.c_void_p]
    L.ekf_record_truth.argtypes = [_H, _dp]
    L.ekf_stream.argtypes = [_H]
    L.ekf_stream.restype = ctypes.c_void_p
    L.ekf_device_bytes.argtypes = [_H]
    L.ekf_device_bytes.restype = ctypes.c_size_t
    _lib = L
    return L


def _chk(rc):
    if rc < 0:
        raise EkfError(rc, load().ekf_last_error().decode())
    return rc


def _p(a):
    return a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _rect_lists(z, R, a):
    """(z, Rc, ids, n) as the C list calls take them, from the ids a [..][n] and arrays with two values of z and a 2x2 R per id."""
    Rc = _f64(np.swapaxes(R.reshape(a.shape + (2, 2)), -1, -2).reshape(a.shape + (4,)))  # column-major blocks
    return _f64(z.reshape(a.shape + (2,))), Rc, np.ascontiguousarray(a, dtype=np.int32), a.shape[-1]


def polar_to_cartesian(z, R):
    """Range-bearing measurements as the Cartesian calls take them (add_landmarks, gate_candidates, locate_scan, update_matched):
    z [..][2] = (range, bearing in the robot frame), R [..][2][2] over (range, bearing).  Returns (z_xy, R_xy): the robot-frame offset
    (r cos b, r sin b) and J R J^T with J = [[cos b, -r sin b], [sin b, r cos b]], the noise linearised at the measurement.  Host
    arithmetic; update_polar takes the polar form itself, without this linearisation."""
    z, R = np.asarray(z, dtype=np.float64), np.asarray(R, dtype=np.float64)
    if z.shape[-1:] != (2,) or R.shape != z.shape[:-1] + (2, 2):
        raise ValueError("z must be [..][2] and R [..][2][2]")
    r, b = z[..., 0], z[..., 1]
    c, s = np.cos(b), np.sin(b)
    J = np.stack([np.stack([c, -r * s], axis=-1), np.stack([s, r * c], axis=-1)], axis=-2)
    C = J @ R @ np.swapaxes(J, -1, -2)
    return np.stack([r * c, r * s], axis=-1), 0.5 * (C + np.swapaxes(C, -1, -2))  # (symmetric to the bit)


def _greedy_matching(pairs, n_landmarks):
    """The pairs (as DUP_DTYPE) and the positions of the accepted ones, in the order they were accepted: greedy one-to-one
    matching by ascending d2, ties by (i, j)."""
    pairs = np.asarray(pairs, dtype=DUP_DTYPE).reshape(-1)
    n = int(n_landmarks)
    matched = np.zeros(n, dtype=bool)
    accepted = []
    for k in np.lexsort((pairs["j"], pairs["i"], pairs["d2"])):
        i, j = int(pairs["i"][k]), int(pairs["j"][k])
        if not (0 <= i < j < n):
            raise ValueError("pair (%d, %d) does not name two landmarks i < j of %d" % (i, j, n))
        if matched[i] or matched[j]:
            continue
        matched[i] = matched[j] = True
        accepted.append(int(k))
    return pairs, np.asarray(accepted, dtype=np.intp)


def duplicate_keep_mask(pairs, n_landmarks):
    """A keep mask for remove_landmarks from a list of duplicate pairs (find_duplicates): greedy one-to-one matching by ascending d2,
    ties by (i, j); a pair is accepted when neither of its landmarks is matched already, and the later landmark j of an accepted
    pair goes (keep[j] = False).  In a chain i-j-k of mutual candidates only the closest link is accepted: search again after the
    removal when several copies of one point are expected."""
    pairs, accepted = _greedy_matching(pairs, n_landmarks)
    keep = np.ones(int(n_landmarks), dtype=bool)
    keep[pairs["j"][accepted]] = False
    return keep


def duplicate_matching(pairs, n_landmarks):
    """The accepted pairs of duplicate_keep_mask's greedy matching as a DUP_DTYPE array ordered by (i, j): every landmark in at most
    one pair, which is what fuse_landmarks takes; its j are the landmarks duplicate_keep_mask drops."""
    pairs, accepted = _greedy_matching(pairs, n_landmarks)
    out = pairs[accepted].copy()
    return out[np.lexsort((out["j"], out["i"]))]


def candidate_matching(cands, n_z):
    """The ids update_matched takes from a candidate list (gate_candidates): greedy one-to-one matching by ascending d2, ties by
    (meas, landmark); a candidate is accepted when neither its measurement nor its landmark is matched already.  Returns an int32
    [n_z] array, -1 for a measurement without a match.  The counterpart of duplicate_matching."""
    cands = np.asarray(cands, dtype=CAND_DTYPE).reshape(-1)
    n_z = int(n_z)
    if n_z < 0:
        raise ValueError("n_z must not be negative")
    ids = np.full(n_z, -1, dtype=np.int32)
    taken = set()
    for k in np.lexsort((cands["landmark"], cands["meas"], cands["d2"])):
        m, l = int(cands["meas"][k]), int(cands["landmark"][k])
        if not (0 <= m < n_z) or l < 0:
            raise ValueError("candidate (%d, %d) does not name one of %d measurements and a landmark" % (m, l, n_z))
        if ids[m] >= 0 or l in taken:
            continue
        ids[m] = l
        taken.add(l)
    return ids


def same_pose(a, b, tol, reach):
    """Two poses (x, y, heading) are the same pose for a search of inlier radius tol: positions within 2 tol, headings (their
    difference wrapped into [-pi, pi]) within 2 tol / reach, reach = the largest |z_k| of the scan (<= 0: the heading says nothing).
    The rule ekf_relocalize's acceptance applies (plan_locate_same_pose)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.hypot(a[0] - b[0], a[1] - b[1]) <= 2.0 * tol:
        return False
    if not reach > 0.0:
        return True
    return bool(abs(np.remainder(a[2] - b[2] + np.pi, 2.0 * np.pi) - np.pi) <= 2.0 * tol / reach)


def distinct_poses(hyps, tol, reach):
    """The hypotheses of locate_scan with the repeats of one pose merged: the same true pose recurs once per base pair and landmark
    pair that hits it.  In list order, a hypothesis joins the first kept one whose fitted pose is the same pose (same_pose: within
    2 tol in position and 2 tol / reach in heading), else it is kept.  Returns (kept, group): the kept records (a LOCATE_DTYPE array,
    best first, as the list is) and for every input hypothesis the position of its pose in `kept`."""
    hyps = np.asarray(hyps, dtype=LOCATE_DTYPE).reshape(-1)
    tol, reach = float(tol), float(reach)
    if not tol > 0.0:
        raise ValueError("tol must be positive")
    keep, group = [], np.empty(len(hyps), dtype=np.int64)
    for k in range(len(hyps)):
        for g, first in enumerate(keep):
            if same_pose(hyps["pose"][k], hyps["pose"][first], tol, reach):
                group[k] = g
                break
        else:
            group[k] = len(keep)
            keep.append(k)
    return hyps[keep].copy(), group


def joint_gates(confidence=0.99):
    """The joint gates associate_joint uses by default (ekf_joint_gates): [q - 1] is the `confidence` quantile of chi-square with
    2 q degrees of freedom, q = 1 .. 32."""
    confidence = float(confidence)
    if not 0.0 < confidence < 1.0:
        raise ValueError("confidence must lie inside (0, 1)")
    out = np.empty(ASSOC_MAX_MEAS)
    _chk(load().ekf_joint_gates(confidence, _p(out)))
    return out


def _pair_buffer(pairs):
    """A pair list (DUP_DTYPE array, or anything with rows (i, j)) as a contiguous DUP_DTYPE array."""
    a = np.asarray(pairs)
    if a.dtype != DUP_DTYPE:
        ij = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) if a.size else np.zeros((0, 2), dtype=np.int64)
        if ij.size and (np.abs(ij) > 2**31 - 1).any():
            raise ValueError("landmark numbers out of range")
        a = np.zeros(ij.shape[0], dtype=DUP_DTYPE)
        a["i"], a["j"] = ij[:, 0], ij[:, 1]
    return np.ascontiguousarray(a.reshape(-1))


def default_params(**kw):
    p = EkfParams()
    load().ekf_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class FilterBatch:
    """`batch` independent filters on one MI355X behind one handle (ekf_batch_create)."""

    def __init__(self, batch, capacity_landmarks, device=0, **params):
        self.L = load()
        self.h = _H()
        p = default_params(**params)
        _chk(self.L.ekf_batch_create(ctypes.byref(self.h), batch, capacity_landmarks, device, ctypes.byref(p)))
        self.batch = batch
        self.capacity = capacity_landmarks
        self.window = int(self.L.ekf_window(self.h))  # effective max_pending
        self.overlap = bool(self.L.ekf_overlap(self.h))
        self.fused_pass = bool(self.L.ekf_fused_pass(self.h))

    def reserve(self, capacity_landmarks):
        """Grow the landmark capacity (ekf_reserve: the state moves to larger device buffers, the handle stays)."""
        _chk(self.L.ekf_reserve(self.h, int(capacity_landmarks)))
        self.capacity = int(self.L.ekf_capacity(self.h))
        self.window = int(self.L.ekf_window(self.h))
        self.overlap = bool(self.L.ekf_overlap(self.h))
        self.fused_pass = bool(self.L.ekf_fused_pass(self.h))

    def close(self):
        if self.h:
            self.L.ekf_destroy(self.h)
            self.h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batched operations ------------------------------------------------------------------
    def propagate(self, v, w, dt):
        v, w, dt = (_f64(np.broadcast_to(a, (self.batch,))) for a in (v, w, dt))
        _chk(self.L.ekf_batch_propagate(self.h, _p(v), _p(w), _p(dt)))

    def propagate_q(self, v, w, Q, dt):
        v, w, dt = (_f64(np.broadcast_to(a, (self.batch,))) for a in (v, w, dt))
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim == 2:
            Q = np.broadcast_to(Q, (self.batch, 2, 2))
        Qc = _f64(np.transpose(Q, (0, 2, 1)).reshape(self.batch, 4))  # column-major blocks
        _chk(self.L.ekf_batch_propagate_q(self.h, _p(v), _p(w), _p(Qc), _p(dt)))

    def update(self, z, R, valid=None, want_decisions=True):
        """z (batch, n_z, 2); R (batch, n_z, 2, 2) matrices.  Returns decisions (batch, n_z) list of tuples."""
        z = _f64(z).reshape(self.batch, -1, 2)
        n_z = z.shape[1]
        R = np.asarray(R, dtype=np.float64).reshape(self.batch, n_z, 2, 2)
        Rc = _f64(np.transpose(R, (0, 1, 3, 2)).reshape(self.batch, n_z, 4))
        vp = None
        if valid is not None:
            valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(self.batch, n_z)
            vp = valid.ctypes.data_as(_up)
        dec = (EkfDecision * (self.batch * n_z))() if want_decisions else None
        _chk(self.L.ekf_batch_update(self.h, _p(z), _p(Rc), vp, n_z, dec))
        if not want_decisions:
            return None
        return [[(dec[b * n_z + j].decision, dec[b * n_z + j].matched, dec[b * n_z + j].mahal) for j in range(n_z)]
                for b in range(self.batch)]

    def update_compass(self, z, R, valid=None):
        z, R = (_f64(np.broadcast_to(a, (self.batch,))) for a in (z, R))
        vp = None
        if valid is not None:
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
            vp = valid.ctypes.data_as(_up)
        _chk(self.L.ekf_batch_update_compass(self.h, _p(z), _p(R), vp))

    def poses(self):
        out = np.empty((self.batch, 3))
        _chk(self.L.ekf_batch_get_pose(self.h, _p(out)))
        return out

    def robot_cov(self):
        out = np.empty((3, 3))
        _chk(self.L.ekf_get_robot_cov(self.h, _p(out)))
        return out

    def get_x(self, index=0):
        n = _chk(self.L.ekf_get_x(self.h, index, _p(np.empty(1)), 0))
        x = np.empty(n)
        _chk(self.L.ekf_get_x(self.h, index, _p(x), n))
        return x

    def num_landmarks(self):
        out = np.empty(self.batch, dtype=np.int32)
        _chk(self.L.ekf_batch_num_landmarks(self.h, out.ctypes.data_as(_ip)))
        return out

    def get_state(self, index=0):
        n = _chk(self.L.ekf_get_state(self.h, index, None, None, 0))
        x = np.empty(n)
        P = np.empty((n, n))
        _chk(self.L.ekf_get_state(self.h, index, _p(x), _p(P), n))
        return x, P

    def set_state(self, x, P, index=0):
        x = _f64(x)
        P = _f64(P)
        _chk(self.L.ekf_set_state(self.h, index, _p(x), _p(P), P.shape[1], x.size))

    def broadcast_state(self):
        _chk(self.L.ekf_broadcast_state(self.h))

    # -- map management ------------------------------------------------------------------------
    def remove_landmarks(self, keep, index=None):
        """Marginalise landmarks out on the device (ekf_remove_landmarks): keep[l] true keeps landmark l (state rows 3+2l, 4+2l).
        index=None: keep is [batch][N], one pass over every filter (ekf_batch_remove_landmarks); returns the new counts (batch,).
        With an index: keep is [N] for that filter; returns its new count."""
        if index is None:
            k = np.ascontiguousarray(keep, dtype=bool).astype(np.uint8)
            if k.ndim == 1 and self.batch == 1:
                k = k.reshape(1, -1)
            if k.ndim != 2 or k.shape[0] != self.batch:
                raise ValueError("keep must be [batch][N]")
            n_out = np.empty(self.batch, dtype=np.int32)
            _chk(self.L.ekf_batch_remove_landmarks(self.h, k.ctypes.data_as(_up), k.shape[1], n_out.ctypes.data_as(_ip)))
            return n_out
        k = np.ascontiguousarray(keep, dtype=bool).astype(np.uint8).reshape(-1)
        return _chk(self.L.ekf_remove_landmarks(self.h, int(index), k.ctypes.data_as(_up), k.size))

    def landmark_covs(self, index=0):
        """The 2x2 covariance of every landmark of filter `index` as (N, 3) rows (xx, xy, yy) (ekf_get_landmark_covs: the always-
        current diagonal blocks; no dense pass, the open window stays open)."""
        out = np.empty((max(int(self.capacity), 1), 3))
        n = _chk(self.L.ekf_get_landmark_covs(self.h, int(index), _p(out), int(self.capacity)))
        return out[:n].copy()

    def transform_frame(self, frame, index=None):
        """A known rigid transform of the whole estimate on the device (ekf_transform_frame): frame = (t_x, t_y, theta), the pose of
        the new frame's origin in the current frame.  index=None: frame is [batch][3], one frame per filter in one pass
        (ekf_batch_transform_frame).  The heading is not wrapped; compass readings shift by -theta."""
        if index is None:
            fr = _f64(frame)
            if fr.ndim == 1 and self.batch == 1:
                fr = fr.reshape(1, 3)
            if fr.shape != (self.batch, 3):
                raise ValueError("frame must be [batch][3]")
            _chk(self.L.ekf_batch_transform_frame(self.h, _p(fr)))
            return
        fr = _f64(frame).reshape(-1)
        if fr.size != 3:
            raise ValueError("frame must be (t_x, t_y, theta)")
        _chk(self.L.ekf_transform_frame(self.h, int(index), _p(fr)))

    def anchor_at_robot(self, index=None):
        """Re-express the map relative to the robot's estimated pose on the device (ekf_anchor_at_robot; index=None: every filter,
        ekf_batch_anchor_at_robot): the pose becomes exactly (0, 0, 0) with P_RR = 0, its uncertainty moves into the landmarks."""
        if index is None:
            _chk(self.L.ekf_batch_anchor_at_robot(self.h))
        else:
            _chk(self.L.ekf_anchor_at_robot(self.h, int(index)))

    def join_map(self, src, index=0, src_index=0):
        """Append the landmarks of filter src_index of `src` (a FilterBatch; may be this one when the indices differ) behind those of
        filter `index` on the device (ekf_join_map).  src's frame origin must be this filter's current estimated pose and the two
        estimates independent; duplicates are not fused here (find_duplicates, fuse_landmarks).  Returns the new landmark count; `src` is only read."""
        return _chk(self.L.ekf_join_map(self.h, int(index), src.h, int(src_index)))

    def batch_join_map(self, src):
        """Filter b of `src` into filter b of this batch for every b (ekf_batch_join_map; equal batch sizes, another handle)."""
        _chk(self.L.ekf_batch_join_map(self.h, src.h))

    # -- submap extraction ---------------------------------------------------------------------
    def extract_map(self, src, ids=None, index=0, src_index=0):
        """Replace filter `index` with the marginal of filter src_index of `src` (a FilterBatch; may be this one when the indices
        differ) over the robot and the landmarks `ids`, on the device (ekf_extract_map): landmark k becomes src's landmark ids[k],
        any order, no id twice; ids=None: every landmark, a copy or fork.  The bits of src.get_state() indexed by the selection.
        Returns the new landmark count; `src` is only read.  The result is NOT independent of src: never join it back."""
        if ids is None:
            return _chk(self.L.ekf_extract_map(self.h, int(index), src.h, int(src_index), None, 0))
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        return _chk(self.L.ekf_extract_map(self.h, int(index), src.h, int(src_index), a.ctypes.data_as(_ip), a.size))

    def batch_extract_map(self, src, ids=None, counts=None):
        """Filter b of `src` into filter b of this batch for every b (ekf_batch_extract_map; equal batch sizes, another handle).
        ids: [batch][ld] landmark lists with counts[b] entries each (counts=None: all ld), or a sequence of per-filter lists, or
        None: every landmark of every filter.  Returns the new landmark counts (batch,)."""
        n_out = np.empty(self.batch, dtype=np.int32)
        if ids is None:
            _chk(self.L.ekf_batch_extract_map(self.h, src.h, None, 0, None, n_out.ctypes.data_as(_ip)))
            return n_out
        if counts is None and not isinstance(ids, np.ndarray):
            rows = [np.asarray(r, dtype=np.int32).reshape(-1) for r in ids]
            counts = [r.size for r in rows]
            tab = np.zeros((len(rows), max(counts + [1])), dtype=np.int32)
            for b, r in enumerate(rows):
                tab[b, :r.size] = r
            ids = tab
        a = np.ascontiguousarray(ids, dtype=np.int32)
        if a.ndim != 2 or a.shape[0] != self.batch:
            raise ValueError("ids must be [batch][ld]")
        c = np.full(self.batch, a.shape[1], dtype=np.int32) if counts is None else np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if c.size != self.batch:
            raise ValueError("counts must be [batch]")
        _chk(self.L.ekf_batch_extract_map(self.h, src.h, a.ctypes.data_as(_ip), a.shape[1], c.ctypes.data_as(_ip), n_out.ctypes.data_as(_ip)))
        return n_out

    def get_submap(self, ids, index=0):
        """(x, P) of the robot and the landmarks `ids` of filter `index` (ekf_get_submap): get_state()[sel] bit for bit, gathered on
        the device into a dense buffer of that size alone.  The filter is left as get_state leaves it."""
        a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        ip = a.ctypes.data_as(_ip) if a.size else None
        n = _chk(self.L.ekf_get_submap(self.h, int(index), ip, a.size, None, None, 0))
        x = np.empty(n)
        P = np.empty((n, n))
        _chk(self.L.ekf_get_submap(self.h, int(index), ip, a.size, _p(x), _p(P), n))
        return x, P

    # -- map assessment ------------------------------------------------------------------------
    def joint_consistency(self, x_true=None, index=None):
        """Whole-state consistency on the device (ekf_joint_consistency): joint and map NEES against x_true, log det P, the pivots
        of the factorisation of P_LL and the pose covariance conditioned on the map, as a structured array (JOINT_DTYPE) with one row
        per filter.  index=None: every filter in one launch sequence, x_true [batch][>= largest state] (or [n] for a batch of one);
        with an index: that filter alone, x_true [n].  x_true=None: a health check, the NEES fields are NaN.  The filter is only
        read; `info` != 0 is a result (see include/ekfslam_c.h), not an exception."""
        if index is None:
            buf = (EkfJoint * self.batch)()
            xt, ld = None, 0
            if x_true is not None:
                t = _f64(x_true)
                if t.ndim == 1 and self.batch == 1:
                    t = t.reshape(1, -1)
                if t.ndim != 2 or t.shape[0] != self.batch:
                    raise ValueError("x_true must be [batch][n]")
                xt, ld = _p(t), t.shape[1]
            _chk(self.L.ekf_batch_joint_consistency(self.h, xt, ld, buf))
            return np.frombuffer(buf, dtype=JOINT_DTYPE, count=self.batch)  # (the array keeps the buffer alive)
        buf = (EkfJoint * 1)()
        xt = None
        if x_true is not None:
            t = _f64(x_true).reshape(-1)
            n = _chk(self.L.ekf_get_state(self.h, int(index), None, None, 0)) if 0 <= int(index) < self.batch else 0
            if t.size < n:
                raise ValueError("x_true is shorter than the filter's state (%d < %d)" % (t.size, n))
            xt = _p(t)
        _chk(self.L.ekf_joint_consistency(self.h, int(index), xt, buf))
        return np.frombuffer(buf, dtype=JOINT_DTYPE, count=1)

    def find_duplicates(self, gate=9.21, max_dist=None, split=0, index=0, max_pairs=4096):
        """Duplicate landmarks on the device (ekf_find_duplicates): the pairs i < j whose difference passes the gate
        d^T (P_ii + P_jj - P_ij - P_ij^T)^-1 d <= gate (9.21: 99 % of chi-square with 2 dof), cross covariance included.  max_dist: only
        pairs at most that far apart (None: no bound); split = Ng: only pairs i < Ng <= j, old x new after a join_map that appended
        behind Ng landmarks.  Returns (pairs, n_found, n_degenerate): a DUP_DTYPE array ordered by (i, j) with the first
        min(n_found, max_pairs) pairs, the number of pairs that pass, and the number of considered pairs whose S is not positive
        definite (never listed).  index=None: every filter in one launch sequence (ekf_batch_find_duplicates), split an int or
        [batch]; returns a list of such triples, one per filter.  The filter is only read; duplicate_keep_mask turns the list into
        the mask remove_landmarks takes."""
        md = 0.0 if max_dist is None else float(max_dist)
        max_pairs = int(max_pairs)
        if max_pairs < 0:
            raise ValueError("max_pairs must not be negative")
        if index is None:
            sp = np.ascontiguousarray(np.broadcast_to(np.asarray(split, dtype=np.int32), (self.batch,)))
            buf = (EkfDupPair * max(self.batch * max_pairs, 1))()
            found, degen = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
            _chk(self.L.ekf_batch_find_duplicates(self.h, float(gate), md, sp.ctypes.data_as(_ip), buf if max_pairs else None, max_pairs,
                                                  found.ctypes.data_as(_ip), degen.ctypes.data_as(_ip)))
            rows = np.frombuffer(buf, dtype=DUP_DTYPE, count=self.batch * max_pairs).reshape(self.batch, max_pairs)
            return [(rows[b, :min(int(found[b]), max_pairs)].copy(), int(found[b]), int(degen[b])) for b in range(self.batch)]
        buf = (EkfDupPair * max(max_pairs, 1))()
        degen = ctypes.c_int(0)
        found = _chk(self.L.ekf_find_duplicates(self.h, int(index), float(gate), md, int(split), buf if max_pairs else None, max_pairs, ctypes.byref(degen)))
        return np.frombuffer(buf, dtype=DUP_DTYPE, count=min(found, max_pairs)).copy(), found, degen.value

    def fuse_landmarks(self, pairs, slack=0.0, index=0):
        """Fuse duplicate landmarks on the device (ekf_fuse_landmarks): every pair (i, j), i < j, is declared the same point -- the
        equality constraint L_i = L_j as one update of the whole state (slack: its isotropic variance, 0 = exact) -- and j is
        removed, the kept landmarks renumbered as remove_landmarks does.  pairs: a DUP_DTYPE array (d2 is ignored; take
        duplicate_matching of what find_duplicates returned) or rows (i, j); each landmark in at most one pair.  Returns
        (n_landmarks, n_fused); n_fused < len(pairs) when a round's S was not positive definite (that round and the later ones
        were not applied).  index=None: pairs is a list of one pair array per filter (ekf_batch_fuse_landmarks); returns two
        (batch,) arrays."""
        slack = float(slack)
        if not (np.isfinite(slack) and slack >= 0.0):
            raise ValueError("slack must be finite and not negative")
        if index is None:
            lists = [_pair_buffer(p) for p in pairs]
            if len(lists) != self.batch:
                raise ValueError("pairs must hold one pair array per filter")
            ld = max([a.size for a in lists] + [1])
            buf = np.zeros((self.batch, ld), dtype=DUP_DTYPE)
            cnt = np.zeros(self.batch, dtype=np.int32)
            for b, a in enumerate(lists):
                buf[b, :a.size] = a
                cnt[b] = a.size
            fused, n_out = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
            _chk(self.L.ekf_batch_fuse_landmarks(self.h, buf.ctypes.data_as(ctypes.POINTER(EkfDupPair)), ld, cnt.ctypes.data_as(_ip), slack,
                                                 fused.ctypes.data_as(_ip), n_out.ctypes.data_as(_ip)))
            return n_out, fused
        a = _pair_buffer(pairs)
        fused = ctypes.c_int(0)
        n = _chk(self.L.ekf_fuse_landmarks(self.h, int(index), a.ctypes.data_as(ctypes.POINTER(EkfDupPair)) if a.size else None, a.size, slack,
                                           ctypes.byref(fused)))
        return n, fused.value

    def _list_update(self, lists, index, single, batch):
        """The call of a list update (ekf_update_matched, ekf_update_fixes: `single`, or `batch` with index=None) on the lists of
        _matched_lists / _fix_lists, and its results as update_matched documents them."""
        z, Rc, a, n = lists
        d2 = np.full(a.shape, np.nan)
        ptrs = (_p(z), _p(Rc), a.ctypes.data_as(_ip)) if n else (None, None, None)
        if index is None:
            applied = np.zeros(self.batch, dtype=np.int32)
            _chk(batch(self.h, *ptrs, n, applied.ctypes.data_as(_ip), _p(d2) if n else None))
            return applied, d2
        applied = ctypes.c_int(0)
        cnt = _chk(single(self.h, int(index), *ptrs, n, ctypes.byref(applied), _p(d2) if n else None))
        return cnt, applied.value, d2

    def _matched_lists(self, z, R, ids, index):
        """(z, Rc, ids, n_z) as the C calls take them.  With an index: ids [n_z], z [n_z][2], R [n_z][2][2]; index=None: a leading
        batch axis on all three (ragged lists: pad ids with -1)."""
        lead = (self.batch,) if index is None else ()
        a = np.ascontiguousarray(ids, dtype=np.int64)
        if a.ndim != len(lead) + 1 or a.shape[:len(lead)] != lead:
            raise ValueError("ids must be [batch][n_z]" if lead else "ids must be [n_z]")
        if a.size and (a.min() < -1 or a.max() > np.iinfo(np.int32).max):
            raise ValueError("an id is a landmark number, or -1 to skip the measurement")
        z, R = np.asarray(z, dtype=np.float64), np.asarray(R, dtype=np.float64)
        if z.size != a.size * 2 or R.size != a.size * 4:
            raise ValueError("z must hold [n_z][2] and R [n_z][2][2] values per filter for %d ids" % a.shape[-1])
        return _rect_lists(z, R, a)

    def update_matched(self, z, R, ids, index=0):
        """Apply a scan with the caller's own data association on the device (ekf_update_matched): measurement k is landmark ids[k]
        (-1: skipped), z [n_z][2], R [n_z][2][2].  The measurements run as joint updates in rounds of `window`, each linearised at
        its entry state; gates, counters and the decision log are not involved.  Returns (n_landmarks, n_applied, d2): n_applied <
        the number of non-skipped measurements when a round's S was not positive definite (that round and the later ones were not
        applied), d2[k] the joint Mahalanobis distance of k's round up to and including k (NaN: skipped or not applied).
        index=None: every filter in one launch sequence (ekf_batch_update_matched), ids [batch][n_z]; returns (n_applied (batch,),
        d2 (batch, n_z))."""
        return self._list_update(self._matched_lists(z, R, ids, index), index, self.L.ekf_update_matched, self.L.ekf_batch_update_matched)

    def update_matched_iter(self, z, R, ids, max_iter=8, tol=1e-8, index=0):
        """update_matched with every round iterated (ekf_update_matched_iter): the round is relinearised -- on the pose and its own
        landmarks alone, inside one kernel -- until the largest change of a touched component is at most tol or max_iter (1 ..
        ITER_MAX) factorisations have run; the last linearisation is applied.  Returns what update_matched returns and two arrays
        more, (n_landmarks, n_applied, d2, iters, step): iters[k] int32, the factorisations of k's round (0: skipped or not
        applied), step[k] its last step (NaN: skipped or not applied; above tol: out of iterations); d2 is the prior's joint
        distance, from the first linearisation.  max_iter=1 is update_matched bit for bit.  index=None: (n_applied (batch,), d2,
        iters, step (batch, n_z))."""
        max_iter, tol = int(max_iter), float(tol)
        if not 1 <= max_iter <= ITER_MAX:
            raise ValueError("max_iter must be in 1 .. %d" % ITER_MAX)
        if not (np.isfinite(tol) and tol >= 0.0):
            raise ValueError("tol must be finite and not negative")
        lists = self._matched_lists(z, R, ids, index)
        iters, step = np.zeros(lists[2].shape, dtype=np.int32), np.full(lists[2].shape, np.nan)
        more = (iters.ctypes.data_as(_ip), _p(step)) if lists[3] else (None, None)

        def single(h, i, z, R, a, n, applied, d2):
            return self.L.ekf_update_matched_iter(h, i, z, R, a, n, max_iter, tol, applied, d2, *more)

        def batch(h, z, R, a, n, applied, d2):
            return self.L.ekf_batch_update_matched_iter(h, z, R, a, n, max_iter, tol, applied, d2, *more)

        return self._list_update(lists, index, single, batch) + (iters, step)

    def joint_compat(self, z, R, ids, index=0):
        """The score of one association hypothesis (ekf_joint_compat), nothing applied: d2[k] is the joint Mahalanobis distance of
        the hypothesis cut after measurement k (at most 32 non-skipped measurements; NaN: skipped, or behind a pivot of S that is
        not positive).  The same bits as update_matched's d2 for a hypothesis that fits one round.  index=None: ids [batch][n_z],
        returns d2 (batch, n_z)."""
        z, Rc, a, n_z = self._matched_lists(z, R, ids, index)
        if int((a >= 0).sum(axis=-1).max(initial=0)) > 32:
            raise ValueError("a hypothesis holds at most 32 measurements")
        d2 = np.full(a.shape, np.nan)
        if n_z == 0:
            return d2
        if index is None:
            _chk(self.L.ekf_batch_joint_compat(self.h, _p(z), _p(Rc), a.ctypes.data_as(_ip), n_z, _p(d2)))
        else:
            _chk(self.L.ekf_joint_compat(self.h, int(index), _p(z), _p(Rc), a.ctypes.data_as(_ip), n_z, _p(d2)))
        return d2

    def _fix_lists(self, z, R, what, index):
        """(z, Rc, what, n) as ekf_update_fixes takes them.  With an index: what [n], z [n][2], R [n][2][2], and a heading entry may
        be given as a scalar z[k] with a scalar variance R[k] (a single heading fix: three scalars); index=None: a leading batch
        axis on all three, every entry with two values of z and four of R (ragged lists: pad what with FIX_SKIP)."""
        lead = (self.batch,) if index is None else ()
        a = np.asarray(what, dtype=np.int64)
        if a.ndim == 0 and not lead:
            a, z, R = a.reshape(1), [z], [R]
        if a.ndim != len(lead) + 1 or a.shape[:len(lead)] != lead:
            raise ValueError("what must be [batch][n]" if lead else "what must be [n]")
        if a.size and (a.min() < FIX_HEADING or a.max() > np.iinfo(np.int32).max):
            raise ValueError("a kind is a landmark number, FIX_POSITION, FIX_HEADING or FIX_SKIP")
        n = a.shape[-1]

        def as_array(v):
            try:
                return np.asarray(v, dtype=np.float64)
            except ValueError:  # ragged: scalars among the entries
                return None

        za, Ra = as_array(z), as_array(R)
        if za is not None and Ra is not None and za.size == a.size * 2 and Ra.size == a.size * 4:
            return _rect_lists(za, Ra, a)

        def entries(v, arr, width, name):
            """v as [count][width] values, an entry given as one scalar standing for (scalar, 0, ..); and the mask of those."""
            count = a.size
            if lead or (arr is not None and arr.size not in (count, count * width)) or (arr is None and len(v) != count):
                raise ValueError("%s must hold %d values per entry for %d entries" % (name, width, n))
            if arr is not None and arr.size == count * width:
                return arr.reshape(count, width), np.zeros(count, dtype=bool)
            out, scalar = np.zeros((count, width)), np.zeros(count, dtype=bool)
            for k in range(count):
                e = np.asarray(arr.reshape(-1)[k] if arr is not None else v[k], dtype=np.float64).reshape(-1)
                if e.size not in (1, width):
                    raise ValueError("%s[%d] must hold %d values (or one, for a heading entry)" % (name, k, width))
                out[k, :e.size], scalar[k] = e, e.size == 1
            return out, scalar

        zz, zs = entries(z, za, 2, "z")
        RR, Rs = entries(R, Ra, 4, "R")
        flat = a.reshape(-1)
        if np.any((zs | Rs) & (flat != FIX_HEADING) & (flat != FIX_SKIP)):
            raise ValueError("only a heading entry takes a scalar z and a scalar variance")
        Rc = np.swapaxes(RR.reshape(-1, 2, 2), -1, -2).reshape(-1, 4)  # column-major blocks (a scalar's [[R, 0], [0, 0]] is its own)
        return _f64(zz.reshape(n, 2)), _f64(Rc), np.ascontiguousarray(a, dtype=np.int32), n

    def update_fixes(self, z, R, what, index=0):
        """Apply absolute observations on the device (ekf_update_fixes): entry k is of kind what[k] -- FIX_POSITION (z = the robot's
        position, R 2x2), FIX_HEADING (z = the heading, R its variance; both may be scalars), a landmark number (z = its position)
        or FIX_SKIP.  The entries run as joint updates in rounds of `window`; gates, counters and the decision log are not involved.
        Returns (n_landmarks, n_applied, d2): n_applied < the number of non-skipped entries when a round's S was not positive
        definite (that round and the later ones were not applied), d2[k] the joint Mahalanobis distance of k's round up to and
        including k (NaN: skipped or not applied).  index=None: every filter in one launch sequence (ekf_batch_update_fixes), what
        [batch][n]; returns (n_applied (batch,), d2 (batch, n))."""
        return self._list_update(self._fix_lists(z, R, what, index), index, self.L.ekf_update_fixes, self.L.ekf_batch_update_fixes)

    def fix_compat(self, z, R, what, index=0):
        """The score of one list of fixes (ekf_fix_compat), nothing applied: d2[k] is the joint Mahalanobis distance of the list cut
        after entry k (at most 32 non-skipped entries; NaN: skipped, or behind a refused pivot of S) -- the chi-square test of a fix
        before it is applied.  The same bits as update_fixes' d2 for a list that fits one round.  index=None: what [batch][n],
        returns d2 (batch, n)."""
        z, Rc, a, n = self._fix_lists(z, R, what, index)
        if int((a != FIX_SKIP).sum(axis=-1).max(initial=0)) > 32:
            raise ValueError("a list to score holds at most 32 entries")
        d2 = np.full(a.shape, np.nan)
        if n == 0:
            return d2
        if index is None:
            _chk(self.L.ekf_batch_fix_compat(self.h, _p(z), _p(Rc), a.ctypes.data_as(_ip), n, _p(d2)))
        else:
            _chk(self.L.ekf_fix_compat(self.h, int(index), _p(z), _p(Rc), a.ctypes.data_as(_ip), n, _p(d2)))
        return d2

    def _polar_lists(self, z, R, ids, kind, index):
        """((z, Rc, ids, n), kind) as ekf_update_polar takes them.  With an index: ids and kind [n], z [n][2] = (range, bearing),
        R [n][2][2] over (range, bearing); index=None: a leading batch axis on all four (ragged lists: pad ids with -1).  A RANGE
        entry reads z[k][0] and R[k][0][0] alone, a BEARING entry z[k][1] and R[k][1][1]: the rest may be anything."""
        lists = self._matched_lists(z, R, ids, index)
        kd = np.asarray(kind, dtype=np.int64)
        if kd.shape != lists[2].shape:
            raise ValueError("kind must have the shape of ids")
        if np.any((lists[2] >= 0) & ((kd < POLAR_RANGE) | (kd > POLAR_BOTH))):
            raise ValueError("a kind is POLAR_RANGE, POLAR_BEARING or POLAR_BOTH")
        return lists, np.ascontiguousarray(np.where(lists[2] >= 0, kd, 0), dtype=np.int32)

    def update_polar(self, z, R, ids, kind, index=0):
        """Apply landmark measurements in polar form on the device (ekf_update_polar): entry k measures landmark ids[k] (-1:
        skipped) by kind[k] -- POLAR_RANGE (z[k][0] = the distance, R[k][0][0] its variance), POLAR_BEARING (z[k][1] = the bearing
        in the robot frame, R[k][1][1] its variance) or POLAR_BOTH (z[k] = (range, bearing), R[k] 2x2).  The entries run as joint
        updates in rounds of `window`, each linearised at its entry state; gates, counters and the decision log are not involved.
        Returns (n_landmarks, n_applied, d2) as update_matched: n_applied < the number of non-skipped entries when a round was
        refused (S not positive definite, or a landmark exactly at the robot's position; that round and the later ones were not
        applied), d2[k] the joint Mahalanobis distance of k's round up to and including k (NaN: skipped or not applied).
        index=None: every filter in one launch sequence (ekf_batch_update_polar), ids and kind [batch][n]; returns (n_applied
        (batch,), d2 (batch, n))."""
        lists, kd = self._polar_lists(z, R, ids, kind, index)
        kp = kd.ctypes.data_as(_ip) if lists[3] else None

        def single(h, i, z, R, a, n, applied, d2):
            return self.L.ekf_update_polar(h, i, z, R, a, kp, n, applied, d2)

        def batch(h, z, R, a, n, applied, d2):
            return self.L.ekf_batch_update_polar(h, z, R, a, kp, n, applied, d2)

        return self._list_update(lists, index, single, batch)

    def polar_compat(self, z, R, ids, kind, index=0):
        """The score of one list of polar measurements (ekf_polar_compat), nothing applied: d2[k] is the joint Mahalanobis distance
        of the list cut after entry k (at most 32 non-skipped entries; NaN: skipped, or behind a refused pivot of S).  The same
        bits as update_polar's d2 for a list that fits one round.  index=None: ids and kind [batch][n], returns d2 (batch, n)."""
        (z, Rc, a, n), kd = self._polar_lists(z, R, ids, kind, index)
        if int((a >= 0).sum(axis=-1).max(initial=0)) > 32:
            raise ValueError("a list to score holds at most 32 entries")
        d2 = np.full(a.shape, np.nan)
        if n == 0:
            return d2
        if index is None:
            _chk(self.L.ekf_batch_polar_compat(self.h, _p(z), _p(Rc), a.ctypes.data_as(_ip), kd.ctypes.data_as(_ip), n, _p(d2)))
        else:
            _chk(self.L.ekf_polar_compat(self.h, int(index), _p(z), _p(Rc), a.ctypes.data_as(_ip), kd.ctypes.data_as(_ip), n, _p(d2)))
        return d2

    def _scan_lists(self, z, R, valid, index):
        """(z, Rc, valid or None, n_z) as ekf_gate_candidates takes them.  With an index: z [n_z][2], R [n_z][2][2]; index=None: a
        leading batch axis on both, and on valid [batch][n_z]."""
        lead = (self.batch,) if index is None else ()
        z, R = np.asarray(z, dtype=np.float64), np.asarray(R, dtype=np.float64)
        if z.ndim != len(lead) + 2 or z.shape[:len(lead)] != lead or z.shape[-1] != 2:
            raise ValueError("z must be [batch][n_z][2]" if lead else "z must be [n_z][2]")
        n_z = z.shape[-2]
        if R.size != z.size * 2:
            raise ValueError("R must hold [n_z][2][2] values per filter for %d measurements" % n_z)
        R = R.reshape(lead + (n_z, 2, 2))
        Rc = _f64(np.swapaxes(R, -1, -2).reshape(lead + (n_z, 4)))  # column-major blocks
        if valid is not None:
            if index is not None:
                raise ValueError("valid masks the entries of the batch form (index=None)")
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
            if valid.shape != lead + (n_z,):
                raise ValueError("valid must be [batch][n_z]")
        look = slice(None) if valid is None else valid != 0  # (a masked entry's z and R are not looked at)
        if not (np.isfinite(z[look]).all() and np.isfinite(Rc[look]).all()):
            raise ValueError("z and R of a valid entry must be finite")
        return _f64(z), Rc, valid, n_z

    def gate_candidates(self, z, R, gate=9.21, index=0, max_cand=4096, valid=None):
        """The individual compatibility table of a scan on the device (ekf_gate_candidates): every measurement of z [n_z][2],
        R [n_z][2][2] against every landmark at the SAME, unchanged state -- res, S and d2 of the association sweep.  Returns
        (cands, n_found, nearest, n_skipped): a CAND_DTYPE array ordered by (meas, d2, landmark) with the first min(n_found, max_cand)
        pairs whose d2 <= gate (9.21: 99 % of chi-square with 2 dof; inf: every kept pair), the number of such pairs, a
        DECISION_DTYPE array [n_z] with what update() of each measurement alone would log (a dry run of the filter's own gate), and
        per measurement the landmarks the condition rule skipped.  index=None: every filter in one launch sequence
        (ekf_batch_gate_candidates), leading batch axes, valid [batch][n_z] masks entries; returns a list of such tuples.  The
        filter is only read and an open window stays open; candidate_matching turns the list into the ids update_matched takes."""
        gate, max_cand = float(gate), int(max_cand)
        if not gate >= 0.0:
            raise ValueError("gate must not be negative or NaN")
        if max_cand < 0:
            raise ValueError("max_cand must not be negative")
        z, Rc, valid, n_z = self._scan_lists(z, R, valid, index)
        nb = self.batch if index is None else 1
        max_cand = min(max_cand, n_z * int(self.capacity))  # (a filter cannot list more; the rows are not cleared and only their used part is copied out)
        buf = np.empty((nb, max_cand), dtype=CAND_DTYPE)
        near, skip = np.zeros((nb, n_z), dtype=DECISION_DTYPE), np.zeros((nb, n_z), dtype=np.int32)
        found = np.zeros(nb, dtype=np.int32)
        ptrs = (_p(z), _p(Rc)) if n_z else (None, None)
        cp = buf.ctypes.data_as(ctypes.POINTER(EkfCandidate)) if max_cand else None
        outs = (near.ctypes.data_as(ctypes.POINTER(EkfDecision)), skip.ctypes.data_as(_ip)) if n_z else (None, None)
        if index is None:
            vp = valid.ctypes.data_as(_up) if valid is not None and n_z else None
            _chk(self.L.ekf_batch_gate_candidates(self.h, *ptrs, vp, n_z, gate, cp, max_cand, found.ctypes.data_as(_ip), *outs))
        else:
            found[0] = _chk(self.L.ekf_gate_candidates(self.h, int(index), *ptrs, n_z, gate, cp, max_cand, *outs))
        out = [(buf[b, :min(int(found[b]), max_cand)].copy(), int(found[b]), near[b].copy(), skip[b].copy()) for b in range(nb)]
        return out if index is None else out[0]

    def _locate_args(self, z, valid, index, tol, min_sep, max_base, max_out):
        """The arguments of locate_scan / relocalize checked and laid out: (z, valid or None, n_z, filters of the call)."""
        if not (np.isfinite(tol) and tol > 0.0 and np.isfinite(min_sep) and min_sep > 0.0):
            raise ValueError("tol and min_sep must be finite and positive")
        if not 1 <= max_base <= LOCATE_MAX_BASE or not 1 <= max_out <= LOCATE_MAX_OUT:
            raise ValueError("max_base must lie in 1 .. %d and max_out in 1 .. %d" % (LOCATE_MAX_BASE, LOCATE_MAX_OUT))
        lead = (self.batch,) if index is None else ()
        z = np.asarray(z, dtype=np.float64)
        if z.ndim != len(lead) + 2 or z.shape[:len(lead)] != lead or z.shape[-1] != 2:
            raise ValueError("z must be [batch][n_z][2]" if lead else "z must be [n_z][2]")
        n_z = z.shape[-2]
        if valid is not None:
            if index is not None:
                raise ValueError("valid masks the entries of the batch form (index=None)")
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
            if valid.shape != lead + (n_z,):
                raise ValueError("valid must be [batch][n_z]")
        look = np.ones(lead + (n_z,), dtype=bool) if valid is None else valid != 0
        if not np.isfinite(z[look]).all():
            raise ValueError("z of a valid entry must be finite")
        if int(look.sum(axis=-1).max(initial=0)) > LOCATE_MAX_MEAS:
            raise ValueError("a search takes at most %d valid measurements per filter" % LOCATE_MAX_MEAS)
        return _f64(z), valid, n_z, (self.batch if index is None else 1)

    def locate_scan(self, z, tol, min_sep=1.0, max_base=4, max_out=16, index=0, valid=None):
        """Where am I on this map?  The read-only scan-to-map pose search on the device (ekf_locate_scan): z [n_z][2] robot-frame
        relative positions (at most 32 valid), tol the inlier radius in metres, min_sep the smallest separation of a base pair,
        max_base (1 .. 16) base pairs, max_out (1 .. 64) hypotheses.  Only x is read -- the search is Euclidean, P and R play no
        part -- and an open window stays open.  Returns (hyps, ids, n_candidates): a LOCATE_DTYPE array of the hypotheses written,
        ordered by (inliers descending, ssr ascending, then base pair and landmark pair), ids [len(hyps)][n_z] int32 (row h: the
        landmark of each measurement under hypothesis h, -1: none -- the ids update_matched takes) and the number of candidates
        scored.  The same true pose recurs once per base pair that hits it: distinct_poses merges the repeats.  index=None: every
        filter in one launch sequence (ekf_batch_locate_scan), a leading batch axis on z, valid [batch][n_z] masks entries; returns a
        list of such tuples."""
        tol, min_sep, max_base, max_out = float(tol), float(min_sep), int(max_base), int(max_out)
        z, valid, n_z, nb = self._locate_args(z, valid, index, tol, min_sep, max_base, max_out)
        hyps = np.zeros((nb, max_out), dtype=LOCATE_DTYPE)
        ids = np.full((nb, max_out, n_z), -1, dtype=np.int32)
        found, ncand = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int64)
        hp, ip, cp = hyps.ctypes.data_as(ctypes.POINTER(EkfLocateHyp)), ids.ctypes.data_as(_ip), ncand.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
        zp = _p(z) if n_z else None
        if index is None:
            vp = valid.ctypes.data_as(_up) if valid is not None and n_z else None
            _chk(self.L.ekf_batch_locate_scan(self.h, zp, vp, n_z, tol, min_sep, max_base, max_out, hp, ip, found.ctypes.data_as(_ip), cp))
        else:
            found[0] = _chk(self.L.ekf_locate_scan(self.h, int(index), zp, n_z, tol, min_sep, max_base, max_out, hp, ip, cp))
        out = [(hyps[b, :found[b]].copy(), ids[b, :found[b]].copy(), int(ncand[b])) for b in range(nb)]
        return out if index is None else out[0]

    def reset_pose(self, pose, P_RR, index=0):
        """The pose replaced and its correlation with the map cut, on the device (ekf_reset_pose): x[0:3] = pose, P_RR = the
        symmetrised P_RR [3][3] (zeros: a known pose), every robot-landmark block of P zero; P_LL and the landmarks stay bit for bit.
        index=None: pose [batch][3], P_RR [batch][3][3], every filter in one launch (ekf_batch_reset_pose)."""
        lead = (self.batch,) if index is None else ()
        pose, P_RR = _f64(pose), _f64(P_RR)
        if pose.shape != lead + (3,) or P_RR.size != pose.size * 3:
            raise ValueError("pose must be [batch][3] and P_RR [batch][3][3]" if lead else "pose must be [3] and P_RR [3][3]")
        P_RR = _f64(P_RR.reshape(lead + (3, 3)))
        if not (np.isfinite(pose).all() and np.isfinite(P_RR).all()):
            raise ValueError("pose and P_RR must be finite")
        if (np.diagonal(P_RR, axis1=-2, axis2=-1) < 0.0).any():
            raise ValueError("a diagonal entry of P_RR is negative")
        if index is None:
            _chk(self.L.ekf_batch_reset_pose(self.h, _p(pose), _p(P_RR)))
        else:
            _chk(self.L.ekf_reset_pose(self.h, int(index), _p(pose), _p(P_RR)))

    def relocalize(self, z, R, tol, P_RR, min_sep=1.0, max_base=4, max_out=16, min_inliers=4, lead=2, index=0, valid=None):
        """locate_scan, the acceptance rule, reset_pose at the best hypothesis's fitted pose with P_RR, update_matched with its ids
        and R, as one call (ekf_relocalize).  Accepted iff the best hypothesis has at least min_inliers inliers and every other
        written hypothesis that is not the same pose (same_pose) has at most best - lead.  Returns (n, hyp, ids, d2): n = the best
        hypothesis's inliers, or 0: refused, the state untouched; hyp a LOCATE_DTYPE record (zeros: nothing found), ids [n_z], d2
        [n_z] that of update_matched (NaN when refused).  index=None: leading batch axes on z, R, valid and P_RR; returns (n
        (batch,), hyps (batch,), ids (batch, n_z), d2 (batch, n_z)); the refused filters are left alone."""
        tol, min_sep, max_base, max_out, min_inliers, lead = float(tol), float(min_sep), int(max_base), int(max_out), int(min_inliers), int(lead)
        if min_inliers < 2 or lead < 0:
            raise ValueError("min_inliers must be at least 2 and lead must not be negative")
        z, Rc, valid, n_z = self._scan_lists(z, R, valid, index)
        self._locate_args(z, valid, index, tol, min_sep, max_base, max_out)
        nb = self.batch if index is None else 1
        P_RR = _f64(P_RR)
        if P_RR.size != 9 * nb:
            raise ValueError("P_RR must be [batch][3][3]" if index is None else "P_RR must be [3][3]")
        P_RR = _f64(P_RR.reshape(nb, 3, 3))
        if not np.isfinite(P_RR).all() or (np.diagonal(P_RR, axis1=-2, axis2=-1) < 0.0).any():
            raise ValueError("P_RR must be finite, without a negative diagonal entry")
        hyp = np.zeros(nb, dtype=LOCATE_DTYPE)
        ids, d2, n = np.full((nb, n_z), -1, dtype=np.int32), np.full((nb, n_z), np.nan), np.zeros(nb, dtype=np.int32)
        ptrs = (_p(z), _p(Rc)) if n_z else (None, None)
        outs = (hyp.ctypes.data_as(ctypes.POINTER(EkfLocateHyp)), ids.ctypes.data_as(_ip), _p(d2) if n_z else None)
        if index is None:
            vp = valid.ctypes.data_as(_up) if valid is not None and n_z else None
            _chk(self.L.ekf_batch_relocalize(self.h, *ptrs, vp, n_z, tol, min_sep, max_base, max_out, min_inliers, lead, _p(P_RR), *outs, n.ctypes.data_as(_ip)))
            return n, hyp, ids, d2
        n[0] = _chk(self.L.ekf_relocalize(self.h, int(index), *ptrs, n_z, tol, min_sep, max_base, max_out, min_inliers, lead, _p(P_RR), *outs))
        return int(n[0]), hyp[0].copy(), ids[0], d2[0]

    def _assoc_args(self, z, R, gate, joint_gate, max_branch, max_nodes, index, valid):
        """The arguments of associate_joint / update_joint checked and laid out: (gate, joint gates or None, max_branch, max_nodes,
        z, Rc, valid, n_z, filters of the call)."""
        gate, max_branch, max_nodes = float(gate), int(max_branch), int(max_nodes)
        if not gate >= 0.0:
            raise ValueError("gate must not be negative or NaN")
        if not 1 <= max_branch <= ASSOC_MAX_BRANCH:
            raise ValueError("max_branch must lie in 1 .. %d" % ASSOC_MAX_BRANCH)
        if not 1 <= max_nodes <= ASSOC_MAX_NODES:
            raise ValueError("max_nodes must lie in 1 .. %d" % ASSOC_MAX_NODES)
        jg = None
        if joint_gate is not None:
            jg = _f64(joint_gate).reshape(-1)
            if jg.shape != (ASSOC_MAX_MEAS,) or not (jg >= 0.0).all():
                raise ValueError("joint_gate must hold %d gates, none negative or NaN" % ASSOC_MAX_MEAS)
        z, Rc, valid, n_z = self._scan_lists(z, R, valid, index)
        nb = self.batch if index is None else 1
        kept = np.full(nb, n_z) if valid is None else (valid != 0).sum(axis=-1)
        if int(np.max(kept, initial=0)) > ASSOC_MAX_MEAS:
            raise ValueError("a scan holds at most %d valid measurements" % ASSOC_MAX_MEAS)
        return gate, jg, max_branch, max_nodes, z, Rc, valid, n_z, nb

    def associate_joint(self, z, R, gate=9.21, joint_gate=None, max_branch=8, max_nodes=65536, index=0, valid=None):
        """The joint-compatibility search of a scan on the device (ekf_associate_joint): the candidates of every measurement are
        those gate_candidates lists at `gate` (the first max_branch of each), a hypothesis pairs every measurement with one of them
        or nothing, every prefix of q pairings within joint_gate[q - 1] (None: joint_gates(0.99)); the result has the most
        pairings, then the smallest joint distance, found by branch and bound within max_nodes expanded nodes.  Returns
        (ids, d2, info, nearest, n_skipped): ids int32 [n_z] as update_matched takes them (-1: unpaired), d2 what joint_compat
        gives for ids, info an ASSOC_DTYPE record (nodes, d2, n_paired, complete, n_candidates, n_dropped), nearest and n_skipped as
        gate_candidates.  index=None: every filter in one launch sequence, leading batch axes, valid [batch][n_z] masks entries.
        At most 32 valid measurements per filter.  The filter is only read; deferred slots are folded when something is searched."""
        gate, jg, max_branch, max_nodes, z, Rc, valid, n_z, nb = self._assoc_args(z, R, gate, joint_gate, max_branch, max_nodes, index, valid)
        ids, d2 = np.full((nb, n_z), -1, dtype=np.int32), np.full((nb, n_z), np.nan)
        near, skip = np.zeros((nb, n_z), dtype=DECISION_DTYPE), np.zeros((nb, n_z), dtype=np.int32)
        info = np.zeros(nb, dtype=ASSOC_DTYPE)
        ptrs = (_p(z), _p(Rc)) if n_z else (None, None)
        outs = (ids.ctypes.data_as(_ip), _p(d2), near.ctypes.data_as(ctypes.POINTER(EkfDecision)), skip.ctypes.data_as(_ip)) if n_z else (None,) * 4
        ip = info.ctypes.data_as(ctypes.POINTER(EkfAssoc))
        jp = _p(jg) if jg is not None else None
        if index is None:
            vp = valid.ctypes.data_as(_up) if valid is not None and n_z else None
            _chk(self.L.ekf_batch_associate_joint(self.h, *ptrs, vp, n_z, gate, jp, max_branch, max_nodes, *outs, ip))
            return [(ids[b].copy(), d2[b].copy(), info[b].copy(), near[b].copy(), skip[b].copy()) for b in range(nb)]
        _chk(self.L.ekf_associate_joint(self.h, int(index), *ptrs, n_z, gate, jp, max_branch, max_nodes, *outs, ip))
        return ids[0], d2[0], info[0], near[0], skip[0]

    def add_landmarks(self, z, R, add=None, index=0):
        """Initialise landmarks from measurements on the device (ekf_add_landmarks): the entries of z [n_z][2], R [n_z][2][2] with
        add[k] != 0 (None: all) become landmarks N, N + 1, .. in list order, all linearised at the entry state; pose, P_RR and every
        old row stay bit for bit.  Returns (n_landmarks, ids): ids int32 [n_z], the new landmark's number or -1.  index=None: every
        filter in one launch sequence (ekf_batch_add_landmarks), leading batch axes on z, R and add; returns (n_landmarks (batch,),
        ids (batch, n_z)).  EkfError ERR_CAPACITY (not sticky, nothing changed) when a filter has no room: reserve(), add again."""
        lead = (self.batch,) if index is None else ()
        z, R = np.asarray(z, dtype=np.float64), np.asarray(R, dtype=np.float64)
        if z.ndim != len(lead) + 2 or z.shape[:len(lead)] != lead or z.shape[-1] != 2:
            raise ValueError("z must be [batch][n_z][2]" if lead else "z must be [n_z][2]")
        n_z = z.shape[-2]
        if R.size != z.size * 2:
            raise ValueError("R must hold [n_z][2][2] values per filter for %d measurements" % n_z)
        Rc = _f64(np.swapaxes(R.reshape(lead + (n_z, 2, 2)), -1, -2).reshape(lead + (n_z, 4)))  # column-major blocks
        z = _f64(z)
        if add is not None:
            add = np.ascontiguousarray(np.asarray(add) != 0, dtype=np.uint8)
            if add.shape != lead + (n_z,):
                raise ValueError("add must be [batch][n_z]" if lead else "add must be [n_z]")
        ids = np.full(lead + (n_z,), -1, dtype=np.int32)
        ptrs = (_p(z), _p(Rc), add.ctypes.data_as(_up) if add is not None else None) if n_z else (None, None, None)
        if index is None:
            n = np.zeros(self.batch, dtype=np.int32)
            _chk(self.L.ekf_batch_add_landmarks(self.h, *ptrs, n_z, ids.ctypes.data_as(_ip) if n_z else None, n.ctypes.data_as(_ip)))
            return n, ids
        n = _chk(self.L.ekf_add_landmarks(self.h, int(index), *ptrs, n_z, ids.ctypes.data_as(_ip) if n_z else None))
        return n, ids

    def update_joint(self, z, R, gate=9.21, joint_gate=None, max_branch=8, max_nodes=65536, index=0, valid=None):
        """One scan with joint-compatibility data association as one call (ekf_update_joint): associate_joint at the entry state,
        update_matched with the pairings, add_landmarks with the measurements the filter's own gate calls New -- at the state the
        matched step left.  Arguments as associate_joint.  Returns (n_landmarks, ids, kinds, d2, info): ids int32 [n_z] the
        landmark each measurement ended as (-1: none), kinds int32 [n_z] OLD / NEW / IGNORE (0: masked), d2 as update_matched, info
        as associate_joint.  index=None: every filter, leading batch axes, valid [batch][n_z]; n_landmarks is (batch,).  Bit for bit
        the three calls in sequence; counters and decision log are not involved."""
        gate, jg, max_branch, max_nodes, z, Rc, valid, n_z, nb = self._assoc_args(z, R, gate, joint_gate, max_branch, max_nodes, index, valid)
        ids, kinds, d2 = np.full((nb, n_z), -1, dtype=np.int32), np.zeros((nb, n_z), dtype=np.int32), np.full((nb, n_z), np.nan)
        info = np.zeros(nb, dtype=ASSOC_DTYPE)
        ptrs = (_p(z), _p(Rc)) if n_z else (None, None)
        outs = (ids.ctypes.data_as(_ip), kinds.ctypes.data_as(_ip), _p(d2)) if n_z else (None,) * 3
        ip = info.ctypes.data_as(ctypes.POINTER(EkfAssoc))
        jp = _p(jg) if jg is not None else None
        if index is None:
            n = np.zeros(nb, dtype=np.int32)
            vp = valid.ctypes.data_as(_up) if valid is not None and n_z else None
            _chk(self.L.ekf_batch_update_joint(self.h, *ptrs, vp, n_z, gate, jp, max_branch, max_nodes, *outs, ip, n.ctypes.data_as(_ip)))
            return n, ids, kinds, d2, info
        n = _chk(self.L.ekf_update_joint(self.h, int(index), *ptrs, n_z, gate, jp, max_branch, max_nodes, *outs, ip))
        return n, ids[0], kinds[0], d2[0], info[0]

    def joint_factor(self, index=0):
        """Diagnostic: the upper factor U (U^T U = P_LL) the last joint_consistency call left for filter `index`, dense (2N, 2N);
        EkfError ERR_STATE when the state has changed since."""
        n = max(2 * int(self.num_landmarks()[int(index)]), 1)
        out = np.zeros((n, n))  # column-major with ld = n: out[j, i] = U[i, j]
        m = _chk(self.L.ekf_debug_joint_factor(self.h, int(index), _p(out), n))
        return np.ascontiguousarray(out[:m, :m].T)

    def script_load(self, ctrl, z, R, valid=None, truth=None):
        """ctrl (steps, batch, 3); z (steps, M, batch, 2); R (steps, M, batch, 4) column-major blocks;
        valid (steps, M, batch); truth (steps, batch, 3)."""
        ctrl = _f64(ctrl)
        steps = ctrl.shape[0]
        z = _f64(z)
        M = z.shape[1] if z.size else 0
        R = _f64(R)
        assert ctrl.shape == (steps, self.batch, 3)
        if M:
            assert z.shape == (steps, M, self.batch, 2) and R.shape == (steps, M, self.batch, 4)
        vp = None
        if valid is not None:
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
            vp = valid.ctypes.data_as(_up)
        tp = None
        if truth is not None:
            truth = _f64(truth)
            assert truth.shape == (steps, self.batch, 3)
            tp = _p(truth)
        _chk(self.L.ekf_script_load(self.h, steps, M, _p(ctrl), _p(z) if M else None, _p(R) if M else None, vp, tp))

    def script_run(self, first, count, use_graph=False):
        _chk(self.L.ekf_script_run(self.h, first, count, int(use_graph)))

    def sync(self):
        _chk(self.L.ekf_sync(self.h))

    def flush(self):
        _chk(self.L.ekf_flush(self.h))

    def close_window(self):
        _chk(self.L.ekf_close_window(self.h))

    def timer_start(self):
        _chk(self.L.ekf_timer_start(self.h))

    def timer_stop(self):
        ms = ctypes.c_double(0)
        _chk(self.L.ekf_timer_stop(self.h, ctypes.byref(ms)))
        return ms.value

    def flush_profile(self, enable):
        _chk(self.L.ekf_flush_profile(self.h, int(enable)))

    def flush_profile_read(self):
        n = ctypes.c_longlong(0)
        ms = ctypes.c_double(0)
        _chk(self.L.ekf_flush_profile_read(self.h, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def decisions(self, index=0, count=4096):
        buf = (EkfDecision * count)()
        n = _chk(self.L.ekf_get_decisions(self.h, index, buf, count))
        return [(buf[i].decision, buf[i].matched, buf[i].mahal) for i in range(n)]

    def stats(self):
        buf = (EkfStats * self.batch)()
        _chk(self.L.ekf_get_stats(self.h, buf))
        return [dict((f, getattr(s, f)) for f, _ in EkfStats._fields_) for s in buf]

    def stats_array(self):
        """The same counters as one NumPy structured array (fields as in ekf_stats), one row per filter: no per-filter Python
        objects (256 filters as dicts cost a millisecond)."""
        buf = (EkfStats * self.batch)()
        _chk(self.L.ekf_get_stats(self.h, buf))
        return np.frombuffer(buf, dtype=_STATS_DTYPE, count=self.batch)  # (the array keeps the buffer alive)

    def reset_stats(self):
        _chk(self.L.ekf_reset_stats(self.h))

    def stats_means_into(self, device_ptr):
        """(mean NIS, mean NEES) per filter, [batch][2] doubles, written by the device into device memory at `device_ptr`
        (e.g. torch_tensor.data_ptr()): the send buffer of the multi-GPU all-gather, no host bounce."""
        _chk(self.L.ekf_stats_means_device(self.h, ctypes.c_void_p(int(device_ptr))))

    def record_truth(self, truth):
        t = _f64(truth).reshape(self.batch, 3)
        _chk(self.L.ekf_record_truth(self.h, _p(t)))

    def device_bytes(self):
        return self.L.ekf_device_bytes(self.h)


MAX_CAPACITY = 16000  # EKF_MAX_CAPACITY of include/ekfslam_c.h


def grown_capacity(cap, need, limit=MAX_CAPACITY):
    """The capacity asked for when `need` landmarks no longer fit `cap` (compat/kalmanfilter.h: grown_capacity): double, but never
    beyond what the library can hold -- only a map that really needs more than `limit` fails (ekf_reserve then says so)."""
    want = max(2 * cap, need)
    if want > limit and need <= limit:
        want = limit
    return want


class KalmanFilter:
    """Python mirror of the reference's class KalmanFilter (odometry/kalmanfilter.h:21-43): same public
    members X, Y, Phi, Num_Landmarks and the same three methods, forwarding to the C ABI.  The ARIA
    velocity reads of doPropagation (kalmanfilter.cpp:17-20) become the v_mm_s / rotvel_deg_s arguments."""

    def __init__(self, capacity_landmarks=1024, device=0, print_decisions=False, **params):
        # one synchronising call per operation (the mirrors must be current after each); the calls travel to a resident streaming
        # launch, and the window's dense pass runs in place for small maps, beside the next window's calls from 2048 landmarks on
        # (compat/kalmanfilter.h has the measurements); overlap=-1 / 0 / 1 can still be asked for
        params.setdefault("overlap", 1 if capacity_landmarks >= 2048 else 0)
        self._f = FilterBatch(1, capacity_landmarks, device, **params)
        self.X = self.Y = self.Phi = 0.0
        self.Num_Landmarks = 0
        self.last_decisions = []
        self.Print_Decisions = print_decisions  # the reference's stdout tokens "New " / "Old " / "Ignore " (Update.cpp:154,183,191)

    def _mirror(self):
        pose = self._f.poses()[0]
        self.X, self.Y, self.Phi = float(pose[0]), float(pose[1]), float(pose[2])
        self.Num_Landmarks = int(self._f.num_landmarks()[0])

    def doPropagation(self, dt, v_mm_s, rotvel_deg_s, covFile=None, knownfeaturesFile=None):
        v = v_mm_s / 1000.0                       # kalmanfilter.cpp:26
        w = rotvel_deg_s * 3.141592654 / 180.0    # kalmanfilter.cpp:19
        self._f.propagate(v, w, dt)
        self._mirror()

    def doUpdate(self, z_chunk, R_chunk):
        """z_chunk (2, n_z), R_chunk (2, 2 n_z) as in kalmanfilter.h:31."""
        z = np.asarray(z_chunk, dtype=np.float64).reshape(2, -1)
        n_z = z.shape[1]
        Rm = np.asarray(R_chunk, dtype=np.float64).reshape(2, 2 * n_z)
        R = np.stack([Rm[:, 2 * j:2 * j + 2] for j in range(n_z)])
        if self.Num_Landmarks + n_z > self._f.capacity:  # the reference's state grows without bound (Update.cpp:158-177): make room first
            self._f.reserve(grown_capacity(self._f.capacity, self.Num_Landmarks + n_z))
        self.last_decisions = self._f.update(z.T.reshape(1, n_z, 2), R.reshape(1, n_z, 2, 2))[0]
        if self.Print_Decisions:
            import sys
            sys.stdout.write("".join({NEW: "New ", OLD: "Old ", IGNORE: "Ignore "}[d[0]] for d in self.last_decisions))
        self._mirror()

    def doUpdateCompass(self, z, R):
        self._f.update_compass(z, R)
        self._mirror()

    def state(self):
        return self._f.get_state(0)

    def set_state(self, x, P):
        self._f.set_state(x, P, 0)
        self._mirror()

    def remove_landmarks(self, keep):
        """Marginalise the landmarks whose keep[l] is false out of the map (kept ones are renumbered in order); refreshes
        Num_Landmarks.  A decision's matched index m names landmark (m - 3) // 2."""
        self._f.remove_landmarks(keep, 0)
        self._mirror()

    def transform_frame(self, frame):
        """A known rigid transform of the estimate, frame = (t_x, t_y, theta) = the new origin's pose in the current frame; refreshes
        X, Y, Phi (Phi is not wrapped).  Compass readings passed to doUpdateCompass afterwards must be shifted by -theta."""
        self._f.transform_frame(frame, 0)
        self._mirror()

    def anchor_at_robot(self):
        """Re-express the map relative to the estimated pose: X = Y = Phi = 0 with zero robot covariance afterwards."""
        self._f.anchor_at_robot(0)
        self._mirror()

    def get_submap(self, ids):
        """(x, P) of the robot and the landmarks `ids` alone (FilterBatch.get_submap): state()[sel] without the dense export."""
        return self._f.get_submap(ids, 0)

    def joint_consistency(self, x_true=None):
        """Joint / map NEES, log det P, pivots and the pose covariance given the map (FilterBatch.joint_consistency): one record."""
        return self._f.joint_consistency(x_true, 0)[0]

    def find_duplicates(self, gate=9.21, max_dist=None, split=0, max_pairs=4096):
        """Pairs of landmarks that pass the duplicate gate (FilterBatch.find_duplicates): (pairs, n_found, n_degenerate)."""
        return self._f.find_duplicates(gate, max_dist, split, 0, max_pairs)

    def fuse_landmarks(self, pairs, slack=0.0):
        """Fuse the pairs (i, j) of duplicate landmarks and remove every j (FilterBatch.fuse_landmarks): (n_landmarks, n_fused);
        refreshes X, Y, Phi and Num_Landmarks."""
        out = self._f.fuse_landmarks(pairs, slack, 0)
        self._mirror()
        return out

    def update_matched(self, z, R, ids):
        """Apply measurements with given landmarks as joint updates (FilterBatch.update_matched): (n_landmarks, n_applied, d2);
        refreshes X, Y, Phi."""
        out = self._f.update_matched(z, R, ids, 0)
        self._mirror()
        return out

    def update_matched_iter(self, z, R, ids, max_iter=8, tol=1e-8):
        """update_matched with every round iterated (FilterBatch.update_matched_iter): (n_landmarks, n_applied, d2, iters, step);
        refreshes X, Y, Phi."""
        out = self._f.update_matched_iter(z, R, ids, max_iter, tol, 0)
        self._mirror()
        return out

    def joint_compat(self, z, R, ids):
        """The running joint Mahalanobis distance of one association hypothesis (FilterBatch.joint_compat); nothing is applied."""
        return self._f.joint_compat(z, R, ids, 0)

    def update_fixes(self, z, R, what):
        """Apply absolute position, heading and landmark fixes as joint updates (FilterBatch.update_fixes): (n_landmarks, n_applied,
        d2); refreshes X, Y, Phi."""
        out = self._f.update_fixes(z, R, what, 0)
        self._mirror()
        return out

    def fix_compat(self, z, R, what):
        """The running joint Mahalanobis distance of one list of fixes (FilterBatch.fix_compat); nothing is applied."""
        return self._f.fix_compat(z, R, what, 0)

    def update_polar(self, z, R, ids, kind):
        """Apply range, bearing and range-bearing measurements of known landmarks as joint updates (FilterBatch.update_polar):
        (n_landmarks, n_applied, d2); refreshes X, Y, Phi."""
        out = self._f.update_polar(z, R, ids, kind, 0)
        self._mirror()
        return out

    def polar_compat(self, z, R, ids, kind):
        """The running joint Mahalanobis distance of one list of polar measurements (FilterBatch.polar_compat); nothing is applied."""
        return self._f.polar_compat(z, R, ids, kind, 0)

    def associate_joint(self, z, R, gate=9.21, joint_gate=None, max_branch=8, max_nodes=65536):
        """The joint-compatibility search of a scan (FilterBatch.associate_joint): (ids, d2, info, nearest, n_skipped); nothing is
        applied -- update_matched(z, R, ids) applies the decision."""
        return self._f.associate_joint(z, R, gate, joint_gate, max_branch, max_nodes, 0)

    def gate_candidates(self, z, R, gate=9.21):
        """The gate-passing landmarks of every measurement, the filter's own decision for each and the skip counts
        (FilterBatch.gate_candidates): (cands, n_found, nearest, n_skipped); nothing is applied."""
        return self._f.gate_candidates(z, R, gate, 0)

    def locate_scan(self, z, tol, min_sep=1.0, max_base=4, max_out=16):
        """The scan-to-map pose search (FilterBatch.locate_scan): (hyps, ids, n_candidates); only x is read."""
        return self._f.locate_scan(z, tol, min_sep, max_base, max_out, 0)

    def reset_pose(self, pose, P_RR):
        """Replace the pose and cut its correlation with the map (FilterBatch.reset_pose); refreshes X, Y, Phi."""
        self._f.reset_pose(pose, P_RR, 0)
        self._mirror()

    def relocalize(self, z, R, tol, P_RR, min_sep=1.0, max_base=4, max_out=16, min_inliers=4, lead=2):
        """Search, accept, reset the pose and apply the scan (FilterBatch.relocalize): (n, hyp, ids, d2), n = 0: refused, nothing
        changed; refreshes X, Y, Phi."""
        out = self._f.relocalize(z, R, tol, P_RR, min_sep, max_base, max_out, min_inliers, lead, 0)
        self._mirror()
        return out

    def add_landmarks(self, z, R, add=None):
        """Initialise landmarks from measurements (FilterBatch.add_landmarks): (n_landmarks, ids)."""
        out = self._f.add_landmarks(z, R, add, 0)
        self._mirror()
        return out

    def update_joint(self, z, R, gate=9.21, joint_gate=None, max_branch=8, max_nodes=65536):
        """One scan with joint-compatibility data association (FilterBatch.update_joint): (n_landmarks, ids, kinds, d2, info);
        refreshes X, Y, Phi."""
        out = self._f.update_joint(z, R, gate, joint_gate, max_branch, max_nodes, 0)
        self._mirror()
        return out
