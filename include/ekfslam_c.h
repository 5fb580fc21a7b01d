/*
 * ekfslam_c.h -- C ABI of the MI355X-native EKF-SLAM core (libekfslam_hip.so).
 *
 * Drop-in boundary for the one hot path of kentsommer/2D-EKF-SLAM: the Propagate + Update loop
 * behind odometry/kalmanfilter.h.  Plain pointers and sizes only; no C++/torch types.
 * Each entry point cites the reference interface it replaces (paths relative to the reference).
 *
 * A handle owns `batch` independent filters (batch = 1 for the reference's single filter), all
 * resident in the HBM of one device and driven through one HIP stream.  Host buffers passed in are
 * caller-owned and are only read/written during the call.  A handle is not thread-safe; distinct
 * handles are independent.
 *
 * Layout conventions (match Eigen's data() so the reference's matrices can be passed as they are):
 *   x        : n = 3 + 2*N doubles [x_R, y_R, phi, L1x, L1y, ...]          (Update.cpp:106)
 *   P        : n x n, column-major with leading dimension ld (P is symmetric, exported bitwise
 *              symmetric)                                                   (kalmanfilter.h:38)
 *   z_chunk  : 2 x n_z column-major -> measurement j is z[2*j + r]          (Update.cpp:85)
 *   R_chunk  : 2 x 2n_z column-major -> R_j(r,c) is R[4*j + 2*c + r]        (Update.cpp:86)
 * For batched calls every per-filter argument gains a leading [batch] dimension.
 *
 * Every function returns an int status (the reference has no error channel at all:
 * kalmanfilter.h:29-32 are void).  Device work is asynchronous unless a function's comment says it
 * synchronises.
 */
#ifndef EKFSLAM_C_H
#define EKFSLAM_C_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EKF_OK 0
#define EKF_ERR_BAD_ARG (-1)
#define EKF_ERR_CAPACITY (-2)  /* a New landmark did not fit capacity_landmarks (sticky until ekf_set_state) */
#define EKF_ERR_HIP (-3)       /* HIP runtime error, see ekf_last_error() */
#define EKF_ERR_NO_DEVICE (-4) /* no usable gfx950 device: the product path has no CPU fallback */
#define EKF_ERR_STATE (-5)     /* call not valid in the handle's current state (also: the GPU cannot keep this handle's
                                  chain workgroups resident beside those of the handles already live, see ekf_batch_create) */
#define EKF_ERR_TIMEOUT (-6)   /* a bounded device-side wait ran out (a filter's workgroups were not all running at once, or the
                                  dense pass a launch depends on did not complete): the launch stopped applying operations and
                                  the filter's state is invalid; sticky until ekf_set_state */

/* Gate decisions, as printed by Update.cpp:154,183,191 ("New " / "Old " / "Ignore "). */
#define EKF_DECISION_NEW 1
#define EKF_DECISION_OLD 2
#define EKF_DECISION_IGNORE 3

/* Largest capacity_landmarks a handle can have (ekf_create / ekf_batch_create / ekf_reserve reject more with EKF_ERR_BAD_ARG). */
#define EKF_MAX_CAPACITY 16000

typedef struct ekf_batch *ekf_handle;

/* Tunables; defaults equal the reference's literals. */
typedef struct ekf_params {
    double sigma_v;     /* 0.01  kalmanfilter.cpp:28 */
    double sigma_w;     /* 0.04  kalmanfilter.cpp:29 */
    double gamma_max;   /* 50    kalmanfilter.cpp:67 (int there) */
    double gamma_min;   /* 10    kalmanfilter.cpp:68 (int there) */
    double cond_limit;  /* 80    Update.cpp:131 */
    int max_pending;    /* measurements whose P_LL change is deferred into ONE dense pass over P_LL
                           (each is a rank-2 slot of that pass); 1 = a dense pass per measurement as the
                           reference does (Update.cpp:188).  1..32, default 16; may be shortened at
                           creation, see ekf_window().  Results do not depend on it beyond rounding; x, the robot rows and the landmark 2x2 blocks are always
                           current, and ekf_get_state / ekf_flush fold everything on demand. */
    int log_capacity;   /* decision-log entries kept per filter (ring) */
    int overlap;        /* 1: a window's dense pass runs on its own HIP stream, buffer to buffer, beside the next
                           window's chain kernels (twice the P_LL memory); 0: the pass runs in place between the
                           windows; -1 (default): on when both windows fit the chain kernel's on-chip buffer
                           without shortening max_pending.  Same results up to rounding. */
} ekf_params;

typedef struct ekf_decision {
    int decision;    /* EKF_DECISION_* */
    int matched;     /* the reference's Opt_i: 0-based state index 2*i+1 of the arg-min landmark, 0 if none (Update.cpp:101,143) */
    double mahal;    /* the reference's Mahal_dist (Update.cpp:136,142); 999999999999 if none */
} ekf_decision;

typedef struct ekf_stats {
    double nis_sum;   /* sum of accepted (Old) Mahalanobis distances = NIS, 2 dof */
    double nees_sum;  /* sum of e^T P_RR^-1 e at every ekf_record_truth / scripted truth, 3 dof */
    long long nis_count;
    long long nees_count;
    long long n_new, n_old, n_ignore;
} ekf_stats;

const char *ekf_last_error(void);
void ekf_default_params(ekf_params *p);

/* KalmanFilter::KalmanFilter, kalmanfilter.cpp:4-12: x = 0_3, P = 0_3x3, no landmarks.
 * capacity_landmarks bounds N; all device memory is allocated here, none later (except a transient
 * staging buffer inside ekf_get_state / ekf_set_state, inside ekf_remove_landmarks / ekf_batch_remove_landmarks the
 * landmark maps and, in the in-place pipeline (ekf_overlap() == 0), a scratch copy of the reduced maps' tiles -- and the
 * factorisation scratch of ekf_joint_consistency, allocated at its first call and kept: one more P_LL buffer per filter -- and
 * the scratch of ekf_find_duplicates, likewise: a box per 32 landmarks and a pair list that grows with what a call finds -- and
 * the scratch of ekf_fuse_landmarks, likewise: a pair table and one round's 64 x 64 factor per filter -- and the measurement
 * table of ekf_update_matched / ekf_joint_compat, likewise, which grows with the longest list a call brings).
 * The sequential part of a filter runs on a few workgroups that exchange their arg-min candidates while they
 * run, so all of them must be resident on the GPU at once: creation fails with EKF_ERR_STATE when this
 * handle's workgroups do not fit beside those of the handles already live on the device (in this process).
 * The registry behind that check is PER PROCESS: two processes that share one GPU do not see each other's handles, there is no
 * admission control between them, and a filter whose workgroups cannot all run because another process holds the CUs ends in the
 * bounded device-side wait (EKF_ERR_TIMEOUT, sticky) instead of a refusal at creation.  One process per GPU -- the layout of the
 * multi-GPU runs (one rank per device) -- never meets this. */
int ekf_create(ekf_handle *out, int capacity_landmarks, int device_id, const ekf_params *params);
int ekf_batch_create(ekf_handle *out, int batch, int capacity_landmarks, int device_id, const ekf_params *params);
int ekf_destroy(ekf_handle h);
/* Grow the landmark capacity of every filter of the handle to at least capacity_landmarks (no-op when it is there already).  The
 * reference grows x and P by two rows and columns with every New landmark (Update.cpp:158-177, the O(n^2) copy of
 * kalmanfilter.cpp:78-84) and never runs out; here all device memory is sized by the capacity, so growth is an explicit, rare
 * step: device buffers of the larger capacity are allocated, the state moves over on the device, counters, decision log and a
 * loaded script are kept, the handle stays valid -- and so do ekf_stream() (the handle keeps its stream), a timer started with
 * ekf_timer_start and the dense-pass profile collected so far (ekf_flush_profile*).  Synchronises; clears a sticky EKF_ERR_CAPACITY.
 * EKF_ERR_STATE when the larger chain launch would not fit the GPU beside the other live handles, EKF_ERR_BAD_ARG beyond
 * EKF_MAX_CAPACITY (the handle is unchanged then). */
int ekf_reserve(ekf_handle h, int capacity_landmarks);
int ekf_batch_size(ekf_handle h);
int ekf_capacity(ekf_handle h);
/* The effective max_pending: the requested window, shortened when capacity_landmarks x window does not fit
 * the on-chip buffer of the chain kernel (64 bytes per landmark and slot, about 148 KB per workgroup).  Maps of up to 256
 * landmarks keep windows of up to 32 (the one-workgroup kernel holds the first 16 slots of a longer window in registers). */
int ekf_window(ekf_handle h);
/* 1 when the handle overlaps dense passes with chain kernels (ekf_params.overlap resolved), else 0. */
int ekf_overlap(ekf_handle h);

/* ---- single-filter calls (batch must be 1) ------------------------------------------------ */

/* The arithmetic half of KalmanFilter::doPropagation, kalmanfilter.cpp:26-44: v in m/s, w in
 * rad/s (the ARIA reads and unit conversions of :17-26 stay with the caller),
 * Q = (v*v) * diag(sigma_v, sigma_w)^2, then Propagate. */
int ekf_propagate(ekf_handle h, double v_mps, double w_radps, double dt);
/* KalmanFilter::Propagate, Propagate.cpp:15-75 / kalmanfilter.h:40: Q is 2x2 column-major. */
int ekf_propagate_q(ekf_handle h, double v, double w, const double Q[4], double dt);
/* KalmanFilter::doUpdate -> Update, kalmanfilter.cpp:64-90 / Update.cpp:22-204, with Gamma and
 * the condition limit taken from params.  decisions_out[n_z] may be NULL; when it is not, the call
 * synchronises. */
int ekf_update(ekf_handle h, const double *z_chunk, const double *R_chunk, int n_z, ekf_decision *decisions_out);
/* KalmanFilter::doUpdateCompass, kalmanfilter.cpp:96-130. */
int ekf_update_compass(ekf_handle h, double z, double R);
/* The public mirrors X, Y, Phi, Num_Landmarks of kalmanfilter.h:24-27 (synchronises). */
int ekf_get_pose(ekf_handle h, double pose_out[3]);
int ekf_num_landmarks(ekf_handle h);  /* >= 0, or a negative status */
/* The robot block P[0:3,0:3], row-major (what kalmanfilter.cpp:51 logs a corner of); synchronises. */
int ekf_get_robot_cov(ekf_handle h, double P_RR_out[9]);
/* The state vector of filter `index` (what kalmanfilter.cpp:56-59 logs from); copies min(n, n_max)
 * entries, returns n; synchronises.  The covariance stays on the device. */
int ekf_get_x(ekf_handle h, int index, double *x_out, int n_max);

/* ---- batched calls: arrays carry a leading [batch] dimension -------------------------------- */

int ekf_batch_propagate(ekf_handle h, const double *v, const double *w, const double *dt);
int ekf_batch_propagate_q(ekf_handle h, const double *v, const double *w, const double *Q /*[batch][4]*/, const double *dt);
/* z [batch][n_z][2], R [batch][n_z][4], valid [batch][n_z] (NULL = all valid) selects which
 * filters actually receive measurement j; decisions_out [batch][n_z] or NULL. */
int ekf_batch_update(ekf_handle h, const double *z, const double *R, const unsigned char *valid, int n_z, ekf_decision *decisions_out);
int ekf_batch_update_compass(ekf_handle h, const double *z, const double *R, const unsigned char *valid);
int ekf_batch_get_pose(ekf_handle h, double *pose_out /*[batch][3]*/);
int ekf_batch_num_landmarks(ekf_handle h, int *n_out /*[batch]*/);

/* ---- state injection / extraction (tests, checkpoint/resume); both synchronise -------------- */

/* Dense export of filter `index`: x_out[n], P_out n x n with leading dimension ld >= n.  Pass
 * x_out = P_out = NULL to query the state size; returns n (>= 3) or a negative status. */
int ekf_get_state(ekf_handle h, int index, double *x_out, double *P_out, int ld);
/* Replace filter `index`'s state: n = 3 + 2*N, P must be symmetric. Clears a sticky capacity error. */
int ekf_set_state(ekf_handle h, int index, const double *x, const double *P, int ld, int n);
/* Copy filter 0's state into every other filter of the batch (device-side). */
int ekf_broadcast_state(ekf_handle h);

/* ---- map management: marginalising landmarks out, per-landmark covariances ------------------------ */

/* Marginalise landmarks out of filter `index`: keep[l] != 0 keeps landmark l (0-based; state rows 3+2l, 4+2l; an
 * ekf_decision.matched m names landmark (m-3)/2).  Entries l >= that filter's landmark count are ignored; count is the
 * length of keep (landmarks l >= count have no entry and are kept).  Kept landmarks stay in order and are renumbered
 * 0..N'-1; x and P become exactly the kept rows/columns (no arithmetic, bitwise).  Deferred slots are folded first.
 * Synchronises.  Returns N' or a negative status.
 * Pose, P_RR, the counters (ekf_get_stats) and the host mirror's pose are unchanged; ekf_num_landmarks reports N'.  Decision-log
 * entries are NOT rewritten: they keep the indices they were written with.  A sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY is returned
 * unchanged and the state is left as it was; bad arguments return EKF_ERR_BAD_ARG and leave the handle untouched.  Every device
 * buffer of the filter ends as ekf_set_state of the reduced state would leave it: later New landmarks reuse the freed rows, the
 * capacity stays, a loaded script stays loaded, ekf_reserve works before and after, immediate-mode calls stream again afterwards. */
int ekf_remove_landmarks(ekf_handle h, int index, const unsigned char *keep, int count);
/* The same for every filter of a batch in one pass: keep [batch][ld_keep]; n_out[batch] (may be NULL) receives N'.  Returns
 * EKF_OK or a negative status. */
int ekf_batch_remove_landmarks(ekf_handle h, const unsigned char *keep, int ld_keep, int *n_out);
/* The 2x2 covariance of every landmark of filter `index`: cov_out[l][3] = (xx, xy, yy) for l < min(N, n_max), taken from
 * the always-current diagonal blocks.  It does NOT fold the open window and does not launch a dense pass.  Synchronises.
 * Returns N. */
int ekf_get_landmark_covs(ekf_handle h, int index, double *cov_out, int n_max);

/* Frame changes on the device, P <- J P J^T in place (no trip through ekf_get_state / ekf_set_state).
 * ekf_transform_frame: a KNOWN rigid transform of the whole estimate of filter `index`.  frame = (t_x, t_y, theta) is the pose of
 * the NEW frame's origin expressed in the CURRENT frame; with Q = Rot(-theta): p' = Q (p - t), L_l' = Q (L_l - t), phi' = phi - theta,
 * and every block of P is rotated accordingly (theta = 0: P is unchanged bit for bit and x is the single subtraction).  cos(theta) and
 * sin(theta) are taken once on the host (libm).  The heading is NOT wrapped (the filter wraps it nowhere).  A compass measurement is
 * absolute: after a rigid transform the caller's compass readings shift by -theta.  A loaded script's truth poses are not transformed.
 * ekf_anchor_at_robot: re-expresses every landmark relative to the robot's ESTIMATED pose, L_l' = Rot(-phi) (L_l - p), and moves the
 * pose uncertainty into the landmarks (P' = J P J^T with the Jacobian of that map): afterwards the pose is exactly (0, 0, 0) and every
 * robot row and column of P exactly zero -- the reference's start state with a map -- and the landmark blocks are the joint covariance
 * of the predicted relative measurements.  Because P_RR = 0, a NEES sample (ekf_record_truth) is meaningless until the next
 * propagation, and the caller's truth must be re-expressed in the new frame too.
 * Both: deferred slots are folded first (at most one window closes, none on a settled handle); a streaming launch is stopped and
 * immediate-mode calls stream again afterwards; synchronise; return EKF_OK or a negative status.  The landmark count, the counters
 * (ekf_get_stats) and the decision log are unchanged (log entries are frame-free); the host mirror shows the new pose and P_RR.  A
 * sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY is returned unchanged and the state is left as it was; bad arguments (index out of
 * range, NULL, a non-finite frame) return EKF_ERR_BAD_ARG and leave the handle untouched.  Every device buffer ends as
 * ekf_set_state of the transformed state would leave it: the capacity stays, a loaded script stays loaded, ekf_reserve works before
 * and after.  The batch forms transform every filter in one launch sequence (frames [batch][3]: one frame per filter). */
int ekf_transform_frame(ekf_handle h, int index, const double frame[3]);
int ekf_batch_transform_frame(ekf_handle h, const double *frames /*[batch][3]*/);
int ekf_anchor_at_robot(ekf_handle h, int index);
int ekf_batch_anchor_at_robot(ekf_handle h);

/* Map joining on the device: the landmarks of filter src_index of `src` (a local submap) are appended behind the landmarks of
 * filter dst_index of `dst`, without a trip through ekf_get_state / ekf_set_state.
 * CONTRACT, the caller's responsibility: (1) frame -- the origin of src's frame is dst's CURRENT ESTIMATED robot pose, which is
 * what a caller gets who starts the local filter fresh (x = 0_3, P = 0) or anchors it at the moment the previous join ended;
 * (2) independence -- the two estimates share no information (no measurement went into both).
 * With dst = (pose p = (t, phi), landmarks L_0..L_{Ng-1}, P_g), src = (pose q = (u, psi), landmarks M_0..M_{Ns-1}, P_s),
 * C = Rot(phi), J = [[0,-1],[1,0]]:  the old landmarks stay bit for bit, M_k' = t + C M_k becomes landmark Ng + k (order kept),
 * the robot becomes src's robot, t' = t + C u, phi' = phi + psi (not wrapped), and dst's old pose is marginalised out:
 * P' = J_g P_g J_g^T + J_s P_s J_s^T.  With G_k = [I | C J M_k], G_R = [[I, C J u], [0 0 1]], C3 = diag(C, 1):
 *   old m x old l  unchanged bit for bit        old m x new k  P_mR G_k^T        new k x new l  G_k P_RR G_l^T + C P_s,kl C^T
 *   old m x robot  P_mR G_R^T                   new k x robot  G_k P_RR G_R^T + C P_s,kR C3^T
 *   robot x robot  G_R P_RR G_R^T + C3 P_s,RR C3^T
 * cos(phi) and sin(phi) are taken once on the host (libm).  Joining into a fresh filter reproduces src's state exactly; joining a
 * fresh src leaves dst exactly as it was.  Landmarks that both maps hold are NOT recognised or fused here: they stay two landmarks
 * (ekf_find_duplicates lists them, ekf_fuse_landmarks fuses them).
 * A NEES sample (ekf_record_truth) needs the caller's truth to be a pose in dst's frame, as before the join.
 * src may be the same handle as dst when the indices differ, or a handle of another capacity, kernel family and pipeline mode on
 * the same device (another device: EKF_ERR_BAD_ARG).  src is only read: its state, counters, decision log and loaded script stay
 * bitwise what they were, and its immediate-mode calls stream again afterwards.  Both filters' deferred slots are folded first
 * (at most one window each, none on a settled handle), streaming launches are stopped, the call orders the two handles' streams
 * itself and synchronises.  Returns the new landmark count Ng + Ns or a negative status.
 * Ng + Ns > ekf_capacity(dst): EKF_ERR_CAPACITY with both filters' exported states untouched (their deferred slots have been
 * folded and streaming launches stopped nonetheless); it is NOT sticky (no join kernel ran): call ekf_reserve and join again.
 * Other bad arguments (NULL, an index out of range, src == dst with equal indices) return EKF_ERR_BAD_ARG and leave both
 * handles untouched; a sticky EKF_ERR_TIMEOUT / EKF_ERR_CAPACITY of either handle is returned unchanged with nothing modified.
 * dst afterwards: counters and decision log unchanged, the host mirror shows the new pose, P_RR and landmark count, and every
 * device buffer ends as ekf_set_state of the joined state would leave it (a loaded script stays loaded, ekf_reserve works before
 * and after).
 * ekf_batch_join_map: filter b of src into filter b of dst for every b in one launch sequence; equal batch sizes, src != dst.
 * Returns EKF_OK or a negative status; one filter without room fails the whole call with nothing modified. */
int ekf_join_map(ekf_handle dst, int dst_index, ekf_handle src, int src_index);
int ekf_batch_join_map(ekf_handle dst, ekf_handle src);

/* Submap extraction on the device: the way OUT of a filter without the dense export.  ekf_extract_map replaces filter dst_index of
 * `dst` with the marginal of filter src_index of `src` over the robot and the landmarks ids[0..count): landmark k of dst is
 * landmark ids[k] of src.  The ids are 0-based, pairwise distinct, in [0, N_src), and may come in ANY order.
 *     x' = x[sel],  P' = P[sel, sel],  sel = [0, 1, 2, 3 + 2 ids[0], 4 + 2 ids[0], 3 + 2 ids[1], ...]
 * There is no arithmetic: the result is bitwise what ekf_get_state(src) returns at the same point, indexed by sel.
 * ids == NULL selects every landmark in order (count is ignored): a device-side copy or fork, also between handles of different
 * capacity, kernel family and pipeline mode.  count == 0 with ids != NULL selects the pose and P_RR alone.  The ids are the
 * caller's choice (the landmarks near the robot, one side of a split, a handful for a joint-compatibility test): ekf_get_x is 16
 * bytes per landmark to choose from.  Returns the new landmark count of dst or a negative status.
 * NOT INDEPENDENT: an extracted map shares all its information with its source.  Joining it back with ekf_join_map breaks that
 * call's contract (2) and counts the information twice.  Extraction is for read-outs, forks, checkpoints and hand-offs.
 * src is only read, exactly as in ekf_join_map: its deferred slots are folded first (at most one window), a streaming launch is
 * stopped and its immediate-mode calls stream again afterwards; its state, counters, decision log and loaded script stay bitwise
 * the same.  A sticky EKF_ERR_TIMEOUT of src is returned unchanged with nothing modified; a sticky EKF_ERR_CAPACITY of src does not
 * block the call (its state is valid and only read, as for ekf_find_duplicates).  src may be dst itself when the indices differ, or
 * any handle on the same device.
 * dst is treated as ekf_set_state treats it: every device buffer ends as ekf_set_state of the extracted state would leave it (the
 * tiles and vector entries of a larger previous map are zeroed), sticky errors are cleared, counters and decision log stay, a
 * loaded script stays loaded, the host mirror shows the new pose, P_RR and count, and immediate-mode calls stream again.
 * count > ekf_capacity(dst): EKF_ERR_CAPACITY, NOT sticky, neither filter's exported state changes (src has been folded
 * nonetheless): call ekf_reserve and extract again.  EKF_ERR_BAD_ARG: a NULL handle, an index out of range, count < 0, an id out
 * of range or repeated, handles on different devices, dst == src with equal indices (in-place reordering is not offered).  The list
 * is checked on the host before any handle is touched, and against src's landmark count once src is at rest, before any kernel of
 * the call runs.
 * ekf_batch_extract_map: filter b of src into filter b of dst for every b in one launch sequence; equal batch sizes, src != dst;
 * filter b's list is ids[b * ld_ids .. + count[b]).  One filter without room fails the whole call with nothing modified; filter b
 * gets the bits of the one-filter call on b.  Returns EKF_OK or a negative status, n_out[b] = new landmark count.
 * ekf_get_submap: the same marginal to the host.  x_out[3 + 2 count], P_out column-major with ld >= 3 + 2 count, bitwise
 * symmetric; the padding rows between 3 + 2 count and ld are not written.  x_out = P_out = NULL returns the size 3 + 2 count.
 * Follows ekf_get_state's quiescing rule, synchronises and leaves the filter bitwise as ekf_get_state at the same point would.
 * The device gathers straight into a transient dense staging buffer of (3 + 2 count)^2 doubles and one copy follows: the full P
 * is never formed.  Returns 3 + 2 count or a negative status. */
int ekf_extract_map(ekf_handle dst, int dst_index, ekf_handle src, int src_index, const int *ids, int count);
int ekf_batch_extract_map(ekf_handle dst, ekf_handle src, const int *ids /*[batch][ld_ids] or NULL*/, int ld_ids,
                          const int *count /*[batch]; ignored when ids == NULL*/, int *n_out /*[batch] or NULL*/);
int ekf_get_submap(ekf_handle h, int index, const int *ids, int count, double *x_out, double *P_out, int ld);

/* Map assessment on the device: is the whole state (pose AND map) consistent, and is P still a covariance?  A Cholesky
 * factorisation P_LL = U^T U of the settled landmark covariance in a scratch copy (64-row tile steps over the tile layout; the
 * filter itself is only read), the robot block last:
 *     U^T [y | W] = [e_L | P_LR],   S_R = P_RR - W^T W,   r = e_R - W^T y,
 *     nees_map = |y|^2,  nees_joint = |y|^2 + r^T S_R^-1 r,  logdet_map = 2 sum log U_ii,  logdet_joint = logdet_map + log det S_R.
 * e = x - x_true with the heading component wrapped to [-pi, pi) as ekf_record_truth wraps it; x_true lists the landmarks in the
 * filter's own order (the caller's contract).  x_true == NULL: the NEES fields are NaN, everything else is filled (a health check).
 * info = k > 0: every NEES and log-det field and cov_robot_given_map are NaN, min_pivot holds the offending pivot; info = -1: the
 * map fields and cov_robot_given_map are valid, the joint fields NaN.  N = 0: the map fields are 0, the joint fields come from P_RR.
 * A pivot that is not positive is NOT an error status: the call returns EKF_OK with info set, and the filter works on as before.
 * The filter's exported state, counters, decision log, loaded script and host mirror are bitwise what ekf_get_state at the same
 * point would leave: deferred slots are folded first, a streaming launch is stopped and immediate-mode calls stream again
 * afterwards.  The call synchronises.  A sticky EKF_ERR_TIMEOUT is returned unchanged; a sticky EKF_ERR_CAPACITY does not block
 * the call.  Bad arguments (NULL out, index out of range, ld_true smaller than the largest state of the batch when x_true is given)
 * return EKF_ERR_BAD_ARG.  No floating-point atomics, every sum in a fixed order: two calls on an unchanged state return the same
 * bits, and filter b of the batch form returns the bits of the one-filter call on b.  The batch form factors every filter in the
 * same launch sequence (3 launches per tile step, whatever the batch).
 * The scratch -- one P_LL buffer per filter plus four right-hand-side columns -- is allocated at the first call, kept on the handle
 * (ekf_device_bytes counts it, ekf_reserve re-sizes it) and freed by ekf_destroy. */
typedef struct ekf_joint {
    int n_landmarks;               /* N of the filter at the call */
    int info;                      /* 0 ok; k > 0: the leading minor of order k of P_LL is not positive (pivot <= 0 or NaN at
                                      landmark-space row k-1), LAPACK's potrf convention; -1: P_LL is fine, but the pose block
                                      conditioned on the map is not positive definite (fresh or anchored filter: P_RR = 0) */
    double nees_map;               /* e_L^T P_LL^-1 e_L, 2N dof  */
    double nees_joint;             /* e^T P^-1 e, 3 + 2N dof     */
    double logdet_map;             /* log det P_LL               */
    double logdet_joint;           /* log det P                  */
    double min_pivot, max_pivot;   /* smallest / largest U_ii^2 over the 2N landmark rows (conditional variances) */
    double cov_robot_given_map[9]; /* S_R = P_RR - P_RL P_LL^-1 P_LR, row-major */
} ekf_joint;
int ekf_joint_consistency(ekf_handle h, int index, const double *x_true /*[n] or NULL*/, ekf_joint *out);
int ekf_batch_joint_consistency(ekf_handle h, const double *x_true /*[batch][ld_true] or NULL*/, int ld_true, ekf_joint *out /*[batch]*/);
/* Diagnostic: the upper factor U (U^T U = P_LL) of filter `index` from the LAST consistency call, dense 2N x 2N column-major,
 * ld >= 2N; EKF_ERR_STATE when the state changed since (or no call covered the filter).  Returns 2N.  Synchronises. */
int ekf_debug_joint_factor(ekf_handle h, int index, double *U_out, int ld);

/* Duplicate search on the device: which landmarks i < j of a filter are the same point?  The pairwise gate with the cross
 * covariance, which after ekf_join_map is of the size of the landmarks' own blocks (leaving it out makes the gate meaningless):
 *     d = L_i - L_j = (dx, dy),   S = P_ii + P_jj - P_ij - P_ij^T = (a b; b c),   det = a c - b^2,
 *     a = P_ii.xx + P_jj.xx - 2 P_ij[0][0],  b = P_ii.xy + P_jj.xy - P_ij[0][1] - P_ij[1][0],  c = P_ii.yy + P_jj.yy - 2 P_ij[1][1],
 *     degenerate: !(a > 0 && det > 0) (catches NaN);   else d2 = (c dx^2 - 2 b dx dy + a dy^2) / det.
 * P_ij is read where it lives, in one streaming read of the settled upper triangle; the filter itself is only read.
 * Considered pairs: max_dist > 0: only pairs with dx^2 + dy^2 <= max_dist^2 (groups of 32 landmarks whose bounding boxes are
 * further apart are skipped unread, with the same result); max_dist <= 0: no Euclidean bound.  split = 0: all pairs; 0 < split <= N:
 * only i < split <= j, the old x new pairs after an ekf_join_map that returned Ng + Ns, called with split = Ng.
 * A considered pair is listed iff it is not degenerate and d2 <= gate; degenerate considered pairs are counted into
 * n_degenerate_out (may be NULL) and never listed.  The list is ordered by (i, j); the first min(found, max_pairs) pairs are
 * written.  ekf_find_duplicates returns `found`, which may exceed max_pairs, or a negative status; pairs_out == NULL with
 * max_pairs == 0 is a count-only call.  ekf_batch_find_duplicates writes filter b's list at pairs_out + b * max_pairs and its count
 * to n_found_out[b], takes one split per filter (NULL: all 0) and returns EKF_OK or a negative status.  N < 2 finds nothing.
 * The filter's exported state, counters, decision log, loaded script and host mirror are bitwise what ekf_get_state at the same
 * point would leave: deferred slots are folded first, a streaming launch is stopped and immediate-mode calls stream again
 * afterwards.  The call synchronises.  A sticky EKF_ERR_TIMEOUT is returned unchanged; a sticky EKF_ERR_CAPACITY does not block
 * the call.  Bad arguments (NULL outputs where not allowed, index out of range, gate not finite or negative, max_dist NaN,
 * split < 0 or > N, max_pairs < 0) return EKF_ERR_BAD_ARG.  Pairs are appended through an integer counter and sorted on the host,
 * no floating-point atomics: every count, index and the bits of every d2 are the same on every call on an unchanged state, and
 * filter b of the batch form returns exactly what the one-filter call on b returns.
 * The scratch -- a bounding box per 32 landmarks, counters, and a pair list that grows when a call finds more than it holds (the
 * search then runs once more) -- is allocated at the first call, kept on the handle (ekf_device_bytes counts it, ekf_reserve
 * re-sizes it) and freed by ekf_destroy.  Marginalising the duplicate out with ekf_remove_landmarks is the conservative way to
 * use the list; ekf_fuse_landmarks below fuses the two estimates instead. */
typedef struct ekf_dup_pair {
    int i, j;   /* landmark numbers, i < j */
    double d2;  /* d^T S^-1 d */
} ekf_dup_pair;
int ekf_find_duplicates(ekf_handle h, int index, double gate, double max_dist, int split, ekf_dup_pair *pairs_out, int max_pairs,
                        int *n_degenerate_out /* may be NULL */);
int ekf_batch_find_duplicates(ekf_handle h, double gate, double max_dist, const int *split /*[batch] or NULL = all 0*/,
                              ekf_dup_pair *pairs_out /*[batch][max_pairs]*/, int max_pairs, int *n_found_out /*[batch]*/,
                              int *n_degenerate_out /*[batch] or NULL*/);

/* Landmark fusion on the device: the pairs (i_k, j_k), k < n_pairs, of one filter are declared the same point.  The equality
 * constraint L_i = L_j of all pairs as ONE update of the whole state, then the removal of every j_k:
 *     H (2m x n): +I_2 at landmark i_k, -I_2 at landmark j_k;   d = H x;   W = P H^T (column pair k = P[:, i_k] - P[:, j_k]);
 *     S = H W + slack I = U^T U;   V = W U^-1;   y = U^-T d;   x <- x - V y;   P <- P - V V^T;
 * then rows and columns of every j_k go and the kept landmarks are renumbered, exactly as ekf_remove_landmarks with keep[j_k] = 0.
 * What is subtracted from P is symmetric and positive semidefinite by construction.  slack >= 0 (m^2) is an isotropic variance on
 * the constraint: 0 is the exact constraint (afterwards, before the removal, the rows of i and j coincide up to rounding), a
 * positive value tolerates pairs that are not quite the same point.  Unlike marginalising j out (ekf_remove_landmarks alone) the
 * second observation's information is kept.
 * Only i and j of a pair are read (d2 is ignored: the list of ekf_find_duplicates, thinned to a one-to-one matching, can be passed
 * on).  Every pair needs 0 <= i < j < N and a landmark may appear in at most one pair of the call; anything else, a negative or
 * non-finite slack, a NULL list with n_pairs > 0 or an index out of range is EKF_ERR_BAD_ARG, found on the host before the handle
 * is touched.  n_pairs = 0 is a no-op that leaves an open window open.
 * Otherwise deferred slots are folded first, a streaming launch is stopped (immediate-mode calls stream again afterwards), and the
 * list is processed in rounds of at most ekf_window(h) pairs in list order, each round a complete joint update of its pairs with
 * one dense pass over P_LL (in place, in either pipeline mode); conditioning on the constraints round after round equals
 * conditioning on all of them at once up to rounding.  If S of a round is not positive definite (a pivot <= 0 or NaN: e.g. j an
 * exact copy of i with slack = 0), that round and all later ones are NOT applied: the state is that after the completed rounds
 * with exactly their j removed, and *n_fused_out (may be NULL) < n_pairs says so.  This is a result, not an error.
 * ekf_fuse_landmarks returns the new landmark count or a negative status.  ekf_batch_fuse_landmarks takes filter b's list at
 * pairs + b * ld_pairs with n_pairs[b] <= ld_pairs pairs (0: the filter stays as it is), writes n_fused_out[b] (may be NULL) and
 * n_landmarks_out[b], runs every filter in the same launch sequence and returns EKF_OK or a negative status.
 * A sticky EKF_ERR_TIMEOUT / EKF_ERR_CAPACITY is returned unchanged with nothing modified.  Counters, decision log and a loaded
 * script stay; the host mirror shows the new pose, P_RR and landmark count, and every device buffer ends as ekf_set_state of the
 * fused, reduced state would leave it.  The call synchronises.  No atomics, one writer per value, every sum in a fixed order: the
 * same call on the same state gives the same bits, and filter b of the batch form gets the bits of the one-filter call on b.
 * The scratch -- the pair table, one round's factor (at most 64 x 64) and right-hand sides -- is allocated at the first call
 * that has a pair, kept on the handle (ekf_device_bytes counts it, ekf_reserve re-sizes it) and freed by ekf_destroy. */
int ekf_fuse_landmarks(ekf_handle h, int index, const ekf_dup_pair *pairs, int n_pairs, double slack, int *n_fused_out /* may be NULL */);
int ekf_batch_fuse_landmarks(ekf_handle h, const ekf_dup_pair *pairs /*[batch][ld_pairs]*/, int ld_pairs, const int *n_pairs /*[batch]*/,
                             double slack, int *n_fused_out /*[batch] or NULL*/, int *n_landmarks_out /*[batch]*/);

/* A scan with the caller's own data association, applied on the device as joint updates: measurement k of the call IS landmark
 * ids[k] (0-based, as in ekf_remove_landmarks); ids[k] == -1: no measurement, skipped (its z and R are not looked at).  z and R use
 * the layouts of ekf_batch_update.  The filter's gates and condition limit are NOT consulted -- the decision is the caller's
 * (joint-compatibility search over ekf_joint_compat below, global nearest neighbour, known ids) -- and counters and decision log
 * stay as they are: book NIS from d2_out if you want it.  (To force a NEW landmark: ekf_add_landmarks below, Update.cpp:155-177 for any number of
 * measurements in one call; ekf_update_joint is search, this update and the additions together.)
 * The non-skipped measurements run in rounds of at most ekf_window(h) in list order.  A round with measurements k = 0..m-1 of
 * landmarks i_k is ONE update, every measurement linearised at the round's entry state (C = Rot(phi), J = [[0,-1],[1,0]]):
 *     dp_k = L_ik - p;   H_R,k = [-C^T | -C^T J dp_k]  (Update.cpp:112-114);   H_L = C^T;   d_k = C^T dp_k - z_k  (= -res);
 *     column pair k of W = P[:, 0:3] H_R,k^T + P[:, L_ik] C;   S = H W + blockdiag(R_k) = U^T U (from the upper triangle);
 *     V = W U^-1;   y = U^-T d;   x <- x - V y  (= x + K res);   P <- P - V V^T.
 * cos phi and sin phi are taken once per round ON THE DEVICE (the device library's cos() and sin() of x[2], which may differ from
 * the host's libm by an ulp).  With a window of 1 this is the reference's sequence of Old updates for those landmarks.  The same
 * landmark may appear several times, in one round too: R keeps S regular.
 * S of a round counts as not positive definite when a pivot of its factorisation is not above 2^-44 of its own diagonal entry of S
 * (or NaN) -- below that a pivot is rounding noise of the elimination, of either sign; e.g. the same landmark twice with R = 0 on
 * an anchored filter.  That round and all later ones are then NOT applied: the state is that after the completed rounds and
 * *n_applied_out (may be NULL) < the number of non-skipped measurements says so.  This is a result, not an error.
 * d2_out[k] (may be NULL): the joint Mahalanobis distance of the measurements of k's round up to and including k, the running
 * sum of y^2 over that round's columns 0 .. 2 k_round + 1 -- the last entry of a round is the round's joint distance, and with
 * rounds of 1 it is the reference's Mahal_dist for that landmark; NaN for skipped and for unapplied measurements.
 * Checked on the host before the handle is touched: n_z < 0, a NULL z / R / ids with n_z > 0, an id < -1, a non-finite z or R of a
 * non-skipped measurement, an index out of range -- EKF_ERR_BAD_ARG; then the ids against the landmark count (id >= N:
 * EKF_ERR_BAD_ARG, the state untouched).  n_z = 0, or every id -1, is a no-op that leaves an open window open.
 * Otherwise, as ekf_fuse_landmarks: deferred slots are folded first, a streaming launch is stopped (immediate-mode calls stream
 * again afterwards), each round costs one dense pass over P_LL (in place, in either pipeline mode), a sticky EKF_ERR_TIMEOUT /
 * EKF_ERR_CAPACITY is returned unchanged with nothing modified, the host mirror shows the new pose and P_RR, every device buffer
 * ends as ekf_set_state of the result would leave it, and the call synchronises.  No atomics, one writer per value, every sum in a
 * fixed order: the same bits on every call, and filter b of the batch form gets the bits of the one-filter call on b.
 * ekf_update_matched returns the landmark count (unchanged) or a negative status; the batch form takes filter b's lists at
 * z + b * n_z * 2, R + b * n_z * 4, ids + b * n_z (ragged lists: pad with -1) and returns EKF_OK or a negative status.
 * The scratch -- the call's measurement table (56 bytes per measurement, for at least 64 per filter), one round's table, and the
 * scratch of ekf_fuse_landmarks -- is allocated at the first call with a measurement, kept on the handle (ekf_device_bytes
 * counts it, ekf_reserve builds it again) and freed by ekf_destroy. */
int ekf_update_matched(ekf_handle h, int index, const double *z /*[n_z][2]*/, const double *R /*[n_z][4], column-major 2x2*/,
                       const int *ids /*[n_z]*/, int n_z, int *n_applied_out /* may be NULL */, double *d2_out /*[n_z] or NULL*/);
int ekf_batch_update_matched(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                             const int *ids /*[batch][n_z]*/, int n_z, int *n_applied_out /*[batch] or NULL*/,
                             double *d2_out /*[batch][n_z] or NULL*/);

/* The score of ONE association hypothesis, nothing applied: the same S, factor and y as a round of ekf_update_matched (the same
 * kernel) for at most EKF_MAX_PENDING = 32 non-skipped measurements, whatever the window; more is EKF_ERR_BAD_ARG, and so is
 * everything ekf_update_matched refuses, and a NULL d2_out with n_z > 0.  d2_out[k] is the joint distance of the hypothesis cut
 * after measurement k -- the quantity a branch-and-bound search (JCBB) extends by one pairing, free from the right-looking
 * factorisation; NaN for skipped entries, and from the first pivot that is not positive (the rule above) on: the call still returns
 * EKF_OK.  For a hypothesis that fits one round of ekf_update_matched the two calls give the same bits of d2.
 * The filter is only read, behind the rule of ekf_find_duplicates (deferred slots folded, a streaming launch stopped; a sticky
 * EKF_ERR_TIMEOUT ends the call, a sticky EKF_ERR_CAPACITY does not); a hypothesis without a measurement folds nothing. */
int ekf_joint_compat(ekf_handle h, int index, const double *z, const double *R, const int *ids, int n_z, double *d2_out /*[n_z]*/);
int ekf_batch_joint_compat(ekf_handle h, const double *z, const double *R, const int *ids, int n_z, double *d2_out /*[batch][n_z]*/);

/* ekf_update_matched with every round ITERATED (the iterated EKF update, Gauss-Newton on the round's MAP cost): the measurement
 * model is bilinear in heading and offset, so one linearisation at a heading that is off by e misplaces a landmark at range r by
 * about r e^2 / 2 -- decimetres behind a blind stretch or a coarse ekf_reset_pose.  Rounds, skips, layouts, host checks, settling,
 * streaming, sticky statuses, the mirror and the synchronising behaviour are exactly those of ekf_update_matched.  One round, entry
 * state (x^, P), linearisation points xi_0 = x^, xi_1, ... (held for the pose and the round's landmarks: nothing else enters H, d):
 *     H_i, h(xi_i): as in ekf_update_matched, at xi_i; cos and sin of xi_i[2] from the device library, once per iteration;
 *     d_0 = h(x^) - z, by ekf_update_matched's own expression;   i > 0:  d_i = (h(xi_i) - z) + H_i (x^ - xi_i);
 *     W_i = P H_i^T;   S_i = H_i W_i + blockdiag(R_k) = U_i^T U_i  (the 2^-44 pivot rule, in every iteration);   y_i = U_i^-T d_i;
 *     xi_i+1 = x^ - W_i S_i^-1 d_i  on the touched components;   step_i = max |xi_i+1 - xi_i| over them, metres and radians alike;
 * the round stops behind iteration i when step_i <= tol or i + 1 == max_iter, and then
 *     x <- x^ - V_i y_i,   P <- P - V_i V_i^T,   V_i = W_i U_i^-1.
 * A pivot refused in ANY iteration refuses the round and all later ones, as in ekf_update_matched: a result, not an error.
 * iters_out[k] (may be NULL): the factorisations of k's round; 0 for skipped and unapplied entries.  step_out[k] (may be NULL): the
 * last step of k's round, NaN for skipped and unapplied entries; a value above tol says that the round ran out of iterations.
 * d2_out: the running joint distance from iteration 0 -- the PRIOR's compatibility, the bits ekf_joint_compat gives at the round's
 * entry state.  max_iter outside 1 .. EKF_ITER_MAX, or a tol that is negative or not finite, is EKF_ERR_BAD_ARG, found on the host
 * before the handle is touched.  With max_iter = 1 the call is ekf_update_matched bit for bit.  The same bits on every call, and
 * filter b of the batch form gets the bits of the one-filter call on b.  The whole iteration runs inside the round's one factor
 * kernel, on the pose and the matched landmarks alone: an iteration more costs one factorisation, not a pass over the state.
 * The scratch of ekf_update_matched and 12 bytes more per measurement (for at least 64 per filter), allocated at the first iterated
 * call with a measurement, kept on the handle (ekf_device_bytes counts it, ekf_reserve builds it again) and freed by ekf_destroy. */
#define EKF_ITER_MAX 16
int ekf_update_matched_iter(ekf_handle h, int index, const double *z, const double *R, const int *ids, int n_z, int max_iter, double tol,
                            int *n_applied_out /* may be NULL */, double *d2_out /*[n_z] or NULL*/, int *iters_out /*[n_z] or NULL*/,
                            double *step_out /*[n_z] or NULL*/);
int ekf_batch_update_matched_iter(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                                  const int *ids /*[batch][n_z]*/, int n_z, int max_iter, double tol, int *n_applied_out /*[batch] or NULL*/,
                                  double *d2_out /*[batch][n_z] or NULL*/, int *iters_out /*[batch][n_z] or NULL*/,
                                  double *step_out /*[batch][n_z] or NULL*/);

/* Absolute observations, applied on the device as joint updates: a position fix of the robot (GNSS, an overhead camera), a heading
 * from another source, a surveyed position of a landmark.  The reference's one absolute observation is its scalar compass
 * (kalmanfilter.cpp:96-130, called at slam.cpp:144-147; here ekf_update_compass); this is its generalisation, the contract that of
 * ekf_update_matched with another H.  Entry k of the call is of kind what[k]: */
#define EKF_FIX_SKIP     (-1)  /* no observation: z and R not looked at */
#define EKF_FIX_POSITION (-2)  /* z = (x_R, y_R) + v,  cov(v) = R (2x2, layout of ekf_update_matched) */
#define EKF_FIX_HEADING  (-3)  /* z[0] = phi + v,  var(v) = R[0];  z[1], R[1..3] not looked at */
/* what[k] >= 0: z = L_what[k] + v, a fix of that landmark's position (0-based, as in ekf_remove_landmarks).
 * The non-skipped entries run in rounds of at most ekf_window(h) in list order.  A round is ONE update, every entry one slot, two
 * columns of W; with n = 3 + 2N and e_r the unit vectors:
 *     POSITION:    rows e_0, e_1 of H;           columns P[:, 0], P[:, 1];            d = (x_R - z_0, y_R - z_1)
 *     HEADING:     row e_2 and an inert row;     columns P[:, 2], 0;                  d = (wrap(phi - z_0), 0)
 *     landmark i:  rows e_{3+2i}, e_{4+2i};      columns P[:, 3+2i], P[:, 4+2i];      d = L_i - z
 *     S = H W + blockdiag(R_k) = U^T U (from the upper triangle: of R's off-diagonal pair R(0,1) is used);
 *     V = W U^-1;   y = U^-T d;   x <- x - V y;   P <- P - V V^T.
 * wrap(e) = e - 2 pi floor((e + pi) / (2 pi)), in [-pi, pi); the heading itself stays unwrapped afterwards, as everywhere else.
 * The inert row of a heading entry has a zero row and column of S, the diagonal entry exactly 1 and d = 0: its pivot is 1, its y
 * and its column of V are exact zeros.  Nothing is linearised, so the result depends on how the list is cut into rounds by rounding
 * alone.  R = 0 is legal (a hard fix); the same thing may be fixed several times in one round where R keeps S regular.
 * S of a round counts as not positive definite by ekf_update_matched's rule: a pivot not above 2^-44 of its own diagonal entry of S
 * (or NaN), e.g. the same thing fixed twice with R = 0.  That round and all later ones are then NOT applied: the state is that after
 * the completed rounds and *n_applied_out (may be NULL) < the number of non-skipped entries says so.  A result, not an error.
 * d2_out[k] (may be NULL): the running sum of y^2 of k's round up to and including k -- the joint Mahalanobis distance of the
 * round's entries so far; NaN for skipped and for unapplied entries.  A HEADING fix alone in a round: wrap(phi - z)^2 / (P_phiphi + R).
 * Checked on the host before the handle is touched: n < 0, a NULL z / R / what with n > 0, what < -3, a non-finite value among
 * those a kind reads (HEADING: z[0] and R[0] only), a negative R[0] of a heading entry, an index out of range -- EKF_ERR_BAD_ARG;
 * then landmark ids against the landmark count (id >= N: EKF_ERR_BAD_ARG, the state untouched).  n = 0, or every entry skipped,
 * is a no-op that leaves an open window open.  A POSITION or HEADING fix is valid on a filter without landmarks.
 * Otherwise, as ekf_update_matched: deferred slots are folded first, a streaming launch is stopped (immediate-mode calls stream
 * again afterwards), each round costs one dense pass over P_LL (in place, in either pipeline mode), a sticky EKF_ERR_TIMEOUT /
 * EKF_ERR_CAPACITY is returned unchanged with nothing modified, counters and decision log stay as they are, the host mirror shows
 * the new pose and P_RR, every device buffer ends as ekf_set_state of the result would leave it, and the call synchronises.  No
 * atomics, one writer per value, every sum in a fixed order: the same bits on every call, and filter b of the batch form gets the
 * bits of the one-filter call on b.
 * ekf_update_fixes returns the landmark count (unchanged) or a negative status; the batch form takes filter b's lists at
 * z + b * n * 2, R + b * n * 4, what + b * n (ragged lists: pad with EKF_FIX_SKIP) and returns EKF_OK or a negative status.
 * The scratch is that of ekf_update_matched (the same blocks: a handle that has made either call has them). */
int ekf_update_fixes(ekf_handle h, int index, const double *z /*[n][2]*/, const double *R /*[n][4], column-major 2x2*/,
                     const int *what /*[n]*/, int n, int *n_applied_out /* may be NULL */, double *d2_out /*[n] or NULL*/);
int ekf_batch_update_fixes(ekf_handle h, const double *z /*[batch][n][2]*/, const double *R /*[batch][n][4]*/,
                           const int *what /*[batch][n]*/, int n, int *n_applied_out /*[batch] or NULL*/,
                           double *d2_out /*[batch][n] or NULL*/);

/* The score of ONE list of fixes, nothing applied -- the chi-square test to run on a GNSS outlier before applying it: the same S,
 * factor and y as a round of ekf_update_fixes (the same kernel) for at most EKF_MAX_PENDING = 32 non-skipped entries, whatever the
 * window; more is EKF_ERR_BAD_ARG, and so is everything ekf_update_fixes refuses, and a NULL d2_out with n > 0.  d2_out[k]: the
 * joint distance of the list cut after entry k; NaN for skipped entries, and from the first refused pivot on (the call still
 * returns EKF_OK).  For a list that fits one round of ekf_update_fixes the two calls give the same bits of d2.  The filter is only
 * read, behind the rule of ekf_joint_compat (deferred slots folded, a streaming launch stopped; a sticky EKF_ERR_TIMEOUT ends the
 * call, a sticky EKF_ERR_CAPACITY does not); a list without an entry folds nothing. */
int ekf_fix_compat(ekf_handle h, int index, const double *z, const double *R, const int *what, int n, double *d2_out /*[n]*/);
int ekf_batch_fix_compat(ekf_handle h, const double *z, const double *R, const int *what, int n, double *d2_out /*[batch][n]*/);

/* Landmark measurements in POLAR form with known ids, applied on the device as joint updates: a range alone (UWB, radio or acoustic
 * beacons), a bearing alone (a camera), or both with the noise in polar coordinates (laser, radar) -- no host-side conversion that
 * linearises the noise first.  The contract is that of ekf_update_matched / ekf_joint_compat with another h and H; everything not
 * said here is theirs word for word.  Entry k measures landmark ids[k] (-1: skipped, its z, R and kind not looked at) by kind[k]: */
#define EKF_POLAR_RANGE   1   /* z[0] = |L_i - p| + v,                  var(v) = R[0];  z[1], R[1..3] not looked at */
#define EKF_POLAR_BEARING 2   /* z[1] = atan2(dy, dx) - phi + v,        var(v) = R[3];  z[0], R[0..2] not looked at */
#define EKF_POLAR_BOTH    3   /* z = (range, bearing) + v,  cov(v) = R  (2x2 column-major over (range, bearing)) */
/* The non-skipped entries run in rounds of at most ekf_window(h) in list order.  A round is ONE update, every entry linearised at
 * the round's entry state, one slot and two columns of W each; with dx = L_i.x - x_R, dy = L_i.y - y_R, q = dx^2 + dy^2, r = sqrt(q):
 *     range row:    h = r,                     H_R = [-dx / r, -dy / r,  0],   d = r - z_range;
 *     bearing row:  h = atan2(dy, dx) - phi,   H_R = [ dy / q, -dx / q, -1],   d = wrap(h - z_bearing);
 *     H_L = -H_R[0:2] for either row;   column pair k of W = P[:, 0:3] H_R,k^T + P[:, L_i] H_L,k^T;
 *     S = H W + blockdiag(R_k) = U^T U (from the upper triangle);   V = W U^-1;   y = U^-T d;   x <- x - V y;   P <- P - V V^T.
 * wrap is ekf_update_fixes' expression with the same constants; the heading itself stays unwrapped.  sqrt and atan2 are taken once
 * per entry and round ON THE DEVICE (the device library's sqrt() and atan2(), which may differ from the host's libm by an ulp).
 * BOTH: row 0 of the slot is the range row, row 1 the bearing row.  A RANGE or BEARING entry keeps the two-column shape: its one
 * live row is row 0 of the slot, row 1 is the inert row of EKF_FIX_HEADING -- a zero row and column of S, the diagonal entry
 * exactly 1, d = 0 --, so its pivot is 1 and its y and its column of V are exact zeros: its d2 adds exactly 0.  The same landmark
 * may appear several times in a round, under different kinds too.
 * S of a round counts as not positive definite by ekf_update_matched's rule: a pivot not above 2^-44 of its own diagonal entry of S
 * (or NaN), e.g. the same landmark's range twice with R = 0.  A landmark exactly at the robot's position (q == 0) has no defined H:
 * its pivot is NaN and its round is refused the same way.  That round and all later ones are then NOT applied: the state is that
 * after the completed rounds, *n_applied_out (may be NULL) counts their entries, their d2 stays valid, the refused and later entries
 * get NaN, and no NaN or Inf is written into the filter.  A result, not an error.
 * d2_out[k] (may be NULL): the running sum of y^2 of k's round up to and including k; NaN for skipped and for unapplied entries.  A
 * RANGE entry alone in a round: (r - z)^2 / (H P H^T + R).
 * Checked on the host before the handle is touched: n < 0, a NULL z / R / ids / kind with n > 0, an id < -1, a kind outside 1..3 of
 * a non-skipped entry, a non-finite value among those the kind reads, a negative variance of a RANGE or BEARING entry, an index out
 * of range -- EKF_ERR_BAD_ARG; then the ids against the landmark count (id >= N: EKF_ERR_BAD_ARG, the state untouched).  n = 0, or
 * every entry skipped, is a no-op that leaves an open window open.
 * Otherwise, as ekf_update_matched: deferred slots are folded first, a streaming launch is stopped (immediate-mode calls stream
 * again afterwards), each round costs one dense pass over P_LL, a sticky EKF_ERR_TIMEOUT / EKF_ERR_CAPACITY is returned unchanged
 * with nothing modified, gates, counters and the decision log are not involved, the host mirror shows the new pose and P_RR, every
 * device buffer ends as ekf_set_state of the result would leave it, and the call synchronises.  No atomics, one writer per value,
 * every sum in a fixed order: the same bits on every call, and filter b of the batch form gets the bits of the one-filter call on b.
 * ekf_update_polar returns the landmark count (unchanged) or a negative status; the batch form takes filter b's lists at
 * z + b * n * 2, R + b * n * 4, ids + b * n, kind + b * n (ragged lists: pad ids with -1) and returns EKF_OK or a negative status.
 * The scratch is that of ekf_update_matched (the same blocks: a handle that has made either call has them). */
int ekf_update_polar(ekf_handle h, int index, const double *z /*[n][2]*/, const double *R /*[n][4], column-major 2x2*/,
                     const int *ids /*[n]*/, const int *kind /*[n]*/, int n, int *n_applied_out /* may be NULL */,
                     double *d2_out /*[n] or NULL*/);
int ekf_batch_update_polar(ekf_handle h, const double *z /*[batch][n][2]*/, const double *R /*[batch][n][4]*/,
                           const int *ids /*[batch][n]*/, const int *kind /*[batch][n]*/, int n, int *n_applied_out /*[batch] or NULL*/,
                           double *d2_out /*[batch][n] or NULL*/);

/* The score of ONE list of polar measurements, nothing applied: the same S, factor and y as a round of ekf_update_polar (the same
 * kernel) for at most EKF_MAX_PENDING = 32 non-skipped entries, whatever the window; more is EKF_ERR_BAD_ARG, and so is everything
 * ekf_update_polar refuses, and a NULL d2_out with n > 0.  d2_out[k]: the joint distance of the list cut after entry k; NaN for
 * skipped entries, and from the first refused pivot on (the call still returns EKF_OK).  For a list that fits one round of
 * ekf_update_polar the two calls give the same bits of d2.  The filter is only read, behind the rule of ekf_joint_compat. */
int ekf_polar_compat(ekf_handle h, int index, const double *z, const double *R, const int *ids, const int *kind, int n,
                     double *d2_out /*[n]*/);
int ekf_batch_polar_compat(ekf_handle h, const double *z, const double *R, const int *ids, const int *kind, int n,
                           double *d2_out /*[batch][n]*/);

/* Where the hypotheses come from: the individual compatibility table of a scan.  For every measurement k and every landmark l of
 * the filter, res, S (symmetrised) and d2 = res^T S^-1 res of the association sweep (Update.cpp:103-136), EVERY measurement against
 * the same, unchanged state -- not the sequential chain of ekf_update.  z and R use the layouts of ekf_batch_update; cos phi and
 * sin phi are taken once per call and filter on the device (sincos of x[2], as the chain kernels take them).
 * A landmark whose S has a condition number >= params.cond_limit is SKIPPED for that measurement (Update.cpp:131): it is no
 * candidate and cannot be the nearest; n_skipped_out[k] (may be NULL) counts them.  A kept pair is LISTED iff d2 <= gate (9.21:
 * 99 % of chi-square with 2 dof; +inf lists every kept pair; a NaN d2 is never listed).  The list is ordered by (meas, d2 ascending,
 * landmark); the first min(found, max_cand) entries are written; cand_out == NULL with max_cand == 0 only counts.
 * nearest_out[k] (may be NULL) is the ekf_decision that ekf_update of measurement k ALONE would log at this state -- a dry run of
 * the filter's own gate: matched and mahal are the arg-min of d2 over the kept landmarks (ties: the lower index; none: matched = 0,
 * mahal = 999999999999), decision is New / Old / Ignore by gamma_max / gamma_min.  A filter without landmarks has no candidate and
 * every measurement New.  An entry with valid[b][k] == 0 (batch form; NULL: all valid) is not looked at: no candidate, nearest_out
 * all zero, n_skipped_out 0.
 * The filter is only read, behind the rule of ekf_get_landmark_covs: the sweep needs x, the robot rows and the landmarks' own 2x2
 * blocks, which the chain kernels keep current inside an open window.  A streaming launch is stopped (immediate-mode calls stream
 * again afterwards); deferred slots are NOT folded, no dense pass runs, the open window stays open, the flush stream is untouched;
 * state, counters, decision log, loaded script and host mirror stay bit for bit.  A sticky EKF_ERR_TIMEOUT is returned unchanged, a
 * sticky EKF_ERR_CAPACITY does not block the call.  The call synchronises.
 * EKF_ERR_BAD_ARG, found on the host before the handle is touched: n_z < 0, a NULL z or R with n_z > 0, a non-finite z or R of a
 * valid entry, gate negative or NaN, max_cand < 0, a NULL cand_out with max_cand > 0, a NULL n_found_out (batch form), an index out
 * of range.  n_z == 0 returns 0 and touches nothing.
 * ekf_gate_candidates returns `found`, which may exceed max_cand, or a negative status; the batch form writes filter b's list at
 * cand_out + b * max_cand and its count to n_found_out[b], and returns EKF_OK or a negative status.
 * Gate-passers are appended through an integer counter and sorted on the host, the nearest is reduced in a fixed order, no
 * floating-point atomics: two calls on an unchanged state give the same bits, and filter b of the batch form gets the bits of the
 * one-filter call on b.
 * The scratch -- the measurement table (48 bytes per measurement, for at least 64 per filter), per-workgroup partial minima,
 * counters, and a candidate list of its own that is replaced by a larger one when a call finds more than it holds (the search then
 * runs once more) -- is allocated at the first call with a valid measurement, kept on the handle (ekf_device_bytes counts it,
 * ekf_reserve builds it again) and freed by ekf_destroy. */
typedef struct ekf_candidate {
    int meas;      /* index of the measurement in the call's list */
    int landmark;  /* 0-based, as in ekf_remove_landmarks */
    double d2;
} ekf_candidate;
int ekf_gate_candidates(ekf_handle h, int index, const double *z /*[n_z][2]*/, const double *R /*[n_z][4], column-major 2x2*/, int n_z,
                        double gate, ekf_candidate *cand_out /*[max_cand] or NULL*/, int max_cand, ekf_decision *nearest_out /*[n_z] or NULL*/,
                        int *n_skipped_out /*[n_z] or NULL*/);
int ekf_batch_gate_candidates(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                              const unsigned char *valid /*[batch][n_z] or NULL*/, int n_z, double gate,
                              ekf_candidate *cand_out /*[batch][max_cand] or NULL*/, int max_cand, int *n_found_out /*[batch]*/,
                              ekf_decision *nearest_out /*[batch][n_z] or NULL*/, int *n_skipped_out /*[batch][n_z] or NULL*/);

/* From the table to a decision: the joint-compatibility branch-and-bound search (JCBB) on the device, one launch whatever the
 * number of nodes.  z, R (and valid, batch form) as for ekf_gate_candidates; at most EKF_MAX_PENDING = 32 valid measurements per
 * filter, more is EKF_ERR_BAD_ARG as for ekf_joint_compat.
 * CANDIDATES of measurement k: the pairs ekf_gate_candidates lists for it at this state and `gate` (so the condition rule
 * applies), in its order (d2 ascending, then landmark), the first max_branch of them (1 .. EKF_ASSOC_MAX_BRANCH = 16);
 * info.n_candidates counts the listed pairs of the filter, info.n_dropped those cut by max_branch.
 * A HYPOTHESIS gives every valid measurement, in list order, one of its candidates or nothing, a landmark at most once.  It is
 * feasible when every prefix is jointly compatible: after each pairing, q pairings so far, D2 <= joint_gate[q - 1], D2 the joint
 * distance ekf_joint_compat defines (S, d, U, y of ekf_update_matched, everything linearised at the one entry state).  An extension
 * whose 2 x 2 Schur complement has a pivot that is not above 2^-44 of its own diagonal entry of S (or NaN) is not compatible: a
 * result, never an error.  joint_gate == NULL: ekf_joint_gates(0.99, .), the 99 % quantiles of chi-square with 2 q dof.
 * THE SEARCH (m valid measurements; Best starts empty: 0 pairings, D2 0; `nodes` counts expanded nodes up to max_nodes,
 * 1 .. EKF_ASSOC_MAX_NODES = 2^20):
 *     search(H, i, cnt, D2):
 *         if cnt + (m - i) <  Best.cnt: return
 *         if cnt + (m - i) == Best.cnt and D2 >= Best.D2: return                  (D2 never decreases along a branch)
 *         if i == m: (H beats Best: more pairings, or as many and a smaller D2)  Best = H; return
 *         if nodes == max_nodes: complete = 0; stop the whole search
 *         nodes += 1
 *         for l in candidates(i) in list order, l not used in H:
 *             D2' = joint distance of H + (i, l);  if D2' <= joint_gate[cnt]: search(H + (i, l), i + 1, cnt + 1, D2')
 *         search(H + (i, nothing), i + 1, cnt, D2)
 * The result is Best: the most pairings, then the smallest D2, then the first found in this order.  complete = 1: the optimum over
 * all feasible hypotheses; complete = 0: the best found when the budget ran out -- the order is fixed, so that is reproducible too.
 * A filter without a candidate (no valid measurement, no landmark, nothing inside the gate) is not searched: everything -1,
 * n_paired = 0, complete = 1, nodes = 0.
 * ids_out[k]: the landmark of measurement k, -1 for unpaired and masked entries -- what ekf_update_matched takes.  d2_out (may be
 * NULL): what ekf_joint_compat returns for ids_out, the same bits (the same kernel runs on the winner).  nearest_out, n_skipped_out
 * (may be NULL): those of ekf_gate_candidates, the same bits (the same sweep).  info.d2: the winner's distance as the search
 * accumulated it (agrees with the last d2_out to rounding, not to the bit: another order of the same elimination).
 * The search reads cross blocks of P_LL, so it follows the rule of ekf_joint_compat and ekf_find_duplicates: a streaming launch is
 * stopped (immediate-mode calls stream again afterwards), deferred slots are folded, a sticky EKF_ERR_TIMEOUT is returned
 * unchanged, a sticky EKF_ERR_CAPACITY does not block the call; the filter is only read: state, counters, decision log, loaded
 * script and host mirror stay what ekf_get_state at the same point would leave.  A call without a candidate in any filter folds
 * nothing.  The call synchronises.
 * EKF_ERR_BAD_ARG, found on the host before the handle is touched: everything ekf_gate_candidates refuses of z, R, valid, n_z and
 * gate; ids_out NULL with n_z > 0; info_out NULL (batch form); max_branch or max_nodes out of range; a joint_gate entry that is
 * NaN or negative; more than 32 valid entries in a filter; an index out of range.
 * ekf_associate_joint returns n_paired or a negative status; the batch form writes filter b's results at ids_out + b * n_z (and
 * so on) and info_out[b], and returns EKF_OK or a negative status.
 * The candidate table is ordered on the host (the one trip ekf_gate_candidates makes for its sort); from there to ids_out one
 * wave per filter runs the whole search: no floating-point atomics, one writer per value, every sum in a fixed order -- two calls
 * on an unchanged state give the same bits, and filter b of the batch form gets the bits of the one-filter call on b.
 * The scratch -- 2 328 bytes per filter beside those of ekf_gate_candidates and ekf_joint_compat -- is allocated at the first call
 * that searches, kept on the handle (ekf_device_bytes counts it, ekf_reserve builds it again) and freed by ekf_destroy. */
#define EKF_ASSOC_MAX_BRANCH 16
#define EKF_ASSOC_MAX_NODES (1 << 20)
typedef struct ekf_assoc {
    long long nodes;   /* expanded nodes */
    double d2;         /* joint distance of the result */
    int n_paired;
    int complete;      /* 1: the optimum; 0: max_nodes ran out */
    int n_candidates;  /* pairs inside the individual gate */
    int n_dropped;     /* ... of which max_branch cut */
} ekf_assoc;
int ekf_associate_joint(ekf_handle h, int index, const double *z /*[n_z][2]*/, const double *R /*[n_z][4], column-major 2x2*/, int n_z, double gate,
                        const double *joint_gate /*[32] or NULL*/, int max_branch, long long max_nodes, int *ids_out /*[n_z]*/,
                        double *d2_out /*[n_z] or NULL*/, ekf_decision *nearest_out /*[n_z] or NULL*/, int *n_skipped_out /*[n_z] or NULL*/,
                        ekf_assoc *info_out /* may be NULL */);
int ekf_batch_associate_joint(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                              const unsigned char *valid /*[batch][n_z] or NULL*/, int n_z, double gate, const double *joint_gate /*[32] or NULL*/,
                              int max_branch, long long max_nodes, int *ids_out /*[batch][n_z]*/, double *d2_out /*[batch][n_z] or NULL*/,
                              ekf_decision *nearest_out /*[batch][n_z] or NULL*/, int *n_skipped_out /*[batch][n_z] or NULL*/,
                              ekf_assoc *info_out /*[batch]*/);
/* out[q - 1], q = 1 .. 32: the `confidence` quantile of chi-square with 2 q degrees of freedom, from the closed form for even dof,
 * CDF(x) = 1 - exp(-x / 2) sum_{i < q} (x / 2)^i / i!, by bisection on the host.  A confidence outside (0, 1): EKF_ERR_BAD_ARG. */
int ekf_joint_gates(double confidence, double *out /*[32]*/);

/* Growing the map without the filter's own gate: the m measurements with add[k] != 0 (NULL: all n_z) become landmarks N, N + 1, ..,
 * N + m - 1 in list order, on the device, ALL linearised at the entry state.  z and R use the layouts of ekf_batch_update.  With
 * p, phi, P the settled entry state, C = Rot(phi), J = [[0,-1],[1,0]]:
 *     h_k = C J z_k = (-(s z_x + c z_y), c z_x - s z_y);   G_k = [I_2 | h_k]  (2 x 3; = -C H_R of Update.cpp:163-166);
 *     L_new,k = p + C z_k  (Update.cpp:155);   P[new k, robot] = G_k P_RR  (:169);   P[new k, old m] = G_k P_R,m;
 *     P[new k, new l] = G_k P_RR G_l^T + [k == l] C R_k C^T  (:168; the k != l term is what the reference's sequential New leaves
 *     between two landmarks initialised from one pose).
 * Only the symmetric part of R_k enters, xy = (R01 + R10) / 2 (Update.cpp:193).  cos phi and sin phi are taken once per call and
 * filter on the device (sincos of x[2], as the chain kernels take them).  This is ekf_join_map of the source x = (0, 0, 0, z_0, ..),
 * P = blockdiag(0_3, R_0, ..) without the source: no second handle, no dense matrix through the host, three launches whatever m,
 * and (N + m) m blocks written -- only the tile columns from N / 32 on are touched.
 * The pose, P_RR, every old row and column, the counters and the decision log stay bit for bit; P stays bitwise symmetric (one home
 * per element); the host mirror shows the new count; every device buffer ends as ekf_set_state of the result would leave it.
 * ids_out[k] (may be NULL): the new landmark's number, -1 for an entry that was not added.
 * As ekf_join_map: deferred slots are folded first, a streaming launch is stopped (immediate-mode calls stream again afterwards),
 * the blocks are written in place into the settled buffer in either pipeline mode, a sticky EKF_ERR_TIMEOUT / EKF_ERR_CAPACITY is
 * returned unchanged with nothing modified, and the call synchronises.  No atomics, one writer per value: the same bits on every
 * call, and filter b of the batch form gets the bits of the one-filter call on b.
 * EKF_ERR_BAD_ARG, found on the host before the handle is touched: n_z < 0, a NULL z or R with n_z > 0, a non-finite z or R of a
 * selected entry, a NULL n_out (batch form), an index out of range.  n_z == 0, or nothing selected in any filter, is a no-op that
 * leaves an open window open, returns the counts from the host mirror and does not look at a sticky status (as the no-ops of
 * ekf_update_matched and ekf_fuse_landmarks).  N + m > ekf_capacity(h): EKF_ERR_CAPACITY with the exported state unchanged (deferred slots have
 * been folded nonetheless); it is NOT sticky (no kernel ran): call ekf_reserve and add again.
 * ekf_add_landmarks returns the new landmark count N + m or a negative status; the batch form takes filter b's lists at
 * z + b * n_z * 2, R + b * n_z * 4, add + b * n_z, writes the counts to n_out[b] and returns EKF_OK or a negative status; one
 * filter without room fails the whole call with nothing modified.
 * The scratch -- the measurement table (48 bytes per addition, for at least 64 per filter) and the new rows' operands (64 bytes
 * each) -- is allocated at the first call that adds, kept on the handle (ekf_device_bytes counts it, ekf_reserve builds it again)
 * and freed by ekf_destroy. */
int ekf_add_landmarks(ekf_handle h, int index, const double *z /*[n_z][2]*/, const double *R /*[n_z][4], column-major 2x2*/,
                      const unsigned char *add /*[n_z] or NULL = all*/, int n_z, int *ids_out /*[n_z] or NULL*/);
int ekf_batch_add_landmarks(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                            const unsigned char *add /*[batch][n_z] or NULL*/, int n_z, int *ids_out /*[batch][n_z] or NULL*/,
                            int *n_out /*[batch]*/);

/* The scan step of a JCBB-SLAM loop as one call: gate, search, joint update, initialisation.  In this order:
 *   1. ekf_associate_joint at the entry state with the same z, R, n_z, gate, joint_gate, max_branch, max_nodes (and valid).
 *   2. The kinds: a paired measurement is EKF_DECISION_OLD; an unpaired valid one is EKF_DECISION_NEW iff the filter's own gate
 *      says New for it at the entry state (ekf_associate_joint's nearest_out: no kept landmark, or the individual arg-min above
 *      gamma_max); every other unpaired valid one is EKF_DECISION_IGNORE (near something, not jointly compatible); masked: 0.
 *   3. The room: N + #NEW > ekf_capacity(h) returns EKF_ERR_CAPACITY, not sticky, with nothing applied (the search only reads).
 *   4. ekf_update_matched with the pairings, then ekf_add_landmarks with the NEW ones AT THE STATE THE MATCHED STEP LEFT: update
 *      first, then augment with the posterior pose.  A paired measurement whose round was not applied (ekf_update_matched's rule
 *      for an S that is not positive definite) is reported EKF_DECISION_IGNORE with id -1 and NaN d2; the additions still run.
 * ids_out[k]: the landmark measurement k ended as -- an id below the entry count: OLD; from the entry count on: NEW; -1 otherwise.
 * kind_out (may be NULL): the EKF_DECISION_* codes above.  d2_out (may be NULL): that of ekf_update_matched.  info_out: that of
 * ekf_associate_joint.  State and outputs are bit for bit those of the three public calls made in sequence with these arguments
 * (the same implementations run).  Counters and decision log stay as they are, as for ekf_update_matched: book NIS from d2_out.
 * Limits and refusals are those of ekf_associate_joint (at most 32 valid measurements per filter), then those of the two others;
 * ekf_update_joint returns the new landmark count, the batch form writes it to n_out[b] (NULL: EKF_ERR_BAD_ARG, as a NULL info_out)
 * and returns EKF_OK; a negative status otherwise. */
int ekf_update_joint(ekf_handle h, int index, const double *z /*[n_z][2]*/, const double *R /*[n_z][4]*/, int n_z, double gate,
                     const double *joint_gate /*[32] or NULL*/, int max_branch, long long max_nodes, int *ids_out /*[n_z]*/,
                     int *kind_out /*[n_z] or NULL*/, double *d2_out /*[n_z] or NULL*/, ekf_assoc *info_out /* may be NULL */);
int ekf_batch_update_joint(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                           const unsigned char *valid /*[batch][n_z] or NULL*/, int n_z, double gate, const double *joint_gate /*[32] or NULL*/,
                           int max_branch, long long max_nodes, int *ids_out /*[batch][n_z]*/, int *kind_out /*[batch][n_z] or NULL*/,
                           double *d2_out /*[batch][n_z] or NULL*/, ekf_assoc *info_out /*[batch]*/, int *n_out /*[batch]*/);

/* ---- relocalisation: where am I on this map? ---------------------------------------------------
 * Every association path above starts from a pose prior that is already good.  After a bump, a long blind stretch, or with a saved
 * map loaded into a robot that does not know where it stands, the gates fail and every measurement is declared New.  The three
 * calls below answer that case on the device: a Euclidean scan-to-map pose search, the pose reset it ends in, and the two with
 * ekf_update_matched as one call.
 *
 * ekf_locate_scan: the read-only pose search.  z [n_z][2] are robot-frame relative positions in the layout of ekf_update; at most
 * EKF_MAX_PENDING = 32 valid measurements per filter, more is EKF_ERR_BAD_ARG as for ekf_joint_compat.  ONLY x IS READ: P and R play
 * no part, the search is Euclidean (tol is a radius in metres, not a chi-square gate).
 *   BASE PAIRS: the pairs (a, b), a < b, of valid measurements with |z_a - z_b| >= min_sep, ordered by separation descending, then
 *     by (a, b) ascending; the first max_base (1 .. EKF_LOCATE_MAX_BASE = 16) are kept, rank r = 0 the farthest apart.
 *   CANDIDATES: for the base pair of rank r, every ordered landmark pair (i, j), i != j, with
 *     | |L_j - L_i| - |z_b - z_a| | <= 2 tol  (lengths as sqrt of the sum of squares): exactly the pairs for which a and b can both
 *     be inliers of their own hypothesis.
 *   PAIR POSE of (r, i, j): dz = z_b - z_a, dl = L_j - L_i, q = |dz| |dl|, c = (dz . dl) / q, s = (dz x dl) / q
 *     (dz x dl = dz_x dl_y - dz_y dl_x; no sincos is taken), C = [[c, -s], [s, c]], p = (L_i + L_j) / 2 - C (z_a + z_b) / 2;
 *     pair_pose = (p_x, p_y, atan2(dz x dl, dz . dl)), the angle for the report only.
 *   SCORE: for every valid k the landmark nearest to p + C z_k in squared distance (ties: the lower index); k is an inlier iff
 *     that squared distance <= tol^2.  The match is then made one-to-one: where several inliers name one landmark, the one with
 *     the smallest distance keeps it (ties: the lower k), the others are no inliers.  inliers = their count, ssr = the sum of
 *     their squared distances, added in ascending k.
 *   ORDER of the hypotheses: inliers descending, then ssr ascending, then (r, i, j) ascending -- a total order that does not
 *     depend on how the device appended its candidate list.  The first min(found, max_out) are written (max_out 1 ..
 *     EKF_LOCATE_MAX_OUT = 64), `found` = the number of candidates.
 *   REFIT of each written hypothesis, one closed-form least-squares rigid fit over its inliers (the inlier set is not computed
 *     again): centroids mz, ml of the inliers' z_k and L_k (sums in ascending k, divided by the count), Sd = sum (z_k - mz) . (L_k - ml),
 *     Sx = sum (z_k - mz) x (L_k - ml), n = sqrt(Sd^2 + Sx^2), c' = Sd / n, s' = Sx / n (n == 0, a single inlier: the pair pose's c
 *     and s), t = ml - C' mz; pose = (t_x, t_y, atan2(Sx, Sd)) (n == 0: the pair pose's angle), rms = sqrt(sum |t + C' z_k - L_k|^2 /
 *     inliers) (0 without an inlier, where pose = pair_pose).
 * hyp_out [max_out]: the records.  meas_a, meas_b are the caller's indices.  ids_out [max_out][n_z]: row h holds the landmark of
 * each measurement under hypothesis h, or -1 (no inlier, masked) -- ready to be the ids of ekf_update_matched; rows from the number
 * written on are left alone.  n_cand_out (may be NULL): the candidates scored.
 * THE SAME TRUE POSE RECURS once per base pair (and landmark pair) that hits it: the list is ordered, not merged.  Hypotheses whose
 * fitted poses agree within 2 tol in position and 2 tol / reach in heading (reach = the largest |z_k|) are the same pose; the
 * Python binding's distinct_poses merges them, ekf_relocalize's acceptance rule applies the same test.
 * The handle is treated exactly as in ekf_gate_candidates: x is current inside an open window; a streaming launch is stopped;
 * nothing is folded, no dense pass runs, the window stays open; state, counters, decision log, loaded script and host mirror stay
 * bit for bit; a sticky EKF_ERR_TIMEOUT is returned unchanged, a sticky EKF_ERR_CAPACITY does not block the call.  The call
 * synchronises.
 * Zero hypotheses with EKF_OK: fewer than two landmarks, fewer than two valid measurements, no base pair.
 * EKF_ERR_BAD_ARG, found on the host before the handle is touched: n_z < 0, a NULL z with n_z > 0, a non-finite z of a valid entry,
 * more than 32 valid entries in a filter, tol or min_sep not finite and positive, max_base or max_out out of range, NULL hyp_out
 * or ids_out (n_found_out, batch form), an index out of range.
 * More than EKF_LOCATE_MAX_CAND = 2^22 candidates in a filter: EKF_ERR_CAPACITY, not sticky, nothing written but n_cand_out -- tol
 * is too loose for this map (a length filter of 2 tol that a fifth of all landmark pairs pass says nothing).
 * Candidates are appended through an integer counter, every score comes out of fixed-order reductions, the selection follows the
 * total order above; no floating-point atomics: two calls on an unchanged state give the same bits, and filter b of the batch form
 * gets the bits of the one-filter call on b.
 * The scratch -- the measurement and base-pair tables, the candidate list (4096 entries per filter at first; replaced by a larger
 * one when a call finds more, the search then runs once more) with a score per entry, and the selection's partial lists -- is
 * allocated at the first call that searches, kept on the handle (ekf_device_bytes counts it, ekf_reserve builds it again) and freed
 * by ekf_destroy.
 * ekf_locate_scan returns the number of hypotheses written, or a negative status; the batch form writes filter b's records at
 * hyp_out + b * max_out, its ids at ids_out + b * max_out * n_z and the number written to n_found_out[b]. */
#define EKF_LOCATE_MAX_BASE 16
#define EKF_LOCATE_MAX_OUT 64
#define EKF_LOCATE_MAX_CAND (1 << 22)
typedef struct ekf_locate_hyp {
    double pose[3];       /* the refit: x, y, heading */
    double pair_pose[3];  /* the pose of the base pair on the landmark pair, which was scored */
    double ssr;           /* sum of the inliers' squared distances at pair_pose */
    double rms;           /* of the inliers at pose */
    int inliers;
    int meas_a, meas_b;   /* the base pair, the caller's indices */
    int lm_i, lm_j;       /* the landmark pair: a on i, b on j */
    int reserved;         /* 0 (the size stays a multiple of 8: 88 bytes) */
} ekf_locate_hyp;
int ekf_locate_scan(ekf_handle h, int index, const double *z /*[n_z][2]*/, int n_z, double tol, double min_sep, int max_base, int max_out,
                    ekf_locate_hyp *hyp_out /*[max_out]*/, int *ids_out /*[max_out][n_z]*/, long long *n_cand_out /* may be NULL */);
int ekf_batch_locate_scan(ekf_handle h, const double *z /*[batch][n_z][2]*/, const unsigned char *valid /*[batch][n_z] or NULL*/, int n_z,
                          double tol, double min_sep, int max_base, int max_out, ekf_locate_hyp *hyp_out /*[batch][max_out]*/,
                          int *ids_out /*[batch][max_out][n_z]*/, int *n_found_out /*[batch]*/, long long *n_cand_out /*[batch] or NULL*/);

/* ekf_reset_pose: the pose replaced and its correlation with the map cut.  x[0..2] <- pose, P_RR <- the symmetrised P_RR (row-major
 * 3 x 3; off-diagonals averaged, 0.5 * (a + b), as Update.cpp:193 does), every robot-landmark block of P becomes exactly +0.0; P_LL
 * and the landmarks of x stay bit for bit.  P_RR = 0 is allowed (a known pose); the caller answers for a P_RR that is positive
 * semi-definite.  Works on a filter without landmarks.
 * Handle discipline of ekf_transform_frame: deferred slots are folded first, a streaming launch is stopped (immediate-mode calls
 * stream again afterwards), the call synchronises; counters and decision log stay as they are; the host mirror shows the new pose
 * and P_RR; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY is returned unchanged with nothing modified.  Every device buffer ends as
 * ekf_set_state of the result would leave it (the robot rows are the only copy of P_RL the kernels keep).
 * EKF_ERR_BAD_ARG: a non-finite entry, a negative diagonal entry of P_RR, an index out of range, NULL.  The batch form takes
 * pose [batch][3] and P_RR [batch][9] and resets every filter in one launch. */
int ekf_reset_pose(ekf_handle h, int index, const double pose[3], const double P_RR[9]);
int ekf_batch_reset_pose(ekf_handle h, const double *pose /*[batch][3]*/, const double *P_RR /*[batch][9]*/);

/* ekf_relocalize: the three steps as one call -- ekf_locate_scan (z, n_z, tol, min_sep, max_base, max_out), the acceptance rule,
 * ekf_reset_pose at the best hypothesis's fitted pose with the caller's P_RR, ekf_update_matched with that hypothesis's ids and
 * the caller's R (which must be finite for every valid entry: checked first, with the arguments of the search).
 * ACCEPTED iff the best hypothesis (the first written) has inliers >= min_inliers (>= 2) and every other written hypothesis that
 * is not the same pose as the best (the rule above: fitted positions within 2 tol, headings within 2 tol / reach) has
 * inliers <= best - lead (lead >= 0).  A runner-up beyond the max_out written is not seen: keep max_out generous.
 * Accepted: returns the best hypothesis's inliers; state and outputs are bit for bit those of the three calls made in sequence.
 * Refused: returns 0 with the state untouched bit for bit and an open window still open (hyp_out and ids_out still show the best
 * hypothesis, if there is one; d2_out NaN).  Otherwise a negative status; a refusal of ekf_reset_pose or ekf_update_matched
 * (sticky statuses) comes back as theirs.
 * hyp_out: the chosen record (all zero when nothing was found); ids_out [n_z]; d2_out [n_z] (may be NULL): that of
 * ekf_update_matched.  The batch form decides per filter, writes the counts to n_out[b] (0: refused), resets and updates the
 * accepted filters only -- each as the one-filter calls on it would -- and returns EKF_OK or a negative status. */
int ekf_relocalize(ekf_handle h, int index, const double *z /*[n_z][2]*/, const double *R /*[n_z][4]*/, int n_z, double tol, double min_sep,
                   int max_base, int max_out, int min_inliers, int lead, const double P_RR[9], ekf_locate_hyp *hyp_out, int *ids_out /*[n_z]*/,
                   double *d2_out /*[n_z] or NULL*/);
int ekf_batch_relocalize(ekf_handle h, const double *z /*[batch][n_z][2]*/, const double *R /*[batch][n_z][4]*/,
                         const unsigned char *valid /*[batch][n_z] or NULL*/, int n_z, double tol, double min_sep, int max_base, int max_out,
                         int min_inliers, int lead, const double *P_RR /*[batch][9]*/, ekf_locate_hyp *hyp_out /*[batch]*/,
                         int *ids_out /*[batch][n_z]*/, double *d2_out /*[batch][n_z] or NULL*/, int *n_out /*[batch]*/);

/* ---- device-resident step scripts (benchmarks, Monte-Carlo runs) ------------------------------
 * A script is `steps` steps; step s of filter b is
 *     Propagate(ctrl[s][b] = v, w, dt)  with Q from params as ekf_propagate does,
 *     then M sequential single-measurement Updates z[s][m][b], R[s][m][b]  (slam.cpp:150-171),
 *     then, when truth != NULL, one NEES sample against truth[s][b] = (x, y, phi).
 * valid[s][m][b] (NULL = all) masks measurements.  Inputs are copied to HBM by ekf_script_load;
 * ekf_script_run only enqueues kernels (no host->device traffic, no synchronisation). */
int ekf_script_load(ekf_handle h, int steps, int M, const double *ctrl, const double *z, const double *R,
                    const unsigned char *valid, const double *truth);
/* use_graph != 0 replays the steps through captured HIP graphs (blocks of a few steps; the remainder
 * goes out as plain launches).  On a handle of ONE filter a short run -- at most half a window of measurements, i.e. a step or
 * two per call -- travels as one command to the resident streaming launch (see "Tunables": EKF_STREAM): 30 us per step at N = 1024
 * where a launch per call costs 42. */
int ekf_script_run(ekf_handle h, int first_step, int n_steps, int use_graph);

/* ---- synchronisation, timing, diagnostics ---------------------------------------------------- */

int ekf_sync(ekf_handle h);  /* waits for the stream, returns a sticky error (EKF_ERR_CAPACITY, EKF_ERR_TIMEOUT) if any filter raised one */
/* Fold the deferred slots into P_LL now (one dense pass, asynchronous).  The caller says "nothing follows for now": in
 * overlap mode the pass goes out on the chain's own stream, on all CUs and in place, and the pipeline restarts empty. */
int ekf_flush(ekf_handle h);
/* Close the open window with a pipeline pass (buffer to buffer on the pass's own stream, as when more measurements
 * follow at once).  Same result as ekf_flush; only the scheduling differs (diagnostics: time that pass alone). */
int ekf_close_window(ekf_handle h);
/* hipEvent pair on the handle's stream. stop synchronises and returns elapsed milliseconds. */
int ekf_timer_start(ekf_handle h);
int ekf_timer_stop(ekf_handle h, double *ms_out);
/* Per-launch timing of the dense P_LL pass (the dominant kernel): when enabled every launch is
 * bracketed by hipEvents on the handle's stream. ekf_flush_profile_read synchronises. */
int ekf_flush_profile(ekf_handle h, int enable);
int ekf_flush_profile_read(ekf_handle h, long long *launches_out, double *total_ms_out);
/* 1 when the handle's chain kernel folds the windows it fills into P_LL itself (maps of up to 256 landmarks, pass in place: one workgroup
 * per filter, k_solo): there is no dense-pass launch to time then -- ekf_flush_profile_read counts the passes and reports the
 * duration of the launches that contain them (measurement loops included). */
int ekf_fused_pass(ekf_handle h);
/* The last `count` decision-log entries of filter `index`, oldest first (synchronises). Returns the number written. */
int ekf_get_decisions(ekf_handle h, int index, ekf_decision *out, int count);
int ekf_get_stats(ekf_handle h, ekf_stats *out /*[batch]*/);
int ekf_reset_stats(ekf_handle h);
/* Per-filter means of the counters, [batch][2] = (mean NIS, mean NEES), NaN without samples, written by a kernel on the
 * handle's stream straight into DEVICE memory at out_device (synchronises): the send buffer of the one collective of a
 * multi-GPU run (RCCL all-gather of [filters_per_gpu][2] doubles) without a trip through the host. */
int ekf_stats_means_device(ekf_handle h, double *out_device /*[batch][2], device memory*/);
/* One NEES sample against a ground-truth pose, truth [batch][3]. */
int ekf_record_truth(ekf_handle h, const double *truth);
/* The HIP stream (hipStream_t) the handle launches on, for callers that want to order their own work. */
void *ekf_stream(ekf_handle h);
/* Bytes of HBM held by the handle. */
size_t ekf_device_bytes(ekf_handle h);
/* Diagnostic: dense-pass windows closed since create (kept across ekf_reserve) and the slot count of the last one -- how a
 * scripted run was cut into windows (tests/test_gpu_parity.py: balanced tail, odd windows). */
int ekf_debug_windows(ekf_handle h, long long *closed_out, int *last_slots_out);
/* Diagnostic: streaming launches started and operations posted to them since create; returns 1 when the handle streams its
 * immediate-mode calls (every handle of ONE filter; EKF_STREAM=0 switches it off), 0 when every call is a launch (batches). */
int ekf_debug_stream(ekf_handle h, long long *starts_out, long long *ops_out);
/* Diagnostic: 1 when the streamed commands' ring lives in device memory the host writes through the PCIe BAR (large-BAR devices), 0 when in
 * host-mapped memory (no large BAR, or EKF_STREAM_RING_HOST=1). */
int ekf_debug_stream_ring(ekf_handle h);

/* ---- Tunables -----------------------------------------------------------------------------------
 * Environment variables read once per handle at ekf_create / ekf_batch_create by the PRODUCT library.  They change scheduling
 * and kernel geometry only -- results are identical whatever they say (the parity suite runs the non-default side of each) --
 * and exist for A/B measurements; bench.py prints every EKF_* variable it saw into its JSON line.
 *   EKF_OVERLAP=0/1        force the in-place / the two-buffer overlapped dense-pass pipeline (default: ekf_params.overlap, -1 = by size)
 *   EKF_PERSIST=0          scripted runs: one chain launch per window instead of multi-segment launches
 *   EKF_BALANCED_TAIL=0    scripted runs close every window at max_pending (default: the last two windows share what is left)
 *   EKF_CHAIN_ONE=0        several-workgroup filters use the general chain kernel, not the one-landmark-per-thread one
 *   EKF_CHAIN_HELPERS=0/1  forbid / force the two helper waves of a one-owner-wave chain workgroup
 *   EKF_CHAIN_WGS, EKF_CHAIN_CUS   chain workgroups per filter / CUs kept for them beside an overlapped pass
 *   EKF_INLINE_REC=0       immediate-mode records travel through the host-mapped ring instead of the kernel arguments
 *   EKF_STREAM=0           immediate-mode calls of a one-filter handle are one launch each (default: a resident launch consumes them
 *                          from a command ring and publishes the host mirror after every operation; it leaves when the
 *                          window is full, when another entry point needs the stream, or after 100 us without a call)
 *   EKF_STREAM_RING_HOST=1 the streamed commands' ring stays in host-mapped memory (default where the device has a large BAR: in device memory,
 *                          written by the host through the BAR, polled by the launch as a local read)
 *   EKF_XCD_MAP=0, EKF_BATCH_INTERLEAVE=0, EKF_FLUSH_ALTERNATE=0   dense-pass tile order experiments
 *   EKF_SOLO=0, EKF_SOLO_FUSE=0, EKF_SOLO_LONG_WINDOW=0, EKF_SOLO_GROUPS=n   one-workgroup filters: general kernel / separate pass launches / short window / phase groups
 *   EKF_INKERNEL_WAIT=0    chain launches wait for their pass by stream event instead of in-kernel
 *   EKF_TRACE=1            progress marks of handle creation on stderr
 * EKF_DEBUG_* hooks (skipped passes, dropped completion marks, short spin limits) exist ONLY in libekfslam_hip_debug.so. */

#ifdef __cplusplus
}
#endif
#endif
