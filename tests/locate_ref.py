"""NumPy statement of ekf_locate_scan, ekf_reset_pose and ekf_relocalize (include/ekfslam_c.h) on the exported x (and P), with an
extended-precision restatement beside it, and the inputs of the GPU tests.

locate(x, z, tol, min_sep, max_base, max_out, valid=None, dtype=np.float64) -> Result: the definition of the header, vectorised
over the candidates (in blocks, so that a map of thousands of landmarks fits): base pairs, the length filter, the pair pose without a
sincos, the nearest landmark of every measurement (np.argmin: the lower index on a tie), the one-to-one pass, inliers and ssr (added
in ascending k: a loop, not np.sum, whose pairwise order is another), the total order, the refit of the written hypotheses with
every sum a loop in ascending k.  dtype=np.longdouble is the restatement: x and z are taken as they are (doubles) and every operation
from there on runs in extended precision.  Result.margins holds, for every threshold the integer outputs depend on, the smallest
relative distance of a compared quantity from it.

What the device may differ in: contraction (fused multiply-adds) and its own atan2; the order of every sum is the reference's.  That
is the kind of difference double has against extended, so the bounds asked of the device are 20 times what
tests/test_locate_scan_cpu.py measures between the two over every input of the GPU tests (the project's rule for GATE_D2_REL)."""
import collections
import math

import numpy as np

import match_ref as mr

LOCATE_DTYPE = np.dtype([("pose", "f8", (3,)), ("pair_pose", "f8", (3,)), ("ssr", "f8"), ("rms", "f8"), ("inliers", "i4"), ("meas_a", "i4"),
                         ("meas_b", "i4"), ("lm_i", "i4"), ("lm_j", "i4"), ("reserved", "i4")])
MAX_MEAS, MAX_BASE, MAX_OUT, MAX_CAND, LIST_FLOOR = 32, 16, 64, 1 << 22, 4096
EDGE = 1e-9   # every threshold lies at least this far (relative) from what is compared to it: the integer outputs are exact on the device

# Measured by tests/test_locate_scan_cpu.py (test_reference_against_extended_precision) over every written hypothesis of every input
# of inputs(): the largest difference between the double reference and its extended-precision restatement (1.574e-15; 3.522e-12 and
# 1.760e-12, both on the map of two landmarks, whose residuals are 3 mm at 20 m from the origin).
MEASURED_POSE_ABS = 1.6e-15   # |pose - pose_ext| and |pair_pose - pair_pose_ext|, metres and radians
MEASURED_SSR_REL = 3.6e-12    # |ssr - ssr_ext| / ssr_ext
MEASURED_RMS_REL = 1.8e-12    # |rms - rms_ext| / rms_ext
POSE_ABS, SSR_REL, RMS_REL = 20.0 * MEASURED_POSE_ABS, 20.0 * MEASURED_SSR_REL, 20.0 * MEASURED_RMS_REL

Result = collections.namedtuple("Result", "hyps ids n_cand margins inliers_all order")


def base_pairs(z, valid, min_sep, max_base, dtype=np.float64):
    """[(a, b, separation)] in the caller's indices: the pairs of valid measurements at least min_sep apart, by separation
    descending, then (a, b), the first max_base."""
    z = np.asarray(z, dtype=dtype).reshape(-1, 2)
    at = [k for k in range(len(z)) if valid is None or valid[k]]
    pairs = []
    for u, a in enumerate(at):
        for b in at[u + 1:]:
            d = z[b] - z[a]
            sep = np.sqrt(d[0] * d[0] + d[1] * d[1])
            if sep >= min_sep:
                pairs.append((a, b, sep))
    pairs.sort(key=lambda p: (-p[2], p[0], p[1]))
    return pairs[:max_base]


def _rel_min(best, values, ref):
    """min(best, the smallest |values - ref| / ref)."""
    values = np.asarray(values, dtype=np.float64)
    return min(best, float(np.min(np.abs(values - ref) / ref))) if values.size else best


def candidates(L, pairs, tol, margins):
    """(r, i, j) int arrays of every ordered landmark pair that passes the length filter of a base pair, in (r, i, j) order."""
    dtype = L.dtype
    N = len(L)
    dx, dy = L[None, :, 0] - L[:, None, 0], L[None, :, 1] - L[:, None, 1]   # [i][j] = L_j - L_i
    length = np.sqrt(dx * dx + dy * dy)
    off = ~np.eye(N, dtype=bool)
    two_tol = dtype.type(2.0) * dtype.type(tol)
    rs, iis, jjs = [], [], []
    for r, (_, _, sep) in enumerate(pairs):
        gap = np.abs(length - sep)
        margins["length"] = _rel_min(margins["length"], gap[off], float(two_tol))
        i, j = np.nonzero((gap <= two_tol) & off)
        rs.append(np.full(len(i), r)), iis.append(i), jjs.append(j)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.int64)  # noqa: E731
    return cat(rs), cat(iis), cat(jjs)


def pair_poses(L, z, pairs, r, i, j):
    """(c, s, px, py, dot, crs) of the candidates, the header's expressions."""
    a = np.array([p[0] for p in pairs], dtype=np.int64)[r]
    b = np.array([p[1] for p in pairs], dtype=np.int64)[r]
    sep = np.array([p[2] for p in pairs], dtype=L.dtype)[r]
    half = L.dtype.type(0.5)
    dzx, dzy = z[b, 0] - z[a, 0], z[b, 1] - z[a, 1]
    dlx, dly = L[j, 0] - L[i, 0], L[j, 1] - L[i, 1]
    q = sep * np.sqrt(dlx * dlx + dly * dly)
    dot, crs = dzx * dlx + dzy * dly, dzx * dly - dzy * dlx
    c, s = dot / q, crs / q
    mx, my = half * (z[a, 0] + z[b, 0]), half * (z[a, 1] + z[b, 1])
    px = half * (L[i, 0] + L[j, 0]) - (c * mx - s * my)
    py = half * (L[i, 1] + L[j, 1]) - (s * mx + c * my)
    return c, s, px, py, dot, crs


def score(L, zv, c, s, px, py, tol, margins):
    """(lm [C][n], d2 [C][n], win [C][n], inliers [C], ssr [C]) of the candidates over the valid measurements zv [n][2]."""
    dtype = L.dtype
    C, n = len(c), len(zv)
    block = max(1, (1 << 23) // max(1, n * len(L)))   # (candidates at a time: 64 MB per temporary)
    tol_sq = dtype.type(tol) * dtype.type(tol)
    lm, d2 = np.empty((C, n), dtype=np.int64), np.empty((C, n), dtype=dtype)
    for c0 in range(0, C, block):
        sl = slice(c0, min(C, c0 + block))
        tx = px[sl, None] + (c[sl, None] * zv[None, :, 0] - s[sl, None] * zv[None, :, 1])
        ty = py[sl, None] + (s[sl, None] * zv[None, :, 0] + c[sl, None] * zv[None, :, 1])
        ex, ey = tx[:, :, None] - L[None, None, :, 0], ty[:, :, None] - L[None, None, :, 1]
        d = ex * ex + ey * ey
        near = np.argmin(d, axis=2)
        lm[sl] = near
        d2[sl] = np.take_along_axis(d, near[:, :, None], axis=2)[:, :, 0]
        if len(L) > 1:   # the runner-up of every measurement that is an inlier: a tie of the nearest index would show here
            two = np.partition(d, 1, axis=2)[:, :, :2]
            second = two.max(axis=2)
            inl = d2[sl] <= tol_sq
            if inl.any():
                margins["nearest"] = min(margins["nearest"], float(np.min(((second - d2[sl]) / second)[inl])))
    margins["radius"] = _rel_min(margins["radius"], d2, float(tol_sq))
    inl = d2 <= tol_sq
    k = np.arange(n)
    same = (lm[:, :, None] == lm[:, None, :]) & inl[:, :, None] & inl[:, None, :] & (k[:, None] != k[None, :])[None]
    beat = (d2[:, None, :] < d2[:, :, None]) | ((d2[:, None, :] == d2[:, :, None]) & (k[None, :] < k[:, None])[None])
    win = inl & ~(same & beat).any(axis=2)
    if same.any():
        hi = np.maximum(d2[:, None, :], d2[:, :, None])
        margins["one_to_one"] = min(margins["one_to_one"], float(np.min((np.abs(d2[:, None, :] - d2[:, :, None]) / hi)[same])))
    ssr = np.zeros(C, dtype=dtype)
    for q in range(n):   # ascending k
        ssr = ssr + np.where(win[:, q], d2[:, q], dtype.type(0.0))
    return lm, d2, win, win.sum(axis=1), ssr


def refit(L, zv, lm, win, pose):
    """(pose (3), rms) of one hypothesis: the closed-form fit over its inliers, every sum in ascending k."""
    dtype = L.dtype
    c, s, px, py, dot, crs = pose
    ks = [k for k in range(len(zv)) if win[k]]
    zero = dtype.type(0.0)
    phi = np.arctan2(crs, dot)
    if not ks:
        return (px, py, phi), zero
    cnt = dtype.type(len(ks))
    mzx = mzy = mlx = mly = zero
    for k in ks:
        mzx, mzy, mlx, mly = mzx + zv[k, 0], mzy + zv[k, 1], mlx + L[lm[k], 0], mly + L[lm[k], 1]
    mzx, mzy, mlx, mly = mzx / cnt, mzy / cnt, mlx / cnt, mly / cnt
    sd = sx = zero
    for k in ks:
        ax, ay, bx, by = zv[k, 0] - mzx, zv[k, 1] - mzy, L[lm[k], 0] - mlx, L[lm[k], 1] - mly
        sd, sx = sd + (ax * bx + ay * by), sx + (ax * by - ay * bx)
    nrm = np.sqrt(sd * sd + sx * sx)
    if nrm > zero:
        c, s, phi = sd / nrm, sx / nrm, np.arctan2(sx, sd)
    tx, ty = mlx - (c * mzx - s * mzy), mly - (s * mzx + c * mzy)
    rss = zero
    for k in ks:
        ex, ey = tx + (c * zv[k, 0] - s * zv[k, 1]) - L[lm[k], 0], ty + (s * zv[k, 0] + c * zv[k, 1]) - L[lm[k], 1]
        rss = rss + (ex * ex + ey * ey)
    return (tx, ty, phi), np.sqrt(rss / cnt)


def locate(x, z, tol, min_sep=1.0, max_base=4, max_out=16, valid=None, dtype=np.float64, floats=None):
    """The reference of ekf_locate_scan.  `floats`: the dtype of the records' float fields (default: float64; the extended restatement
    is asked for np.longdouble records)."""
    dtype = np.dtype(dtype)
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    n_z = len(z)
    at = np.array([k for k in range(n_z) if valid is None or valid[k]], dtype=np.int64)
    assert len(at) <= MAX_MEAS
    L = np.asarray(x, dtype=np.float64)[3:].reshape(-1, 2).astype(dtype)
    margins = {"length": np.inf, "radius": np.inf, "nearest": np.inf, "one_to_one": np.inf, "order": np.inf}
    rec = LOCATE_DTYPE if floats is None else np.dtype([(n, floats if LOCATE_DTYPE[n].base == np.float64 else LOCATE_DTYPE[n].base, LOCATE_DTYPE[n].shape)
                                                       for n in LOCATE_DTYPE.names])
    none = Result(np.zeros(0, dtype=rec), np.zeros((0, n_z), dtype=np.int32), 0, margins, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    if len(L) < 2 or len(at) < 2:
        return none
    zd = z.astype(dtype)
    pairs = base_pairs(zd, valid, dtype.type(min_sep), max_base, dtype)
    if not pairs:
        return none
    r, i, j = candidates(L, pairs, tol, margins)
    if len(r) == 0:
        return none
    pose = pair_poses(L, zd, pairs, r, i, j)
    lm, d2, win, inl, ssr = score(L, zd[at], pose[0], pose[1], pose[2], pose[3], tol, margins)
    key = (r << 28) | (i << 14) | j
    order = np.lexsort((key, ssr, -inl))
    top = order[:max_out + 1]   # the written ones and the first left out: a tie of the order key among these would show in the output
    for u, v in zip(top[:-1], top[1:]):
        if inl[u] == inl[v] and max(ssr[u], ssr[v]) > 0:
            margins["order"] = min(margins["order"], float(abs(ssr[u] - ssr[v]) / max(ssr[u], ssr[v])))
    written = order[:max_out]
    hyps, ids = np.zeros(len(written), dtype=rec), np.full((len(written), n_z), -1, dtype=np.int32)
    for t, q in enumerate(written):
        fitted, rms = refit(L, zd[at], lm[q], win[q], tuple(v[q] for v in pose))
        hyps["pose"][t], hyps["rms"][t], hyps["ssr"][t], hyps["inliers"][t] = fitted, rms, ssr[q], inl[q]
        hyps["pair_pose"][t] = (pose[2][q], pose[3][q], np.arctan2(pose[5][q], pose[4][q]))
        hyps["meas_a"][t], hyps["meas_b"][t], hyps["lm_i"][t], hyps["lm_j"][t] = pairs[r[q]][0], pairs[r[q]][1], i[q], j[q]
        ids[t, at[win[q]]] = lm[q][win[q]]
    return Result(hyps, ids, len(r), margins, inl, order)


def locate_extended(x, z, tol, min_sep=1.0, max_base=4, max_out=16, valid=None):
    return locate(x, z, tol, min_sep, max_base, max_out, valid, dtype=np.longdouble, floats=np.longdouble)


def same_pose(a, b, tol, reach):
    """The header's rule, restated: positions within 2 tol, headings within 2 tol / reach."""
    if not math.hypot(a[0] - b[0], a[1] - b[1]) <= 2.0 * tol:
        return False
    return not reach > 0.0 or abs(math.remainder(a[2] - b[2], 2.0 * math.pi)) <= 2.0 * tol / reach


def reach_of(z, valid=None):
    z = np.asarray(z).reshape(-1, 2)
    keep = np.ones(len(z), dtype=bool) if valid is None else np.asarray(valid) != 0
    return float(np.hypot(z[keep, 0], z[keep, 1]).max(initial=0.0))


def accept(hyps, tol, reach, min_inliers, lead):
    """ekf_relocalize's acceptance rule."""
    if len(hyps) == 0 or hyps["inliers"][0] < min_inliers:
        return False
    return all(h["inliers"] <= hyps["inliers"][0] - lead or same_pose(h["pose"], hyps["pose"][0], tol, reach) for h in hyps[1:])


def reset_pose(x, P, pose, P_RR):
    """The reference of ekf_reset_pose on a dense export."""
    x, P = np.array(x), np.array(P)
    P_RR = np.asarray(P_RR, dtype=np.float64).reshape(3, 3)
    x[:3] = pose
    P[:3, :], P[:, :3] = 0.0, 0.0
    P[:3, :3] = 0.5 * (P_RR + P_RR.T)
    P[[0, 1, 2], [0, 1, 2]] = np.diag(P_RR)
    return x, P


def relocalize(x, P, z, R, tol, P_RR, min_sep=1.0, max_base=4, max_out=16, min_inliers=4, lead=2, window=16):
    """The reference of the composite: (n, x, P, hyp or None, ids, d2); n = 0: refused, x and P as they came."""
    res = locate(x, z, tol, min_sep, max_base, max_out)
    none = np.full(len(z), -1, dtype=np.int32)
    if not accept(res.hyps, tol, reach_of(z), min_inliers, lead):
        return 0, x, P, (res.hyps[0] if len(res.hyps) else None), (res.ids[0] if len(res.hyps) else none), np.full(len(z), np.nan)
    x1, P1 = reset_pose(x, P, res.hyps["pose"][0], P_RR)
    x2, P2, _, d2 = mr.update(x1, P1, z, R, res.ids[0], window)
    return int(res.hyps["inliers"][0]), x2, P2, res.hyps[0], res.ids[0], d2


def check_margins(res, what, ordered=True):
    """Every threshold at least EDGE away from what is compared to it (the order key's ties only where the order is compared)."""
    m = {k: v for k, v in res.margins.items() if ordered or k != "order"}
    assert all(v >= EDGE for v in m.values()), (what, "a compared quantity lies on a threshold: another seed", m)
    return m


def check(got, ref, what, ordered=True):
    """A device result (hyps, ids, n_candidates) against the reference: the integer fields, the ids and the candidate count exactly,
    the floats within POSE_ABS / SSR_REL / RMS_REL.  ordered=False (a scan of two measurements: (i, j) and (j, i) score the same in
    exact arithmetic, the tie is inherent): every candidate must have been written, and the lists are compared by (r, i, j).
    Returns the worst (pose, ssr, rms) differences seen."""
    hyps, ids, n_cand = got
    assert n_cand == ref.n_cand and len(hyps) == len(ref.hyps), (what, n_cand, ref.n_cand, len(hyps), len(ref.hyps))
    assert ids.shape == ref.ids.shape and hyps.dtype == LOCATE_DTYPE and not hyps["reserved"].any(), what
    want, want_ids = ref.hyps, ref.ids
    ints = ("inliers", "meas_a", "meas_b", "lm_i", "lm_j")
    if not ordered:
        assert len(hyps) == n_cand, (what, "the comparison by key needs every candidate written")
        keyed = lambda h: np.lexsort((h["lm_j"], h["lm_i"], h["meas_b"], h["meas_a"]))  # noqa: E731
        assert np.all(np.diff(hyps["inliers"]) <= 0), what
        g, w = keyed(hyps), keyed(want)
        hyps, ids, want, want_ids = hyps[g], ids[g], want[w], want_ids[w]
    for f in ints:
        assert hyps[f].tolist() == want[f].tolist(), (what, f, hyps[f].tolist(), want[f].tolist())
    assert ids.tolist() == want_ids.tolist(), (what, "ids")
    worst = [0.0, 0.0, 0.0]
    if len(hyps):
        dphi = np.abs(np.remainder(hyps["pose"][:, 2] - want["pose"][:, 2] + np.pi, 2.0 * np.pi) - np.pi)
        dpair = np.abs(np.remainder(hyps["pair_pose"][:, 2] - want["pair_pose"][:, 2] + np.pi, 2.0 * np.pi) - np.pi)
        worst[0] = float(max(np.abs(hyps["pose"][:, :2] - want["pose"][:, :2]).max(), np.abs(hyps["pair_pose"][:, :2] - want["pair_pose"][:, :2]).max(),
                             dphi.max(), dpair.max()))
        for n, f in ((1, "ssr"), (2, "rms")):
            some = want[f] != 0.0
            assert np.array_equal(hyps[f] == 0.0, ~some), (what, f)
            worst[n] = float((np.abs(hyps[f] - want[f])[some] / want[f][some]).max()) if some.any() else 0.0
    print("%s: %d hypotheses of %d candidates; pose %.3e, ssr relative %.3e, rms relative %.3e" % ((what, len(hyps), n_cand) + tuple(worst)))
    assert worst[0] <= POSE_ABS and worst[1] <= SSR_REL and worst[2] <= RMS_REL, (what, worst)
    return worst


# ---- the inputs of tests/test_gpu_locate_scan.py and tests/test_gpu_reset_pose.py (checked on the CPU in tests/test_locate_scan_cpu.py) ----
SIZES = mr.SIZES
EDGE_SIZES = [(63, 64), (64, 64), (65, 128), (255, 256), (256, 256), (257, 320), (2, 8), (1, 8), (0, 8)]
WIDE_COUNTS = mr.WIDE_COUNTS
SPURIOUS = (3, 8)            # the two measurements of the planted scans that are replaced by uniform spurious ones
# ... drawn with seed SCAN_SEED[N] + 5000 + SPURIOUS_SEED[N].  At N = 200 the seed is the first for which the THREE farthest-apart base
# pairs all hold a spurious measurement, the fourth none, and no spurious measurement falls on a landmark: one base pair fails where
# four succeed, which is why max_base exists (tests/test_locate_scan_cpu.py asserts all of it).
SPURIOUS_SEED = {100: 0, 200: 55}
OVERFLOW_TOL = 0.3           # on N = 200: more candidates than the list starts with
LOST = (3.0, 2.0)            # the pose error of a lost robot: metres (x and y), radians
Input = collections.namedtuple("Input", "name x P z R valid ids args ordered")
Args = collections.namedtuple("Args", "tol min_sep max_base max_out")


def planted(pkg, N, count=12):
    """(x, P, z, R, ids): match_ref.planted_scan with two measurements replaced by spurious ones (ids -1), uniform in the scan's
    bounding box made a quarter larger about its centre."""
    x, P, z, R, ids = mr.planted_scan(pkg, N, mr.SCAN_SEED[N], count=count)
    rng = np.random.default_rng(mr.SCAN_SEED[N] + 5000 + SPURIOUS_SEED[N])
    z, ids = z.copy(), ids.copy()
    lo, hi = z.min(axis=0), z.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    lo, hi = mid - 1.25 * half, mid + 1.25 * half
    for k in SPURIOUS:
        z[k], ids[k] = rng.uniform(lo, hi), -1
    return x, P, z, R, ids


def scan_of_landmarks(x, lms, seed, sigma=0.01):
    """z [len(lms)][2]: landmark lms[k] seen from the pose of x, with Gaussian noise of sigma metres per axis."""
    c, s = mr.libm_trig(float(x[2]))
    C = np.array([[c, -s], [s, c]])
    rng = np.random.default_rng(seed)
    return np.stack([C.T @ (x[3 + 2 * l:5 + 2 * l] - x[0:2]) for l in lms]) + sigma * rng.normal(size=(len(lms), 2))


def last_landmarks_scan(x, N, seed, count=5):
    """A scan planted on the LAST landmarks of the map, so that a dropped tail shows: landmark N - 1, the landmark f farthest from it,
    and the count - 2 highest-numbered others that lie nearer to both of them than they are apart -- so that (N - 1, f) is the
    farthest-apart pair of the scan, the base pair of rank 0.  Returns (z, lms)."""
    L = x[3:].reshape(-1, 2)
    d_last = np.hypot(L[:, 0] - L[N - 1, 0], L[:, 1] - L[N - 1, 1])
    f = int(np.argmax(d_last))
    d_f = np.hypot(L[:, 0] - L[f, 0], L[:, 1] - L[f, 1])
    inside = [l for l in range(N - 2, -1, -1) if l != f and max(d_last[l], d_f[l]) < 0.9 * d_last[f]][:count - 2]
    lms = [N - 1, f] + inside
    return scan_of_landmarks(x, lms, seed), np.array(lms, dtype=np.int32)


def edge_state(pkg, N):
    if N == 0:
        return np.zeros(3), np.zeros((3, 3))
    return pkg.scenarios.injected_state(N, seed=1700 + N, extent=mr.map_extent(N))


def wide_batch(pkg):
    """[(x, P, z [9][2], valid [9], lms)] of the batch of 257, 0, 33 and 64 landmarks: per-filter scans on the last landmarks, padded to
    nine entries with masked NaN ones (interleaved for filter 0)."""
    out = []
    for b, n in enumerate(WIDE_COUNTS):
        x, P = mr.batch_states(pkg, WIDE_COUNTS, 90)[b]
        z, valid, lms = np.full((9, 2), np.nan), np.zeros(9, dtype=np.uint8), np.full(9, -1, dtype=np.int32)
        if n:
            zs, ls = last_landmarks_scan(x, n, 1900 + b, count=5 + (b % 2))
            at = [0, 2, 3, 5, 6, 8][:len(zs)] if b == 0 else list(range(len(zs)))
            z[at], valid[at], lms[at] = zs, 1, ls
        else:
            z[:3], valid[:3] = [[1.0, 0.0], [0.0, 2.0], [3.0, 1.0]], 1   # a scan on an empty map: nothing to find
        out.append((x, P, z, valid, lms))
    return out


def inputs(pkg):
    """Every search a GPU test compares with the reference."""
    out = []
    for N, _ in SIZES:
        x, P, z, R, ids = planted(pkg, N)
        for tol in ((0.1,) if N == 200 else (0.05, 0.1)):
            out.append(Input("planted N=%d, tol %g" % (N, tol), x, P, z, R, None, ids, Args(tol, 1.0, 4, 16), True))
    x, P, z, R, ids = planted(pkg, 200)
    out.append(Input("planted N=200, one base pair", x, P, z, R, None, ids, Args(0.1, 1.0, 1, 16), True))
    out.append(Input("planted N=200, tol 0.05", x, P, z, R, None, ids, Args(0.05, 1.0, 4, 16), True))
    out.append(Input("overflow N=200, tol %g" % OVERFLOW_TOL, x, P, z, R, None, ids, Args(OVERFLOW_TOL, 1.0, 4, 16), True))
    for N, _ in EDGE_SIZES:
        x, P = edge_state(pkg, N)
        if N >= 3:
            z, lms = last_landmarks_scan(x, N, 1800 + N)
            out.append(Input("edge N=%d" % N, x, P, z, None, None, lms, Args(0.1, 1.0, 1, 1), True))  # (max_out 1: behind the winner come hypotheses of two inliers, whose (i, j) and (j, i) tie)
        elif N == 2:
            out.append(Input("edge N=2", x, P, scan_of_landmarks(x, [1, 0], 1802), None, None, np.array([1, 0], dtype=np.int32), Args(0.1, 0.5, 1, 16), False))
        else:
            out.append(Input("edge N=%d" % N, x, P, np.array([[1.0, 0.0], [0.0, 2.0]]), None, None, np.array([-1, -1], dtype=np.int32), Args(0.1, 1.0, 1, 16), True))
    # scan sizes on N = 100: two measurements (every candidate written: max_out 64), 32 (24 planted and 8 more of the nearest landmarks)
    x, P, z, R, ids = mr.planted_scan(pkg, 100, mr.SCAN_SEED[100])
    far = np.argmax(np.hypot(z[:, 0] - z[0, 0], z[:, 1] - z[0, 1]))
    out.append(Input("two measurements", x, P, z[[0, far]], None, None, ids[[0, far]], Args(0.01, 1.0, 1, 64), False))
    z32, R32, ids32 = mr.hypothesis_of_32(pkg, x, z, R, ids)
    out.append(Input("32 measurements", x, P, z32, R32, None, ids32, Args(0.1, 1.0, 2, 16), True))
    valid = np.ones(12, dtype=np.uint8)
    valid[[0, 5, 11]] = 0
    xm, Pm, zm, Rm, idm = planted(pkg, 100)
    zm = zm.copy()
    zm[valid == 0] = np.nan
    out.append(Input("a valid mask with holes", xm, Pm, zm, Rm, valid, np.where(valid != 0, idm, -1), Args(0.1, 1.0, 4, 16), True))
    for b, (x, P, z, valid, lms) in enumerate(wide_batch(pkg)):
        out.append(Input("wide batch, filter %d" % b, x, P, z, None, valid, lms, Args(0.1, 1.0, 2, 2), True))
    assert len(set(t.name for t in out)) == len(out)
    return out


def reference_of(t):
    return locate(t.x, t.z, t.args.tol, t.args.min_sep, t.args.max_base, t.args.max_out, t.valid)
