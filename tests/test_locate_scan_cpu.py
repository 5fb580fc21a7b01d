"""CPU tests of the relocalisation calls (ekf_locate_scan, ekf_reset_pose, ekf_relocalize and their batch forms): the header declares
the calls and the record, the binding lists them; the plan functions order and cut the base pairs, refuse, accept and tell the same
pose as they must (tests/cpp/locate_plan_check.cpp); and, for every input a GPU test of tests/test_gpu_locate_scan.py compares with
the reference (locate_ref.inputs), the NumPy reference recovers the planted pose and ids, every threshold lies at least 1e-9
(relative) away from what is compared to it -- which lets the GPU tests ask for the integer outputs EXACTLY --, and the reference is
checked against its restatement in extended precision, which MEASURES the bounds the GPU tests use for the floats.  distinct_poses,
the acceptance rule, the reset reference and the composite; the Python layer's argument checks."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_ref as lr  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ekf_locate_scan", "ekf_batch_locate_scan", "ekf_reset_pose", "ekf_batch_reset_pose", "ekf_relocalize", "ekf_batch_relocalize")
INTS = ("inliers", "meas_a", "meas_b", "lm_i", "lm_j")


@pytest.fixture(scope="module")
def results(pkg):
    """[(Input, Result)]"""
    return [(t, lr.reference_of(t)) for t in lr.inputs(pkg)]


def by_name(results, name):
    return next(tr for tr in results if tr[0].name == name)


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    m = re.search(r"typedef\s+struct\s+ekf_locate_hyp\s*\{(.*?)\}\s*ekf_locate_hyp;", src, flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["double pose[3]", "double pair_pose[3]", "double ssr", "double rms", "int inliers", "int meas_a, meas_b", "int lm_i, lm_j", "int reserved"]
    E = pkg.ekfslam
    assert E.LOCATE_DTYPE == lr.LOCATE_DTYPE and E.LOCATE_DTYPE.itemsize == 88 and E.LOCATE_DTYPE.itemsize % 8 == 0
    assert [n for n, _ in E.EkfLocateHyp._fields_] == list(E.LOCATE_DTYPE.names)
    assert (E.LOCATE_MAX_MEAS, E.LOCATE_MAX_BASE, E.LOCATE_MAX_OUT, E.LOCATE_MAX_CAND) == (lr.MAX_MEAS, lr.MAX_BASE, lr.MAX_OUT, lr.MAX_CAND)
    for macro, value in (("EKF_LOCATE_MAX_BASE", "16"), ("EKF_LOCATE_MAX_OUT", "64"), ("EKF_LOCATE_MAX_CAND", "(1 << 22)")):
        assert re.search(r"#define\s+%s\s+%s\s" % (macro, re.escape(value)), src), macro
    assert "P and R play" in raw and "ONLY x IS READ" in raw   # the header says what the search does not look at
    for cls in (pkg.FilterBatch, pkg.KalmanFilter):
        assert callable(cls.locate_scan) and callable(cls.reset_pose) and callable(cls.relocalize)
    assert callable(pkg.distinct_poses) and pkg.distinct_poses is pkg.ekfslam.distinct_poses


def test_plan_functions_order_cut_refuse_and_accept(tmp_path):
    out = run_cpp_check(tmp_path, "locate_plan_check")
    assert out.returncode == 0 and "locate plan ok" in out.stdout, out.stdout + out.stderr


def test_the_kernels_have_names_inside_no_other_kernels_name():
    src = open(os.path.join(ROOT, "2d-ekf-slam_amd", "csrc", "ekf_locate.hip")).read() + open(os.path.join(ROOT, "2d-ekf-slam_amd", "csrc", "ekf_rewrite.hip")).read()
    every = []
    for f in os.listdir(os.path.join(ROOT, "2d-ekf-slam_amd", "csrc")):
        if f.endswith(".hip"):
            every += re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", open(os.path.join(ROOT, "2d-ekf-slam_amd", "csrc", f)).read())
    for name in ("k_loc_pairs", "k_loc_score", "k_loc_pick", "k_loc_fit", "k_reset_pose"):
        assert re.search(r"\bvoid\s+%s\s*\(" % name, src), name
        assert [k for k in set(every) if name in k] == [name], name


def test_reference_recovers_the_planted_pose_and_ids(pkg, results):
    for t, r in results:
        if not t.name.startswith("planted") or "one base pair" in t.name:
            continue
        best = r.hyps[0]
        got = r.ids[0]
        assert np.hypot(*(best["pose"][:2] - t.x[:2])) <= t.args.tol, t.name   # within tol of truth
        assert all(g == w for g, w in zip(got, t.ids) if g >= 0), (t.name, got, t.ids)   # every inlier id is the planted one
        assert best["inliers"] == (got >= 0).sum() >= 9 and (got[list(lr.SPURIOUS)] == -1).all(), t.name
        print("%s: %d of %d inliers, runner-up %d, %d candidates, pose error %.4f m" % (
            t.name, best["inliers"], len(t.z), pkg.distinct_poses(r.hyps, t.args.tol, lr.reach_of(t.z, t.valid))[0]["inliers"][1], r.n_cand, np.hypot(*(best["pose"][:2] - t.x[:2]))))


def test_the_planted_scans_are_what_the_inputs_promise(results):
    """10 of 12 at both sizes and tolerances 0.1; at N = 200 the three farthest-apart base pairs all hold a spurious measurement and
    the fourth none: one base pair fails where four succeed.  N = 200 at tol 0.05 recovers the pose with 9 inliers under the 2 tol
    length filter of the definition (a filter of tol alone does not: the pair-pose error exceeds the radius) -- with ONE base pair it
    does not, which is the refused case of ekf_relocalize.  The tolerance of the overflow case finds more than the list starts with."""
    for name in ("planted N=200, tol 0.1", "planted N=100, tol 0.05", "planted N=100, tol 0.1"):
        assert by_name(results, name)[1].hyps["inliers"][0] == 10, name
    t, r = by_name(results, "planted N=200, tol 0.1")
    pairs = lr.base_pairs(t.z, None, 1.0, 4)
    assert [a in lr.SPURIOUS or b in lr.SPURIOUS for a, b, _ in pairs] == [True, True, True, False]
    assert r.n_cand > lr.LIST_FLOOR and r.hyps["meas_a"][0] == pairs[3][0] and r.hyps["meas_b"][0] == pairs[3][1]
    one = by_name(results, "planted N=200, one base pair")[1]
    assert one.hyps["inliers"][0] == 5 and one.n_cand < lr.LIST_FLOOR
    assert by_name(results, "planted N=200, tol 0.05")[1].hyps["inliers"][0] == 9
    assert lr.locate(t.x, t.z, 0.05, max_base=1).hyps["inliers"][0] == 4
    over = by_name(results, "overflow N=200, tol %g" % lr.OVERFLOW_TOL)[1]
    print("overflow: %d candidates against a list of %d" % (over.n_cand, lr.LIST_FLOOR))
    assert over.n_cand > 3 * lr.LIST_FLOOR
    for N, _ in lr.EDGE_SIZES:
        t, r = by_name(results, "edge N=%d" % N)
        if N >= 3:   # the scan is planted on the last landmarks: the winner's pair holds N - 1, every measurement is an inlier
            assert N - 1 in (r.hyps["lm_i"][0], r.hyps["lm_j"][0]) and r.ids[0].tolist() == t.ids.tolist(), t.name
        elif N == 2:
            assert r.n_cand == 2 and r.hyps["inliers"].tolist() == [2, 2]
        else:
            assert r.n_cand == 0 and len(r.hyps) == 0
    two = by_name(results, "two measurements")[1]
    assert two.n_cand == len(two.hyps) <= lr.MAX_OUT   # every candidate written: the lists are compared by key
    assert by_name(results, "32 measurements")[1].hyps["inliers"][0] == 24
    for b, n in enumerate(lr.WIDE_COUNTS):
        t, r = by_name(results, "wide batch, filter %d" % b)
        assert (len(r.hyps) == 0) if n == 0 else (n - 1 in (r.hyps["lm_i"][0], r.hyps["lm_j"][0]) and r.ids[0].tolist() == t.ids.tolist()), t.name


def test_inputs_lie_off_every_threshold(results):
    """What lets the GPU tests ask for the integer fields, the ids, the candidate count and the order EXACTLY: over every candidate of
    every input, no landmark-pair length within 1e-9 (relative) of a length filter's edge, no nearest squared distance within 1e-9 of
    tol^2, no inlier whose runner-up landmark is within 1e-9 of its nearest, no two inliers of one landmark within 1e-9 of each other,
    and -- among the written hypotheses and the first one left out -- no two equal inlier counts with ssr within 1e-9."""
    for t, r in results:
        m = lr.check_margins(r, t.name, t.ordered)
        print("%s: margins %s" % (t.name, ", ".join("%s %.1e" % kv for kv in m.items())))


def ext_by_key(t, r, e):
    """The reference's and the restatement's records in one order: as written, or by key where the order is not compared."""
    if t.ordered:
        return r.hyps, r.ids, e.hyps, e.ids
    keyed = lambda h: np.lexsort((h["lm_j"], h["lm_i"], h["meas_b"], h["meas_a"]))  # noqa: E731
    a, b = keyed(r.hyps), keyed(e.hyps)
    return r.hyps[a], r.ids[a], e.hyps[b], e.ids[b]


def test_reference_against_extended_precision(results):
    """The measurement behind locate_ref.POSE_ABS, SSR_REL and RMS_REL: the largest difference between the double reference and its
    extended-precision restatement over every written hypothesis of every input, recorded there as MEASURED_*; the bounds are 20
    times them.  The integer outputs agree exactly."""
    worst = [0.0, 0.0, 0.0]
    for t, r in results:
        e = lr.locate_extended(t.x, t.z, t.args.tol, t.args.min_sep, t.args.max_base, t.args.max_out, t.valid)
        assert e.n_cand == r.n_cand and len(e.hyps) == len(r.hyps), t.name
        h, ids, he, ide = ext_by_key(t, r, e)
        assert all(h[f].tolist() == he[f].tolist() for f in INTS) and ids.tolist() == ide.tolist(), t.name
        if not len(h):
            continue
        dp = float(max(np.abs(h["pose"] - he["pose"]).max(), np.abs(h["pair_pose"] - he["pair_pose"]).max()))
        ds = float((np.abs(h["ssr"] - he["ssr"]) / he["ssr"]).max())
        dr = float((np.abs(h["rms"] - he["rms"]) / he["rms"]).max())
        print("%s: pose %.3e, ssr relative %.3e, rms relative %.3e over %d hypotheses" % (t.name, dp, ds, dr, len(h)))
        worst = [max(worst[0], dp), max(worst[1], ds), max(worst[2], dr)]
    print("worst, double against extended: pose %.3e, ssr relative %.3e, rms relative %.3e" % tuple(worst))
    for got, name in zip(worst, ("MEASURED_POSE_ABS", "MEASURED_SSR_REL", "MEASURED_RMS_REL")):
        rec = getattr(lr, name)
        assert got <= rec, (got, "locate_ref.%s is out of date" % name)
        assert got >= rec / 2.0, (got, "locate_ref.%s is not what is measured" % name)
    assert (lr.POSE_ABS, lr.SSR_REL, lr.RMS_REL) == (20.0 * lr.MEASURED_POSE_ABS, 20.0 * lr.MEASURED_SSR_REL, 20.0 * lr.MEASURED_RMS_REL)


def test_check_refuses_what_it_should(results):
    """The comparison the GPU tests use, on the reference itself and on tampered copies."""
    t, r = by_name(results, "planted N=100, tol 0.1")
    lr.check((r.hyps.copy(), r.ids.copy(), r.n_cand), r, t.name)
    for field, delta in (("inliers", 1), ("lm_j", 1), ("ssr", 1e-6), ("rms", 1e-6)):
        h = r.hyps.copy()
        h[field][3] += delta if field in INTS else delta * h[field][3]
        with pytest.raises(AssertionError):
            lr.check((h, r.ids.copy(), r.n_cand), r, t.name)
    h = r.hyps.copy()
    h["pose"][0][2] += 1e-11
    ids = r.ids.copy()
    ids[1, 0] = 5
    for bad in ((h, r.ids, r.n_cand), (r.hyps, ids, r.n_cand), (r.hyps, r.ids, r.n_cand + 1), (r.hyps[::-1].copy(), r.ids[::-1].copy(), r.n_cand)):
        with pytest.raises(AssertionError):
            lr.check(bad, r, t.name)


def test_distinct_poses_merges_the_repeats_of_the_true_pose(pkg, results):
    t, _ = by_name(results, "planted N=100, tol 0.1")
    r = lr.locate(t.x, t.z, t.args.tol, max_base=16, max_out=32)   # sixteen base pairs: every clean one hits the true pose
    reach = lr.reach_of(t.z)
    kept, group = pkg.distinct_poses(r.hyps, t.args.tol, reach)
    hits = [k for k in range(len(r.hyps)) if np.hypot(*(r.hyps["pose"][k][:2] - t.x[:2])) <= t.args.tol and abs(r.hyps["pose"][k][2] - t.x[2]) < 0.05]
    assert len(hits) > 1 and len(set(group[hits].tolist())) == 1 and group[0] == 0   # the repeats of the true pose are one group, the first
    assert kept.dtype == lr.LOCATE_DTYPE and len(kept) == group.max() + 1 < len(r.hyps) and kept[0].tobytes() == r.hyps[0].tobytes()
    for k in range(len(r.hyps)):   # a member is the same pose as its group's first; the firsts are pairwise different
        assert pkg.ekfslam.same_pose(r.hyps["pose"][k], kept["pose"][group[k]], t.args.tol, reach)
    assert not any(pkg.ekfslam.same_pose(kept["pose"][i], kept["pose"][j], t.args.tol, reach) for i in range(len(kept)) for j in range(i))
    for (t2, r2) in results:   # the binding's rule is the reference's restatement of the header's
        for k in range(1, len(r2.hyps)):
            rc = lr.reach_of(t2.z, t2.valid)
            assert pkg.ekfslam.same_pose(r2.hyps["pose"][k], r2.hyps["pose"][0], t2.args.tol, rc) == lr.same_pose(r2.hyps["pose"][k], r2.hyps["pose"][0], t2.args.tol, rc)
    assert pkg.ekfslam.same_pose([0, 0, 3.14], [0, 0, -3.14], 0.1, 5.0) and not pkg.ekfslam.same_pose([0, 0, 0.0], [0, 0, 0.05], 0.1, 5.0)
    empty, g = pkg.distinct_poses(np.zeros(0, dtype=lr.LOCATE_DTYPE), 0.1, 1.0)
    assert len(empty) == 0 and len(g) == 0
    with pytest.raises(ValueError):
        pkg.distinct_poses(r.hyps, 0.0, reach)


def test_acceptance_and_the_composite_reference(pkg, results):
    t, r = by_name(results, "planted N=200, tol 0.1")
    reach = lr.reach_of(t.z)
    assert lr.accept(r.hyps, 0.1, reach, 6, 2) and not lr.accept(r.hyps, 0.1, reach, 11, 2) and not lr.accept(r.hyps, 0.1, reach, 6, 5)
    P_RR = np.diag([0.04, 0.04, 0.01])
    xl = t.x.copy()
    xl[:3] += (lr.LOST[0], lr.LOST[0], lr.LOST[1])
    n, x2, P2, hyp, ids, d2 = lr.relocalize(xl, t.P, t.z, t.R, 0.1, P_RR, min_inliers=6, lead=2)
    assert n == 10 and ids.tolist() == t.ids.tolist() and np.isfinite(d2[ids >= 0]).all() and np.isnan(d2[ids < 0]).all()
    assert np.hypot(*(x2[:2] - t.x[:2])) < 0.05 and abs(x2[2] - t.x[2]) < 0.02   # the lost pose plays no part: found again
    x1, P1 = lr.reset_pose(xl, t.P, hyp["pose"], P_RR)
    assert np.array_equal(x1[3:], t.x[3:]) and np.array_equal(P1[3:, 3:], t.P[3:, 3:]) and not P1[:3, 3:].any() and np.array_equal(P1[:3, :3], P_RR)
    want = mr.update(x1, P1, t.z, t.R, ids, 16)
    assert np.array_equal(x2, want[0]) and np.array_equal(P2, want[1])
    assert np.linalg.eigvalsh(P2).min() > -1e-12 * np.abs(P2).max()
    for tol in (0.05, 0.1):   # one base pair: refused, everything as it came
        n, x3, P3, hyp, ids, d2 = lr.relocalize(xl, t.P, t.z, t.R, tol, P_RR, max_base=1, min_inliers=6, lead=2)
        assert n == 0 and x3 is xl and P3 is t.P and hyp["inliers"] < 6 and np.isnan(d2).all()
    asym = np.array([[4.0, 1.0, 0.5], [3.0, 9.0, -1.0], [0.25, -2.0, 0.0]])
    assert lr.reset_pose(np.zeros(3), np.zeros((3, 3)), [1, 2, 3], asym)[1].tolist() == [[4.0, 2.0, 0.375], [2.0, 9.0, -1.5], [0.375, -1.5, 0.0]]


def test_the_benchmark_script_opens_no_gpu_at_import_and_names_its_kernels_apart():
    import subprocess
    scripts = os.path.join(ROOT, "scripts")
    code = ("import sys; sys.path.insert(0, %r); import bench_locate_scan as b; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('torch', 'ekfslam_amd', '__graft_entry__')], 'the import opened the package'; "
            "print(','.join(b.KERNELS)); print(len(b.CASES))" % scripts)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, n_cases = r.stdout.split()
    assert kernels.split(",") == ["k_loc_pairs", "k_loc_score", "k_loc_pick", "k_loc_fit"] and int(n_cases) == 12
    for name in os.listdir(scripts):   # ... inside no name another benchmark script traces, nor theirs inside these
        if name.startswith("bench_") and name.endswith(".py") and name != "bench_locate_scan.py":
            text = open(os.path.join(scripts, name)).read()
            assert not any(k in text for k in kernels.split(",")), name
    committed = os.path.join(ROOT, "profiles", "locate_scan.jsonl")
    if os.path.exists(committed):
        import json
        lines = [json.loads(ln) for ln in open(committed)]
        assert {ln["tol"] for ln in lines} == {0.1} and {ln["case"] for ln in lines} <= set("n%d_z%d_b%d" % (N, z, b) for N in (256, 1024, 4096) for z in (8, 32) for b in (1, 4))


class _NoLibrary:
    """Stands where the C library would: the Python layer must refuse before it gets here."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_python_layer_validates_its_arguments(pkg):
    f = pkg.FilterBatch.__new__(pkg.FilterBatch)
    f.L, f.h, f.batch = _NoLibrary(), None, 2
    z, R, P_RR = np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1)), np.eye(3)
    for kw in (dict(tol=0.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=0.1, min_sep=0.0), dict(tol=0.1, max_base=0), dict(tol=0.1, max_base=17),
               dict(tol=0.1, max_out=0), dict(tol=0.1, max_out=65), dict(tol=0.1, valid=[1, 1, 1])):
        with pytest.raises(ValueError):
            f.locate_scan(z, **kw)
    zn = z.copy()
    zn[1, 0] = np.nan
    for bad in (zn, np.zeros((3, 3)), z[None], np.zeros((33, 2))):
        with pytest.raises(ValueError):
            f.locate_scan(bad, 0.1)
    with pytest.raises(ValueError):
        f.locate_scan(z, 0.1, index=None)                       # no batch axis without an index
    with pytest.raises(ValueError):
        f.locate_scan(np.zeros((2, 3, 2)), 0.1, index=None, valid=np.ones((2, 2)))
    mask = np.ones((2, 3), dtype=np.uint8)
    mask[1, 1] = 0
    assert f._locate_args(np.stack([z, zn]), mask, None, 0.1, 1.0, 4, 16)[2:] == (3, 2)   # a masked entry is not looked at
    wide, ok = np.zeros((2, 33, 2)), np.ones((2, 33), dtype=np.uint8)
    ok[:, 0] = 0
    assert f._locate_args(wide, ok, None, 0.1, 1.0, 4, 16)[2] == 33                        # 33 entries of which 32 are valid
    for kw in (dict(pose=[0, 0], P_RR=P_RR), dict(pose=[0, 0, np.nan], P_RR=P_RR), dict(pose=[0, 0, 0], P_RR=-P_RR), dict(pose=[0, 0, 0], P_RR=np.eye(2)),
               dict(pose=np.zeros((2, 3)), P_RR=np.zeros((2, 3, 3))), dict(pose=np.zeros(3), P_RR=P_RR, index=None)):
        with pytest.raises(ValueError):
            f.reset_pose(**kw)
    for kw in (dict(min_inliers=1), dict(lead=-1), dict(tol=0.0), dict(P_RR=np.eye(2)), dict(P_RR=-np.eye(3)), dict(max_out=65)):
        args = dict(z=z, R=R, tol=0.1, P_RR=P_RR)
        args.update(kw)
        with pytest.raises(ValueError):
            f.relocalize(**args)
    with pytest.raises(ValueError):
        f.relocalize(z, R[:2], 0.1, P_RR)
