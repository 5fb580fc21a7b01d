"""CPU tests of the map-operation benchmark scripts (scripts/mapbench.py and the five bench_*.py on top of it): the trace reader and
its grouping into calls on synthetic rocprofv3 files, the kernel names against the substring rule the reader matches them by, the
child protocol (timeout -k 10 in front, RESULT line, first failure ends the run, --out rewritten per case) on stub scripts that touch
no GPU, the byte models and case lists against the committed profiles, and that importing any of them opens nothing."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
sys.path.insert(0, SCRIPTS)
import bench_find_duplicates as b_dup  # noqa: E402
import bench_join_map as b_join  # noqa: E402
import bench_joint_consistency as b_joint  # noqa: E402
import bench_reframe as b_reframe  # noqa: E402
import bench_remove_landmarks as b_remove  # noqa: E402
import mapbench  # noqa: E402

BENCHES = (b_remove, b_reframe, b_join, b_joint, b_dup)
KERNELS = ("k_reframe_vec", "k_reframe_tiles", "k_reframe_finish")
VEC, TILES, TILES_F, FINISH = ("k_reframe_vec(EkfDev, int, double const*)", "void k_reframe_tiles<true>(EkfDev, int, double const*)",
                               "void k_reframe_tiles<false>(EkfDev, int, double const*)", "k_reframe_finish(EkfDev, int)")
# four calls in ns, each ending with k_reframe_finish, foreign kernels in between; the first is the one to skip
TRACE = [(VEC, 1000, 3000), (TILES, 4000, 14000), (FINISH, 15000, 16000),
         ("void k_chain<true>(EkfDev, ChainArgs)", 16500, 17000), ("k_set_meta(EkfDev, int)", 17500, 18000),
         (VEC, 20000, 22500), (TILES, 23000, 33000), (TILES_F, 33500, 38500), (FINISH, 39000, 40500),
         ("void k_chain<false>(EkfDev, ChainArgs)", 41000, 49000),
         (VEC, 50000, 53500), (TILES, 54000, 74000), (FINISH, 75000, 77000),
         ("k_set_meta(EkfDev, int)", 78000, 79000),
         (VEC, 80000, 81500), (TILES, 82000, 94000), (TILES_F, 94500, 95500), (FINISH, 96000, 97000)]


@pytest.fixture()
def trace_dir(tmp_path):
    """TRACE as two *kernel_trace.csv files in different directories, rows out of time order, and one *kernel_stats.csv."""
    rows = [TRACE[i] for i in np.random.default_rng(3).permutation(len(TRACE))]
    for sub, part in (("host/1", rows[::2]), ("host/2", rows[1::2])):
        os.makedirs(tmp_path / sub)
        with open(tmp_path / sub / "rf_kernel_trace.csv", "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
            w.writerows(("KERNEL_DISPATCH",) + r for r in part)
    with open(tmp_path / "host/1" / "rf_kernel_stats.csv", "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerows([["Name", "Calls"], [TILES, "4"], ["void k_chain<true>(EkfDev, ChainArgs)", "1"], [FINISH, "4"]])
    return str(tmp_path)


def test_trace_is_read_sorted_and_cut_into_calls(trace_dir):
    rows = mapbench.read_trace(trace_dir, KERNELS)
    assert len(rows) == 14 and rows == sorted(rows) and {k for _, _, k in rows} == set(KERNELS)
    calls = mapbench.group_calls(rows, "k_reframe_finish")
    assert [c["launches"] for c in calls] == [3, 4, 3, 4]
    assert [c["span"] for c in calls] == pytest.approx([15.0, 20.5, 27.0, 17.0])
    assert [c["k_reframe_vec"] for c in calls] == pytest.approx([2.0, 2.5, 3.5, 1.5])
    assert [c["k_reframe_tiles"] for c in calls] == pytest.approx([10.0, 15.0, 20.0, 13.0])
    assert [c["k_reframe_finish"] for c in calls] == pytest.approx([1.0, 1.5, 2.0, 1.0])
    assert mapbench.group_calls(rows, "k_reframe_finish", skip_first=True) == calls[1:]


def test_trace_summary_medians_extras_and_call_count(trace_dir):
    got, stats = mapbench.summarize_trace(trace_dir, "n96_x", 3, KERNELS, "k_reframe_finish", skip_first=True)
    assert got["kernel_us"] == pytest.approx(19.0)  # of 19.0, 25.5, 15.5
    assert got["split_us"] == pytest.approx({"k_reframe_vec": 2.5, "k_reframe_tiles": 15.0, "k_reframe_finish": 1.5})
    assert sorted(r["Name"] for r in stats) == sorted([TILES, FINISH])
    got, _ = mapbench.summarize_trace(trace_dir, "n96_x", 4, KERNELS, "k_reframe_finish")
    assert got["kernel_us"] == pytest.approx(17.25)  # of 13.0, 19.0, 25.5, 15.5
    extras = lambda calls: dict(device_span_us=float(np.median([c["span"] for c in calls])), launches=calls[0]["launches"])  # noqa: E731
    got, _ = mapbench.summarize_trace(trace_dir, "n96_x", 3, KERNELS, "k_reframe_finish", skip_first=True, extras=extras)
    assert got["launches"] == 4 and got["device_span_us"] == pytest.approx(20.5)
    for n_calls, skip in ((4, True), (3, False), (5, False)):
        with pytest.raises(SystemExit, match="n96_x"):
            mapbench.summarize_trace(trace_dir, "n96_x", n_calls, KERNELS, "k_reframe_finish", skip_first=skip)


def test_no_kernel_name_lies_inside_another():
    for b in BENCHES:
        for k in b.KERNELS:
            assert [o for o in b.KERNELS if k in o] == [k], (b.__name__, k)
            for other in BENCHES:
                assert other is b or not [o for o in other.KERNELS if k in o], (b.__name__, k, other.__name__)


STUB = """import os, sys
sys.path.insert(0, %r)
import mapbench
def child(case, reps, baselines):
    with open(%r, "a") as fh:
        fh.write(case + "\\n")
    if case == "b":
        sys.exit(3)
    if case == "silent":
        os._exit(0)
    return dict(case=case, reps=reps, baselines=baselines, marker=os.environ.get("STUB_MARKER"), third=1.0 / 3.0)
if __name__ == "__main__":
    mapbench.main(__file__, ["a", "b", "c"], child)
"""


@pytest.fixture()
def stub(tmp_path):
    path, log = str(tmp_path / "stub.py"), str(tmp_path / "log")
    with open(path, "w") as fh:
        fh.write(STUB % (SCRIPTS, log))
    return path, log


def test_child_command_and_result_line(stub):
    path, log = stub
    cmd = mapbench.child_command(path, "a", 2, False, prefix=["rocprofv3", "--kernel-trace", "--"], timeout_s=77)
    assert cmd == ["timeout", "-k", "10", "77", "rocprofv3", "--kernel-trace", "--", sys.executable, path, "--child", "a", "--reps", "2", "--no-baselines"]
    assert mapbench.child_command(path, "a", 2, True)[:5] == ["timeout", "-k", "10", "420", sys.executable]
    line = mapbench.run_child(path, "a", 2, True, prefix=["env", "STUB_MARKER=under_prefix"], timeout_s=60)
    assert line == dict(case="a", reps=2, baselines=True, marker="under_prefix", third=1.0 / 3.0)
    with pytest.raises(SystemExit, match=r"case b failed \(3\)"):
        mapbench.run_child(path, "b", 2, True, timeout_s=60)
    with pytest.raises(SystemExit, match="case silent printed no result"):
        mapbench.run_child(path, "silent", 2, True, timeout_s=60)


def test_first_failing_child_ends_the_run_and_out_keeps_what_was_measured(stub, tmp_path):
    path, log = stub
    out = str(tmp_path / "out.jsonl")
    r = subprocess.run([sys.executable, path, "--reps", "2", "--child-timeout", "60", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "case b failed (3)" in r.stderr, r.stdout + r.stderr
    assert open(log).read().split() == ["a", "b"]  # c was never started
    want = dict(case="a", reps=2, baselines=True, marker=None, third=0.33333)
    assert [json.loads(ln) for ln in open(out)] == [want] and [json.loads(ln) for ln in r.stdout.splitlines()] == [want]


def _recorded(name):
    return [json.loads(ln) for ln in open(os.path.join(ROOT, "profiles", name))]


def test_byte_models_and_case_lists_equal_the_committed_profiles():
    for b, name, n in ((b_reframe, "reframe.jsonl", 12), (b_join, "join_map.jsonl", 5)):
        rec = _recorded(name)
        assert len(rec) == n and [ln["case"] for ln in rec] == b.CASES
        for ln in rec:
            assert b.algorithmic_bytes(b.parse(ln["case"])) == ln["bytes"], ln["case"]
    rec = _recorded("remove_landmarks.jsonl")
    assert len(rec) == 10 and [ln["case"] for ln in rec] == b_remove.CASES
    for ln in rec:
        c = b_remove.parse(ln["case"])
        assert b_remove.algorithmic_bytes(c, b_remove.masks(c, np.random.default_rng(11))) == ln["bytes"], ln["case"]


@pytest.mark.parametrize("module", ["mapbench"] + [b.__name__ for b in BENCHES])
def test_import_opens_no_gpu(module):
    code = "import sys; sys.path.insert(0, %r); import %s; bad = [m for m in ('torch', 'ekfslam_amd') if m in sys.modules]; assert not bad, bad"
    r = subprocess.run([sys.executable, "-c", code % (SCRIPTS, module)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
