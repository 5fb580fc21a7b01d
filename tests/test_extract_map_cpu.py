"""CPU tests of submap extraction (ekf_extract_map / ekf_batch_extract_map / ekf_get_submap): the header declares the calls and the
binding lists them; the destination -> source index functions the kernels run (ekf_device.h) reproduce the tile packing of
P[sel, sel] for selections in any order (tests/cpp/extract_map_check.cpp); and the benchmark script's case table, byte model and dry
path, which touch no GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
sys.path.insert(0, SCRIPTS)
import bench_extract_map as b_ext  # noqa: E402

NEW_FUNCTIONS = ("ekf_extract_map", "ekf_batch_extract_map", "ekf_get_submap")


def test_header_declares_and_binding_lists_the_extraction_calls(pkg):
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    for meth in ("extract_map", "batch_extract_map", "get_submap"):
        assert callable(getattr(pkg.FilterBatch, meth))
    assert callable(pkg.KalmanFilter.get_submap)
    # what a caller must be told: an extracted map is not independent of its source
    comment = src[src.index("Submap extraction on the device"):src.index("int ekf_extract_map(")]
    assert "NOT INDEPENDENT" in comment and "ekf_join_map" in comment and "ekf_get_x" in comment


def test_extraction_gather_reproduces_the_packing_of_the_selected_matrix(tmp_path):
    out = run_cpp_check(tmp_path, "extract_map_check")
    assert out.returncode == 0 and "extract map ok" in out.stdout, out.stdout + out.stderr


def test_map_plan_checks_and_tables(tmp_path):
    """csrc/ekf_map_plan.h called directly (tests/cpp/map_plan_check.cpp): the refusals of the map calls' lists with the library's
    codes and texts, and the removal, extraction and pair tables against a restatement, at landmark counts around the tile edges."""
    out = run_cpp_check(tmp_path, "map_plan_check")
    assert out.returncode == 0 and "map plan ok" in out.stdout, out.stdout + out.stderr


def test_kept_scratch_layout_and_growth_rule(tmp_path):
    """csrc/ekf_map_scratch.h and plan_grown_cap called directly (tests/cpp/map_scratch_check.cpp): every kept block's size is the
    byte count the hand-written reserve functions computed, its arrays are aligned, disjoint and fill it, at capacities around the
    tile and workgroup edges; the growth rule against a brute-force loop."""
    out = run_cpp_check(tmp_path, "map_scratch_check")
    assert out.returncode == 0 and "map scratch ok" in out.stdout, out.stdout + out.stderr


def test_bench_case_table_and_byte_model():
    assert b_ext.CASES == list(b_ext.TABLE)
    c = {case: b_ext.parse(case) for case in b_ext.CASES}
    near = [c["near256_of_4096_inplace"], c["near256_of_4096_overlap"]]
    assert [(v["N"], v["count"], v["cap_d"]) for v in near] == [(4096, 256, 256)] * 2 and [v["overlap"] for v in near] == [False, True]
    assert (c["copy_4096"]["N"], c["copy_4096"]["count"], c["copy_4096"]["cap_d"]) == (4096, None, 4096)
    assert (c["n64_of_1024"]["N"], c["n64_of_1024"]["count"]) == (1024, 64)
    assert (c["batch256_n64_of_256"]["B"], c["batch256_n64_of_256"]["N"], c["batch256_n64_of_256"]["count"]) == (256, 256, 64)
    assert c["submap256_of_4096"]["kind"] == "submap" and [v["kind"] for k, v in c.items() if k != "submap256_of_4096"] == ["extract"] * 5
    for v in c.values():
        assert v["cap_d"] == 0 or (v["count"] or v["N"]) <= v["cap_d"]
    # the whole copy reads and writes the 8256 stored tiles of 4096 landmarks, 270.5 MB each way; 256 landmarks are 36 tiles
    assert b_ext.algorithmic_bytes(c["copy_4096"]) == 2 * 8256 * 32768 == 2 * 270532608
    assert b_ext.algorithmic_bytes(c["near256_of_4096_inplace"]) == 2 * 36 * 32768
    assert b_ext.algorithmic_bytes(c["batch256_n64_of_256"]) == 256 * 2 * 3 * 32768
    assert b_ext.algorithmic_bytes(c["submap256_of_4096"]) == 2 * 515 * 515 * 8


def test_robot_nearest_ids_are_distinct_and_nearest_first():
    rng = np.random.default_rng(5)
    x = np.concatenate([[1.0, -2.0, 0.3], rng.uniform(-30.0, 30.0, 2 * 500)])
    ids = b_ext.nearest_ids(x, 64)
    assert ids.dtype == np.int32 and ids.size == 64 and np.unique(ids).size == 64
    r = np.hypot(*(x[3:].reshape(-1, 2) - x[:2]).T)
    assert np.all(np.diff(r[ids]) >= 0.0) and r[ids].max() <= np.sort(r)[63]
    assert not np.array_equal(ids, np.sort(ids))  # a scattered selection


def test_no_kernel_name_lies_inside_another():
    import bench_find_duplicates, bench_join_map, bench_joint_consistency, bench_reframe, bench_remove_landmarks  # noqa: E401
    others = (bench_find_duplicates, bench_join_map, bench_joint_consistency, bench_reframe, bench_remove_landmarks)
    for k in b_ext.KERNELS:
        assert [o for o in b_ext.KERNELS if k in o] == [k], k
        for other in others:
            assert not [o for o in other.KERNELS if k in o or o in k], (k, other.__name__)


def test_dry_run_prints_every_case_and_opens_nothing(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "bench_extract_map.py"), "--dry"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    lines = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert [ln["case"] for ln in lines] == b_ext.CASES
    for ln in lines:
        assert ln == b_ext.plan(ln["case"]) and ln["bytes"] == b_ext.algorithmic_bytes(b_ext.parse(ln["case"]))
    assert os.listdir(str(tmp_path)) == []  # nothing written
    code = "import sys; sys.path.insert(0, %r); import bench_extract_map; bad = [m for m in ('torch', 'ekfslam_amd') if m in sys.modules]; assert not bad, bad"
    r = subprocess.run([sys.executable, "-c", code % SCRIPTS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_recorded_profile_matches_the_case_table():
    """profiles/extract_map.jsonl, once the script has run: one line per case, in order, with the byte model's figures."""
    path = os.path.join(ROOT, "profiles", "extract_map.jsonl")
    if not os.path.exists(path):
        design = open(os.path.join(ROOT, "DESIGN.md")).read()
        section = design[design.index("### 4.13"):design.index("## 5. Measurement")]
        assert "not measured" in section.lower(), "no profile and DESIGN.md 4.13 does not say so"
        return
    rec = [json.loads(ln) for ln in open(path)]
    assert [ln["case"] for ln in rec] == b_ext.CASES
    for ln in rec:
        assert ln["bytes"] == b_ext.algorithmic_bytes(b_ext.parse(ln["case"])), ln["case"]
