"""GPU tests of the five map-operation benchmark scripts: each one run as a subprocess at small cases (N = 96 and 160: three and five
tiles per side, across a tile edge, and for removal a tile emptied), no trace.  Its lines are compared with the lines the scripts
printed for the same cases before they were moved onto scripts/mapbench.py (profiles/mapbench_parent_small.jsonl): the same keys, and
the same values in every field that does not depend on timing.  No time is compared."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"bench_remove_landmarks.py": ["n96_spread_overlap", "n160_block64_inplace"],
         "bench_reframe.py": ["n96_overlap_rigid", "n96_inplace_anchor"],
         "bench_join_map.py": ["n96_inplace", "n96_overlap"],  # (90 + 6 landmarks)
         "bench_joint_consistency.py": ["n96_inplace", "n96_overlap"],
         "bench_find_duplicates.py": ["n96_all", "n96_split64", "n96_path2m"]}
UNTIMED = ("case", "N", "Ng", "Ns", "batch", "overlap", "call", "split", "max_dist", "bytes", "tiles", "tile_steps", "scratch_bytes",
           "removed_per_filter_mean", "found", "degenerate", "matches_host")


def _parent_lines(script):
    with open(os.path.join(ROOT, "profiles", "mapbench_parent_small.jsonl")) as fh:
        return {r["line"]["case"]: r["line"] for r in map(json.loads, fh) if r["script"] == script}


@pytest.mark.parametrize("script", sorted(SMALL))
def test_small_cases_give_the_lines_of_the_unrefactored_script(script, tmp_path):
    cases, out = SMALL[script], str(tmp_path / "out.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--cases", ",".join(cases), "--reps", "2", "--child-timeout", "120",
                        "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(ln) for ln in open(out)]
    assert [ln["case"] for ln in lines] == cases and [json.loads(ln) for ln in r.stdout.splitlines()] == lines
    want = _parent_lines(script)
    assert sorted(want) == sorted(cases)
    for ln in lines:
        old = want[ln["case"]]
        assert set(ln) == set(old), (ln["case"], sorted(set(ln) ^ set(old)))
        for k in UNTIMED:
            assert (k in ln) == (k in old) and ln.get(k) == old.get(k), (ln["case"], k, ln.get(k), old.get(k))
        assert ln.get("matches_host", True) is True
