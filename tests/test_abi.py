"""CPU tests of the drop-in boundary: the C-ABI library builds, loads and exports exactly what
include/ekfslam_c.h declares; the HBM index maps are bijections; the product path refuses to run
without a gfx950 device (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(pkg):
    import __graft_entry__ as ge
    ge.build()
    return pkg


def header_functions():
    src = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ekf_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built.ekfslam.LIB_PATH)
    names = header_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "libekfslam_hip.so does not export %s" % n
    assert sorted(built.ekfslam.ABI_SYMBOLS) == names


def test_library_is_gfx950_only(built):
    blob = open(built.ekfslam.LIB_PATH, "rb").read()
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob))
    assert targets == {b"gfx950"}, targets


def test_default_params_equal_reference_literals(built):
    p = built.ekfslam.default_params()
    assert (p.sigma_v, p.sigma_w) == (0.01, 0.04)            # kalmanfilter.cpp:28-29
    assert (p.gamma_max, p.gamma_min) == (50.0, 10.0)        # kalmanfilter.cpp:67-68
    assert p.cond_limit == 80.0                              # Update.cpp:131


def test_no_cpu_fallback(built):
    from helpers import gpu_present
    if gpu_present():
        pytest.skip("a GPU is present")
    with pytest.raises(built.EkfError) as ei:
        built.FilterBatch(1, 8)
    assert ei.value.code == built.ekfslam.ERR_NO_DEVICE


def test_product_sources_never_touch_the_oracle():
    pdir = os.path.join(ROOT, "2d-ekf-slam_amd")
    for dp, _, files in os.walk(pdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.lower(), "%s mentions the oracle" % f
    for f in os.listdir(os.path.join(ROOT, "compat")) if os.path.isdir(os.path.join(ROOT, "compat")) else []:
        if f.endswith((".h", ".cpp", ".hpp")):
            assert "oracle" not in open(os.path.join(ROOT, "compat", f)).read().lower()


def test_hbm_index_maps_are_bijections(tmp_path):
    exe = str(tmp_path / "layout_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "layout_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "layout ok" in out.stdout, out.stdout + out.stderr


def test_chain_geometry_matches_the_recorded_table(tmp_path):
    """plan_geometry (csrc/ekf_geometry.h) decides workgroups, threads, LDS, kernel and window of every handle.  The table was dumped
    from create_impl's own text before the function was cut out of it; every field of every row must agree, and a doctored row must
    make the check fail."""
    exe = str(tmp_path / "geometry_check")
    table = os.path.join(ROOT, "tests", "golden", "chain_geometry.csv")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "geometry_check.cpp")])
    out = subprocess.run([exe, table], capture_output=True, text=True)
    assert out.returncode == 0 and "geometry ok" in out.stdout, out.stdout + out.stderr
    rows = open(table).read().splitlines()
    at = next(i for i, r in enumerate(rows) if r.startswith("1,4096,32,-1,163840,-99,-99,-99,-99,-99,-99,-99,0,1,64,"))  # 64 workgroups
    rows[at] = rows[at].replace(",0,1,64,", ",0,1,63,", 1)
    doctored = tmp_path / "doctored.csv"
    doctored.write_text("\n".join(rows) + "\n")
    out = subprocess.run([exe, str(doctored)], capture_output=True, text=True)
    assert out.returncode == 1 and "chain_wgs = 64, want 63" in out.stdout, out.stdout + out.stderr


def test_window_plans_match_the_recorded_decisions(tmp_path):
    """The window scheduler (csrc/ekf_window_plan.h) decides every segment, chain launch and dense-pass order.  The record was taken
    from the text of close_set, launch_ops, launch_ops_grouped, stream_op and settle before the header was cut out of them (its first
    line names the commit); every field of every line must agree, the planner's own invariants must hold, and a doctored line must
    make the check fail and name the field."""
    exe = str(tmp_path / "window_plan_check")
    import gzip
    record = str(tmp_path / "window_plans.txt")  # (12 289 lines: kept packed)
    lines = gzip.open(os.path.join(ROOT, "tests", "golden", "window_plans.txt.gz"), "rt").read().splitlines()
    open(record, "w").write("\n".join(lines) + "\n")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "window_plan_check.cpp")])
    out = subprocess.run([exe, record], capture_output=True, text=True)
    assert out.returncode == 0 and "window plans ok" in out.stdout, out.stdout + out.stderr
    # the balanced tail's pass of 18 slots behind the stream gate of a multi-segment launch (32 workgroups, second launch of the handle)
    at = lines.index("pass 0 1 flush 1 18 1 0 10 1 0 1 64 0 0 0 none 0 flush0 1 2 0 0 flush0")
    lines[at] = lines[at].replace(" 1 64 0 ", " 1 63 0 ", 1)
    doctored = tmp_path / "doctored.txt"
    doctored.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(doctored)], capture_output=True, text=True)
    assert out.returncode == 1 and "pass gate_seq = 64, want 63" in out.stdout and "overlap_persist_w32" in out.stdout, out.stdout + out.stderr


def test_generated_assembly_passes_the_exec_mask_lint(built):
    """The build's guard against the live-range-split miscompile: no run of register copies directly
    in front of an exec-widening s_or_b64 in any kernel."""
    import subprocess
    csrc = os.path.join(ROOT, "2d-ekf-slam_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "lint"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 suspicious site(s)" in r.stdout


def test_register_half_of_the_long_window_is_what_the_lint_guards(built):
    """k_solo<true> keeps 16 slots of a long window in accumulation registers a128..a255 through inline asm the register allocator
    does not see (csrc/solo_agpr.h).  The header is generated (scripts/r04_gen_solo_agpr.py --check), and the assembly lint reports the
    highest accumulation register the compiler itself uses in k_solo: it must stay below a128."""
    import re
    import subprocess
    import sys
    for gen in ("r04_gen_solo_agpr.py", "r04_gen_solo_pass.py"):  # (the window's first half; the tile of the workgroup's own dense pass)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", gen), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "2d-ekf-slam_amd", "csrc"), "lint"], capture_output=True, text=True)
    m = re.search(r"highest accumulation register the compiler itself uses: a(-?\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout + r.stderr
    assert int(m.group(1)) < 128
    # the lint does flag a compiler-generated use: feed it a doctored listing
    asm = os.path.join(ROOT, "2d-ekf-slam_amd", "lib", "asm", "ekf_kernels.s")
    text = open(asm).read()
    at = text.index("_Z6k_soloILb1ELb0EE")  # k_solo<true, false>: the long window, not streaming
    at = text.index("\n", text.index("s_waitcnt", at)) + 1
    doctored = os.path.join(ROOT, "2d-ekf-slam_amd", "lib", "asm", "doctored.s")
    open(doctored, "w").write(text[:at] + "\tv_accvgpr_write_b32 a130, v1\n" + text[at:])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_exec_split.py"), doctored], capture_output=True, text=True)
        assert r.returncode == 1 and "reserved for solo_agpr.h" in r.stdout, r.stdout
    finally:
        os.remove(doctored)


def test_lint_checks_the_hand_written_accumulation_register_code(built, tmp_path):
    """What the register allocator cannot see in k_solo (solo_agpr.h, solo_pass_agpr.h): the kernel descriptors of both instantiations must
    grant a128..a255 (512 registers, accumulation half from 256), and no `global_store ... a[` may come closer than 18 wait states behind a
    v_mfma (pt_settle).  The lint reports both; doctored listings -- a shortened settle, a smaller register grant -- must fail it."""
    import re
    import subprocess
    import sys
    asm = os.path.join(ROOT, "2d-ekf-slam_amd", "lib", "asm", "ekf_kernels.s")
    lint = [sys.executable, os.path.join(ROOT, "scripts", "check_exec_split.py")]
    r = subprocess.run(lint + [asm], capture_output=True, text=True)
    m = re.search(r"k_solo: (\d+) stores from accumulation registers, the closest (\d+) wait states behind an MFMA", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= 32 and int(m.group(2)) >= 18, r.stdout
    text = open(asm).read()
    for name, doctored in (("settle", text.replace("s_nop 7", "s_nop 0")), ("grant", text.replace(".amdhsa_next_free_vgpr 512", ".amdhsa_next_free_vgpr 300"))):
        f = tmp_path / (name + ".s")
        f.write_text(doctored)
        r = subprocess.run(lint + [str(f)], capture_output=True, text=True)
        assert r.returncode == 1 and "accumulation-register checks" in r.stdout, (name, r.stdout[-600:])


def test_capacity_growth_is_clamped_at_the_library_limit(built, tmp_path):
    """The KalmanFilter shims double the capacity when a chunk could overflow it (the reference's state grows without bound,
    Update.cpp:158-177); ekf_reserve refuses more than EKF_MAX_CAPACITY, so doubling must stop THERE instead of failing once the
    capacity passes half of it (8192 -> 16384 used to throw although 8193 landmarks fit).  Same rule in the Python mirror and in the
    C++ header (compiled here against the stand-ins: a static function, no GPU)."""
    import re
    import subprocess
    pkg = built
    hdr = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    limit = int(re.search(r"#define EKF_MAX_CAPACITY (\d+)", hdr).group(1))
    g = pkg.ekfslam.grown_capacity
    lib_dir = os.path.dirname(pkg.ekfslam.LIB_PATH)
    assert pkg.ekfslam.MAX_CAPACITY == limit
    cases = [(4, 5), (4, 20), (4096, 4097), (8000, 8001), (8001, 8002), (8192, 8193), (12000, limit), (limit - 1, limit), (limit, limit + 1), (9000, limit + 5)]
    want = []
    for cap, need in cases:
        w = g(cap, need)
        assert w >= need  # never less than what is needed ...
        assert w == max(2 * cap, need) or (w == limit and need <= limit)  # ... doubling, or the limit when doubling would pass it
        if need <= limit:
            assert w <= limit  # only a map that really needs more than the limit is refused (by ekf_reserve)
        want.append(w)
    src = tmp_path / "grow.cpp"
    src.write_text('#include "%s"\n#include <cstdio>\nint main() { %s return 0; }\n' % (
        os.path.join(ROOT, "compat", "kalmanfilter.h"),
        " ".join('std::printf("%%d\\n", KalmanFilter::grown_capacity(%d, %d));' % c for c in cases)))
    exe = tmp_path / "grow"
    out = subprocess.run(["g++", "-std=c++17", "-o", str(exe), str(src), "-L" + lib_dir, "-lekfslam_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
