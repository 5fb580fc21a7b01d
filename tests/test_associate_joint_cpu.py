"""CPU tests of ekf_associate_joint: the declarations, the host-side planning and the shared search core as stand-alone programs, the
joint gates, and the reference of tests/assoc_ref.py on the inputs the GPU tests use (off their edges; greedy matching wrong and the
search right on the ambiguous scans; the pruned recursion equal to an unpruned enumeration on small inputs; the double reference
against its extended-precision twin)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import gate_ref as gr  # noqa: E402
import match_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ekf_associate_joint", "ekf_batch_associate_joint", "ekf_joint_gates")


@pytest.fixture(scope="module")
def built(pkg):
    import __graft_entry__ as ge
    ge.build()
    return pkg


def test_header_declares_and_binding_lists_the_calls(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ekfslam_c.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in built.ekfslam.ABI_SYMBOLS
        assert getattr(built.ekfslam.load(), name).argtypes
    assert "#define EKF_ASSOC_MAX_BRANCH 16" in hdr and "#define EKF_ASSOC_MAX_NODES (1 << 20)" in hdr
    assert (built.ekfslam.ASSOC_MAX_BRANCH, built.ekfslam.ASSOC_MAX_NODES) == (16, 1 << 20)


@pytest.mark.parametrize("prog,ok", [("assoc_plan_check", "assoc plan ok"), ("assoc_search_check", "assoc search ok")])
def test_plan_and_search_core_programs(tmp_path, prog, ok):
    exe = str(tmp_path / prog)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", prog + ".cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr


def test_joint_gates(built):
    g = built.joint_gates(0.99)
    exact = -2.0 * np.log(0.01)
    # 1 - 0.99 differs from 0.01 by 9e-16 relative: 1.8e-15 in the quantile, one ulp of it; the bisection ends on neighbouring doubles
    assert abs(g[0] - exact) <= 4 * np.spacing(exact)
    assert round(float(g[1]), 4) == 13.2767
    for q in range(1, 33):
        assert abs(ar.chi2_even_cdf(g[q - 1], q) - 0.99) < 1e-12
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            built.joint_gates(bad)
    assert built.ekfslam.load().ekf_joint_gates(1.5, g.ctypes.data_as(built.ekfslam._dp)) == built.ekfslam.ERR_BAD_ARG


@pytest.fixture(scope="module")
def searched(built):
    jg = built.joint_gates(0.99)
    return jg, {name: (x, P, z, R, valid, ids, kw, ar.search(x, P, z, R, jg, valid=valid, **kw)) for name, _, x, P, z, R, valid, ids, kw in ar.inputs(built)}


def test_every_input_is_off_its_edges(built, searched):
    for name, (x, P, z, R, valid, _, _, r) in searched[1].items():
        m = ar.margins(r)
        print("%s: %d nodes, %d paired, margin %.3g" % (name, r.nodes, r.n_paired, m))
        assert m > gr.EDGE, (name, m)
        gr.assert_off_the_edges(gr.table_of(x, P, z, R, valid, gr.COND_LIMIT), (ar.GATE,), gr.COND_LIMIT, name)


def test_greedy_is_wrong_and_the_search_right_on_the_ambiguous_scans(built, searched):
    want = {"ambiguous N=100": (4, 62), "ambiguous N=200": (6, 113)}
    for name, (wrong, nodes) in want.items():
        x, P, z, R, valid, ids, _, r = searched[1][name]
        greedy = built.candidate_matching(gr.find(gr.table_of(x, P, z, R, None, gr.COND_LIMIT), ar.GATE, gr.COND_LIMIT)[0], len(z))
        assert int((greedy != ids).sum()) == wrong and r.ids.tolist() == ids.tolist() and (r.nodes, r.complete) == (nodes, 1)
        cut = searched[1]["%s, budget %d" % (name, ar.BUDGET)][7]
        assert cut.complete == 0 and cut.nodes == ar.BUDGET and cut.n_paired == len(z) and cut.ids.tolist() != ids.tolist()
    for N, _ in mr.SIZES:
        r = searched[1]["planted N=%d" % N][7]
        assert r.nodes == 24 and r.ids.tolist() == searched[1]["planted N=%d" % N][5].tolist()
    assert searched[1]["ambiguous N=100, max_branch 1"][7].n_dropped > 0


def test_pruned_search_is_the_unpruned_optimum_on_small_inputs(built, searched):
    """Every feasible hypothesis of the first 6 measurements of the ambiguous scans, enumerated without pruning."""
    jg = searched[0]
    for name in ("ambiguous N=100", "ambiguous N=200"):
        x, P, z, R = searched[1][name][:4]
        z, R = z[:6], R[:6]
        r = ar.search(x, P, z, R, jg)
        cands = gr.find(gr.table(x, P, z, R), ar.GATE)[0]
        lists = [[int(c["landmark"]) for c in cands if c["meas"] == k][:8] for k in range(6)]
        best = (0, 0.0, [-1] * 6)

        def rec(ids, i, cnt, D2):
            nonlocal best
            if i == 6:
                if cnt > best[0] or (cnt == best[0] and D2 < best[1]):
                    best = (cnt, D2, list(ids))
                return
            for l in lists[i]:
                if l in ids:
                    continue
                ids[i] = l
                d = mr.joint_compat(x, P, z, R, np.array(ids))[i]
                if d <= jg[cnt]:
                    rec(ids, i + 1, cnt + 1, d)
                ids[i] = -1
            rec(ids, i + 1, cnt, D2)
        rec([-1] * 6, 0, 0, 0.0)
        assert (r.n_paired, r.d2, r.ids.tolist()) == best, (name, r, best)


def test_double_reference_against_its_extended_twin(built, searched):
    """MEASURES the relative difference of the winner's D2 between double and np.longdouble scoring; the GPU tests ask match_ref.D2_REL
    (5e-12), which must be at least 20 times the worst figure here."""
    jg, worst = searched[0], 0.0
    for name in ("ambiguous N=100", "ambiguous N=200", "planted N=100", "32 measurements"):
        x, P, z, R, valid, _, kw, r = searched[1][name]
        e = ar.search(x, P, z, R, jg, valid=valid, dtype=np.longdouble, **kw)
        assert e.ids.tolist() == r.ids.tolist() and e.nodes == r.nodes
        rel = abs(float(e.d2) - r.d2) / r.d2
        print("%s: D2 relative %.3e" % (name, rel))
        worst = max(worst, rel)
    assert 20.0 * worst <= mr.D2_REL, worst


class _NoLibrary:
    """Stands where the C library would: the Python layer must refuse before it gets here."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_python_layer_validates_its_arguments(pkg):
    f = pkg.FilterBatch.__new__(pkg.FilterBatch)
    f.L, f.h, f.batch = _NoLibrary(), None, 2
    z, R = np.zeros((3, 2)), np.tile(np.eye(2), (3, 1, 1))
    jg = np.linspace(9.0, 90.0, 32)
    short, neg, nan = jg[:31], jg.copy(), jg.copy()
    neg[4], nan[31] = -1.0, np.nan
    for kw in (dict(gate=-1.0), dict(gate=float("nan")), dict(max_branch=0), dict(max_branch=17), dict(max_nodes=0), dict(max_nodes=(1 << 20) + 1),
               dict(joint_gate=short), dict(joint_gate=neg), dict(joint_gate=nan), dict(valid=[1, 1, 1])):
        with pytest.raises(ValueError):
            f.associate_joint(z, R, **kw)
    with pytest.raises(ValueError):
        f.associate_joint(z, R[:2])                          # fewer R than z
    with pytest.raises(ValueError):
        f.associate_joint(np.zeros((3, 3)), R)               # not [n_z][2]
    with pytest.raises(ValueError):
        f.associate_joint(z[None], R[None])                  # a batch axis with an index
    with pytest.raises(ValueError):
        f.associate_joint(z, R, index=None)                  # no batch axis without one
    zn = z.copy()
    zn[1, 0] = np.nan
    with pytest.raises(ValueError):
        f.associate_joint(zn, R)                             # a non-finite z
    z33, R33 = np.zeros((33, 2)), np.tile(np.eye(2), (33, 1, 1))
    with pytest.raises(ValueError):
        f.associate_joint(z33, R33)                          # 33 valid measurements
    mask = np.ones((2, 33), dtype=np.uint8)
    mask[0, 5] = 0
    with pytest.raises(ValueError):
        f.associate_joint(np.stack([z33, z33]), np.stack([R33, R33]), index=None, valid=mask)   # filter 1 still has 33
    mask[1, 7] = 0
    with pytest.raises(AssertionError, match="the library was called"):   # 32 valid in both: the checks pass
        f.associate_joint(np.stack([z33, z33]), np.stack([R33, R33]), index=None, valid=mask)
