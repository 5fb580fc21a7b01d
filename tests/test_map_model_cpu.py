"""The sequence generator and the host model of tests/map_model.py, without a GPU: what tests/test_map_sequences.py relies on when
it replays every committed seed without skipping a seed or a step.  Determinism, coverage of the operations and of the tile-edge
branches, decision margins (no measurement within REL_TOL of a gate, so the library and the model, which agree to about 1e-12, cannot
decide differently), and the error of the float64 references themselves against the same expressions in np.longdouble."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_ref as jr  # noqa: E402
import map_model as mm  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import REL_TOL, assert_state_close  # noqa: E402

ALL = [(p, s) for p in mm.PROFILES for s in mm.SEEDS[p]]


@pytest.fixture(scope="module")
def sequences():
    return {ps: mm.make_sequence(ps[1], ps[0]) for ps in ALL}


def replay(ops):
    """The sequence on the model alone: yields (op, the runner after it, landmark counts and capacity before it, the op's result)."""
    run = mm.ModelRunner()
    for op in ops:
        before, cap = [m.n_landmarks for m in run.models], run.cap
        yield op, run, before, cap, run.step(op)


def test_seed_lists():
    assert [len(mm.SEEDS[p]) for p in mm.PROFILES] == [8, 8, 8, 6]
    assert all(len(set(s)) == len(s) for s in mm.SEEDS.values())


@pytest.mark.parametrize("profile", mm.PROFILES)
def test_sequences_are_deterministic(sequences, profile):
    for seed in mm.SEEDS[profile]:
        assert mm.ops_equal(sequences[profile, seed], mm.make_sequence(seed, profile)), seed
    assert not mm.ops_equal(sequences[profile, mm.SEEDS[profile][0]], sequences[profile, mm.SEEDS[profile][1]])


@pytest.mark.parametrize("profile", mm.PROFILES)
def test_profile_parameters(sequences, profile):
    for seed in mm.SEEDS[profile]:
        ops = sequences[profile, seed]
        c = ops[0][1]
        assert ops[0][0] == "create"
        if profile == "solo":
            assert 40 <= c["cap"] <= 256 and c["window"] in mm.WINDOWS and c["B"] == 1 and c["wgs"] is None
        elif profile == "chain":
            assert 257 <= c["cap"] <= 700 and c["B"] == 1 and c["wgs"] is None
        elif profile == "chain_wgs":
            assert c["cap"] <= 120 and 2 <= c["wgs"] <= 4 and c["B"] == 1
        else:
            assert 3 <= c["B"] <= 5
            loaded = {a["index"]: (a["x"].size - 3) // 2 for k, a in ops if k == "load"}
            assert len(loaded) == c["B"] - 1 and len(set(loaded.values())) == len(loaded)  # one starts empty, each its own count
        assert sum(1 for k, _ in ops if k == "propagate") == mm.N_STEPS
        assert sum(1 for k, _ in ops if k == "twin_begin") == sum(1 for k, _ in ops if k == "twin_end") == 2
        assert all(a["cap"] in mm.SRC_CAPS for k, a in ops if k == "src_create")


@pytest.mark.parametrize("profile", mm.PROFILES)
def test_coverage(sequences, profile):
    count = dict.fromkeys(mm.KINDS + ("join_refused", "twin", "theta_0", "across_256", "single_index", "open"), 0)
    aligned_joins = tile_drops = removed_all = 0
    families = set()
    for seed in mm.SEEDS[profile]:
        last, open_here = None, 0
        for (kind, a), run, before, cap, res in replay(sequences[profile, seed]):
            # a rewrite straight behind filter traffic without an export first: the window open, a streaming launch live
            if kind in ("remove", "transform", "anchor", "join") and not a["settle"] and last in ("propagate", "update", "compass", "src_propagate", "src_update"):
                open_here += 1
            last = kind
            if kind in count and not (kind == "join" and a["expect"] != "ok"):
                count[kind] += 1
            if kind == "join" and a["expect"] == "ok":
                dst = range(len(before)) if a["index"] is None else [a["index"]]
                aligned_joins += any(before[b] > 0 and before[b] % 32 == 0 and res[i] > before[b] for i, b in enumerate(dst))
                families.add(run.src_cap > 256)
            if kind == "join" and a["expect"] == "capacity":
                count["join_refused"] += 1
            if kind == "remove":
                which = range(len(before)) if a["index"] is None else [a["index"]]
                tile_drops += any(mm.lm_tiles(res[i]) < mm.lm_tiles(before[b]) for i, b in enumerate(which))
                removed_all += any(res[i] == 0 and before[b] > 0 for i, b in enumerate(which))
            if kind == "transform":
                count["theta_0"] += any(f[2] == 0.0 for f in a["frames"].values())
            if kind == "reserve":
                count["across_256"] += cap <= 256 < run.cap
            if kind == "twin_begin":
                count["twin"] += 1
            if kind in ("remove", "transform", "anchor", "join", "joint") and len(before) > 1 and a["index"] is not None:
                count["single_index"] += 1
        count["open"] += open_here
        assert open_here >= 1, seed
    print(profile, count, "aligned joins", aligned_joins, "tile drops", tile_drops, "removed all", removed_all)
    for k in mm.KINDS:
        assert count[k] >= 5, (k, count[k])
    assert aligned_joins >= 1 and tile_drops >= 1 and removed_all >= 1
    assert count["twin"] == 2 * len(mm.SEEDS[profile]) and count["open"] >= 5 and count["theta_0"] >= 1 and count["join_refused"] >= 1
    assert families == {False, True}  # source capacities on both sides of 256 (the other kernel family, except under EKF_CHAIN_WGS)
    if profile == "solo":
        assert count["across_256"] >= 1
    if profile == "batch":
        assert count["single_index"] >= 5


@pytest.mark.parametrize("profile,seed", ALL)
def test_decision_margins(sequences, profile, seed):
    """Every accepted or rejected measurement of the sequence is at least REL_TOL (relative) away from both gates."""
    run = None
    for _, run, _, _, _ in replay(sequences[profile, seed]):
        pass
    print("%s seed %d: smallest |mahal - gamma| / gamma %.3e" % (profile, seed, run.margin))
    assert run.margin >= REL_TOL


@pytest.mark.parametrize("profile,seed", ALL)
def test_reference_precision(sequences, profile, seed):
    """The float64 references against np.longdouble restatements of the dense Jacobian forms, on every state the sequence meets, held
    to the tolerance the GPU comparison uses: the reference's own error is far below it (the maxima are printed)."""
    worst = {"rigid": [0.0, 0.0, 0], "anchor": [0.0, 0.0, 0], "join": [0.0, 0.0, 0]}
    ld = np.longdouble
    run = mm.ModelRunner()
    for op in sequences[profile, seed]:
        kind, a = op
        if kind in ("transform", "anchor", "join") and a.get("expect", "ok") == "ok":
            M = run.models
            pairs = [(b, b) for b in range(len(M))] if a["index"] is None else [(a["index"], a.get("src_index", 0))]
            want = {}
            for b, s in pairs:
                x, P = M[b].x, M[b].P
                if kind == "transform":
                    f = a["frames"][b]
                    want[b] = rr.apply_dense(x, P, lambda v, dtype: rr.rigid_g(v, f, dtype), lambda v, dtype: rr.rigid_J(v, f, dtype), dtype=ld)
                elif kind == "anchor":
                    want[b] = rr.apply_dense(x, P, rr.anchor_g, rr.anchor_J, dtype=ld)
                else:
                    want[b] = jr.join(x, P, run.src[s].x, run.src[s].P, dtype=ld)
            run.step(op)
            for b, (xw, Pw) in want.items():
                assert xw.dtype == ld and Pw.dtype == ld
                e = assert_state_close(M[b].x, M[b].P, np.asarray(xw, dtype=np.float64), np.asarray((Pw + Pw.T) / 2, dtype=np.float64),
                                       what="%s, float64 vs longdouble" % kind)
                name = "rigid" if kind == "transform" else kind
                worst[name] = [max(worst[name][0], e[0]), max(worst[name][1], e[1]), worst[name][2] + 1]
        else:
            run.step(op)
    for k, (ex, eP, cases) in worst.items():
        print("%s seed %d %s: float64 vs longdouble over %d cases, max |dx| %.3e, max |dP| / max |P| %.3e" % (profile, seed, k, cases, ex, eP))
    assert sum(w[2] for w in worst.values()) >= 1
