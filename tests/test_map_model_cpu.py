"""The sequence generator and the host model of tests/map_model.py, without a GPU: what tests/test_map_sequences.py relies on when
it replays every committed seed without skipping a seed or a step.  Determinism, coverage of the operations and of the tile-edge
branches, decision margins (no measurement within REL_TOL of a gate, so the library and the model, which agree to about 1e-12, cannot
decide differently), and the error of the float64 references themselves against the same expressions in np.longdouble.
For the *_maps profiles also: what they must cover of the duplicate search, the fusion and the extraction; that every `dups` op meets
the precondition under which its LIST may be compared (margins to the gate and to max_dist, no near-degenerate pair) and every `fuse`
op's list is one the library accepts, with every round's S clearly positive definite; fuse_ref.fuse against its np.longdouble
restatement.  The four older profiles generate what they generated before the *_maps profiles were appended (compared once against the
previous tests/map_model.py, value for value), and all seven what they generated before the *_match profiles were (likewise).
For the *_match profiles: what they must cover of the matched updates; that every `match` and `compat` op meets the generator's
precondition (every round's S clearly definite, so every entry is applied); that the model takes its rounds from the op's window;
match_ref against its np.longdouble restatement on every state such an op meets, d2 within 1/20 of map_model.MATCH_D2_REL."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref as fu  # noqa: E402
import join_ref as jr  # noqa: E402
import map_model as mm  # noqa: E402
import match_ref as mr  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import REL_TOL, assert_state_close  # noqa: E402

ALL = [(p, s) for p in mm.PROFILES for s in mm.SEEDS[p]]
OLD_PROFILES = mm.PROFILES[:4]
TRAFFIC = ("propagate", "update", "compass", "src_propagate", "src_update")


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
    assert mm.PROFILES[:4] == ("solo", "chain", "chain_wgs", "batch") and mm.MAP_PROFILES == ("solo_maps", "chain_maps", "batch_maps")
    assert mm.MATCH_PROFILES == ("solo_match", "chain_match", "batch_match") == mm.PROFILES[7:]
    assert [len(mm.SEEDS[p]) for p in mm.PROFILES] == [8, 8, 8, 6, 6, 6, 6, 6, 6, 6]
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
        maps, base = profile in mm.MAP_PROFILES + mm.MATCH_PROFILES, profile.replace("_maps", "").replace("_match", "")
        if base == "solo":
            assert 40 <= c["cap"] <= 256 and c["window"] in mm.WINDOWS and c["B"] == 1 and c["wgs"] is None
        elif base == "chain":
            assert 257 <= c["cap"] <= 700 and c["B"] == 1 and c["wgs"] is None
        elif base == "chain_wgs":
            assert c["cap"] <= 120 and 2 <= c["wgs"] <= 4 and c["B"] == 1
        else:
            assert 3 <= c["B"] <= 5
            loaded = {a["index"]: (a["x"].size - 3) // 2 for k, a in ops if k == "load"}
            assert len(loaded) == c["B"] - 1 and len(set(loaded.values())) == len(loaded)  # one starts empty, each its own count
        if maps:  # (a fuse may have propagations of its own in front of it)
            assert sum(1 for k, _ in ops if k == "propagate") >= mm.N_STEPS
            assert all(a["window"] == c["window"] for k, a in ops if k in ("fuse", "match"))
            assert profile in mm.MATCH_PROFILES or not any(k in ("match", "compat") for k, _ in ops)
            assert all(a["scratch_cap"] in mm.SCRATCH_CAPS for k, a in ops if k == "extract" and a["mode"] != "fork")
            behind = [ops[i - 1] for i, (k, _) in enumerate(ops) if k == "twin_begin"]
            assert all(k != "extract" or a["mode"] != "probe" for k, a in behind)
            assert any(k in ("fuse", "extract") for k, _ in behind), seed  # one twin at least goes on behind a fuse or an extraction
        else:
            assert sum(1 for k, _ in ops if k == "propagate") == mm.N_STEPS
            assert not any(k in ("dups", "fuse", "extract", "match", "compat") for k, _ in ops)
        assert sum(1 for k, _ in ops if k == "twin_begin") == sum(1 for k, _ in ops if k == "twin_end") == 2
        assert all(a["cap"] in mm.SRC_CAPS for k, a in ops if k == "src_create")


@pytest.mark.parametrize("profile", OLD_PROFILES)
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


@pytest.mark.parametrize("profile", mm.MAP_PROFILES)
def test_coverage_of_the_map_profiles(sequences, profile):
    count = dict.fromkeys(mm.MAP_KINDS + ("twin", "open", "single_index", "multi_round", "nine_in_window_8", "fuse_open", "extract_open", "fuse_tile_drop",
                                          "fuse_empty", "dups_split", "dups_max_dist", "dups_matched", "ids_empty", "ids_none", "extract_rewrite", "across_256"), 0)
    scratch, modes = set(), set()
    for seed in mm.SEEDS[profile]:
        last, open_here = None, 0
        for (kind, a), run, before, cap, res in replay(sequences[profile, seed]):
            B = len(before)
            which = list(range(B)) if a.get("index") is None else [a["index"]]
            changes = kind in ("remove", "transform", "anchor", "join", "fuse") or kind == "extract" and a["mode"] != "probe"
            behind_open = changes and not a["settle"] and last in TRAFFIC
            open_here += behind_open
            last = kind
            if kind in count and not (kind == "join" and a["expect"] != "ok"):
                count[kind] += 1
            count["twin"] += kind == "twin_begin"
            count["across_256"] += kind == "reserve" and cap <= 256 < run.cap
            if kind in ("dups", "fuse", "extract") and B > 1 and a["index"] is not None:
                count["single_index"] += 1
            if kind == "dups":
                count["dups_split"] += any(v > 0 for v in a["split"].values())
                count["dups_max_dist"] += a["max_dist"] is not None
                count["dups_matched"] += a["matched"] is not None
            if kind == "fuse":
                longest = max(len(p) for p in a["pairs"].values())
                count["fuse_empty"] += longest == 0
                count["multi_round"] += longest > a["window"]
                count["nine_in_window_8"] += a["window"] == 8 and longest >= 9
                count["fuse_open"] += behind_open and longest > 0
                count["fuse_tile_drop"] += any(mm.lm_tiles(res[i][0]) < mm.lm_tiles(before[b]) for i, b in enumerate(which))
            if kind == "extract":
                count["ids_none"] += any(v is None for v in a["ids"].values())
                count["ids_empty"] += any(v is not None and len(v) == 0 for v in a["ids"].values())
                count["extract_rewrite"] += a["mode"] != "probe"
                count["extract_open"] += behind_open
                modes.add(a["mode"])
                if a["mode"] != "fork":
                    scratch.add(a["scratch_cap"] > 256)
                    assert mm.lm_tiles(a["scratch_cap"]) != mm.lm_tiles(cap)  # a scratch of another tile count
        count["open"] += open_here
        assert open_here >= 1, seed
    print(profile, count, "scratch above 256", scratch, "modes", modes)
    for k in mm.MAP_KINDS:
        assert count[k] >= 5, (k, count[k])
    assert count["twin"] == 2 * len(mm.SEEDS[profile]) and count["open"] >= 5
    for k in ("multi_round", "nine_in_window_8", "fuse_open", "extract_open", "fuse_tile_drop", "fuse_empty", "dups_split", "dups_max_dist", "dups_matched", "ids_empty",
              "ids_none", "extract_rewrite"):
        assert count[k] >= 1, (k, count)
    assert scratch == {False, True}  # scratch capacities on both sides of 256
    if profile == "solo_maps":
        assert count["across_256"] >= 1 and modes == {"probe", "self"}
    if profile == "batch_maps":
        assert count["single_index"] >= 5 and modes == {"probe", "fork", "batch"}


@pytest.mark.parametrize("profile", mm.MATCH_PROFILES)
def test_coverage_of_the_match_profiles(sequences, profile):
    """Every profile: a match of more rounds than one, a match behind an open window, a landmark measured twice in one list, a skipped
    entry among measured ones, a compat; every seed a match and a compat.  chain_match: a measured landmark >= 256 in three seeds
    at least (k_match_gather's second block).  batch_match: the batch form more than once, with one filter's list all -1, at least once
    settled, and single-index calls."""
    count = dict.fromkeys(("match", "compat", "multi_round", "open", "repeat", "skip", "longer_than_64", "all_skip", "all_skip_settled", "batch_form", "single_index", "settled", "twin_behind"), 0)
    seeds_past_256 = 0
    for seed in mm.SEEDS[profile]:
        last, here, past = None, dict(match=0, compat=0), False
        for (kind, a), run, before, cap, res in replay(sequences[profile, seed]):
            if kind in ("match", "compat"):
                here[kind] += 1
                count[kind] += 1
                B = len(before)
                lists = list(a["ids"].values())
                assert len(set(len(v) for v in lists)) == 1 and len(lists) == (B if a["index"] is None else 1)
                assert all(v[v >= 0].max(initial=-1) < before[b] for b, v in a["ids"].items())
                count["single_index"] += B > 1 and a["index"] is not None
            if kind == "compat":
                for b, v in a["ids"].items():
                    w = a["swapped"][b]
                    assert int((v >= 0).sum()) <= 32 and sorted(v.tolist()) == sorted(w.tolist()) and np.array_equal(v >= 0, w >= 0)
                    assert int((v != w).sum()) in (0, 2) and (int((v != w).sum()) == 2 or len(set(v[v >= 0].tolist())) <= 1)
            if kind == "match":
                kept = [v[v >= 0] for v in a["ids"].values()]
                count["multi_round"] += max(len(k) for k in kept) > a["window"]
                count["longer_than_64"] += max(len(k) for k in kept) > 64
                count["open"] += not a["settle"] and last in TRAFFIC
                count["settled"] += bool(a["settle"])
                count["repeat"] += any(len(set(k.tolist())) < len(k) for k in kept)
                count["skip"] += any(0 < len(k) < len(v) for k, v in zip(kept, a["ids"].values()))
                count["all_skip"] += a["index"] is None and len(kept) > 1 and any(len(k) == 0 for k in kept)
                # (only a settled call has the export in front of it that the replay compares the all -1 filter with, bit for bit)
                count["all_skip_settled"] += bool(a["settle"]) and a["index"] is None and len(kept) > 1 and any(len(k) == 0 for k in kept)
                count["batch_form"] += a["index"] is None and len(kept) > 1
                past = past or any((k >= 256).any() for k in kept)
                assert [r[:2] for r in res] == [(before[b], len(k)) for b, k in zip(a["ids"], kept)]  # every entry applied
            if kind == "twin_begin":
                count["twin_behind"] += last == "match"
            last = kind
        assert here["match"] >= 1 and here["compat"] >= 1, (seed, here)
        seeds_past_256 += past
    print(profile, count, "seeds with a measured landmark >= 256:", seeds_past_256)
    for k in ("multi_round", "open", "repeat", "skip", "compat", "settled"):
        assert count[k] >= 1, (k, count)
    if profile == "chain_match":
        assert seeds_past_256 >= 3
    if profile == "batch_match":
        assert count["all_skip"] >= 1 and count["all_skip_settled"] >= 1 and count["batch_form"] >= 2 and count["single_index"] >= 1


@pytest.mark.parametrize("profile,seed", [ps for ps in ALL if ps[0] in mm.MATCH_PROFILES])
def test_match_preconditions(sequences, profile, seed):
    """Every `match` op: every round's S clearly positive definite on the model's state (smallest eigenvalue above FUSE_MIN_EIG times
    the largest), so every entry is applied and the library cannot decide otherwise.  Every `compat` op: the same for the one round
    of either hypothesis, no NaN in either answer, and the exchanged hypothesis is the larger distance in the end."""
    n = 0
    run = mm.ModelRunner()
    for op in sequences[profile, seed]:
        kind, a = op
        which = list(range(len(run.models))) if a.get("index") is None else [a["index"]]
        if kind in ("match", "compat"):
            for b in which:
                m = run.models[b]
                for ids in ([a["ids"][b]] if kind == "match" else [a["ids"][b], a["swapped"][b]]):
                    assert mm.match_rounds_definite(m.x, m.P, a["z"][b], a["R"][b], ids, a["window"] if kind == "match" else None), (kind, b)
            n += 1
        res = run.step(op)
        if kind == "compat":
            for (true, swapped), b in zip(res, which):
                kept = a["ids"][b] >= 0
                assert not np.isnan(true[kept]).any() and not np.isnan(swapped[kept]).any() and np.isnan(true[~kept]).all()
                if not np.array_equal(a["ids"][b], a["swapped"][b]):
                    assert np.nanmax(swapped) > np.nanmax(true), (b, np.nanmax(swapped), np.nanmax(true))
    assert n >= 2
    print("%s seed %d: %d match and compat ops" % (profile, seed, n))


def test_model_matches_in_rounds_of_the_window():
    """MapModel.update_matched takes the list in rounds of the op's window, every round linearised at its entry state.  As with
    fusion, a state comparison within the sequences' tolerances may not tell one round size from the next (the difference is the
    relinearisation, second order in the correction); d2 can -- a running distance starts again with every round -- and so can the
    number of applied entries where a round holds an exact copy.  The replay asserts the handle's window against the op's."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    x, P = pkg.scenarios.injected_state(12, seed=3, extent=8.0)
    ids = [0, 5, 7, 9, 3, 3, 1]
    z, R = mr.scan_of(pkg, x, ids, 11)
    by_window = {w: mm.MapModel(x, P).update_matched(z, R, ids, w) for w in (1, 2, 3, 4, 8)}
    for w, (n, applied, d2) in by_window.items():
        assert (n, applied) == (12, 7)
        falls = [k for k in range(1, 7) if d2[k] < d2[k - 1]]  # the running distance falls where a round begins, nowhere else
        assert all(k % w == 0 for k in falls), (w, falls)
    assert not np.array_equal(by_window[3][2], by_window[4][2])
    R[4:6] = 0.0
    z[5] = z[4]  # landmark 3 twice, exactly: the round that holds both is refused (rounds of 5 would part them: not asked)
    assert [mm.MapModel(x, P).update_matched(z, R, ids, w)[1] for w in (2, 3, 4, 6, 8)] == [4, 3, 4, 0, 0]
    run = mm.ModelRunner()
    run.step(("create", dict(B=1, cap=16, window=3, wgs=None)))
    run.step(("load", dict(index=0, x=x, P=P)))
    got = run.step(("match", dict(index=0, z={0: z}, R={0: R}, ids={0: np.array(ids)}, window=3, settle=True)))
    assert got[0][:2] == (12, 3) and np.isnan(got[0][2][3:]).all()


@pytest.mark.parametrize("profile,seed", [ps for ps in ALL if ps[0] in mm.MAP_PROFILES + mm.MATCH_PROFILES])
def test_dups_and_fuse_preconditions(sequences, profile, seed):
    """Every `dups` op: on the model's state no pair within DUP_MARGIN of the gate or of max_dist and no near-degenerate pair, which
    is what entitles the replay to compare the library's LIST with the model's.  Every `fuse` op: a list the library accepts (i < j < N,
    no landmark twice), every pair fused by the reference, every round's S clearly positive definite."""
    n_dups = n_fuse = 0
    run = mm.ModelRunner()
    for op in sequences[profile, seed]:
        kind, a = op
        which = list(range(len(run.models))) if a.get("index") is None else [a["index"]]
        if kind == "dups":
            assert a["gate"] in mm.DUP_GATES
            for b in which:
                m = run.models[b]
                assert 0 <= a["split"][b] <= m.n_landmarks
                assert mm.dups_precondition(m.x, m.P, a["gate"], a["max_dist"], a["split"][b]), (a["gate"], b)
                assert all(not mm.dups_precondition(m.x, m.P, g, a["max_dist"], a["split"][b]) for g in mm.DUP_GATES[:mm.DUP_GATES.index(a["gate"])]) or len(which) > 1
            n_dups += 1
        if kind == "fuse":
            for b in which:
                m = run.models[b]
                fu.check_pairs(a["pairs"][b], m.n_landmarks)
                assert mm.fuse_rounds_definite(m.x, m.P, a["pairs"][b], a["slack"], a["window"])
            assert a["slack"] in (0.0, 1e-4)
            n_fuse += 1
        res = run.step(op)
        if kind == "fuse":
            assert [r[1] for r in res] == [len(a["pairs"][b]) for b in which]
    print("%s seed %d: %d dups, %d fuse ops" % (profile, seed, n_dups, n_fuse))


def test_model_fuses_in_rounds_of_the_window():
    """MapModel.fuse takes the pairs in rounds of the op's window, as the handle does.  Conditioning round after round equals
    conditioning at once up to rounding (about 1e-15 on the sequences' states), so no state comparison can tell one round size from
    another; where a round meets an exact copy (S singular with slack 0) the number of fused pairs can."""
    rng = np.random.default_rng(5)
    n = 3 + 2 * 12
    A = rng.normal(size=(n, n))
    x, P = fu.with_exact_copy(rng.normal(size=n) * 5.0, A @ A.T + n * np.eye(n), 3)  # landmark 12 is landmark 3 again
    ij = [(0, 6), (1, 7), (2, 8), (3, 12), (4, 9)]
    for window, want in ((3, (10, 3)), (2, (11, 2)), (1, (10, 3)), (4, (13, 0)), (8, (13, 0))):
        assert mm.MapModel(x, P).fuse(ij, 0.0, window) == want, window
    m = mm.MapModel(x, P)
    assert m.fuse(ij, 1e-4, 3) == (8, 5)
    run = mm.ModelRunner()
    run.step(("create", dict(B=1, cap=16, window=3, wgs=None)))
    run.step(("load", dict(index=0, x=x, P=P)))
    assert run.step(("fuse", dict(index=0, pairs={0: np.array(ij)}, slack=0.0, window=3, settle=True))) == [(10, 3)]


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
    worst = {"rigid": [0.0, 0.0, 0], "anchor": [0.0, 0.0, 0], "join": [0.0, 0.0, 0], "fuse": [0.0, 0.0, 0], "match": [0.0, 0.0, 0]}
    worst_d2 = 0.0
    ld = np.longdouble
    run = mm.ModelRunner()
    for op in sequences[profile, seed]:
        kind, a = op
        if kind == "compat":  # d2 of either hypothesis, double against extended: 1/20 of the bound the replay uses
            for b, (true, swapped) in zip(range(len(run.models)) if a["index"] is None else [a["index"]], run.step(op)):
                m = run.models[b]
                for got, ids in ((true, a["ids"][b]), (swapped, a["swapped"][b])):
                    worst_d2 = max(worst_d2, mr.assert_d2_close(got, mr.joint_compat(m.x, m.P, a["z"][b], a["R"][b], ids, dtype=ld), "compat", mm.MATCH_D2_REL / 20.0))
            continue
        if kind in ("transform", "anchor", "join", "fuse", "match") and a.get("expect", "ok") == "ok":
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
                elif kind == "fuse":
                    want[b] = fu.fuse_extended(x, P, a["pairs"][b], a["slack"], a["window"])[:2]
                elif kind == "match":
                    want[b] = mr.update_extended(x, P, a["z"][b], a["R"][b], a["ids"][b], a["window"])
                else:
                    want[b] = jr.join(x, P, run.src[s].x, run.src[s].P, dtype=ld)
            res = run.step(op)
            if kind == "match":
                for (_, applied, d2), b in zip(res, list(want)):
                    assert applied == want[b][2]
                    worst_d2 = max(worst_d2, mr.assert_d2_close(d2, want[b][3], "match", mm.MATCH_D2_REL / 20.0))
                    want[b] = want[b][:2]
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
    if profile in mm.MATCH_PROFILES:
        print("%s seed %d: d2 of the match and compat ops, float64 vs longdouble: %.3e relative" % (profile, seed, worst_d2))
    assert sum(w[2] for w in worst.values()) >= 1
