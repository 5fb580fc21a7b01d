"""Random operation sequences that mix the map rewrites with live filter traffic: landmark removal, rigid transform, anchoring, map
joining (from a source handle of another capacity, so another tile layout and often the other kernel family), ekf_reserve (now and
then across capacity 256, where the kernel family changes under the state) and the read-only probes (ekf_joint_consistency,
ekf_get_landmark_covs, a full state read), between propagations, measurement chunks and compass updates.

tests/map_model.py generates every sequence from (seed, profile) and holds the host model (C oracle for the filter steps, the NumPy
references for the rewrites); this file replays the list on the library and on the model in lockstep.  No seed and no step is
skipped: tests/test_map_model_cpu.py checks on the CPU that no measurement of a committed seed lies within REL_TOL of a gate.
Tolerances are the project's own (helpers.assert_state_close, REL_TOL, ABS_P); the observed maxima are printed per sequence.

About half of the rewrites are made behind an open window (`settle` false: only the model says what must come out); the others
export the state first, which adds the bitwise contracts -- removal is np.delete, theta = 0 leaves P alone, a join leaves the
old x old block and the source alone, a single-index call leaves the other filters of the handle alone.  Twice per sequence a twin
handle is loaded with set_state(get_state()) behind a rewrite and replays the next five steps beside the handle: exports and
decisions must be bitwise equal, which is the only check that sees what a rewrite leaves behind the map (the zeros new landmarks
grow into).  It cannot see the places of a diagonal tile that are nobody's home (a landmark's own block, whose home is D, and the
blocks below the diagonal): no kernel and no export reads them, the dense pass only updates each from itself.

The *_maps profiles (solo_maps, chain_maps, batch_maps) add the three newer map operations to the same mix.  `dups`:
ekf_find_duplicates behind whatever the last call left (nothing read in front of it unless `settle`), held to the contract of
tests/test_find_duplicates.py against tests/dup_ref.py on the export (helpers.check_duplicates) and, list and counts, to the model's
own answer; twice the same bytes; the handle unchanged.  `fuse`: ekf_fuse_landmarks with the one-to-one matching of the duplicates
that a join of re-observed landmarks planted in the map the filter built -- the `dups` op in front of it asserts that the device's
own list gives that matching --, often behind an open window, in rounds of the handle's window, against tests/fuse_ref.py; every
check a rewrite gets.  `extract`: a scratch handle of another tile count, as a probe (ekf_extract_map and ekf_get_submap are NumPy
indexing of the export, bit for bit) or as a rewrite: the handle replaced by its own shuffled marginal through the scratch, every
filter of a batch by ekf_batch_extract_map, or one filter by a fork of a sibling.  At least one of the two twins of such a sequence
goes on behind a fuse or an extraction.  No more than three handles are open at any time (tests/test_extract_map.py says why).

The *_match profiles (solo_match, chain_match, batch_match) add the matched updates to that mix.  `match`: ekf_update_matched with
the true associations of a scan of the landmarks nearest the robot -- one to about 2.5 windows' worth of measurements, now and then
more than 64, landmarks repeated, -1 entries interleaved, in chain_match on maps past 256 landmarks --, about half of them behind an
open window, in rounds of the handle's window, against tests/match_ref.py on the model's state (and on the export where there is
one): (n, applied) exact, d2 within map_model.MATCH_D2_REL, every check a rewrite gets, a list that is all -1 leaves its filter
bit for bit.  `compat`: ekf_joint_compat for the true hypothesis and for one with two ids exchanged, twice the same bits, the
handle unchanged, counters and decision log unmoved.  The set_state twins may start right behind a `match`.

In the chain_wgs profile EKF_CHAIN_WGS is set for the whole test, which keeps the one-workgroup kernel out of every handle: sources
and twins run the chain kernel there too; "a source of the other kernel family" happens in the solo and chain profiles."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_model as mm  # noqa: E402
import match_ref as mr  # noqa: E402
from helpers import (ABS_P, REL_TOL, assert_bitwise, assert_bitwise_symmetric, assert_state_close, check_duplicates, check_joint,  # noqa: E402
                     ij, index_state, stream_starts, windows_closed)

pytestmark = pytest.mark.gpu

REWRITES = ("remove", "transform", "anchor", "join", "reserve", "fuse", "extract", "match")  # (an extract of mode "probe" is none)
TRAFFIC = ("propagate", "update", "compass", "src_propagate", "src_update")
WORST = {}  # profile -> the largest errors seen so far in this session (printed behind every sequence)


def real_decisions(dec, valid):
    """Per filter, the decisions of the measurements that were not masked out (they sit at the end of the filter's row)."""
    out = []
    for b, row in enumerate(dec):
        k = int(np.sum(valid[b]))
        out.append(row[len(row) - k:] if k else [])
    return out


def per_filter(d, B, width, fill):
    arr = np.full((B, width), fill)
    for b, v in d.items():
        arr[b, :len(v)] = v
    return arr


def extract(pkg, h, a, counts):
    """An `extract` op on handle h: (new landmark counts, what the scratch handle held, ekf_get_submap's answer for a probe).  The
    scratch lives inside the call."""
    mode, b, ids = a["mode"], a["index"], a["ids"]
    if mode == "fork":
        return [h.extract_map(h, ids[b], index=b, src_index=a["src_index"])], None, None
    s = pkg.FilterBatch(h.batch if mode == "batch" else 1, a["scratch_cap"], max_pending=16, log_capacity=4096)
    try:
        sub = None
        if mode == "batch":
            if all(v is None for v in ids.values()):
                n = s.batch_extract_map(h)
            else:  # (the batch form has one NULL for all: a filter copied whole lists every landmark)
                n = s.batch_extract_map(h, [np.arange(counts[c], dtype=np.int32) if ids[c] is None else ids[c] for c in range(h.batch)])
        else:
            n = [s.extract_map(h, ids[b], index=0, src_index=b)]
        held = [s.get_state(c) for c in range(s.batch)]
        assert [int(v) for v in n] == [(st[0].size - 3) // 2 for st in held] == [int(v) for v in s.num_landmarks()]
        assert not any(st[k] for st in s.stats() for k in ("n_new", "n_old", "n_ignore")) and not any(s.decisions(c) for c in range(s.batch))
        if mode == "probe":
            sub = h.get_submap(np.arange(counts[b], dtype=np.int32) if ids[b] is None else ids[b], index=b)
        elif mode == "batch":
            n = h.batch_extract_map(s)
        else:
            n = [h.extract_map(s)]
        return [int(v) for v in n], held, sub
    finally:
        s.close()


def apply(pkg, h, src, op, counts=None):
    """One operation on handle h (the handle under test or its twin); returns what the library answered."""
    kind, a = op
    B = h.batch
    if kind == "load":
        h.set_state(a["x"], a["P"], index=a["index"])
    elif kind == "propagate":
        h.propagate(a["v"], a["w"], a["dt"])
    elif kind == "compass":
        h.update_compass(a["z"], a["R"], valid=None if np.all(a["valid"]) else a["valid"])
    elif kind == "update":
        return real_decisions(h.update(a["z"], a["R"], valid=None if np.all(a["valid"]) else a["valid"]), a["valid"])
    elif kind == "remove":
        if a["index"] is None:
            return [int(n) for n in h.remove_landmarks(per_filter(a["keep"], B, max(len(k) for k in a["keep"].values()), True))]
        return [h.remove_landmarks(a["keep"][a["index"]], index=a["index"])]
    elif kind == "transform":
        if a["index"] is None:
            h.transform_frame(per_filter(a["frames"], B, 3, 0.0))
        else:
            h.transform_frame(a["frames"][a["index"]], index=a["index"])
    elif kind == "anchor":
        h.anchor_at_robot(index=a["index"])
    elif kind == "reserve":
        h.reserve(a["cap"])
    elif kind == "join":
        if a["expect"] == "capacity":
            rc = h.L.ekf_batch_join_map(h.h, src.h) if a["index"] is None else h.L.ekf_join_map(h.h, a["index"], src.h, a["src_index"])
            assert rc == pkg.ekfslam.ERR_CAPACITY, rc
            h.sync(), src.sync()  # EKF_OK: nothing sticky
            return None
        if a["index"] is None:
            h.batch_join_map(src)
            return [int(n) for n in h.num_landmarks()]
        return [h.join_map(src, index=a["index"], src_index=a["src_index"])]
    elif kind == "joint":
        if a["index"] is None:
            return h.joint_consistency(per_filter(a["x_true"], B, max(len(t) for t in a["x_true"].values()), 0.0)).copy()
        return h.joint_consistency(a["x_true"][a["index"]], a["index"]).copy()
    elif kind == "covs":
        return h.landmark_covs(a["index"])
    elif kind == "read":
        return h.get_state(a["index"])
    elif kind == "dups":
        if a["index"] is None:
            return h.find_duplicates(a["gate"], a["max_dist"], split=[a["split"][b] for b in range(B)], index=None)
        return [h.find_duplicates(a["gate"], a["max_dist"], split=a["split"][a["index"]], index=a["index"])]
    elif kind == "fuse":
        assert h.window == a["window"], (h.window, a["window"])  # the round size the model fuses with
        if a["index"] is None:
            n, fused = h.fuse_landmarks([a["pairs"][b] for b in range(B)], slack=a["slack"], index=None)
            return [(int(n[b]), int(fused[b])) for b in range(B)]
        return [h.fuse_landmarks(a["pairs"][a["index"]], slack=a["slack"], index=a["index"])]
    elif kind == "extract":
        return extract(pkg, h, a, counts)
    elif kind == "match":
        assert h.window == a["window"], (h.window, a["window"])  # the round size the model updates with
        if a["index"] is None:
            applied, d2 = h.update_matched(*(np.stack([a[k][b] for b in range(B)]) for k in ("z", "R", "ids")), index=None)
            return [(int(n), int(applied[b]), d2[b]) for b, n in enumerate(h.num_landmarks())]
        b = a["index"]
        return [h.update_matched(a["z"][b], a["R"][b], a["ids"][b], index=b)]
    elif kind == "compat":  # the true hypothesis, and the one with two ids exchanged
        if a["index"] is None:
            z, R = (np.stack([a[k][b] for b in range(B)]) for k in ("z", "R"))
            both = [h.joint_compat(z, R, np.stack([a[k][b] for b in range(B)]), index=None) for k in ("ids", "swapped")]
            return [(both[0][b], both[1][b]) for b in range(B)]
        b = a["index"]
        return [tuple(h.joint_compat(a["z"][b], a["R"][b], a[k][b], index=b) for k in ("ids", "swapped"))]
    else:
        raise ValueError(kind)
    return None


class Replay:
    def __init__(self, pkg, monkeypatch, ops):
        self.pkg, self.ops = pkg, ops
        c = ops[0][1]
        assert ops[0][0] == "create"
        if c["wgs"]:
            monkeypatch.setenv("EKF_CHAIN_WGS", str(c["wgs"]))
        else:
            monkeypatch.delenv("EKF_CHAIN_WGS", raising=False)
        self.B, self.window = c["B"], c["window"]
        self.f = pkg.FilterBatch(self.B, c["cap"], max_pending=self.window, log_capacity=4096)
        self.twin = self.src = None
        self.twin_decs = ([], [])
        self.run = mm.ModelRunner()
        self.run.step(ops[0])
        self.err = {"x": 0.0, "P": 0.0, "d2": 0.0, "joint": 0.0, "covs": 0.0, "match_d2": 0.0}
        self.n_twins = self.n_twins_new = self.n_bitwise = self.n_open = self.n_live = 0
        self.want_log, self.want_src_log = [[] for _ in range(self.B)], []
        self.last = None  # the kind of the last library call on the handle

    def close(self):
        for h in (self.f, self.twin, self.src):
            if h is not None:
                h.close()

    def export(self, h=None):
        h = h or self.f
        return [h.get_state(b) for b in range(h.batch)]

    def compare(self, b, what, state=None):
        """Filter b of the handle against its model: the whole state, symmetry, the count and the host mirror."""
        x, P = state or self.f.get_state(b)
        m = self.run.models[b]
        e = assert_state_close(x, P, m.x, m.P, what="%s, filter %d" % (what, b))
        self.err["x"], self.err["P"] = max(self.err["x"], e[0]), max(self.err["P"], e[1])
        assert_bitwise_symmetric(P)
        assert int(self.f.num_landmarks()[b]) == m.n_landmarks == (x.size - 3) // 2
        assert np.array_equal(self.f.poses()[b], x[:3]), what
        if self.B == 1:  # (ekf_get_robot_cov is a one-filter call)
            assert np.array_equal(self.f.robot_cov(), P[:3, :3]), what
        return x, P

    def match_d2(self, got, want, what):
        self.err["match_d2"] = max(self.err["match_d2"], mr.assert_d2_close(got, want, what, mm.MATCH_D2_REL))

    def logs(self, h):
        return h.stats(), [h.decisions(b) for b in range(h.batch)]

    def check_logs(self, h, want, what):
        """Counters and decision log of every filter against the model's record of its measurements."""
        st = h.stats()
        for b, w in enumerate(want):
            assert [(d[0], d[1]) for d in h.decisions(b)] == w, (what, b)
            E = self.pkg.ekfslam
            assert [st[b]["n_new"], st[b]["n_old"], st[b]["n_ignore"]] == [sum(1 for d in w if d[0] == k) for k in (E.NEW, E.OLD, E.IGNORE)], (what, b)

    # -- one operation on the handle, its twin and the model
    def step(self, i, op):
        kind, a = op
        pkg, f, B = self.pkg, self.f, self.B
        what = "op %d (%s)" % (i, kind)
        prev = self.last
        if kind in ("twin_begin", "twin_end"):
            self.last = kind  # (both export the state)
        if kind == "twin_begin":
            self.n_twins_new += prev in ("fuse", "extract")  # (the generator starts none behind a probe)
            states = self.export()
            self.twin = pkg.FilterBatch(B, f.capacity, max_pending=self.window, log_capacity=4096)
            for b in range(B):
                self.twin.set_state(*states[b], index=b)
            self.twin_decs = ([], [])
            return
        if kind == "twin_end":
            sa, sb = self.export(), self.export(self.twin)
            for b in range(B):
                assert_bitwise(sa[b], sb[b], "%s: handle vs set_state twin, filter %d" % (what, b))
            assert self.twin_decs[0] == self.twin_decs[1] and np.array_equal(f.poses(), self.twin.poses())
            self.twin.close()
            self.twin, self.n_twins = None, self.n_twins + 1
            return
        if kind == "src_create":
            self.src = pkg.FilterBatch(a["B"], a["cap"], max_pending=a["window"], log_capacity=4096)
            self.want_src_log = [[] for _ in range(a["B"])]
            self.run.step(op)
            return
        if kind in ("src_propagate", "src_update"):
            got = apply(pkg, self.src, None, (kind[4:], a))
            want = self.run.step(op)
            if kind == "src_update":
                assert [[(d[0], d[1]) for d in row] for row in got] == [[(d[0], d[1]) for d in row] for row in want], what
                for b, row in enumerate(want):
                    self.want_src_log[b] += [(d[0], d[1]) for d in row]
            self.last = kind
            return
        if kind == "src_close":
            self.src.close()
            self.src = None
            self.run.step(op)
            return

        which = list(range(B)) if a.get("index") is None else [a["index"]]
        rewrite = kind in REWRITES and not (kind == "extract" and a["mode"] == "probe")
        settle = bool(a.get("settle")) or kind == "joint" or (kind == "reserve" and i % 2 == 0)
        # a rewrite that is not `settle` meets the handle (and a join its source) as the last immediate call left it: the window open,
        # the streaming launch of a one-filter handle live -- nothing is read in front of it, reading the counters would stop the launch
        before = self.export() if settle else None
        if settle and kind == "fuse" and self.twin is not None and not any(len(p) for p in a["pairs"].values()):
            self.export(self.twin)  # (a fuse of no pair leaves an open window open: the twin's window ends where the handle's does)
        src_before = self.export(self.src) if (kind == "join" and settle) else None
        if (rewrite or kind == "compat") and settle:
            logs0 = self.logs(f)
            src_logs0 = self.logs(self.src) if kind == "join" else None
        if rewrite and not settle and self.last in TRAFFIC:
            self.n_open += 1
            self.n_live += stream_starts(f)[0] > 0  # (host counters only: this handle streams its immediate calls)
        if kind in ("covs", "fuse", "match", "compat"):
            closed0 = windows_closed(f)
        counts0 = [m.n_landmarks for m in self.run.models]

        got = apply(pkg, f, self.src, op, counts0)
        if self.twin is not None:
            got_twin = apply(pkg, self.twin, self.src, op, counts0)
            if kind == "fuse" and not any(len(p) for p in a["pairs"].values()):
                # ... and the handle is exported behind every rewrite, settled or not: so is the twin behind this no-op.  (This
                # makes the twin's export in front of a settled no-pair fuse, above, redundant: the call touches nothing, so it does
                # not matter on which side of it the window ends.  It stays, so that both handles are read at the same points.)
                self.export(self.twin)
            if kind == "update":
                self.twin_decs[0].extend(got), self.twin_decs[1].extend(got_twin)
        want = self.run.step(op)

        if kind == "update":
            assert [[(d[0], d[1]) for d in row] for row in got] == [[(d[0], d[1]) for d in row] for row in want], (what, got, want)
            for b, row in enumerate(want):
                self.want_log[b] += [(d[0], d[1]) for d in row]
        elif kind == "read":
            self.compare(a["index"], what, got)
        elif kind == "covs":
            assert windows_closed(f) == closed0, what  # no dense pass: the window stays open
            P = self.run.models[a["index"]].P
            assert got.shape == want.shape, what
            if want.size:
                d = np.abs(got - want)
                assert np.all(d <= REL_TOL * np.abs(want) + ABS_P * np.abs(P).max()), (what, d.max())
                self.err["covs"] = max(self.err["covs"], float(d.max() / np.abs(P).max()))
        elif kind == "joint":
            for k, b in enumerate(which):
                self.err["joint"] = max(self.err["joint"], check_joint(got[k], want[k], self.run.models[b].P, "%s, filter %d" % (what, b)))
            again = apply(pkg, f, self.src, op)
            assert again.tobytes() == got.tobytes(), what  # an unchanged state: the same bits
            for b in range(B):
                assert_bitwise(f.get_state(b), before[b], "%s: the call only reads, filter %d" % (what, b))
        elif kind == "dups":
            after = self.export()
            again = apply(pkg, f, self.src, op)
            assert [(r[0].tobytes(), r[1], r[2]) for r in again] == [(r[0].tobytes(), r[1], r[2]) for r in got], what  # an unchanged state: the same bits
            for k, b in enumerate(which):
                e = check_duplicates(got[k], *after[b], gate=a["gate"], max_dist=a["max_dist"], split=a["split"][b], what="%s, filter %d" % (what, b))
                self.err["d2"] = max(self.err["d2"], e)
                assert len(got[k][0]) == got[k][1] and (ij(got[k][0]), got[k][1], got[k][2]) == want[k], (what, b, got[k], want[k])
                if a["matched"] is not None:  # what the fuse behind this search is given: the device's own list gives it too
                    assert pkg.duplicate_matching(got[k][0], counts0[b])[["i", "j"]].tolist() == [tuple(p) for p in a["matched"][b].tolist()], (what, b)
            for b in range(B):
                self.compare(b, what, after[b])
                if settle:
                    assert_bitwise(after[b], before[b], "%s: the call only reads, filter %d" % (what, b))
        elif kind == "extract" and not rewrite:
            b, (_, held, sub) = a["index"], got
            after = self.export()
            ref = index_state(after[b], a["ids"][b])
            assert_bitwise(held[0], ref, "%s: ekf_extract_map into the scratch" % what)
            assert_bitwise(sub, ref, "%s: ekf_get_submap" % what)
            for c in range(B):
                self.compare(c, what, after[c])
                if settle:
                    assert_bitwise(after[c], before[c], "%s: the call only reads, filter %d" % (what, c))
        elif kind == "compat":
            # a probe: the window is folded (at most the open one), nothing else moves; twice the same bits
            assert windows_closed(f) - closed0 <= (0 if settle else 1), what
            after = self.export()
            again = apply(pkg, f, self.src, op)
            assert windows_closed(f) - closed0 <= (0 if settle else 1), what
            for k, b in enumerate(which):
                for h in (0, 1):
                    assert again[k][h].tobytes() == got[k][h].tobytes(), what  # an unchanged state: the same bits
                    self.match_d2(got[k][h], want[k][h], "%s, filter %d, hypothesis %d" % (what, b, h))
                    if settle:  # ... and against the reference on the export itself
                        self.match_d2(got[k][h], mr.joint_compat(*before[b], a["z"][b], a["R"][b], a[("ids", "swapped")[h]][b]), what)
            self.check_logs(f, self.want_log, what)  # counters and decision log do not move
            assert not settle or self.logs(f) == logs0, what
            for b in range(B):
                self.compare(b, what, after[b])
                if settle:
                    assert_bitwise(after[b], before[b], "%s: the call only reads, filter %d" % (what, b))
        self.last = kind
        if not rewrite:
            return

        held = None
        if kind == "match":
            # the rounds' passes are the call's own: at most the open window was closed, none on a settled handle
            assert windows_closed(f) - closed0 <= (0 if settle else 1), what
            for k, b in enumerate(which):
                assert got[k][:2] == want[k][:2], (what, b, got[k][:2], want[k][:2])  # (n, applied): exact
                self.match_d2(got[k][2], want[k][2], "%s, filter %d" % (what, b))
                if settle:  # ... and against the reference on the export itself, in rounds of the handle's window
                    ref = mr.update(*before[b], a["z"][b], a["R"][b], a["ids"][b], f.window)
                    assert ref[2] == got[k][1], what
                    self.match_d2(got[k][2], ref[3], "%s, filter %d, on the export" % (what, b))
            got, want = [g[:2] for g in got], [w[:2] for w in want]
        if kind == "extract":
            got, held, _ = got
        if kind == "fuse":  # the rounds' passes are the call's own: at most the open window was closed, none on a settled handle
            assert windows_closed(f) - closed0 <= (0 if settle or not any(len(p) for p in a["pairs"].values()) else 1), what
        self.check_logs(f, self.want_log, what)  # counters and decision log do not move
        if kind == "join":
            self.check_logs(self.src, self.want_src_log, what + ", source")
        if settle:
            assert self.logs(f) == logs0, what
        after = self.export()
        if kind == "join" and a["expect"] == "capacity":
            for b in range(B):
                assert_bitwise(after[b], before[b], "%s: destination after EKF_ERR_CAPACITY, filter %d" % (what, b))
            for b, s in enumerate(self.export(self.src)):
                assert_bitwise(s, src_before[b], "%s: source after EKF_ERR_CAPACITY, filter %d" % (what, b))
            assert self.logs(self.src) == src_logs0
            return
        if got is not None:
            assert got == want, (what, got, want)  # the new landmark counts
        for b in range(B):
            self.compare(b, what, after[b])
        if kind == "anchor":
            for b in which:
                assert not after[b][0][:3].any() and not after[b][1][:3, :].any() and not after[b][1][:, :3].any(), what
            assert not f.poses()[which].any()
        if kind == "join":
            assert not settle or self.logs(self.src) == src_logs0, what
            for b, s in enumerate(self.export(self.src)):  # the source is only read: bitwise where it was exported, else its own model
                if settle:
                    assert_bitwise(s, src_before[b], "%s: the source, filter %d" % (what, b))
                m = self.run.src[b]
                assert_state_close(s[0], s[1], m.x, m.P, what="%s: the source, filter %d" % (what, b))
        if held is not None:  # through the scratch and back: what it held is what the handle holds now
            for k, b in enumerate(which):
                assert_bitwise(after[b], held[k], "%s: the scratch handle, filter %d" % (what, b))
        if not settle:
            return
        self.n_bitwise += 1
        for b in range(B):
            if b not in which or kind == "reserve":
                assert_bitwise(after[b], before[b], "%s: filter %d is not touched" % (what, b))
        for b in which:
            if kind == "remove":
                assert_bitwise(after[b], mm.reduce_state(*before[b], a["keep"][b]), "%s: np.delete, filter %d" % (what, b))
            elif kind == "transform" and a["frames"][b][2] == 0.0:
                assert np.array_equal(after[b][1], before[b][1]), what
            elif kind == "join":
                e = 3 + 2 * counts0[b]
                assert np.array_equal(after[b][1][3:e, 3:e], before[b][1][3:, 3:]) and np.array_equal(after[b][0][3:e], before[b][0][3:]), what
            elif kind == "fuse" and not len(a["pairs"][b]):
                assert_bitwise(after[b], before[b], "%s: no pair, filter %d" % (what, b))
            elif kind == "match" and not (a["ids"][b] >= 0).any():
                assert_bitwise(after[b], before[b], "%s: a list that is all -1, filter %d" % (what, b))
            elif kind == "extract":  # no arithmetic: the bits of the export, indexed
                assert_bitwise(after[b], index_state(before[a["src_index"] if a["mode"] == "fork" else b], a["ids"][b]), "%s: filter %d" % (what, b))


def run_sequence(pkg, monkeypatch, profile, seed):
    ops = mm.make_sequence(seed, profile)
    r = Replay(pkg, monkeypatch, ops)
    try:
        for i, op in enumerate(ops[1:], 1):
            r.step(i, op)
        assert r.twin is None and r.src is None
        assert r.n_twins == 2 and r.n_open >= 1 and (profile not in mm.MAP_PROFILES + mm.MATCH_PROFILES or r.n_twins_new >= 1)
    finally:
        r.close()
    print("%s seed %d: %d ops, %d twins, %d exported rewrites, %d behind open traffic (%d on a streaming handle); max |dx| %.3e, "
          "max |dP| / max |P| %.3e, d2 %.3e, joint worst %.3e, covs %.3e, d2 of the matched updates %.3e"
          % (profile, seed, len(ops), r.n_twins, r.n_bitwise, r.n_open, r.n_live, r.err["x"], r.err["P"], r.err["d2"], r.err["joint"], r.err["covs"], r.err["match_d2"]))
    w = WORST.setdefault(profile, dict.fromkeys(r.err, 0.0))
    for k in w:
        w[k] = max(w[k], r.err[k])
    print("%s, worst so far: max |dx| %.3e, max |dP| / max |P| %.3e, d2 %.3e, joint %.3e, covs %.3e, d2 of the matched updates %.3e"
          % (profile, w["x"], w["P"], w["d2"], w["joint"], w["covs"], w["match_d2"]))


@pytest.mark.parametrize("seed", mm.SEEDS["solo"])
def test_solo_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """One filter, capacity 40-256 (the one-workgroup kernel where the pipeline mode allows it), windows of 1 to 32."""
    run_sequence(pkg, monkeypatch, "solo", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["chain"])
def test_chain_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """One filter, capacity 257-700: the several-workgroup chain kernel."""
    run_sequence(pkg, monkeypatch, "chain", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["chain_wgs"])
def test_chain_wgs_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """A small capacity on two to four workgroups (EKF_CHAIN_WGS)."""
    run_sequence(pkg, monkeypatch, "chain_wgs", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["batch"])
def test_batch_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """Three to five filters of one handle, each with its own landmark count; the batch forms with masks, and single-index calls on a
    filter b > 0 that must leave the others bit for bit."""
    run_sequence(pkg, monkeypatch, "batch", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["solo_maps"])
def test_solo_maps_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """The solo profile with duplicate searches, join -> find -> fuse on the map the filter built, and extractions through a scratch
    handle of another tile count (a probe, or the handle replaced by its own shuffled marginal)."""
    run_sequence(pkg, monkeypatch, "solo_maps", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["chain_maps"])
def test_chain_maps_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """The same on the several-workgroup chain kernel (capacity 257-700), scratch handles on either side of 256."""
    run_sequence(pkg, monkeypatch, "chain_maps", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["batch_maps"])
def test_batch_maps_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """Three to five filters: the batch forms (a split and a pair list per filter, ekf_batch_extract_map through a scratch batch) and
    single-index calls -- a fuse on one filter, a filter replaced by a fork of a sibling -- that leave the others bit for bit."""
    run_sequence(pkg, monkeypatch, "batch_maps", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["solo_match"])
def test_solo_match_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """The solo_maps mix with matched updates (ekf_update_matched with the true associations, one to about 2.5 windows' worth of
    measurements, landmarks repeated, -1 entries interleaved, about half of them behind an open window) and ekf_joint_compat probes."""
    run_sequence(pkg, monkeypatch, "solo_match", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["chain_match"])
def test_chain_match_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """The same on the chain kernel's geometry (capacity 257-700): maps that grow past 256 landmarks, k_match_gather's second block."""
    run_sequence(pkg, monkeypatch, "chain_match", seed)


@pytest.mark.parametrize("seed", mm.SEEDS["batch_match"])
def test_batch_match_sequences(pkg, monkeypatch, pipeline_mode, seed):
    """Three to five filters: the batch form with one filter's list all -1 (it must stay bit for bit), and single-index calls on a
    filter b > 0 that leave the others bit for bit."""
    run_sequence(pkg, monkeypatch, "batch_match", seed)
