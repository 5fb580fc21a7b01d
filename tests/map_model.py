"""Host model of a filter handle and generator of random operation sequences that mix the map rewrites (landmark removal, frame
change, anchoring, map joining, ekf_reserve, the joint-consistency probe; in the *_maps profiles also the duplicate search, the join
-> find -> match -> fuse workflow and submap extraction as a probe and as a rewrite of the handle) with live filter traffic.  No GPU
and no library here: the filter steps go through the C oracle (oracle/oracle_c.py), the rewrites through the NumPy references
beside this file (the package is imported for its pure-Python duplicate_matching only).

A sequence is a plain list of (kind, args) pairs with every argument spelled out; tests/test_map_sequences.py replays it on the
library and on `ModelRunner` in lockstep, tests/test_map_model_cpu.py on the model alone.  The generator runs a ModelRunner of its own
(estimated heading for the compass offset, landmark counts, capacity), so a sequence is a function of (seed, profile) only.

Hidden world per filter: a true pose and world landmarks pairwise >= 1 m apart (no arg-min near a tie), both kept in the world frame
for good: measurements are relative to the true pose, so they do not care about the filter's frame.  Compass readings do; the
generator tracks the offset between the filter's heading and the true one (-theta after a rigid transform, -(estimated phi) after
an anchor; a join keeps it).

The *_maps profiles (appended, so that the four older profiles keep their place in the rng seed and their sequences value for value):
  dups     ekf_find_duplicates as a read-only probe.  The gate is the first of DUP_GATES for which the model's state keeps every pair
           DUP_MARGIN (relative) away from the gate and from max_dist and no pair of the split is near-degenerate
           (dups_precondition); the library's list is then the model's list.  No gate qualifies: a `covs` op instead.
  fuse     the workflow on a map the filter built: a source handle re-observes world landmarks the destination has mapped (the
           isolated ones nearest the robot), join, dups with split = old count (the op carries the one-to-one matching of the
           model's list, which the device's own list must reproduce), perhaps propagations and a compass update -- no measurement:
           the world's 1 m separation does not hold while duplicates exist --, fuse with slack 0 or 1e-4 in rounds of the handle's
           window, then the removal of a planted duplicate the gate did not match.  Now and then a fuse of no pair (a no-op).
  extract  a scratch handle of another tile count (created and closed inside the op): a probe (ekf_extract_map into the scratch and
           ekf_get_submap, both NumPy indexing of the export, bit for bit), or a rewrite: the handle replaced by its own shuffled
           marginal through the scratch (one-filter profiles, and the batch form in batch_maps), or filter b replaced by a fork of
           its sibling c (batch_maps; b's hidden world becomes a copy of c's).
The round size of a fuse is the handle's effective window (ekf_window): ekf_batch_create may shorten max_pending to what fits the
LDS and ekf_reserve plans the geometry again (ekf_geometry.h: plan_geometry), so the generator checks with a restatement of that
plan (planned_window) that the window of every capacity the handle takes is the max_pending it was created with, in either pipeline
mode; the op carries it and the replay asserts it.

The *_match profiles (appended behind those in turn: the seven older profiles generate what they generated) are the *_maps profiles
with two more kinds in the deck, twice each; chain_match starts from maps on either side of 256 landmarks:
  match    ekf_update_matched with the true associations (the hidden world's in_map): per filter a scan of the truly associated
           landmarks nearest the true pose, 1 to about 2.5 windows' worth of measurements, now and then more than 64, landmarks
           repeated, entries with id -1 interleaved; about half of them behind an open window.  In batch_match the batch form with
           one filter's list all -1, or a single-index call on a filter b > 0.  The rounds are the handle's window, which the op
           carries as for a fuse; on the model every round's S is clearly definite (match_rounds_definite), so every entry is applied.
  compat   ekf_joint_compat as a read-only probe: up to 32 pairings with the true associations, and the same with two ids exchanged."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dup_ref as dr  # noqa: E402
import factor_ref as fr  # noqa: E402
import fuse_ref as fu  # noqa: E402
import join_ref as jr  # noqa: E402
import match_ref as mr  # noqa: E402
import reframe_ref as rr  # noqa: E402
from helpers import index_state, shuffled_ids  # noqa: E402

PROFILES = ("solo", "chain", "chain_wgs", "batch", "solo_maps", "chain_maps", "batch_maps", "solo_match", "chain_match", "batch_match")
MAP_PROFILES = PROFILES[4:7]
MATCH_PROFILES = PROFILES[7:]
# (a seed whose replay on the model leaves a measurement within 1e-6 relative of a gate is replaced here, never skipped at run time;
# tests/test_map_model_cpu.py checks every one of these.  The *_maps lists: the first six seeds that the generator's own assertions
# -- every source landmark mapped, every matched pair a planted one, every pair fused, S clearly definite -- and the coverage
# the CPU tests ask of a profile let through)
SEEDS = {"solo": [0, 1, 2, 3, 4, 5, 6, 7], "chain": [0, 1, 2, 3, 4, 5, 6, 7], "chain_wgs": [0, 1, 2, 3, 4, 5, 6, 7], "batch": [0, 1, 2, 3, 4, 5],
         "solo_maps": [0, 1, 2, 3, 4, 5], "chain_maps": [0, 1, 2, 3, 6, 10], "batch_maps": [3, 4, 5, 6, 7, 13],
         # (the *_match lists: the first seeds in which the generator's assertions hold -- every round's S clearly definite, every entry
         # applied -- and a match and a compat op occur; chain_match: 0, 1, 2 and the next three in which a match measures a landmark >= 256)
         "solo_match": [1, 2, 3, 4, 5, 6], "chain_match": [0, 1, 2, 9, 18, 24], "batch_match": [0, 1, 3, 5, 6, 7]}
N_STEPS = 40
GAMMA_MIN, GAMMA_MAX = 10.0, 50.0  # the gates (ekf_default_params; oracle_c.update's defaults)
COMPASS_VAR = 0.0005
SRC_CAPS = (40, 96, 300)
WINDOWS = (1, 3, 8, 16, 24, 32)
REWRITES = ("remove", "transform", "anchor", "reserve", "join", "joint", "covs", "read")
KINDS = ("propagate", "update", "compass") + REWRITES
MAP_REWRITES = REWRITES + ("dups", "fuse", "extract")  # the deck of the *_maps profiles
MAP_KINDS = KINDS + ("dups", "fuse", "extract")
MATCH_REWRITES = MAP_REWRITES + MAP_REWRITES[-3:] + ("match", "compat") * 2  # the deck of the *_match profiles
MATCH_KINDS = MAP_KINDS + ("match", "compat")
DUP_GATES = (9.21, 7.0, 12.0, 5.0, 16.0)
DUP_MARGIN = 1e-3   # tests/helpers.py: MARGIN
DUP_MIN_REL = 1e-6  # a pair's S = (a b; b c): a > DUP_MIN_REL (P_ii.xx + P_jj.xx) and det > DUP_MIN_REL a c
FUSE_MIN_EIG = 1e-6  # every round's S: smallest eigenvalue > FUSE_MIN_EIG x the largest
# Relative agreement asked of d2 in the `match` and `compat` ops: 20 times what tests/test_map_model_cpu.py measures between
# match_ref's double arithmetic and its extended-precision restatement on the states the committed *_match seeds meet (5.85e-13 at
# worst: chain_match seed 0, some seventy rounds of one measurement on a map of four landmarks; 1.05e-12 with cos phi and sin phi
# an ulp off).  More than match_ref.D2_REL, which stays what it is for the inputs it was measured on.
MATCH_D2_REL = 1.2e-11
SCRATCH_CAPS = (8, 40, 96, 130, 200, 300, 400)
LDS_PER_BLOCK = 163840  # hipDeviceProp_t::sharedMemPerBlock of the MI355X


def lm_tiles(n):
    """64 x 64 tiles (32 landmarks) along one side of P_LL (ekf_device.h)."""
    return (2 * n + 63) >> 6


def _oc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


def duplicate_matching(pairs, n_landmarks):
    """The package's greedy one-to-one matching (pure Python; importing the package loads no library)."""
    import __graft_entry__ as ge
    return ge.load_package().ekfslam.duplicate_matching(pairs, n_landmarks)


def planned_window(batch, cap, max_pending, overlap, wgs=None):
    """ekf_window() of a handle as plan_geometry (csrc/ekf_geometry.h) plans it with EKF_OVERLAP forced to `overlap`, the other
    tunables at their defaults (EKF_CHAIN_WGS = wgs), on a device with LDS_PER_BLOCK bytes of LDS per workgroup."""
    return planned_geometry(batch, cap, max_pending, overlap, wgs)[2]


def planned_geometry(batch, cap, max_pending, overlap, wgs=None):
    """(workgroups per filter, whether the one-workgroup kernel k_solo runs the handle, ekf_window()) of the same plan."""
    maxp = min(max(int(max_pending), 1), 32)
    budget = LDS_PER_BLOCK - 16384
    sets = 2 if overlap else 1
    ceil64 = lambda v: (v + 63) // 64 * 64  # noqa: E731
    G = max((cap + 191) // 192, (ceil64(cap) * maxp * sets * 32 + budget - 1) // budget, min((cap + 63) // 64, 32))
    G = max(min(G, 64, max(256 // batch, 1)), 1)
    g_cap = 1 if batch >= 256 else min(64, 256 // batch)
    while G < g_cap and ceil64((cap + G - 1) // G) * maxp * sets * 32 > budget:
        G += 1
    want_solo = not overlap and wgs is None
    if want_solo and cap <= 256 and ceil64(cap) * (maxp if maxp <= 16 else 16) * 32 <= budget:
        G = 1
    if wgs:
        G = wgs
    G = min(G, 64)
    if G * batch > 256:
        G = max(256 // batch, 1)
    solo_kernel = not overlap and G == 1 and want_solo and cap <= 256
    lpw64 = ceil64((cap + G - 1) // G)
    if lpw64 * maxp * sets * 32 > budget:
        if solo_kernel and budget // (lpw64 * 32) >= 16:
            maxp = min(maxp, 32)
        else:
            maxp = budget // (lpw64 * sets * 32)
            if maxp > 1:
                maxp &= ~1
    return G, solo_kernel, maxp


def dups_precondition(x, P, gate, max_dist, split):
    """What makes the LIST of a duplicate search comparable between the model and the library (which agree to about 1e-12): every
    pair DUP_MARGIN (relative) away from the gate and from max_dist (dup_ref.margins), and no pair of the split near-degenerate,
    S = (a b; b c) with a > DUP_MIN_REL (P_ii.xx + P_jj.xx) and det > DUP_MIN_REL a c."""
    N = (len(x) - 3) // 2
    if N < 2:
        return True
    m_gate, m_dist = dr.margins(x, P, gate, max_dist, split)
    if not (m_gate > DUP_MARGIN and m_dist > DUP_MARGIN):
        return False
    _, _, a, _, c, det = dr.terms(x, P)
    i, j = np.triu_indices(N, 1)
    if split > 0:
        m = (i < split) & (j >= split)
        i, j = i[m], j[m]
    xx = np.diag(P)[3::2]
    a, c, det = a[i, j], c[i, j], det[i, j]
    return bool(np.all(a > DUP_MIN_REL * (xx[i] + xx[j])) and np.all(det > DUP_MIN_REL * a * c))


def fuse_rounds_definite(x, P, ij, slack, window):
    """Every round's S = H W + slack I of fuse_ref.fuse(x, P, ij, slack, window) clearly positive definite: its smallest eigenvalue
    above FUSE_MIN_EIG times its largest."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    ij = np.asarray(ij, dtype=np.int64).reshape(-1, 2)
    for r0 in range(0, len(ij), window):
        r = ij[r0:r0 + window]
        ci = np.stack([3 + 2 * r[:, 0], 4 + 2 * r[:, 0]], axis=1).reshape(-1)
        cj = np.stack([3 + 2 * r[:, 1], 4 + 2 * r[:, 1]], axis=1).reshape(-1)
        W = P[:, ci] - P[:, cj]
        ev = np.linalg.eigvalsh(W[ci] - W[cj] + slack * np.eye(len(ci)))
        if not ev[0] > FUSE_MIN_EIG * ev[-1]:
            return False
        x, P = fu.update(x, P, r, slack)
    return True


def match_rounds_definite(x, P, z, R, ids, window):
    """Every round's S = H W + blockdiag(R_k) of match_ref.update(x, P, z, R, ids, window) clearly positive definite: its smallest
    eigenvalue above FUSE_MIN_EIG times its largest (window None: one round over everything, as ekf_joint_compat takes it)."""
    x, P = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    z, R = np.asarray(z, dtype=np.float64).reshape(-1, 2), np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
    kept = np.flatnonzero(ids >= 0)
    rs = window or max(len(kept), 1)
    for r0 in range(0, len(kept), rs):
        sel = kept[r0:r0 + rs]
        _, S, _ = mr.linearise(x, P, z[sel], R[sel], ids[sel])
        ev = np.linalg.eigvalsh(0.5 * (S + S.T))
        if not ev[0] > FUSE_MIN_EIG * ev[-1]:
            return False
        x, P, _ = mr.round_update(x, P, z[sel], R[sel], ids[sel])
        if x is None:
            return False
    return True


def reduce_state(x, P, keep):
    """np.delete of the rows and columns of the landmarks whose keep[l] is false (landmarks beyond the mask are kept)."""
    N = (x.size - 3) // 2
    k = np.ones(N, dtype=bool)
    m = min(N, len(keep))
    k[:m] = np.asarray(keep, dtype=bool)[:m]
    gone = np.flatnonzero(~k)
    rows = np.concatenate([3 + 2 * gone, 4 + 2 * gone]).astype(np.int64)
    return np.delete(x, rows), np.delete(np.delete(P, rows, axis=0), rows, axis=1)


class MapModel:
    """One filter as a dense (x, P) in float64, one method per library call."""

    def __init__(self, x=None, P=None):
        self.oc = _oc()
        self.x = np.zeros(3) if x is None else np.array(x, dtype=np.float64)
        self.P = np.zeros((3, 3)) if P is None else np.array(P, dtype=np.float64)

    @property
    def n_landmarks(self):
        return (self.x.size - 3) // 2

    def propagate(self, v, w, dt):
        self.x, self.P = self.oc.propagate(self.x, self.P, float(v), float(w), self.oc.make_Q(float(v)), float(dt))

    def update(self, z, R):
        """z (n_z, 2), R (n_z, 2, 2): one chunk.  Returns [(decision, matched, mahal)]."""
        z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
        R = np.asarray(R, dtype=np.float64).reshape(-1, 2, 2)
        self.x, self.P, dec, mat, mah = self.oc.update(self.x, self.P, z.T, np.concatenate(list(R), axis=1))
        return list(zip(dec, mat, mah))

    def compass(self, z, R):
        self.x, self.P = self.oc.compass(self.x, self.P, float(z), float(R))

    def remove(self, keep):
        self.x, self.P = reduce_state(self.x, self.P, keep)
        return self.n_landmarks

    def transform(self, frame):
        self.x, self.P = rr.rigid(self.x, self.P, frame)

    def anchor(self):
        self.x, self.P = rr.anchor(self.x, self.P)

    def join(self, src):
        self.x, self.P = jr.join(self.x, self.P, src.x, src.P)
        return self.n_landmarks

    def reserve(self, capacity):
        pass

    def find_duplicates(self, gate, max_dist, split):
        """((i, j) list, n_found, n_degenerate)."""
        pairs, degen = dr.find(self.x, self.P, gate, max_dist, split)
        return list(zip(pairs["i"].tolist(), pairs["j"].tolist())), len(pairs), degen

    def fuse(self, ij, slack, window):
        """(n_landmarks, n_fused) in rounds of `window` pairs, as the handle takes them."""
        self.x, self.P, fused = fu.fuse(self.x, self.P, np.asarray(ij, dtype=np.int64).reshape(-1, 2), slack, window)
        return self.n_landmarks, fused

    def extract(self, src, ids):
        self.x, self.P = index_state((src.x, src.P), ids)
        return self.n_landmarks

    def update_matched(self, z, R, ids, window):
        """(n_landmarks, n_applied, d2) in rounds of `window` measurements, as the handle takes them."""
        self.x, self.P, applied, d2 = mr.update(self.x, self.P, z, R, ids, window)
        return self.n_landmarks, applied, d2

    def joint_compat(self, z, R, ids):
        return mr.joint_compat(self.x, self.P, z, R, ids)

    def joint(self, x_true):
        return fr.lapack(self.x, self.P, x_true)

    def landmark_covs(self):
        l = np.arange(self.n_landmarks)
        return np.stack([self.P[3 + 2 * l, 3 + 2 * l], self.P[3 + 2 * l, 4 + 2 * l], self.P[4 + 2 * l, 4 + 2 * l]], axis=1).reshape(-1, 3)

    def clearly_positive_definite(self):
        """P well inside the positive definite cone (condition below 1e8): the joint quantities then have one answer to far
        better than the tolerance they are compared with."""
        if not np.all(np.isfinite(self.P)):
            return False
        ev = np.linalg.eigvalsh(self.P)
        return bool(ev[0] > 1e-8 * ev[-1])


class ModelRunner:
    """The models of one sequence: the destination handle's filters and, during a join, the source handle's.  step(op) applies one
    operation and returns what the library must answer (None where there is nothing to compare)."""

    def __init__(self):
        self.models, self.src = [], []
        self.cap = self.src_cap = 0
        self.margin = math.inf  # the smallest |mahal - gamma| / gamma seen at either gate

    def _note(self, decs):
        for _, _, mah in decs:
            for g in (GAMMA_MIN, GAMMA_MAX):
                self.margin = min(self.margin, abs(mah - g) / g)

    def _update(self, models, a, cap):
        out = []
        for b, m in enumerate(models):
            idx = np.flatnonzero(a["valid"][b])
            decs = m.update(a["z"][b, idx], a["R"][b, idx]) if idx.size else []
            self._note(decs)
            out.append(decs)
            assert m.n_landmarks <= cap  # (a sequence never runs a handle into its sticky EKF_ERR_CAPACITY)
        return out

    def step(self, op):
        kind, a = op
        M = self.models
        which = lambda: range(len(M)) if a.get("index") is None else [a["index"]]  # noqa: E731
        if kind == "create":
            self.models, self.cap = [MapModel() for _ in range(a["B"])], a["cap"]
        elif kind == "load":
            M[a["index"]] = MapModel(a["x"], a["P"])
        elif kind == "propagate":
            for b, m in enumerate(M):
                m.propagate(a["v"][b], a["w"][b], a["dt"][b])
        elif kind == "compass":
            for b, m in enumerate(M):
                if a["valid"][b]:
                    m.compass(a["z"][b], a["R"])
        elif kind == "update":
            return self._update(M, a, self.cap)
        elif kind == "remove":
            return [M[b].remove(a["keep"][b]) for b in which()]
        elif kind == "transform":
            for b in which():
                M[b].transform(a["frames"][b])
        elif kind == "anchor":
            for b in which():
                M[b].anchor()
        elif kind == "reserve":
            self.cap = a["cap"]
        elif kind == "src_create":
            self.src, self.src_cap = [MapModel() for _ in range(a["B"])], a["cap"]
        elif kind == "src_propagate":
            for b, m in enumerate(self.src):
                m.propagate(a["v"][b], a["w"][b], a["dt"][b])
        elif kind == "src_update":
            return self._update(self.src, a, self.src_cap)
        elif kind == "join":
            pairs = [(b, b) for b in range(len(M))] if a["index"] is None else [(a["index"], a["src_index"])]
            if a["expect"] == "capacity":
                assert any(M[d].n_landmarks + self.src[s].n_landmarks > self.cap for d, s in pairs)
                return None
            assert all(M[d].n_landmarks + self.src[s].n_landmarks <= self.cap for d, s in pairs)
            return [M[d].join(self.src[s]) for d, s in pairs]
        elif kind == "src_close":
            self.src = []
        elif kind == "joint":
            return [M[b].joint(a["x_true"][b]) for b in which()]
        elif kind == "covs":
            return M[a["index"]].landmark_covs()
        elif kind == "dups":
            return [M[b].find_duplicates(a["gate"], a["max_dist"], a["split"][b]) for b in which()]
        elif kind == "fuse":
            return [M[b].fuse(a["pairs"][b], a["slack"], a["window"]) for b in which()]
        elif kind == "extract":
            if a["mode"] == "probe":
                return None
            return [M[b].extract(M[a["src_index"] if a["mode"] == "fork" else b], a["ids"][b]) for b in which()]
        elif kind == "match":
            return [M[b].update_matched(a["z"][b], a["R"][b], a["ids"][b], a["window"]) for b in which()]
        elif kind == "compat":  # the true hypothesis and the one with two ids exchanged
            return [(M[b].joint_compat(a["z"][b], a["R"][b], a["ids"][b]), M[b].joint_compat(a["z"][b], a["R"][b], a["swapped"][b])) for b in which()]
        elif kind in ("read", "twin_begin", "twin_end"):
            pass
        else:
            raise ValueError(kind)
        return None


# ---- the generator ----------------------------------------------------------------------------------
def _world(rng, n, extent):
    pts = []
    while len(pts) < n:
        p = rng.uniform(-extent, extent, 2)
        if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 >= 1.0 for q in pts) and math.hypot(p[0], p[1]) >= 1.0:
            pts.append(p)
    return np.array(pts)


class _Sim:
    """The hidden side of one filter: true pose, world, which world landmark every map landmark is (-1: a spurious one made by an
    outlier), the compass offset."""

    def __init__(self, rng, n_world, extent):
        self.world = _world(rng, n_world, extent)
        self.pose = np.zeros(3)
        self.in_map = []
        self.offset = 0.0

    def move(self, v, w, dt):
        self.pose = self.pose + dt * np.array([v * math.cos(self.pose[2]), v * math.sin(self.pose[2]), w])

    def rel(self, k):
        c, s = math.cos(self.pose[2]), math.sin(self.pose[2])
        d = self.world[k] - self.pose[:2]
        return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])

    def unseen(self):
        seen = set(self.in_map)
        return [k for k in range(len(self.world)) if k not in seen]


def _measurement(oc, z):
    return oc.make_measurement(1000.0 * z[0], 1000.0 * z[1])[1]


def _initial_state(rng, sim, n0):
    """n0 world landmarks already mapped: the estimate within its own covariance of the truth, P = D + U U^T."""
    n = 3 + 2 * n0
    x = np.empty(n)
    x[:3] = sim.pose
    x[3:] = (sim.world[:n0] + rng.normal(0.0, 0.03, (n0, 2))).reshape(-1)
    d = rng.uniform(0.002, 0.004, n)
    d[:3] *= 0.05
    U = rng.normal(0.0, 3e-3, (n, 6))
    P = U @ U.T
    P[np.diag_indices(n)] += d
    sim.in_map = list(range(n0))
    return x, 0.5 * (P + P.T)


class _Gen:
    def __init__(self, seed, profile):
        assert profile in PROFILES
        self.oc = _oc()
        self.rng = rng = np.random.default_rng([PROFILES.index(profile), seed, 20261018])
        self.profile = profile
        self.match = profile in MATCH_PROFILES
        self.maps = profile in MAP_PROFILES or self.match  # (a *_match profile is its *_maps profile with two more kinds in the deck)
        for suffix in ("_maps", "_match"):  # (the parameters of the profile it extends)
            profile = profile[:-len(suffix)] if profile.endswith(suffix) else profile
        self.ops = []
        self.run = ModelRunner()
        self.deck = []
        self.n_open, self.behind_traffic, self.force_open = 0, False, False
        wgs = None
        if profile == "solo":
            cap, window, n_world, extent = int(rng.integers(40, 257)), int(rng.choice(WINDOWS)), 170, 13.0
            starts = [[0, 5, 30, 31, 33, 60, 64, 70][int(rng.integers(0, 8))]]
            if rng.random() < 0.5:  # little room: a join will be refused first
                cap = max(40, starts[0] + int(rng.integers(8, 24)))
        elif profile == "chain":
            cap, window, n_world, extent = int(rng.integers(257, 701)), int(rng.choice(WINDOWS)), 420, 20.0
            # (chain_match: maps on either side of 256 landmarks, where k_match_gather's second block of 256 begins)
            starts = [([0, 64, 130, 250, 257, 270, 300, 330] if self.match else [0, 31, 64, 95, 130, 225, 245, 250])[int(rng.integers(0, 8))]]
            if starts[0] >= 225:  # little room: a join will be refused first
                cap = int(rng.integers(257, 275))
                if self.match:
                    cap = max(cap, starts[0] + int(rng.integers(8, 24)))
        elif profile == "chain_wgs":
            cap, window, n_world, extent = int(rng.integers(30, 121)), int(rng.choice((1, 2, 4, 8, 16))), 170, 13.0
            wgs = int(rng.integers(2, 5))
            starts = [[0, 5, 20, 31, 33, 64][int(rng.integers(0, 6))]]
        else:
            B = int(rng.integers(3, 6))
            cap, window, n_world, extent = int(rng.integers(40, 121)), int(rng.choice((2, 4, 8, 16))), 130, 11.0
            pool = [5, 20, 31, 32, 33, 64]
            starts = [pool[int(k)] for k in rng.choice(len(pool), size=B, replace=False)]
            starts[int(rng.integers(0, B))] = 0  # one filter starts empty
            if rng.random() < 0.5:  # little room: a join will be refused first
                cap = max(40, max(starts) + int(rng.integers(8, 24)))
        starts = [min(n0, cap - 6) for n0 in starts]
        self.B = len(starts)
        self.base, self.window, self.wgs = profile, window, wgs
        self.twin_wish, self.twin_kind = None, None
        self.sims = [_Sim(rng, n_world, extent) for _ in starts]
        self.emit("create", B=self.B, cap=cap, window=window, wgs=wgs)
        for b, n0 in enumerate(starts):
            if n0:
                x, P = _initial_state(rng, self.sims[b], n0)
                self.emit("load", index=b, x=x, P=P)

    # -- plumbing
    def emit(self, kind, **a):
        # (a rewrite straight behind filter traffic that does not export first meets an open window and a live streaming launch)
        if (kind in ("remove", "transform", "anchor", "join", "fuse", "match") or kind == "extract" and a["mode"] != "probe") and not a["settle"] \
                and self.behind_traffic:
            self.n_open += 1
        if self.maps and kind in ("create", "reserve"):  # the effective window stays the one asked for, whatever the capacity
            assert all(planned_window(self.B, a["cap"], self.window, ov, self.wgs) == self.window for ov in (False, True)), a["cap"]
        self.behind_traffic = kind in ("propagate", "update", "compass", "src_propagate", "src_update")
        op = (kind, a)
        self.ops.append(op)
        return self.run.step(op)

    @property
    def models(self):
        return self.run.models

    def counts(self):
        return [m.n_landmarks for m in self.models]

    def grow(self, need):
        """Room for `need` landmarks in every filter: an ekf_reserve, now and then across 256 (the kernel family changes)."""
        cap = self.run.cap
        new = max(need, cap) + int(self.rng.integers(4, 40))
        if cap <= 256 and self.base != "batch" and self.rng.random() < 0.4:
            new = max(new, int(self.rng.integers(257, 300)))
        self.emit("reserve", cap=new)

    def note_new(self, sim, decs, world_ids):
        for (dec, _, _), k in zip(decs, world_ids):
            if dec == self.oc.NEW:
                sim.in_map.append(k)

    # -- one step of filter traffic
    def traffic(self):
        rng, B = self.rng, self.B
        still = rng.random() < 0.1
        v = np.zeros(B) if still else rng.uniform(0.05, 0.6, B)
        w, dt = rng.uniform(-0.4, 0.4, B), rng.uniform(0.02, 0.3, B)
        for b, s in enumerate(self.sims):
            s.move(v[b], w[b], dt[b])
        self.emit("propagate", v=v, w=w, dt=dt)
        if rng.random() < 0.2:
            valid = np.ones(B, dtype=bool) if B == 1 else rng.random(B) < 0.6
            z = np.array([(s.pose[2] + s.offset) % 6.283185307 + rng.normal(0.0, 0.02) for s in self.sims])
            self.emit("compass", z=z, R=COMPASS_VAR, valid=valid)
        n_z = int(rng.integers(0, 5)) if B == 1 else int(rng.integers(1, 4))
        if not n_z:
            return
        if max(self.counts()) + n_z > self.run.cap:
            self.grow(max(self.counts()) + n_z)
        z, R = np.zeros((B, n_z, 2)), np.tile(np.eye(2), (B, n_z, 1, 1))
        valid = np.ones((B, n_z), dtype=bool) if B == 1 else rng.random((B, n_z)) < 0.75
        ids = [[] for _ in range(B)]
        for b, s in enumerate(self.sims):
            mapped = [k for k in s.in_map if k >= 0]
            fresh = s.unseen()
            used = set()
            for j in range(n_z):
                if not valid[b, j]:
                    continue
                r = rng.random()  # < 0.55: a re-observation, < 0.88: a first sighting, else an outlier of a mapped landmark
                pool = [k for k in (mapped if ((r < 0.55 or r >= 0.88) and mapped) else fresh) if k not in used]
                if not pool:
                    valid[b, j] = False
                    continue
                near = sorted(pool, key=lambda k: float(np.hypot(*(s.world[k] - s.pose[:2]))))[:12]
                k = int(near[int(rng.integers(0, len(near)))])
                used.add(k)
                zz = s.rel(k) + rng.normal(0.0, 0.03, 2)
                tag = k
                if r >= 0.88 and k in mapped:  # an outlier between the gates, steered there by a trial on the model
                    m = self.models[b]
                    for _ in range(4):
                        a = rng.uniform(0.0, 2.0 * math.pi)
                        cand = zz + rng.uniform(0.15, 0.5) * np.array([math.cos(a), math.sin(a)])
                        trial = self.oc.update(m.x, m.P, cand.reshape(2, 1), _measurement(self.oc, cand))
                        if trial[2][0] == self.oc.IGNORE:
                            break
                    else:  # no trial fell between the gates: no measurement (a New one would sit half a metre from a real landmark)
                        valid[b, j] = False
                        continue
                    zz, tag = cand, -1
                z[b, j], R[b, j] = zz, _measurement(self.oc, zz)
                ids[b].append(tag)
        if not valid.any():
            return
        decs = self.emit("update", z=z, R=R, valid=valid)
        for b, s in enumerate(self.sims):
            self.note_new(s, decs[b], ids[b])

    # -- rewrites and probes
    def removal_mask(self, b, variant=None):
        rng, N = self.rng, self.counts()[b]
        keep = np.ones(N, dtype=bool)
        if N == 0:
            return keep
        v = variant or str(rng.choice(["subset", "subset", "first", "last", "tile", "all", "edge"]))
        if v == "subset":
            keep = rng.random(N) > rng.uniform(0.1, 0.6)
        elif v == "first":
            keep[0] = False
        elif v == "last":
            keep[-1] = False
        elif v == "tile":  # a whole tile's worth of landmarks, from a random start
            a = int(rng.integers(0, max(N - 32, 0) + 1))
            keep[a:a + 32] = False
        elif v == "all":
            keep[:] = False
        else:  # "edge": down to a whole number of tiles
            drop = N % 32 if N % 32 and N > 32 else min(N, 32)
            if drop < N or rng.random() < 0.3:
                keep[rng.choice(N, size=drop, replace=False)] = False
        return keep

    def do_remove(self, index, variant=None):
        which = range(self.B) if index is None else [index]
        keep = {b: self.removal_mask(b, variant) for b in which}
        if index is None:  # the batch form: one [B][ld] array, landmarks beyond a filter's own count ignored
            ld = max(max(len(k) for k in keep.values()), 1)
            arr = np.ones((self.B, ld), dtype=bool)
            for b, k in keep.items():
                arr[b, :len(k)] = k
            keep = {b: arr[b] for b in which}
        for b in which:
            k = keep[b][:len(self.sims[b].in_map)]
            self.sims[b].in_map = [w for w, kept in zip(self.sims[b].in_map, k) if kept]
        self.emit("remove", index=index, keep=keep, settle=bool(index is not None and self.B > 1 or self.rng.random() < 0.5) and not self.force_open)

    def do_join(self, index):
        rng, B = self.rng, self.B
        dst = list(range(B)) if index is None else [index]
        if any(len(self.sims[b].unseen()) < 30 for b in dst):
            return False
        if rng.random() < 0.5:  # the destination on a tile edge: no straddling old x new tile
            for b in dst:
                if self.counts()[b] > 32 and self.counts()[b] % 32:
                    self.do_remove(b if B > 1 else index, "edge")
        src_B = len(dst)
        mine = [[] for _ in dst]  # world landmarks of the source's map, in its order
        pools = []
        room = min(self.run.cap - self.counts()[b] for b in dst)
        refuse = room <= 40 and rng.random() < 0.7  # more landmarks than there is room for: EKF_ERR_CAPACITY first
        for b in dst:
            s = self.sims[b]
            fresh = sorted(s.unseen(), key=lambda k: float(np.hypot(*(s.world[k] - s.pose[:2]))))
            pools.append(fresh[:room + int(rng.integers(1, 4)) if refuse else int(rng.integers(3, 14))])
        src_cap = int(rng.choice([c for c in SRC_CAPS if c >= max(len(p) for p in pools)]))
        self.emit("src_create", B=src_B, cap=src_cap, window=int(rng.choice(WINDOWS)))
        idle = int(rng.integers(0, src_B)) if src_B > 1 and rng.random() < 0.5 else -1  # a source filter that stays fresh
        for t in range(8 if refuse else int(rng.integers(3, 9))):
            v, w, dt = rng.uniform(0.05, 0.6, src_B), rng.uniform(-0.4, 0.4, src_B), rng.uniform(0.02, 0.3, src_B)
            for i, b in enumerate(dst):
                self.sims[b].move(v[i], w[i], dt[i])
            self.emit("src_propagate", v=v, w=w, dt=dt)
            n_z = (room + 10) // 8 if refuse else int(rng.integers(1, 4))
            z, R = np.zeros((src_B, n_z, 2)), np.tile(np.eye(2), (src_B, n_z, 1, 1))
            valid = np.zeros((src_B, n_z), dtype=bool)
            ids = [[] for _ in dst]
            for i, b in enumerate(dst):
                if i == idle:
                    continue
                pick = rng.choice(len(pools[i]), size=min(n_z, len(pools[i])), replace=False)
                if refuse:  # the pool in order, so that all of it is mapped
                    pick = sorted(set((n_z * t + j) % len(pools[i]) for j in range(n_z)))
                for j, p in enumerate(pick):
                    k = pools[i][int(p)]
                    z[i, j] = self.sims[b].rel(k) + rng.normal(0.0, 0.03, 2)
                    R[i, j] = _measurement(self.oc, z[i, j])
                    valid[i, j] = True
                    ids[i].append(k)
            decs = self.emit("src_update", z=z, R=R, valid=valid)
            for i in range(src_B):
                for (dec, _, _), k in zip(decs[i], ids[i]):
                    if dec == self.oc.NEW:
                        mine[i].append(k)
        need = max(self.counts()[b] + self.run.src[i].n_landmarks for i, b in enumerate(dst))
        settle = bool(rng.random() < 0.5 or B > 1 and index is not None)
        if need > self.run.cap:
            self.emit("join", index=index, src_index=0, expect="capacity", settle=True)
            self.emit("reserve", cap=need + int(rng.integers(0, 40)))
        self.emit("join", index=index, src_index=0, expect="ok", settle=settle)
        for i, b in enumerate(dst):
            self.sims[b].in_map += mine[i]
        self.emit("src_close")
        return True

    def do_joint(self, index):
        which = range(self.B) if index is None else [index]
        xt = {}
        for b in which:
            m = self.models[b]
            if m.clearly_positive_definite():
                t = fr.draw_truth(m.x, m.P, int(self.rng.integers(0, 2 ** 31)))
                t[2] += 2.0 * math.pi  # a full turn away: the error's heading component is wrapped
                xt[b] = t
            elif index is None:
                return False
            else:
                xt[b] = None
                if not (m.P[:3, :3] == 0.0).all() or (m.n_landmarks and not MapModel(m.x[3:], m.P[3:, 3:]).clearly_positive_definite()):
                    return False  # neither clearly definite nor the exact zero pose block of an anchor: `info` would be a coin toss
        self.emit("joint", index=index, x_true=xt)
        return True

    def rewrite(self, state_changing=False):
        rng, B = self.rng, self.B
        if not self.deck:
            self.deck = [str(k) for k in rng.permutation(REWRITES)]
        kind = str(rng.choice(["remove", "transform", "anchor"])) if state_changing else self.deck.pop()
        # the batch profile: the batch form, or a single-index call on a filter b > 0 (the others must not move)
        index = 0 if B == 1 else (int(rng.integers(1, B)) if rng.random() < 0.4 and not self.force_open else None)
        if kind == "remove":
            self.do_remove(index)
        elif kind == "transform":
            frames = {}
            for b in (range(B) if index is None else [index]):
                th = 0.0 if rng.random() < 0.25 else float(rng.uniform(-3.0, 3.0))
                frames[b] = np.array([rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 5.0), th])
                self.sims[b].offset -= th
            self.emit("transform", index=index, frames=frames, settle=bool(index is not None and B > 1 or rng.random() < 0.5) and not self.force_open)
        elif kind == "anchor":
            for b in (range(B) if index is None else [index]):
                self.sims[b].offset -= float(self.models[b].x[2])
            self.emit("anchor", index=index, settle=bool(index is not None and B > 1))
        elif kind == "reserve":
            self.grow(self.run.cap)
        elif kind == "join":
            if not self.do_join(index):
                self.emit("read", index=int(rng.integers(0, B)))
        elif kind == "joint":
            if not self.do_joint(index) and not (index is None and self.do_joint(int(rng.integers(0, B)))):
                self.emit("covs", index=int(rng.integers(0, B)))
        elif kind == "covs":
            self.emit("covs", index=int(rng.integers(0, B)))
        else:
            self.emit("read", index=int(rng.integers(0, B)))
        return kind

    # -- the *_maps profiles: duplicate search, fusion, extraction
    def twin_point(self, kind):
        """Behind a state-changing op: a twin starts here if build_maps wished for one and this kind may carry it."""
        if self.twin_wish == "any" or self.twin_wish == "new" and kind in ("fuse", "extract"):
            self.emit("twin_begin")
            self.twin_wish, self.twin_kind = None, kind

    def do_dups(self, index, splits=None, max_dist=None, matched=False):
        """A duplicate search whose list the model can vouch for (a `covs` op where no gate of DUP_GATES qualifies).  Returns the
        gate, or None."""
        rng, B = self.rng, self.B
        which = list(range(B)) if index is None else [index]
        if splits is None:
            splits = {b: int(rng.integers(1, self.counts()[b] + 1)) if self.counts()[b] and rng.random() < 0.5 else 0 for b in which}
            max_dist = float(rng.choice([0.5, 1.5, 4.0])) if rng.random() < 0.5 else None
        settle = bool(index is not None and B > 1 or rng.random() < 0.5)
        for gate in DUP_GATES:
            if all(dups_precondition(self.models[b].x, self.models[b].P, gate, max_dist, splits[b]) for b in which):
                match = None
                if matched:  # the one-to-one matching of the model's list: what the fuse behind this search is given
                    match = {}
                    for b in which:
                        m = self.models[b]
                        found, _ = dr.find(m.x, m.P, gate, max_dist, splits[b])
                        match[b] = fu.as_ij(duplicate_matching(found, m.n_landmarks))
                self.emit("dups", index=index, gate=gate, max_dist=max_dist, split=splits, matched=match, settle=settle)
                return gate
        self.emit("covs", index=int(rng.integers(0, B)))
        return None

    def between(self):
        """Traffic that is no measurement, on every filter: a propagation, now and then a compass update behind it."""
        rng, B = self.rng, self.B
        v, w, dt = rng.uniform(0.05, 0.6, B), rng.uniform(-0.4, 0.4, B), rng.uniform(0.02, 0.3, B)
        for b, s in enumerate(self.sims):
            s.move(v[b], w[b], dt[b])
        self.emit("propagate", v=v, w=w, dt=dt)
        if rng.random() < 0.4:
            valid = np.ones(B, dtype=bool) if B == 1 else rng.random(B) < 0.6
            z = np.array([(s.pose[2] + s.offset) % 6.283185307 + rng.normal(0.0, 0.02) for s in self.sims])
            self.emit("compass", z=z, R=COMPASS_VAR, valid=valid)

    def do_fuse(self, index):
        """join -> find -> match -> fuse on the map the filter built.  False (nothing emitted but perhaps a removal down to a tile
        edge) where there is nothing to re-observe."""
        rng, B = self.rng, self.B
        dst = list(range(B)) if index is None else [index]
        if any(len(self.sims[b].unseen()) < 30 for b in dst):
            return False
        if rng.random() < 0.5:  # the destination on a tile edge
            for b in dst:
                if self.counts()[b] > 32 and self.counts()[b] % 32:
                    self.do_remove(b if B > 1 else index, "edge")
        many = self.window <= 8 and rng.random() < 0.7  # more pairs than a round takes
        only_dups = rng.random() < 0.3  # a source that maps nothing new: the fuse gives back every row of the join
        pools, seen = [], []
        for b in dst:
            s, m = self.sims[b], self.models[b]
            L = m.x[3:].reshape(-1, 2)
            # re-observed: landmarks no other ESTIMATE of the map comes within 1 m of (a spurious one made by an outlier would
            # be a second candidate at the gate), nearest the robot first
            # ... and 2 m from the robot at least: the source drives up to a metre and a half meanwhile
            cand = [l for l, k in enumerate(s.in_map) if k >= 0 and (len(L) == 1 or np.sort(np.hypot(*(L - L[l]).T))[1] >= 1.0)
                    and np.hypot(*(s.world[k] - s.pose[:2])) >= 2.0]
            cand.sort(key=lambda l: float(np.hypot(*(s.world[s.in_map[l]] - s.pose[:2]))))
            cand = cand[:int(rng.integers(9, 12)) if many else int(rng.integers(1, 5))]
            fresh = sorted(s.unseen(), key=lambda k: float(np.hypot(*(s.world[k] - s.pose[:2]))))
            seen.append(cand)
            pools.append([s.in_map[l] for l in cand] + ([] if only_dups and cand else fresh[:int(rng.integers(1, 8))]))
        if not any(seen):
            return False
        old = self.counts()
        src_B, T = len(dst), 8
        n_z = -(-max(len(p) for p in pools) // 6)  # the whole pool is mapped by step 6, the first of it seen again behind that
        self.emit("src_create", B=src_B, cap=int(rng.choice([c for c in SRC_CAPS if c >= max(len(p) for p in pools)])), window=int(rng.choice(WINDOWS)))
        mine = [[] for _ in dst]
        for t in range(T):
            v, w, dt = rng.uniform(0.05, 0.6, src_B), rng.uniform(-0.4, 0.4, src_B), rng.uniform(0.02, 0.3, src_B)
            for i, b in enumerate(dst):
                self.sims[b].move(v[i], w[i], dt[i])
            self.emit("src_propagate", v=v, w=w, dt=dt)
            z, R = np.zeros((src_B, n_z, 2)), np.tile(np.eye(2), (src_B, n_z, 1, 1))
            valid = np.zeros((src_B, n_z), dtype=bool)
            ids = [[] for _ in dst]
            for i, b in enumerate(dst):
                for j, p in enumerate(sorted(set((n_z * t + j) % len(pools[i]) for j in range(n_z)))):
                    k = pools[i][p]
                    z[i, j] = self.sims[b].rel(k) + rng.normal(0.0, 0.03, 2)
                    R[i, j] = _measurement(self.oc, z[i, j])
                    valid[i, j] = True
                    ids[i].append(k)
            decs = self.emit("src_update", z=z, R=R, valid=valid)
            for i in range(src_B):
                for (dec, _, _), k in zip(decs[i], ids[i]):
                    if dec == self.oc.NEW:
                        mine[i].append(k)
        need = max(old[b] + self.run.src[i].n_landmarks for i, b in enumerate(dst))
        if need > self.run.cap:
            self.emit("reserve", cap=need + int(rng.integers(0, 40)))
        self.emit("join", index=index, src_index=0, expect="ok", settle=bool(rng.random() < 0.5 or B > 1 and index is not None))
        for i, b in enumerate(dst):
            self.sims[b].in_map += mine[i]
        self.emit("src_close")
        # the planted pairs (old landmark, its re-observation), per destination filter
        planted = {}
        for i, b in enumerate(dst):
            assert sorted(mine[i]) == sorted(pools[i]), "a source landmark was not mapped"
            planted[b] = sorted((l, old[b] + mine[i].index(self.sims[b].in_map[l])) for l in seen[i])
        gate = self.do_dups(index, splits={b: old[b] for b in dst}, matched=True)
        assert gate is not None, "no gate keeps the joined map's pairs off its edge"
        pairs = self.ops[-1][1]["matched"]
        for b in dst:
            assert set(map(tuple, pairs[b].tolist())) <= set(planted[b]), "a matched pair that was not planted"
        open_fuse = rng.random() < 0.6
        if open_fuse:  # the fuse meets an open window
            for _ in range(int(rng.integers(1, 3))):
                self.between()
        slack = float(rng.choice([0.0, 1e-4]))
        for b in dst:
            fu.check_pairs(pairs[b], self.counts()[b])
            assert fuse_rounds_definite(self.models[b].x, self.models[b].P, pairs[b], slack, self.window), "S of a round is not clearly definite"
        res = self.emit("fuse", index=index, pairs=pairs, slack=slack, window=self.window,
                        settle=bool(index is not None and B > 1 or not open_fuse and rng.random() < 0.5))
        assert [r[1] for r in res] == [len(pairs[b]) for b in dst], "the reference did not fuse every pair"
        left = {}
        for b in dst:
            gone = set(pairs[b][:, 1].tolist())
            alive = [l for l in range(len(self.sims[b].in_map)) if l not in gone]
            self.sims[b].in_map = [self.sims[b].in_map[l] for l in alive]
            left[b] = [alive.index(j) for _, j in planted[b] if j not in gone]  # planted, but not matched: it must not meet traffic
        if any(len(p) for p in pairs.values()):
            self.twin_point("fuse")
        if any(left.values()):
            keep = {b: np.ones(max(max(self.counts()), 1) if index is None else self.counts()[b], dtype=bool) for b in dst}
            for b in dst:
                keep[b][left[b]] = False
                k = keep[b][:len(self.sims[b].in_map)]
                self.sims[b].in_map = [w for w, kept in zip(self.sims[b].in_map, k) if kept]
            self.emit("remove", index=index, keep=keep, settle=bool(index is not None and B > 1 or rng.random() < 0.5))
        return True

    def draw_ids(self, N, rewrite):
        rng = self.rng
        r = rng.random()
        if r < 0.15:
            return None  # every landmark in order: a copy
        if r < (0.22 if rewrite else 0.3) or N == 0:
            return np.zeros(0, dtype=np.int32)  # the pose and P_RR alone
        count = int(rng.integers(max(1, N - 8), N + 1)) if rewrite and rng.random() < 0.7 else int(rng.integers(1, N + 1))
        return shuffled_ids(N, count, seed=int(rng.integers(0, 2 ** 31)))

    def do_extract(self, index, rewrite):
        """Submap extraction through a scratch handle of another tile count: a probe of one filter, or a rewrite -- the handle
        replaced by its own marginal (one filter, or the batch form), or filter `index` by a fork of a sibling."""
        rng, B = self.rng, self.B
        counts = self.counts()
        src_index = None
        if not rewrite:
            mode, index = "probe", int(rng.integers(0, B)) if index is None else index
        elif B == 1:
            mode = "self"
        elif index is None:
            mode = "batch"
        else:
            mode, src_index = "fork", int(rng.choice([c for c in range(B) if c != index]))
        which = list(range(B)) if index is None else [index]
        ids = {b: self.draw_ids(counts[src_index if mode == "fork" else b], rewrite) for b in which}
        size = lambda b: counts[src_index if mode == "fork" else b] if ids[b] is None else len(ids[b])  # noqa: E731
        caps = [c for c in SCRATCH_CAPS if c >= max(max(size(b) for b in which), 1) and lm_tiles(c) != lm_tiles(self.run.cap)]
        if rewrite:
            for b in which:
                s = self.sims[src_index] if mode == "fork" else self.sims[b]
                sel = list(range(len(s.in_map))) if ids[b] is None else ids[b].tolist()
                if mode == "fork":  # b's hidden world becomes a copy of its sibling's
                    t = _Sim.__new__(_Sim)
                    t.world, t.pose, t.offset = s.world, s.pose.copy(), s.offset
                    self.sims[b] = t
                self.sims[b].in_map = [s.in_map[l] for l in sel]
        self.emit("extract", mode=mode, index=index, src_index=src_index, ids=ids, scratch_cap=int(rng.choice(caps)) if mode != "fork" else None,
                  settle=bool(index is not None and B > 1 or rng.random() < 0.5) and not self.force_open)
        if rewrite:
            self.twin_point("extract")

    # -- the *_match profiles: matched updates and the score of a hypothesis
    def scan_of(self, b, n_meas):
        """(ids, z, R) of n_meas measurements of filter b: truly associated mapped landmarks (the hidden world's in_map says which)
        nearest the true pose, about two thirds as many landmarks as measurements, so that some are measured again;
        z = rel(k) + N(0, 0.03), R of the oracle's measurement model as in `traffic`.  None where nothing true is mapped."""
        rng, s = self.rng, self.sims[b]
        cand = [l for l, k in enumerate(s.in_map) if k >= 0]
        if not cand:
            return None
        cand.sort(key=lambda l: float(np.hypot(*(s.world[s.in_map[l]] - s.pose[:2]))))
        distinct = cand[:max(1, -(-2 * n_meas // 3))]
        ids = [distinct[int(p)] for p in rng.permutation(len(distinct))][:n_meas]
        ids += [distinct[int(rng.integers(0, len(distinct)))] for _ in range(n_meas - len(ids))]
        z = np.array([s.rel(s.in_map[l]) + rng.normal(0.0, 0.03, 2) for l in ids])
        return np.array(ids, dtype=np.int32), z, np.array([_measurement(self.oc, zz) for zz in z])

    def padded(self, scans, n_z):
        """The scans (b -> (ids, z, R) or None) as lists of n_z entries each, the entries that are none of the scan's (ids -1, z = 0,
        R = I) interleaved at random places."""
        ids, z, R = {}, {}, {}
        for b, sc in scans.items():
            ids[b], z[b], R[b] = np.full(n_z, -1, dtype=np.int32), np.zeros((n_z, 2)), np.tile(np.eye(2), (n_z, 1, 1))
            if sc is not None:
                at = np.sort(self.rng.permutation(n_z)[:len(sc[0])])
                ids[b][at], z[b][at], R[b][at] = sc
        return ids, z, R

    def match_index(self, index):
        """Which filters a match or a compat op addresses.  One filter: itself.  A batch: the batch form with one filter's list all -1
        about a third of the time (and whenever an open window is wanted), else a single-index call on a filter b > 0.  Returns
        (index, the filters of the call, the one that sits out or None)."""
        rng, B = self.rng, self.B
        if B == 1:
            return 0, [0], None
        if self.force_open or rng.random() < 0.35:
            return None, list(range(B)), int(rng.integers(0, B))
        index = index if index is not None else int(rng.integers(1, B))
        return index, [index], None

    def do_match(self, index):
        """ekf_update_matched with the true associations: between 1 and about 2.5 windows' worth of measurements per filter, now and
        then more than the 64 the measurement table starts with; every round's S clearly definite on the model, so every entry is
        applied.  The op carries the handle's window: the model takes its rounds from there."""
        rng = self.rng
        index, which, idle = self.match_index(index)
        scans = {}
        for b in which:
            n_meas = int(rng.integers(65, 76)) if rng.random() < 0.12 else int(rng.integers(1, int(2.5 * self.window) + 2))
            scans[b] = None if b == idle else self.scan_of(b, n_meas)
        if not any(sc is not None for sc in scans.values()):
            self.emit("read", index=int(rng.integers(0, self.B)))  # nothing true is mapped: a call without a measurement is no rewrite
            return
        ids, z, R = self.padded(scans, max(len(sc[0]) for sc in scans.values() if sc is not None) + int(rng.integers(0, 4)))
        for b in which:
            assert match_rounds_definite(self.models[b].x, self.models[b].P, z[b], R[b], ids[b], self.window), "S of a round is not clearly definite"
        # (a single-index call on a batch exports first, for the siblings' sake; the batch form makes up for it)
        res = self.emit("match", index=index, z=z, R=R, ids=ids, window=self.window,
                        settle=bool(index is not None and self.B > 1 or rng.random() < (0.5 if self.B == 1 else 0.2)) and not self.force_open)
        assert [r[1] for r in res] == [int((ids[b] >= 0).sum()) for b in which], "the reference did not apply every measurement"
        self.twin_point("match")

    def do_compat(self, index):
        """ekf_joint_compat as a read-only probe: up to 32 pairings with the true associations, and the same with two ids exchanged."""
        rng = self.rng
        index, which, idle = self.match_index(index)
        scans = {b: None if b == idle else self.scan_of(b, int(rng.integers(2, 33))) for b in which}
        if not any(sc is not None for sc in scans.values()):
            self.emit("read", index=int(rng.integers(0, self.B)))
            return
        ids, z, R = self.padded(scans, max(len(sc[0]) for sc in scans.values() if sc is not None) + int(rng.integers(0, 4)))
        swapped = {}
        for b in which:
            swapped[b] = ids[b].copy()
            kept = np.flatnonzero(ids[b] >= 0)
            other = [k for k in kept if ids[b][k] != ids[b][kept[0]]] if len(kept) else []
            if other:  # (a filter with one landmark has nothing to exchange)
                k = int(other[int(rng.integers(0, len(other)))])
                swapped[b][kept[0]], swapped[b][k] = ids[b][k], ids[b][kept[0]]
            m = self.models[b]
            assert all(match_rounds_definite(m.x, m.P, z[b], R[b], h, None) for h in (ids[b], swapped[b])), "S of the hypothesis is not clearly definite"
        self.emit("compat", index=index, z=z, R=R, ids=ids, swapped=swapped, settle=bool(index is not None and self.B > 1 or rng.random() < 0.5))

    def rewrite_maps(self, forced=None):
        """One rewrite or probe of the *_maps deck; forced "state": a state-changing one, "new": a fuse or an extraction."""
        rng, B = self.rng, self.B
        if not self.deck:
            self.deck = [str(k) for k in rng.permutation(MATCH_REWRITES if self.match else MAP_REWRITES + MAP_REWRITES[-3:])]  # (the three newer kinds twice)
        if forced == "new":
            kind = str(rng.choice(["fuse", "extract"]))
        elif forced == "state":
            kind = str(rng.choice(["remove", "transform", "anchor", "extract"]))
        else:
            kind = self.deck.pop()
        index = 0 if B == 1 else (int(rng.integers(1, B)) if rng.random() < 0.4 and not self.force_open else None)
        if kind == "dups":
            self.do_dups(index)
        elif kind == "fuse":
            if (forced or rng.random() < 0.75) and self.do_fuse(index):
                pass
            elif forced:
                self.do_extract(index, True)
            else:  # a fuse of no pair: a no-op, whatever the window holds
                which = range(B) if index is None else [index]
                self.emit("fuse", index=index, pairs={b: np.zeros((0, 2), dtype=np.int64) for b in which}, slack=0.0, window=self.window,
                          settle=bool(index is not None and B > 1 or rng.random() < 0.5))
        elif kind == "extract":
            self.do_extract(index, bool(forced or rng.random() < 0.6))
        elif kind == "match":
            self.do_match(index)
        elif kind == "compat":
            self.do_compat(index)
        else:
            self.deck.append(kind)
            n = len(self.ops)
            self.rewrite()  # (pops it again)
            if kind in ("remove", "transform", "anchor", "reserve", "join") and any(k == kind for k, _ in self.ops[n:]):
                self.twin_point(kind)
        return kind

    def build_maps(self):
        rng = self.rng
        twins_left, twin_end, twin_new = 2, -1, False
        for step in range(N_STEPS):
            self.traffic()
            if step == twin_end:
                self.emit("twin_end")
            due = twins_left == 2 and step == 20 or twins_left >= 1 and step == 30
            self.force_open = self.n_open == 0 and step >= 25 and step != twin_end
            if rng.random() < 0.35 or step in (3, 17) or due or self.force_open:
                # two twins per sequence, one of them at least behind a fuse or an extraction (the second, if the first was not)
                self.twin_wish, self.twin_kind = None, None
                if twins_left and step > twin_end and step + 6 < N_STEPS and (due or rng.random() < 0.4 + 0.03 * step):
                    self.twin_wish = "any" if twin_new or twins_left == 2 and not due else "new"
                self.rewrite_maps("new" if due and self.twin_wish == "new" else "state" if due or self.force_open else None)
                self.twin_wish = None
                if self.twin_kind:
                    twins_left, twin_end, twin_new = twins_left - 1, step + 5, twin_new or self.twin_kind in ("fuse", "extract")
        for b in range(self.B):
            self.emit("read", index=b)
        return self.ops

    def build(self):
        rng = self.rng
        if self.maps:
            return self.build_maps()
        twins_left, twin_end = 2, -1
        for step in range(N_STEPS):
            self.traffic()
            if step == twin_end:
                self.emit("twin_end")
            # two twins per sequence at random rewrite points; a rewrite is made for one at steps 20 / 30 if chance has not
            due = twins_left == 2 and step == 20 or twins_left >= 1 and step == 30
            # ... and one that meets an open window (no export in front of it), should none have come by step 25
            self.force_open = self.n_open == 0 and step >= 25 and step != twin_end
            if rng.random() < 0.2 or step in (3, 17) or due or self.force_open:
                kind = self.rewrite(state_changing=due or self.force_open)
                # a set_state twin behind a rewrite: it runs the next five steps beside the handle, bit for bit
                if twins_left and step > twin_end and step + 6 < N_STEPS and kind in ("remove", "transform", "anchor", "reserve", "join") \
                        and (due or rng.random() < 0.4 + 0.03 * step):
                    self.emit("twin_begin")
                    twins_left, twin_end = twins_left - 1, step + 5
        for b in range(self.B):
            self.emit("read", index=b)
        return self.ops


def make_sequence(seed, profile):
    """The operations of (seed, profile) as a list of (kind, args): create, load, then N_STEPS steps of traffic with a rewrite or
    a probe about every fifth, then a read of every filter.  Per-filter arguments of the rewrites are dicts keyed by filter index;
    `index` None is the batch form.  The *_maps profiles draw from a deck that holds dups, fuse and extract as well (the module docstring)."""
    return _Gen(seed, profile).build()


def ops_equal(a, b):
    """Two sequences, equal value for value."""
    def eq(u, v):
        if isinstance(u, dict):
            return isinstance(v, dict) and u.keys() == v.keys() and all(eq(u[k], v[k]) for k in u)
        if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
            return np.array_equal(np.asarray(u), np.asarray(v))
        return u == v
    return len(a) == len(b) and all(p[0] == q[0] and eq(p[1], q[1]) for p, q in zip(a, b))
