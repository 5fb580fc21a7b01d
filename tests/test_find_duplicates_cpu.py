"""CPU tests of the duplicate search (ekf_find_duplicates / ekf_batch_find_duplicates): the header declares the calls and the struct
and the binding lists them; the pair enumeration the tile kernel runs (ekf_device.h: dup_tile_count, dup_tile_ij, dup_pair) is
checked by brute force (tests/cpp/dup_map_check.cpp); the NumPy reference the GPU tests compare with (tests/dup_ref.py) is checked
against its own restatement in extended precision; the state builder plants pairs with the d2 it was asked for, and its states fail
a gate that ignores the cross blocks; duplicate_keep_mask on hand-made lists."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dup_ref as dr  # noqa: E402
from helpers import run_cpp_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (23, 24, 25, 92, 172, 272)  # + 8 planted landmarks: the GPU tests' 31, 32, 33, 100, 180, 280


def built(pkg, N, seed=5):
    x, P = pkg.scenarios.injected_state(N, seed=seed, extent=12.0 * (N / 64.0) ** 0.5 + 8.0)
    return dr.with_duplicates(x, P, seed=seed + 1)


def test_header_declares_and_binding_lists_the_calls(pkg):
    raw = open(os.path.join(ROOT, "include", "ekfslam_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("ekf_find_duplicates", "ekf_batch_find_duplicates"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in pkg.ekfslam.ABI_SYMBOLS, name
    assert re.search(r"typedef struct ekf_dup_pair\s*\{\s*int i, j;\s*double d2;\s*\}\s*ekf_dup_pair;", src)
    E = pkg.ekfslam
    assert E.DUP_DTYPE.itemsize == 16 and E.DUP_DTYPE == dr.DUP_DTYPE and [f[0] for f in E.EkfDupPair._fields_] == ["i", "j", "d2"]
    assert callable(pkg.FilterBatch.find_duplicates) and callable(pkg.KalmanFilter.find_duplicates) and callable(E.duplicate_keep_mask)


def test_pair_enumeration_agrees_with_brute_force(tmp_path):
    out = run_cpp_check(tmp_path, "dup_map_check")
    # N in {1, 2, 31, 32, 33, 64, 65, 100} x the valid, distinct splits of {0, 1, 31, 32, 33, N - 1, N}
    assert out.returncode == 0 and "dup map ok (39 cases)" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("N", SIZES)
def test_reference_against_extended_precision(pkg, N):
    x, P, _ = built(pkg, N)
    for max_dist, split in ((None, 0), (1.0, 0), (None, (N + 8) // 2), (0.05, 3)):
        got, gdeg = dr.find(x, P, dr.GATE, max_dist, split)
        want, wdeg = dr.find(x, P, dr.GATE, max_dist, split, dtype=np.longdouble)
        assert got["i"].tolist() == want["i"].tolist() and got["j"].tolist() == want["j"].tolist() and gdeg == wdeg == 0
        _, _, t64 = dr.find(x, P, dr.GATE, max_dist, split, with_terms=True)
        _, _, tld = dr.find(x, P, dr.GATE, max_dist, split, dtype=np.longdouble, with_terms=True)
        err = float((np.abs(t64["d2"] - tld["d2"]) / np.maximum(np.abs(tld["d2"]), 1e-300)).max())
        print("N=%d max_dist=%s split=%d: %d pairs, worst relative error of d2 over all pairs %.3e" % (N + 8, max_dist, split, len(got), err))
        assert err <= 1e-9


@pytest.mark.parametrize("N", SIZES)
def test_builder_plants_the_targets(pkg, N):
    x, P, planted = built(pkg, N)
    assert len(x) == 3 + 2 * (N + 8) and np.array_equal(P, P.T)
    lo = np.linalg.eigvalsh(P).min()
    pairs, deg = dr.find(x, P, dr.GATE)
    listed = {(int(p["i"]), int(p["j"])): float(p["d2"]) for p in pairs}
    _, _, t = dr.find(x, P, dr.GATE, with_terms=True)
    every = {(int(i), int(j)): float(d) for i, j, d in zip(t["i"], t["j"], t["d2"])}
    for i, j, target in planted:
        got = every[(i, j)]
        assert abs(got - target) <= 1e-8 * max(target, 1.0), (i, j, got, target)
        assert ((i, j) in listed) == (target <= dr.GATE)
    natural = len(pairs) - sum(1 for p in planted if p[2] <= dr.GATE)
    print("N=%d: smallest eigenvalue %.3e, %d listed pairs of which %d natural, %d degenerate" % (N + 8, lo, len(pairs), natural, deg))
    assert lo > 1e-5 and deg == 0 and natural >= 0
    tiles = {(i // 32, j // 32) for i, j, _ in planted}
    if N + 8 > 64:
        assert any(a != b for a, b in tiles)  # the permutation puts planted pairs into off-diagonal tiles
    m_gate, m_dist = dr.margins(x, P, dr.GATE, 1.0)
    assert m_gate > 1e-3 and m_dist > 1e-3, (m_gate, m_dist)


@pytest.mark.parametrize("N", SIZES)
def test_a_gate_without_the_cross_blocks_returns_another_list(pkg, N):
    x, P, planted = built(pkg, N)
    full, _ = dr.find(x, P, dr.GATE)
    blind, _ = dr.find(x, dr.without_cross_blocks(P), dr.GATE)
    a = [(int(p["i"]), int(p["j"])) for p in full]
    b = [(int(p["i"]), int(p["j"])) for p in blind]
    print("N=%d: %d pairs with the cross blocks, %d without, %d in both" % (N + 8, len(a), len(b), len(set(a) & set(b))))
    assert a != b


def test_exact_copy_is_degenerate(pkg):
    x, P = pkg.scenarios.injected_state(40, seed=9, extent=15.0)
    x1, P1, planted = dr.with_duplicates(x, P, seed=10, exact=1)
    pairs, deg = dr.find(x1, P1, dr.GATE)
    listed = {(int(p["i"]), int(p["j"])) for p in pairs}
    i, j, target = planted[-1]
    assert target is None and deg == 1 and (i, j) not in listed
    for i, j, target in planted[:-1]:  # the other pairs are not disturbed
        assert ((i, j) in listed) == (target <= dr.GATE)


def pairs_of(rows):
    return np.array(rows, dtype=dr.DUP_DTYPE)


def test_keep_mask_on_hand_made_lists(pkg):
    mask = pkg.ekfslam.duplicate_keep_mask
    assert mask(pairs_of([]), 5).tolist() == [True] * 5
    assert mask(pairs_of([(1, 3, 0.5)]), 5).tolist() == [True, True, True, False, True]
    # a chain 0-1-2: the closer link wins, the other one is refused (1 is matched), 2 stays
    assert mask(pairs_of([(0, 1, 2.0), (1, 2, 1.0)]), 4).tolist() == [True, True, False, True]
    assert mask(pairs_of([(0, 1, 1.0), (1, 2, 2.0)]), 4).tolist() == [True, False, True, True]
    # ties in d2 fall by (i, j): (0, 2) before (1, 2)
    assert mask(pairs_of([(1, 2, 1.0), (0, 2, 1.0), (1, 3, 1.0)]), 4).tolist() == [True, True, False, False]
    # the order of the list does not matter
    rows = [(0, 4, 3.0), (1, 4, 0.1), (2, 3, 0.2), (0, 3, 0.15)]
    want = mask(pairs_of(rows), 6).tolist()
    assert want == [True, True, True, False, False, True]
    assert mask(pairs_of(rows[::-1]), 6).tolist() == want
    # a truncated list (the leading pairs by (i, j)) is a valid input: fewer matches, never a landmark dropped twice
    assert mask(pairs_of(sorted(rows)[:2]), 6).tolist() == [True, True, True, False, True, True]
    with pytest.raises(ValueError):
        mask(pairs_of([(2, 2, 0.0)]), 4)
    with pytest.raises(ValueError):
        mask(pairs_of([(1, 4, 0.0)]), 4)
