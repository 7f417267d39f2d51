"""The subsets model (subsets_model.py) pinned on hand-built units and on data: the exact removals of a
naked pair, triple and quad and of a hidden pair and triple; that F_4 does not depend on the order of
application; that sizes above 4 add nothing; that no rule removes a digit of the completion; the counts
the feature was proposed with; and that the inputs of the GPU tests exercise every subset size."""
import numpy as np
import pytest

import grade_model as G
import subsets_model as S
from prop_model import ALL, _closed


def m(*digits):
    return sum(1 << (d - 1) for d in digits)


REST = tuple(range(1, 10))


def unit(*cells):
    """Nine candidate sets; the cells not given hold every digit."""
    cells = list(cells) + [REST] * (9 - len(cells))
    return np.array([[m(*c) for c in cells]], dtype=np.uint16)


def check_unit(before, after):
    got = S.unit_pass(before)
    assert got.tolist() == after.tolist(), ([bin(v) for v in got[0]], [bin(v) for v in after[0]])
    # the hidden side of the same subset (and nothing else) with every size allowed
    assert S.unit_pass(before, kmax=8).tolist() == after.tolist()
    assert S.unit_pass(after).tolist() == after.tolist()


def test_naked_pair():
    rest = (3, 4, 5, 6, 7, 8, 9)
    check_unit(unit((1, 2), (1, 2)), unit((1, 2), (1, 2), *[rest] * 7))


def test_naked_triple_of_pairs():
    rest = (4, 5, 6, 7, 8, 9)
    check_unit(unit((1, 2), (2, 3), (1, 3)), unit((1, 2), (2, 3), (1, 3), *[rest] * 6))


def test_naked_quad():
    rest = (5, 6, 7, 8, 9)
    check_unit(unit((1, 2), (2, 3), (3, 4), (1, 4)), unit((1, 2), (2, 3), (3, 4), (1, 4), *[rest] * 5))


def test_hidden_pair():
    rest = (3, 4, 5, 6, 7, 8, 9)
    check_unit(unit((1, 2, 3, 4, 5), (1, 2, 6, 7), *[rest] * 7), unit((1, 2), (1, 2), *[rest] * 7))


def test_hidden_triple():
    rest = (4, 5, 6, 7, 8, 9)
    check_unit(unit((1, 2, 4, 5), (2, 3, 6), (1, 3, 7, 8, 9), *[rest] * 6),
               unit((1, 2), (2, 3), (1, 3), *[rest] * 6))


def test_size_one_is_the_singles():
    """k = 1: a closed cell clears its digit from the unit (N), a digit with one place closes it (H)."""
    before = unit((5,), (1, 5, 6), (2, 5, 7))
    got = S.unit_pass(before, kmax=1)
    rest = m(1, 2, 3, 4, 6, 7, 8, 9)
    assert got.tolist() == [[m(5), m(1, 6), m(2, 7)] + [rest] * 6]
    before = unit((1, 2, 3), *[(2, 3, 4, 5, 6, 7, 8, 9)] * 8)
    assert S.unit_pass(before, kmax=1).tolist() == [[m(1)] + [m(2, 3, 4, 5, 6, 7, 8, 9)] * 8]


def test_transpose_is_an_involution():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, ALL + 1, size=(50, 9)).astype(np.uint16)
    assert np.array_equal(S.transpose(S.transpose(rows)), rows)
    assert S.transpose(unit((1, 2), (2,)))[0, :3].tolist() == [0x1FD, 0x1FF, 0x1FC]


@pytest.fixture(scope="module")
def pool4():
    """The level-4 boards of grade_model's pool: (boards, sol, open, F_4 from F_3)."""
    boards, sol, level, open_, open4 = S.pool()
    rows = level == 4
    F, passes = S.fixpoint4(G.candidates(boards[rows]), order="f3")
    print("subset passes from F_3:", passes)
    return boards[rows], sol[rows], open_[rows], open4[rows], F


def test_three_orders_one_state(pool4):
    boards, sol, open_, open4, F = pool4
    assert len(boards) == 296
    assert np.array_equal((~_closed(F)).sum(axis=1), open4)
    for order in ("input", "mixed"):
        other, passes = S.fixpoint4(G.candidates(boards), order=order)
        print(order, "passes:", passes)
        assert np.array_equal(other, F), order


def test_sizes_above_four_add_nothing(pool4):
    boards, sol, open_, open4, F = pool4
    wide, _ = S.fixpoint4(G.candidates(boards), kmax=8)
    assert np.array_equal(wide, F)


def test_the_completion_survives(pool4):
    boards, sol, open_, open4, F = pool4
    assert ((F >> (sol.astype(np.uint16) - 1)) & 1).all()
    assert (F != 0).all() and (F <= ALL).all()


def test_counts_on_the_pool(pool4):
    boards, sol, open_, open4, F = pool4
    print("open4 == 0:", (open4 == 0).sum(), "open4 < open:", (open4 < open_).sum())
    assert (open4 <= open_).all()
    assert (open4 == 0).sum() == 38 and (open4 < open_).sum() == 95


def test_counts_on_minimal_puzzles_and_every_size_path():
    """make_minimal(2048): 934 boards of level 4, 143 of them closed by subsets; and the inputs of the
    GPU tests (this set and the pool) need every size: boards that close with sizes <= 3 but not with
    pairs alone, and a board whose count differs between sizes <= 3 and <= 4."""
    boards, sol, level, open_, open4 = S.minimal()
    rows = level == 4
    assert rows.sum() == 934 and (open4[rows] == 0).sum() == 143
    assert (open4[~rows] == S.NONE).all() and (open4[rows] < open_[rows]).sum() == 339
    pairs = S.open4_of(boards, level, kmax=2)
    triples = S.open4_of(boards, level, kmax=3)
    need3 = np.flatnonzero((triples == 0) & (pairs != 0))
    need4 = np.flatnonzero(triples != open4)
    print("pairs close", (pairs[rows] == 0).sum(), "sizes <= 3 close", (triples[rows] == 0).sum())
    print("closed only with a triple:", need3, "count differs with quads:", need4)
    assert (pairs[rows] == 0).sum() == 135 and (triples[rows] == 0).sum() == 143
    assert len(need3) >= 3 and {9, 34, 47} <= set(need3.tolist())
    assert len(need4) >= 1
