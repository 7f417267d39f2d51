"""The fish model (fish_model.py) pinned on hand-built matrices and on data: the exact removals of an
X-wing by rows and by columns, of a 2-2-2 swordfish and of a jellyfish, and a shape that must fire nothing;
that F_5 does not depend on the order of application; that sizes above 4 add nothing; that no fish removes
a digit of the completion; that F_5 lies inside F_4; and the counts the feature was proposed with."""
import numpy as np
import pytest

import fish_model as F
import grade_model as G
import subsets_model as S
from prop_model import ALL, _closed


def cols(*c):
    return sum(1 << x for x in c)


def matrix(rows, rest=ALL):
    """M_d from {row: columns}; the rows not given hold `rest`."""
    return np.array([[cols(*rows[r]) if r in rows else rest for r in range(9)]], dtype=np.uint16)


def check(before, lost):
    """`lost` {row: columns}: exactly what the fish of `before` remove, with sizes <= 4 and with every size;
    and the state after them loses nothing more."""
    want = [cols(*lost.get(r, ())) for r in range(9)]
    got = F.fish_removals(before)
    assert (got & before).tolist() == [want], [bin(v) for v in (got & before)[0]]
    assert (F.fish_removals(before, kmax=8) & before).tolist() == [want]
    after = before & ~got
    assert not (F.fish_removals(after) & after).any()


def test_x_wing_by_rows():
    """Rows 1 and 5 hold the digit in columns 2 and 7 only: the other rows lose both columns."""
    before = matrix({1: (2, 7), 5: (2, 7)})
    check(before, {r: (2, 7) for r in range(9) if r not in (1, 5)})


def test_x_wing_by_columns():
    """Columns 0 and 4 hold the digit in rows 3 and 8 only: those rows lose every other column."""
    before = matrix({}, rest=ALL & ~cols(0, 4))
    before[0, 3] = before[0, 8] = ALL
    other = tuple(c for c in range(9) if c not in (0, 4))
    check(before, {3: other, 8: other})
    assert np.array_equal(S.transpose(before), matrix({0: (3, 8), 4: (3, 8)}))


def test_swordfish_2_2_2():
    """Three rows with two columns each, over three columns in all."""
    before = matrix({0: (1, 4), 3: (4, 8), 6: (1, 8)})
    check(before, {r: (1, 4, 8) for r in range(9) if r not in (0, 3, 6)})
    # pairs alone see nothing in it
    assert not (F.fish_removals(before, kmax=2) & before).any()


def test_jellyfish():
    before = matrix({0: (0, 3), 2: (3, 5), 4: (5, 7), 7: (0, 7)})
    check(before, {r: (0, 3, 5, 7) for r in range(9) if r not in (0, 2, 4, 7)})
    assert not (F.fish_removals(before, kmax=3) & before).any()


def test_three_rows_over_four_columns_fire_nothing():
    before = matrix({0: (1, 4), 3: (4, 8), 6: (1, 6)})
    check(before, {})


def test_fish_pass_clears_the_digit_of_the_cells():
    """An X-wing of digit 3 by rows on a candidate grid: the cells of the two columns lose digit 3, nothing else."""
    X = np.full((1, 81), ALL, dtype=np.uint16)
    bit = np.uint16(1 << 2)
    for r in (1, 5):
        for c in range(9):
            if c not in (2, 7):
                X[0, 9 * r + c] &= ~bit
    got = F.fish_pass(X)
    want = X.copy()
    for r in range(9):
        if r not in (1, 5):
            want[0, 9 * r + 2] &= ~bit
            want[0, 9 * r + 7] &= ~bit
    assert np.array_equal(got, want)
    assert F.digit_matrix(X, 2)[0].tolist() == [ALL if r not in (1, 5) else cols(2, 7) for r in range(9)]


@pytest.fixture(scope="module")
def pool4():
    """The level-4 boards of grade_model's pool: (boards, sol, open4, open5, F_4, F_5 from F_4)."""
    boards, sol, level, open_, open4, open5 = F.pool()
    rows = level == 4
    X = G.candidates(boards[rows])
    F4, _ = S.fixpoint4(X, order="input")
    F5, passes = F.fixpoint5(X, order="f4")
    print("fish passes from F_4:", passes)
    return boards[rows], sol[rows], open4[rows], open5[rows], F4, F5


def test_three_orders_one_state(pool4):
    boards, sol, open4, open5, F4, F5 = pool4
    assert len(boards) == 296
    assert np.array_equal((~_closed(F5)).sum(axis=1), open5)
    for order in ("fish", "mixed"):
        other, passes = F.fixpoint5(G.candidates(boards), order=order)
        print(order, "passes:", passes)
        assert np.array_equal(other, F5), order


def test_sizes_above_four_add_nothing(pool4):
    boards, sol, open4, open5, F4, F5 = pool4
    wide, _ = F.fixpoint5(G.candidates(boards), kmax=8)
    assert np.array_equal(wide, F5)


def test_the_completion_survives(pool4):
    boards, sol, open4, open5, F4, F5 = pool4
    assert ((F5 >> (sol.astype(np.uint16) - 1)) & 1).all()
    assert (F5 != 0).all() and (F5 <= ALL).all()


def test_f5_lies_inside_f4(pool4):
    boards, sol, open4, open5, F4, F5 = pool4
    assert not (F5 & ~F4).any() and (open5 <= open4).all()


def counts(boards, level, open4, open5):
    """(level-4 boards, F_5 != F_4, open5 < open4, open4 == 0, open5 == 0) and F_4, F_5 of the level-4 rows."""
    rows = np.flatnonzero(level == 4)
    X = G.candidates(boards[rows])
    F4, _ = S.fixpoint4(X, order="input")
    F5, passes = F.fixpoint5(X)
    assert passes <= 3
    assert np.array_equal((~_closed(F4)).sum(axis=1), open4[rows])
    assert np.array_equal((~_closed(F5)).sum(axis=1), open5[rows])
    assert (open5[level != 4] == F.NONE).all()
    o4, o5 = open4[rows], open5[rows]
    return (len(rows), int((F5 != F4).any(axis=1).sum()), int((o5 < o4).sum()), int((o4 == 0).sum()),
            int((o5 == 0).sum())), rows, X, F5


def test_counts_on_the_pool_and_on_minimal_puzzles():
    boards, sol, level, open_, open4, open5 = F.pool()
    assert counts(boards, level, open4, open5)[0] == (296, 24, 7, 38, 39)
    boards, sol, level, open_, open4, open5 = F.minimal()
    assert counts(boards, level, open4, open5)[0] == (934, 65, 14, 143, 145)


def test_counts_and_rows_on_8192_minimal_puzzles():
    """make_minimal(8192): the table's line, the rows that need a fish, a swordfish, a jellyfish.

    The line the feature was proposed with reads (3770, 308, 64, 552, 565).  Its 64 came from an alternation
    that re-entered subsets_model.fixpoint4(order="input") after each fish pass: on a state that is not an
    input row that order stops at an unchanged subset pass without trying locked candidates.  On row 2806 a
    fish enables a locked candidate and no subset: the state that alternation left (46 open cells, as F_4) is
    not a fixpoint of R5; F_5 has 43.  Every other figure of the three lines is the same either way."""
    boards, sol, level, open_, open4, open5 = F.minimal(8192)
    got, rows, X, F5 = counts(boards, level, open4, open5)
    assert got == (3770, 308, 65, 552, 565)
    assert (open4[2806], open5[2806]) == (46, 43)
    stale, _ = S.fixpoint4(F.fish_pass(S.fixpoint4(G.candidates(boards[2806:2807]), order="input")[0]), order="input")
    assert (~_closed(stale)).sum() == 46 and (stale != F5[rows == 2806]).any()
    o4, o5 = open4[rows], open5[rows]
    assert tuple(rows[(o4 > 0) & (o5 == 0)]) == F.NEEDS_FISH_8192
    assert o5[o5 > 0].min() == 11
    assert ((F5 >> (sol[rows].astype(np.uint16) - 1)) & 1).all()
    F2, _ = F.fixpoint5(X, kmax=2)
    F3, _ = F.fixpoint5(X, kmax=3)
    d2 = (F2 != F5).any(axis=1)
    assert d2.sum() == 59 and ((~_closed(F2)).sum(axis=1) != o5).sum() == 7
    assert tuple(rows[d2][:8]) == F.SWORDFISH_8192
    d3 = (F3 != F5).any(axis=1)
    assert tuple(rows[d3]) == F.JELLYFISH_8192 and np.array_equal((~_closed(F3)).sum(axis=1), o5)
    other, _ = F.fixpoint5(X[:1000], order="fish")
    assert np.array_equal(other, F5[:1000])
