"""The wings model (wings_model.py) pinned on hand-built candidate states and on data: the exact removals of
an XY-wing, of an XYZ-wing (only from cells that see all three), of a colour trap and of a colour wrap; near
misses that must fire nothing; that F_6 does not depend on the order of application; that no rule removes a
digit of the completion; that F_6 lies inside F_5; and every count the feature was proposed with."""
import numpy as np
import pytest

import fish_model as F
import grade_model as G
import wings_model as W
from prop_model import ALL, _closed


def bits(*digits):
    return sum(1 << (d - 1) for d in digits)


def cell(r, c):
    return 9 * r + c


def state(cells):
    """{(r, c): digits}: a candidate state, every other cell holding all nine digits."""
    X = np.full((1, 81), ALL, dtype=np.uint16)
    for (r, c), digits in cells.items():
        X[0, cell(r, c)] = bits(*digits)
    return X


def places(d, where):
    """A state in which digit d is a candidate of the cells `where` only."""
    X = np.full((1, 81), ALL & ~bits(d), dtype=np.uint16)
    for r, c in where:
        X[0, cell(r, c)] = ALL
    return X


def check(before, lost, digit, passes=(W.wing_pass, W.colour_pass, W.wide_pass)):
    """`lost` cells lose `digit` and nothing else changes, under the first of `passes` and under the whole
    W + C pass (the last); the others change nothing."""
    want = before.copy()
    for r, c in lost:
        assert want[0, cell(r, c)] & bits(digit)
        want[0, cell(r, c)] &= ALL & ~bits(digit)
    fire, quiet, both = passes
    assert np.array_equal(fire(before), want), np.flatnonzero(fire(before) != want)
    assert np.array_equal(quiet(before), before)
    assert np.array_equal(both(before), want)


def test_xy_wing():
    """Pivot (0,0) = {1,2}, pincers (0,4) = {1,3} and (4,0) = {2,3}: the one cell that sees both pincers,
    (4,4), loses 3."""
    check(state({(0, 0): (1, 2), (0, 4): (1, 3), (4, 0): (2, 3)}), [(4, 4)], 3)


def test_xyz_wing_removes_only_from_cells_that_see_all_three():
    """Pivot (1,1) = {1,2,3}, pincers (0,0) = {1,3} in its box and (1,5) = {2,3} in its row.  (1,0) and (1,2)
    see all three and lose 3; (0,3), (0,4) and (0,5) see both pincers but not the pivot and keep it."""
    before = state({(1, 1): (1, 2, 3), (0, 0): (1, 3), (1, 5): (2, 3)})
    check(before, [(1, 0), (1, 2)], 3)
    assert np.array_equal(W.wing_pass(before, xyz=False), before)
    for c in (3, 4, 5):
        assert W.PEERS[cell(0, 0)] >> cell(0, c) & 1 and W.PEERS[cell(1, 5)] >> cell(0, c) & 1
        assert not W.PEERS[cell(1, 1)] >> cell(0, c) & 1


TRAP = [(0, 0), (0, 5), (6, 5), (7, 3), (7, 0), (3, 0), (7, 8)]


def test_colour_trap():
    """Links: row 0 (0,0)-(0,5), column 5 (0,5)-(6,5), box 7 (6,5)-(7,3).  Colours {(0,0), (6,5)} and
    {(0,5), (7,3)}.  (7,0) sees (0,0) down its column and (7,3) along its row: it loses the digit.  (3,0) and
    (7,8) keep column 0 and row 7 from being links and see one colour only."""
    before = places(5, TRAP)
    assert W.colour_components(sum(1 << cell(r, c) for r, c in TRAP)) == [
        (1 << cell(0, 0) | 1 << cell(6, 5), 1 << cell(0, 5) | 1 << cell(7, 3))]
    check(before, [(7, 0)], 5, passes=(W.colour_pass, W.wing_pass, W.wide_pass))
    assert np.array_equal(W.colour_pass(before, wrap=False), W.colour_pass(before))


WRAP = [(0, 0), (0, 4), (5, 4), (5, 1), (2, 1), (1, 2)]


def test_colour_wrap():
    """Links: row 0, column 4, row 5, column 1: (0,0) A, (0,4) B, (5,4) A, (5,1) B, (2,1) A.  (0,0) and (2,1)
    share box 0, which (1,2) keeps from being a link: every place of colour A loses the digit, (1,2) sees A
    only and keeps it."""
    before = places(7, WRAP)
    check(before, [(0, 0), (5, 4), (2, 1)], 7, passes=(W.colour_pass, W.wing_pass, W.wide_pass))
    assert np.array_equal(W.colour_pass(before, wrap=False), before)


@pytest.mark.parametrize("cells", [
    {(0, 0): (1, 2), (0, 4): (1, 3), (4, 0): (1, 3)},             # Q == R
    {(0, 0): (1, 2), (0, 4): (1, 3), (4, 0): (2, 4)},             # pincers with no common digit
    {(0, 0): (1, 2, 3, 4), (0, 4): (1, 3), (4, 0): (2, 3)},       # a pivot with four candidates
    {(1, 1): (1, 2, 3, 4), (0, 0): (1, 3), (1, 5): (2, 3)},       # the same around an XYZ shape
    {(0, 0): (1, 2), (0, 4): (1, 3), (4, 5): (2, 3)},             # a pincer that is not a peer of the pivot
], ids=["same-pincers", "no-common-digit", "pivot-of-four", "xyz-pivot-of-four", "pincer-not-a-peer"])
def test_wing_near_misses(cells):
    before = state(cells)
    assert np.array_equal(W.wide_pass(before), before)


@pytest.mark.parametrize("where", [
    TRAP + [(0, 7)],                                    # row 0 has three places: no link, (7,0) sees one colour
    [(0, 0), (0, 5), (6, 5), (3, 3)],                   # a component without conflict
    [(0, 0), (0, 5), (6, 5), (7, 3)],                   # the trap's component without the trapped cell
], ids=["three-places-no-link", "no-conflict", "nothing-to-trap"])
def test_colour_near_misses(where):
    before = places(5, where)
    assert np.array_equal(W.wide_pass(before), before)


@pytest.fixture(scope="module")
def pool4():
    """The level-4 boards of grade_model's pool: (boards, sol, open5, open6, F_5, F_6 in the kernel's order)."""
    boards, sol, level, open_, open4, open5, open6 = W.pool()
    rows = level == 4
    X = G.candidates(boards[rows])
    F5, _ = F.fixpoint5(X)
    F6, passes = W.fixpoint6(X)
    print("changing wide passes:", np.bincount(passes).tolist())
    return boards[rows], sol[rows], open5[rows], open6[rows], F5, F6


def test_three_orders_one_state(pool4):
    boards, sol, open5, open6, F5, F6 = pool4
    assert len(boards) == 296
    assert np.array_equal((~_closed(F6)).sum(axis=1), open6)
    for order in ("split", "mixed"):
        other, _ = W.fixpoint6(G.candidates(boards), order=order)
        differ = int((other != F6).any(axis=1).sum())
        print(order, "differs from f5 on", differ, "boards")
        assert differ == 0, order
    # F_6 is a fixpoint of every rule of R6
    assert np.array_equal(W.wide_pass(F6), F6) and np.array_equal(F.fixpoint5(F6)[0], F6)


def test_the_completion_survives(pool4):
    boards, sol, open5, open6, F5, F6 = pool4
    assert ((F6 >> (sol.astype(np.uint16) - 1)) & 1).all()
    assert (F6 != 0).all() and (F6 <= ALL).all()


def test_f6_lies_inside_f5(pool4):
    boards, sol, open5, open6, F5, F6 = pool4
    assert not (F6 & ~F5).any() and (open6 <= open5).all()


def counts(data):
    """(level-4 boards, F_6 != F_5, open6 < open5, open5 == 0, open6 == 0, open5 > 0 and open6 == 0), and
    rows, candidates, F_6, changing passes of the level-4 rows."""
    boards, sol, level, open_, open4, open5, open6 = data
    rows = np.flatnonzero(level == 4)
    X = G.candidates(boards[rows])
    F5, _ = F.fixpoint5(X)
    F6, passes = W.fixpoint6(X)
    assert np.array_equal((~_closed(F5)).sum(axis=1), open5[rows])
    assert np.array_equal((~_closed(F6)).sum(axis=1), open6[rows])
    assert (open6[level != 4] == W.NONE).all()
    assert ((F6 >> (sol[rows].astype(np.uint16) - 1)) & 1).all()
    o5, o6 = open5[rows], open6[rows]
    return (len(rows), int((F6 != F5).any(axis=1).sum()), int((o6 < o5).sum()), int((o5 == 0).sum()),
            int((o6 == 0).sum()), int(((o5 > 0) & (o6 == 0)).sum())), rows, X, F6, passes


def test_counts_on_the_pool():
    assert counts(W.pool())[0] == (296, 152, 99, 39, 122, 83)


def test_counts_and_the_rule_split_on_2048_minimal_puzzles():
    """The table's line, the passes a board needs, and what each part of the rule set closes alone."""
    got, rows, X, F6, passes = counts(W.minimal())
    assert got == (934, 423, 254, 145, 348, 203)
    assert np.bincount(passes).tolist() == [511, 365, 53, 4, 1]
    o5, o6 = W.minimal()[5][rows], W.minimal()[6][rows]
    need = o5 > 0

    def closes(**rules):
        Fx, _ = W.fixpoint6(X[need], **rules)
        return (~_closed(Fx)).sum(axis=1) == 0

    xy, wings, colour = closes(xyz=False, colour=False), closes(colour=False), closes(wings=False)
    both = o6[need] == 0
    print("closed by XY-wings", xy.sum(), "wings", wings.sum(), "colouring", colour.sum(), "all", both.sum())
    assert (int(xy.sum()), int(wings.sum()), int(colour.sum()), int(both.sum())) == (87, 99, 96, 203)
    assert int((both & ~wings & ~colour).sum()) == 16 and int((wings & ~xy).sum()) == 12
    r = rows[need]
    assert tuple(r[xy & ~colour][:2]) == W.NEEDS_WINGS_2048
    assert tuple(r[colour & ~wings][:2]) == W.NEEDS_COLOUR_2048
    assert tuple(r[both & ~wings & ~colour][:2]) == W.NEEDS_BOTH_2048
    assert tuple(r[wings & ~xy][:2]) == W.NEEDS_XYZ_2048
    # without the wrap: another open6 on 65 boards
    Fn, _ = W.fixpoint6(X, wrap=False)
    assert int(((~_closed(Fn)).sum(axis=1) != o6).sum()) == 65
    assert o6[o6 > 0].min() == 13
    for order in ("split", "mixed"):
        other, _ = W.fixpoint6(X, order=order)
        assert np.array_equal(other, F6), order


def test_counts_on_8192_minimal_puzzles():
    got, rows, X, F6, passes = counts(W.minimal(8192))
    assert got == (3770, 1797, 1098, 565, 1414, 849)
    o6 = W.minimal(8192)[6][rows]
    assert (o6[o6 > 0].min(), o6.max()) == (13, 56)
    print("share of level-4 boards that need the new rules: %.1f %%" % (100.0 * got[5] / got[0]))
