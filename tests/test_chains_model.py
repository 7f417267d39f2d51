"""The chains model (chains_model.py) pinned on hand-built candidate states and on data: the exact removals of
a skyscraper, of a two-string kite, of a longer X-chain, of an XY-chain of four cells and of a remote pair;
near misses that must fire nothing; that F_7 does not depend on the order of application; that no rule removes
a digit of the completion; that F_7 lies inside F_6; and every count the feature was proposed with."""
import numpy as np
import pytest

import chains_model as C
import grade_model as G
import wings_model as W
from prop_model import ALL, _closed
from test_wings_model import bits, cell, places, state


def lose(before, lost, *digits):
    """`before` with the cells `lost` losing `digits` (each holds them)."""
    want = before.copy()
    for r, c in lost:
        assert want[0, cell(r, c)] & bits(*digits) == bits(*digits)
        want[0, cell(r, c)] &= ALL & ~bits(*digits)
    return want


def check(before, want, fire, quiet):
    """`fire` (x or xy) alone and the whole X + Y pass give `want`; `quiet` alone changes nothing."""
    on = {"x": dict(x=True, xy=False), "xy": dict(x=False, xy=True)}
    got = C.chain_pass(before, **on[fire])
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert np.array_equal(C.chain_pass(before, **on[quiet]), before)
    assert np.array_equal(C.chain_pass(before), want)


# rows 0 and 5 are links with one end each in column 1, itself a link; the other ends (0,7) and (5,8) are seen
# together by (1,8), (2,8) (box 2, column 8) and (3,7), (4,7) (column 7, box 5).  Those four keep columns 7 and 8
# and boxes 2 and 5 from being links.
SKYSCRAPER = [(0, 1), (0, 7), (5, 1), (5, 8), (1, 8), (2, 8), (3, 7), (4, 7)]


def test_skyscraper():
    """From s = (0,7): ON = {(0,1)}, OFF gains (5,1), the link of row 5 puts (5,8) into ON: either (0,7) or
    (5,8) holds the digit, and the four cells that see both lose it."""
    before = places(5, SKYSCRAPER)
    assert C.xchain_on(sum(1 << cell(r, c) for r, c in SKYSCRAPER), cell(0, 7)) == 1 << cell(0, 1) | 1 << cell(5, 8)
    check(before, lose(before, [(1, 8), (2, 8), (3, 7), (4, 7)], 5), "x", "xy")


def test_two_string_kite():
    """The links of row 0, (0,2)-(0,6), and of column 1, (1,1)-(6,1), meet in box 0: either (0,6) or (6,1)
    holds the digit, and (6,6) sees both.  (6,7) and (7,6) keep row 6, column 6 and box 8 from being links."""
    before = places(3, [(0, 2), (0, 6), (1, 1), (6, 1), (6, 6), (6, 7), (7, 6)])
    check(before, lose(before, [(6, 6)], 3), "x", "xy")


LONG = [(0, 0), (0, 4), (3, 4), (3, 8), (7, 8), (7, 2), (6, 0), (8, 0), (1, 2), (2, 2)]


def test_x_chain_of_six_places():
    """(0,0) - (0,4) - (3,4) - (3,8) - (7,8) - (7,2): the links of row 0, column 4, row 3, column 8 and row 7.
    If (0,0) lacks the digit then (0,4), (3,8) and (7,2) hold it.  (6,0) and (8,0) see (0,0) down column 0 and
    (7,2) in box 6; (1,2) and (2,2) see (0,0) in box 0 and (7,2) down column 2."""
    before = places(9, LONG)
    on = C.xchain_on(sum(1 << cell(r, c) for r, c in LONG), cell(0, 0))
    assert on == 1 << cell(0, 4) | 1 << cell(3, 8) | 1 << cell(7, 2)
    check(before, lose(before, [(6, 0), (8, 0), (1, 2), (2, 2)], 9), "x", "xy")


XY4 = {(0, 0): (1, 2), (0, 5): (2, 3), (4, 5): (3, 4), (4, 8): (4, 1)}


def test_xy_chain_of_four_cells():
    """(0,0) = {1,2}, (0,5) = {2,3}, (4,5) = {3,4}, (4,8) = {4,1}: if (0,0) is not 1 then (4,8) is.  (0,8) and
    (4,0) see both ends and lose 1.  No three of the cells make an XY-wing."""
    before = state(XY4)
    assert C.xychain_ends([int(v) for v in before[0]], cell(0, 0), bits(1)) == 1 << cell(4, 8)
    check(before, lose(before, [(0, 8), (4, 0)], 1), "xy", "x")
    assert np.array_equal(W.wide_pass(before), before)


def test_remote_pair():
    """A = (0,0), B = (0,4), C = (2,5), D = (7,5), all {1,2}: A-B share row 0, B-C box 1, C-D column 5.
    Neighbours in the chain are a naked pair; A and D, three steps apart, hold different digits, so (7,0), which
    sees only those two, loses both digits as well."""
    four = [(0, 0), (0, 4), (2, 5), (7, 5)]
    before = state({rc: (1, 2) for rc in four})
    row0 = [(0, c) for c in range(9)]
    box1 = [(r, c) for r in range(3) for c in range(3, 6)]
    col5 = [(r, 5) for r in range(9)]
    lost = sorted(set(row0 + box1 + col5 + [(7, 0)]) - set(four))
    check(before, lose(before, lost, 1, 2), "xy", "x")


@pytest.mark.parametrize("where", [
    SKYSCRAPER + [(5, 4)],                       # row 5 has three places: no link carries the chain on
    [(0, 1), (0, 7), (5, 1), (5, 8)],            # the skyscraper with no place that sees both ends
], ids=["three-places-no-link", "ends-share-no-place"])
def test_x_chain_near_misses(where):
    before = places(5, where)
    assert np.array_equal(C.chain_pass(before), before)


def test_xy_step_into_a_trivalue_cell():
    before = state({**XY4, (4, 5): (3, 4, 5)})
    assert np.array_equal(C.chain_pass(before), before)


def test_xy_end_that_is_the_start_itself():
    """A = (0,0) = {1,2}, B = (0,5) = {2,3}, C = (5,5) = {3,4}, D = (5,0) = {4,2}, a loop.  From A with z = 1:
    A is 2, B is 3, C is 4, D is 2 -- and D sees A.  Were A allowed as a chain cell, the state (A, 1) would be
    reached and every peer of A would lose 1.  It is not: the peers of A keep 1.  The one removal is A's own 2,
    from the chain B - C - D (either B or D is 2, and A sees both)."""
    before = state({(0, 0): (1, 2), (0, 5): (2, 3), (5, 5): (3, 4), (5, 0): (4, 2)})
    assert C.xychain_ends([int(v) for v in before[0]], cell(0, 0), bits(1)) == 0
    check(before, lose(before, [(0, 0)], 2), "xy", "x")


@pytest.fixture(scope="module")
def pool4():
    """The level-4 boards of grade_model's pool: (boards, sol, open6, open7, F_6, F_7 in the kernel's order,
    changing chain passes)."""
    boards, sol, level, open_, open4, open5, open6, open7 = C.pool()
    rows = level == 4
    X = G.candidates(boards[rows])
    F6, _ = W.fixpoint6(X)
    F7, passes = C.fixpoint7(X)
    return boards[rows], sol[rows], open6[rows], open7[rows], F6, F7, passes


def test_three_orders_one_state(pool4):
    boards, sol, open6, open7, F6, F7, passes = pool4
    assert len(boards) == 296
    assert np.array_equal((~_closed(F7)).sum(axis=1), open7)
    for order in ("split", "mixed"):
        other, _ = C.fixpoint7(G.candidates(boards), order=order)
        differ = int((other != F7).any(axis=1).sum())
        print(order, "differs from f6 on", differ, "boards")
        assert differ == 0, order
    # F_7 is a fixpoint of every rule of R7
    assert np.array_equal(C.chain_pass(F7), F7) and np.array_equal(W.fixpoint6(F7)[0], F7)


def test_the_completion_survives(pool4):
    boards, sol, open6, open7, F6, F7, passes = pool4
    assert ((F7 >> (sol.astype(np.uint16) - 1)) & 1).all()
    assert (F7 != 0).all() and (F7 <= ALL).all()


def test_f7_lies_inside_f6(pool4):
    boards, sol, open6, open7, F6, F7, passes = pool4
    assert not (F7 & ~F6).any() and (open7 <= open6).all()


def counts(data):
    """The table's line for `data`: (level-4 boards, open6 == 0, left open by F_6, (changed, fewer open cells,
    closed) for X alone, for XY alone and for both, open7 == 0), the pass histogram of both, and the rows left
    open with what closes them."""
    boards, sol, level, open_, open4, open5, open6, open7 = data
    rows = np.flatnonzero(level == 4)
    assert (open7[level != 4] == C.NONE).all()
    X = G.candidates(boards[rows])
    F6, _ = W.fixpoint6(X)
    o6 = open6[rows]
    assert np.array_equal((~_closed(F6)).sum(axis=1), o6)
    need = o6 > 0
    line, closed, hist = [], {}, None
    for name, rules in (("x", dict(xy=False)), ("xy", dict(x=False)), ("both", {})):
        F7, passes = C.fixpoint7(F6[need], **rules)
        o7 = (~_closed(F7)).sum(axis=1)
        assert ((F7 >> (sol[rows][need].astype(np.uint16) - 1)) & 1).all() and not (F7 & ~F6[need]).any()
        line.append((int((F7 != F6[need]).any(axis=1).sum()), int((o7 < o6[need]).sum()), int((o7 == 0).sum())))
        closed[name] = o7 == 0
        if name == "both":
            assert np.array_equal(o7, open7[rows][need])
            hist = np.bincount(passes).tolist()
            print("open cells of the boards that stay open:", o7[o7 > 0].min(), "..", o7.max())
    return ((len(rows), int((o6 == 0).sum()), int(need.sum()), *line, int((open7[rows] == 0).sum())), hist,
            rows[need], closed)


def test_counts_on_the_pool():
    line, hist, rows, closed = counts(C.pool())
    assert line == (296, 122, 174, (67, 35, 29), (85, 71, 67), (115, 86, 80), 202)
    assert hist == [59, 97, 15, 3]
    o7 = C.pool()[7]
    assert (o7[(o7 > 0) & (o7 != C.NONE)].min(), o7[o7 != C.NONE].max()) == (24, 55)


def test_counts_and_the_family_split_on_2048_minimal_puzzles():
    line, hist, rows, closed = counts(C.minimal())
    assert line == (934, 348, 586, (228, 107, 67), (271, 214, 198), (399, 281, 248), 596)
    assert hist == [187, 317, 58, 19, 4, 1]
    o7 = C.minimal()[7]
    assert (o7[(o7 > 0) & (o7 != C.NONE)].min(), o7[o7 != C.NONE].max()) == (24, 55)
    x, xy, both = closed["x"], closed["xy"], closed["both"]
    assert tuple(rows[x & ~xy][:2]) == C.NEEDS_X_2048
    assert tuple(rows[xy & ~x][:2]) == C.NEEDS_XY_2048
    assert tuple(rows[both & ~x & ~xy][:2]) == C.NEEDS_XANDXY_2048
    boards, level = C.minimal()[0], C.minimal()[2]
    four = np.flatnonzero(level == 4)
    F7, _ = C.fixpoint7(G.candidates(boards[four]))
    for order in ("split", "mixed"):
        other, _ = C.fixpoint7(G.candidates(boards[four]), order=order)
        assert np.array_equal(other, F7), order
