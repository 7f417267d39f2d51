"""The scalar model of the propagation pass (prop_model.py) is itself sound on the inputs the kernel is
compared on (test_gpu_prop32_model.py): what it solves is the known solution, what it refutes has no
completion, what it hands to the search keeps every completion, and no board comes near the kernel's
step limit.  Runs without a GPU."""
import numpy as np
import pytest

import prop_model as M
from oracle import oracle as O
from prop_inputs import DEFAULT_LC, SNAPSHOT_STEPS, STEP_CAP, model_of, named_set

UNIQUE_SETS = ["minimal", "hard", "17clue", "30clue"]
# every schedule the kernel is compared at; 64: see test_step_cap
SCHEDULES = [DEFAULT_LC, 1, 4, 7 | (1 << 8), 64]


def _run(kind, lc=DEFAULT_LC, handover=True):
    return model_of(kind, lc, handover)


def test_schedule_decoding():
    assert M.schedule(DEFAULT_LC) == (3, 5)
    assert M.schedule(4) == (4, 4) and M.schedule(1) == (1, 1)
    assert M.schedule(7 | (1 << 8)) == (1, 7) and M.schedule(64) == (64, 64)


@pytest.mark.parametrize("kind", UNIQUE_SETS)
def test_unique_sets_solved_or_handed_soundly(kind):
    boards, sol = named_set(kind)
    cls, grids, steps, reason = _run(kind)
    assert steps.max() <= STEP_CAP, steps.max()
    assert not (cls == M.REFUTED).any()               # every board has its one completion
    solved, listed = cls == M.SOLVED, cls == M.LISTED
    assert np.array_equal(grids[solved], sol[solved])
    assert (reason[listed] == M.R_STUCK).all()
    # a handed grid: the solution on its closed cells, the givens among them
    g, s, b = grids[listed], sol[listed], boards[listed]
    assert np.array_equal(g[g != 0], s[g != 0])
    assert np.array_equal(g[b != 0], b[b != 0])
    if kind in ("minimal", "hard"):
        assert solved.sum() >= 100 and listed.sum() >= 100, (solved.sum(), listed.sum())
        assert (np.count_nonzero(g, axis=1) > np.count_nonzero(b, axis=1)).any()   # and some of them grew
    else:
        assert solved.all()


def test_class_counts_of_the_named_sets():
    """The split the comparison rests on (first 300 / 500 rows of the 17- and 30-clue sets: all solved)."""
    c = _run("minimal")[0]
    assert ((c == M.SOLVED).sum(), (c == M.LISTED).sum()) == (818, 682)
    c = _run("hard")[0]
    assert ((c == M.SOLVED).sum(), (c == M.LISTED).sum()) == (195, 1305)


def test_edge_set_against_the_oracle():
    boards, _ = named_set("edge")
    cls, grids, steps, reason = _run("edge")
    assert steps.max() <= STEP_CAP
    ref_out, ref_st, _ = O.naive_solve_batch(boards, threads=8)
    solved, refuted, listed = cls == M.SOLVED, cls == M.REFUTED, cls == M.LISTED
    assert solved.sum() >= 100 and listed.sum() >= 100, (solved.sum(), listed.sum())
    assert refuted.any() and (ref_st[refuted] == 0).all()       # (few here: test_broken_set_against_the_oracle)
    assert np.array_equal(grids[refuted], boards[refuted])
    # a solved board has one completion, so the oracle's first is it
    assert (ref_st[solved] == 1).all() and np.array_equal(grids[solved], ref_out[solved])
    # inexact boards go to the search as they came
    inexact = reason == M.R_INEXACT
    assert inexact.sum() >= 100 and np.array_equal(grids[inexact], boards[inexact])
    # a stuck board's handed grid keeps the oracle's completion (and every other one)
    stuck = (reason == M.R_STUCK) & (ref_st == 1)
    g, s = grids[stuck], ref_out[stuck]
    assert np.array_equal(g[g != 0], s[g != 0])
    b = boards[stuck]
    assert np.array_equal(g[b != 0], b[b != 0])


@pytest.mark.parametrize("handover", [True, False])
def test_broken_set_against_the_oracle(handover):
    """Boards with a wrong given: what the model refutes -- by an empty cell or a missing digit, or at
    handover by a digit closed twice in a unit of a stuck board -- has no completion."""
    boards, _ = named_set("broken")
    cls, grids, steps, reason = _run("broken", handover=handover)
    assert steps.max() <= STEP_CAP
    ref_out, ref_st, _ = O.naive_solve_batch(boards, threads=8)
    refuted, solved = cls == M.REFUTED, cls == M.SOLVED
    assert (reason == M.R_CONTRA).sum() >= 100
    assert (ref_st[refuted] == 0).all() and np.array_equal(grids[refuted], boards[refuted])
    assert (ref_st[solved] == 1).all() and np.array_equal(grids[solved], ref_out[solved])
    if handover:
        assert (reason == M.R_DUP_CLOSED).sum() >= 20
    else:
        assert not (reason == M.R_DUP_CLOSED).any()
        assert np.array_equal(grids[cls == M.LISTED], boards[cls == M.LISTED])


@pytest.mark.parametrize("lc", SCHEDULES)
@pytest.mark.parametrize("kind", ["minimal", "hard", "edge", "broken"])
def test_step_cap(kind, lc):
    """No compared board passes STEP_CAP steps at any schedule but 64.  With a period of 64 the first
    locked-candidates pass follows step 64, so every board that needs one waits at least that long and
    one that needs a second reaches max_steps = 96: no seed avoids that.  The kernel's give-up at
    max_steps is the same for a board in any group (the counter advances while any board is live, the
    board itself is), so the model follows it and those boards are compared as well."""
    cls, grids, steps, reason = _run(kind, lc)
    if lc != 64:
        assert steps.max() <= STEP_CAP, steps.max()
        assert not (reason == M.R_MAX_STEPS).any()
    else:
        assert steps.max() <= 96
        assert (steps[reason == M.R_STUCK] == 64).all() and (steps[reason == M.R_MAX_STEPS] == 96).all()


@pytest.mark.parametrize("kind", ["minimal", "hard", "edge", "broken"])
def test_schedule_changes_no_class_and_no_grid(kind):
    """(Which of the two refutations meets a board without a completion first may change.)"""
    base = _run(kind)
    for lc in (1, 4, 7 | (1 << 8)):
        cls, grids, _, reason = _run(kind, lc)
        assert np.array_equal(cls, base[0]) and np.array_equal(grids, base[1])


@pytest.mark.parametrize("kind", ["minimal", "edge", "broken"])
def test_without_handover(kind):
    boards, _ = named_set(kind)
    c1, g1, s1, r1 = _run(kind)
    c0, g0, s0, r0 = _run(kind, handover=False)
    assert np.array_equal(c0 == M.SOLVED, c1 == M.SOLVED)
    assert np.array_equal(c0 == M.LISTED, (c1 == M.LISTED) | (r1 == M.R_DUP_CLOSED))
    assert np.array_equal(g0[c0 == M.LISTED], boards[c0 == M.LISTED])
    assert np.array_equal(s0, s1)


@pytest.mark.parametrize("kind", ["minimal", "hard"])
def test_snapshots_grow_towards_the_fixpoint(kind):
    """tail_step: every board still live at that step is handed over as it stands.  Decided boards are
    the ones decided by then, a snapshot's closed cells are the solution's and contain the earlier
    snapshot's, and the snapshots differ from step to step (so each one pins its own step)."""
    boards, sol = named_set(kind)
    full = model_of(kind)
    prev = boards
    for k in SNAPSHOT_STEPS:
        cls, grids, steps, reason = model_of(kind, tail_step=k)
        early = full[2] <= k            # decided, or found stuck, at step k or before
        assert np.array_equal(cls[early], full[0][early]) and np.array_equal(grids[early], full[1][early])
        tail = reason == M.R_TAIL
        assert np.array_equal(tail, ~early) and (steps[tail] == k).all()
        assert tail.sum() >= 100
        g = grids[tail]
        assert np.array_equal(g[g != 0], sol[tail][g != 0])
        assert np.array_equal(g[prev[tail] != 0], prev[tail][prev[tail] != 0])
        assert (np.count_nonzero(g, axis=1) > np.count_nonzero(prev[tail], axis=1)).sum() >= 50, k
        prev = np.where(tail[:, None], grids, prev)


def test_one_board_is_its_row_of_the_batch():
    """No value of one board reaches another: a board alone gives its row of the batch's result."""
    boards = np.concatenate([named_set("minimal")[0][:40], named_set("edge")[0][:60]])
    cls, grids, steps, reason = M.propagate_batch(boards)
    perm = np.random.default_rng(1).permutation(len(boards))
    pc, pg, ps, pr = M.propagate_batch(boards[perm])
    assert np.array_equal(pc, cls[perm]) and np.array_equal(pg, grids[perm]) and np.array_equal(ps, steps[perm])
    for i in range(len(boards)):
        c, g, s, r = M.propagate(boards[i])
        assert (c, s, r) == (cls[i], steps[i], reason[i]) and np.array_equal(g, grids[i]), i


# ---------------------------------------------------------------- the rules on hand-made boards
SOL = np.array([[(3 * (r % 3) + r // 3 + c) % 9 + 1 for c in range(9)] for r in range(9)], dtype=np.uint8).reshape(81)


def test_rules_complete_grid_and_empty_board():
    c, g, s, r = M.propagate(SOL)
    assert (c, s) == (M.SOLVED, 0) and np.array_equal(g, SOL)
    c, g, s, r = M.propagate(np.zeros(81, dtype=np.uint8))
    assert (c, r) == (M.LISTED, M.R_STUCK) and not g.any()
    assert s == 3                                    # found stuck by the first pass, after step 3
    assert M.propagate(np.zeros(81, dtype=np.uint8), 1, 7)[2] == 1


def test_rules_naked_and_hidden_single():
    b = SOL.copy()
    b[40] = 0                                        # one open cell: closed at step 0, solved at step 1
    c, g, s, r = M.propagate(b)
    assert (c, s) == (M.SOLVED, 1) and np.array_equal(g, SOL)
    # a hidden single only: digit d placed in rows 1, 2 and columns 1, 2 around box 0, whose other
    # cells but (0, 0) are closed by other digits -- (0, 0) takes d although it has other candidates
    b = np.zeros(81, dtype=np.uint8)
    b[9 * 1 + 3], b[9 * 2 + 6], b[9 * 3 + 1], b[9 * 6 + 2] = 5, 5, 5, 5
    c, g, s, r = M.propagate(b)
    assert c == M.LISTED and g[0] == 5
    assert np.count_nonzero(g) == 5


def test_rules_inexact_and_contradiction():
    b = SOL.copy()
    b[3] = 10
    assert M.propagate(b)[::3] == (M.LISTED, M.R_INEXACT)
    b = np.zeros(81, dtype=np.uint8)
    b[0] = b[8] = 7                                  # a digit given twice in a row
    c, g, s, r = M.propagate(b)
    assert (c, r) == (M.LISTED, M.R_INEXACT) and np.array_equal(g, b)
    b = SOL.copy()
    b[0] = 0
    b[1] = SOL[0]                                    # (row 0 now holds SOL[0] twice: inexact, not refuted)
    assert M.propagate(b)[3] == M.R_INEXACT
    # cell 0 sees all nine digits, no unit holds one twice: refuted at step 1 (empty cell)
    b = np.zeros(81, dtype=np.uint8)
    b[1:9] = [1, 2, 3, 4, 5, 6, 7, 8]
    b[9] = 9
    c, g, s, r = M.propagate(b)
    assert (c, r, s) == (M.REFUTED, M.R_CONTRA, 1) and np.array_equal(g, b)


def test_rules_pointing_needs_the_locked_pass():
    """Rows 1 and 2 of box 0 are closed with 2..7, so 1, 8 and 9 of box 0 are confined to row 0 and
    row 0's cells outside the box lose them (pointing): cell (0, 8), which column 8 leaves at
    {1, 7, 8, 9}, closes to 7 -- by the locked-candidates pass only."""
    b = np.zeros(81, dtype=np.uint8)
    b[9:12] = [2, 3, 4]
    b[18:21] = [5, 6, 7]
    for r, v in zip(range(3, 8), (2, 3, 4, 5, 6)):
        b[9 * r + 8] = v
    c, g, s, r = M.propagate(b)
    assert c == M.LISTED and r == M.R_STUCK
    assert g[8] == 7
    c, g, s, r = M.propagate(b, lc_first=64, lc_every=64, max_steps=10)    # given up before any pass
    assert (c, r, s) == (M.LISTED, M.R_MAX_STEPS, 10) and g[8] == 0
