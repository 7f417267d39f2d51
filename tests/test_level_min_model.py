"""The model of level-minimal clue removal (level_min_model.py) against the figures it was designed
on: rows 0..255 of the default stream, each grid in its own removal order.  Runs on the CPU."""
import functools

import numpy as np
import pytest

import grade_model as G
import level_min_model as M
from distributed_sudoku_solver_amd import synth

LEVELS = (1, 2, 3)
# per cap L: the results' levels (1, 2, 3) and their clues (min, mean to one decimal, max)
TABLE = {1: ((256, 0, 0), (22, 25.7, 29)),
         2: ((3, 253, 0), (22, 24.5, 28)),
         3: ((2, 197, 57), (21, 24.5, 28))}


stream = M.stream_rows
reduced = M.stream_reduced


@functools.lru_cache(maxsize=None)
def puzzles():
    """(512 uniqueness-minimal puzzles, their model levels); read-only."""
    p, _ = synth.make_minimal(512)
    lv, _ = G.grade(p)
    p.setflags(write=False)
    return p, lv


def removable(out, L):
    """bool[n,81]: the clue at that cell can go under R_L."""
    can = np.zeros(out.shape, dtype=bool)
    for c in range(81):
        idx = np.flatnonzero(out[:, c] != 0)
        trial = out[idx].copy()
        trial[:, c] = 0
        can[idx, c] = M.closes(trial, L)
    return can


@pytest.mark.parametrize("L", LEVELS)
def test_table(L):
    out, st = reduced(L)
    assert (st == 1).all()
    lv, _ = G.grade(out)
    clues = (out != 0).sum(axis=1)
    got = (tuple(int((lv == k).sum()) for k in (1, 2, 3)), (int(clues.min()), round(float(clues.mean()), 1),
                                                           int(clues.max())))
    print(L, got)
    assert got == TABLE[L]
    assert (lv <= L).all()


@pytest.mark.parametrize("which", ["own", "identity", "reversed"])
@pytest.mark.parametrize("L", LEVELS)
def test_results_are_level_minimal(L, which):
    g, _ = stream()
    out, st = reduced(L, which)
    assert (st == 1).all()
    # a subset of the grid's cells, with the grid's digits
    assert ((out == 0) | (out == g)).all()
    assert (G.grade(out)[0] <= L).all() and M.closes(out, L).all()
    assert not removable(out, L).any()


@pytest.mark.parametrize("L", LEVELS)
def test_minimal_puzzles_come_back_unchanged(L):
    """A uniqueness-minimal puzzle of level <= L is L-minimal already (status 1, nothing goes); one of a
    higher level is not eligible (status 0, nothing is tried)."""
    p, lv = puzzles()
    assert (lv <= L).any() and (lv > L).any()
    _, o = stream()
    order = np.tile(o, (2, 1))
    out, st = M.reduce_level(p, order, L)
    assert np.array_equal(out, p)
    assert np.array_equal(st, (lv <= L).astype(np.int8))


def test_ineligible_boards_come_back_byte_for_byte():
    g, o = stream()
    out3, _ = reduced(3)
    boards = out3[:8].copy()
    boards[1, np.flatnonzero(boards[1] == 0)[0]] = 10          # inert givens
    boards[2, 80] = 255
    boards[3, np.flatnonzero(boards[3])[:6]] = 0               # several completions
    r = np.flatnonzero(boards[4, :9])                          # a digit twice in row 0
    boards[4, r[0]] = boards[4, r[1]]
    boards[5] = 0
    out, st = M.reduce_level(boards, o[:8], 3)
    assert st.tolist() == [1, 0, 0, 0, 0, 0, 1, 1]
    assert np.array_equal(out, boards)                          # (the eligible ones are minimal already)


def test_a_byte_above_80_is_no_cell():
    g, o = stream()
    order = o[:16].copy()
    order[:, ::2] = 200
    out, st = M.reduce_level(g[:16], order, 2)
    assert (st == 1).all()
    skipped = np.zeros((16, 81), dtype=bool)
    np.put_along_axis(skipped, o[:16, ::2].astype(np.int64), True, axis=1)
    assert (out[skipped] == g[:16][skipped]).all()
    assert (out == 0).any()
