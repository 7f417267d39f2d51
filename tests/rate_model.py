"""A plain model of the rating pass (csrc/rate32_kernel.h): the single-cell backdoors of ONE board,
restated from include/sudoku_hip.h (sdk_rate_batch) with grade_model's fixpoints.

For a board of level 4 with completion S: child(c) is the board with S[c] written into the empty
cell c; c is a backdoor when every cell of F_3(child(c)) is closed.  `backdoors` is the number of
backdoor cells, `key` the lowest one (0xFF if there is none); both are 0xFF for a board of any other
level.  Three ways to build and choose the children, which the header says agree:
  "empty"   children of the input, over its empty cells (the definition);
  "open"    children of the input, over the open cells of F_3 only (a closed one is never a backdoor);
  "closed"  children of the grid that holds F_3's closed cells as givens, over its empty cells.

The boards are assumed uniquely solvable with clean givens, `sol` their completions (grade_model's
assumption); the children are numpy rows closed by grade_model.fixpoint(., 3), each on its own.
"""
import functools

import numpy as np

import grade_model as G
from prop_model import _closed

NONE = 0xFF
VARIANTS = ("empty", "open", "closed")


def children(board, sol, cells):
    """The children of one board over `cells`: uint8[len(cells), 81]."""
    kids = np.tile(np.asarray(board, dtype=np.uint8), (len(cells), 1))
    kids[np.arange(len(cells)), cells] = sol[cells]
    return kids


def rate(boards, sol, variant="empty", grades=None):
    """boards, sol uint8[n,81] -> (backdoors uint8[n], key uint8[n]).  grades: grade_model.grade_states
    of the boards, if the caller has it."""
    if variant not in VARIANTS:
        raise ValueError(f"variant must be one of {VARIANTS}")
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    sol = np.ascontiguousarray(sol, dtype=np.uint8).reshape(-1, 81)
    level, _, F = grades if grades is not None else G.grade_states(boards)
    n = len(boards)
    backdoors = np.full(n, NONE, dtype=np.uint8)
    key = np.full(n, NONE, dtype=np.uint8)
    kids, owner, cell = [], [], []
    for i in np.flatnonzero(level == 4):
        closed = _closed(F[i:i + 1])[0]
        base = np.where(closed, sol[i], 0).astype(np.uint8) if variant == "closed" else boards[i]
        cells = np.flatnonzero(~closed) if variant == "open" else np.flatnonzero(base == 0)
        kids.append(children(base, sol[i], cells))
        owner.append(np.full(len(cells), i))
        cell.append(cells)
        backdoors[i] = 0
    if kids:
        kids, owner, cell = np.concatenate(kids), np.concatenate(owner), np.concatenate(cell)
        done = _closed(G.fixpoint(G.candidates(kids), 3)).all(axis=1)
        np.add.at(backdoors, owner[done], 1)
        # cells ascend inside a parent, so the first closed child of a parent names its key
        for i, c in zip(owner[done][::-1], cell[done][::-1]):
            key[i] = c
    return backdoors, key


def is_backdoor(board, sol, c):
    """Is the empty cell c of this one board a backdoor?"""
    kid = children(board, np.asarray(sol, dtype=np.uint8), np.array([c]))
    return bool(_closed(G.fixpoint(G.candidates(kid), 3)).all())


@functools.lru_cache(maxsize=None)
def pool():
    """grade_model.make_pool() with its grades and model ratings: (boards, sol, level, open, backdoors,
    key), computed once; read-only."""
    boards, sol = G.make_pool()
    level, open_, F = G.grade_states(boards)
    backdoors, key = rate(boards, sol, grades=(level, open_, F))
    for a in (level, open_, backdoors, key):
        a.setflags(write=False)
    return boards, sol, level, open_, backdoors, key
